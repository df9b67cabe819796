"""Helper, not a test: the yardstick of the regression-based and haze-corrected MTF baselines FS, HPM-R, HPM-H and BT-H (lgteun_amd/mtf_hr.py, the k_hr_*
kernels of lgteun_amd/csrc/k_classical.hip).

A numpy / scipy restatement of the definitions in DESIGN.md 3.17, literally and one image at a time: mtf_glp_ref.lowpass of the RAW pan with a replicate
border, the samples [2::4, 2::4], classical_ref.interp23 of that plane (minus the pivot, the sample's first PAN pixel, which is added back), the
statistics over whole arrays, the regression by lstsq on [ms, 1], the rule.
Parametrised by dtype like classical_ref.py: float64 is the yardstick, the distance of the float32 run to it sets the error bar of the GPU tests.  Arrays
are CHW: ms [C, h, w], pan [4h, 4w], results [C, 4h, 4w]; stats is the device's vector of 2C + 2 numbers.  Also the closed forms the kernels use (centred
sums, the centred normal equations), the smallest ratio denominator of a case, and the designed inputs of the haze rules (make_haze_scene): a dark pixel
per band well below everything else, so that the haze terms sit below L and I everywhere."""
import numpy as np

import classical_ref as cr
import mtf_glp_ref as mr

RULES = ('fs', 'hpm_r', 'hpm_h', 'bt_h')
HAZE_RULES = ('hpm_h', 'bt_h')
EQUAL_GAIN, GAIN_PAN = 0.3, 0.15
HAZE_SEED = 7000
# C, h, w, B.  fs / hpm_r run mtf_glp_ref.SHAPES on classical_ref.make_batch; the haze rules these on make_haze_batch
HAZE_SHAPES = [(2, 8, 8, 2), (2, 12, 8, 2), (3, 8, 8, 2), (5, 8, 8, 2), (4, 8, 8, 2), (4, 5, 7, 2), (4, 8, 16, 1), (8, 12, 8, 3), (9, 4, 8, 1), (16, 16, 8, 1),
               (8, 32, 32, 3), (4, 40, 24, 2), (4, 136, 256, 1)]
HAZE_PER_BAND_SHAPES = [(4, 5, 7, 2), (8, 12, 8, 3), (16, 16, 8, 1)]      # hpm_h only: bt_h has one plane


def _swap(shapes, swaps):
    return [swaps.get(s, s) for s in shapes]


# The element-wise cases per rule.  Three listed cases miss the clip-share precondition (at most 2 % of the float64 result within CLIP_MARGIN of 0 or 1) in the
# restatement and are replaced, for that rule only, by the nearest shape that meets all preconditions and covers the same ground (measured in float64, whole case):
#   fs    (4, 5, 7, 2)   2.4 % (equal gains), 4.6 % (per band): on 20 x 28 PAN pixels the gain overshoots -> (4, 7, 9, 2): 2 x 2 ragged tiles, odd sides; 0.4 % / 1.2 %
#   bt_h  (2, 8, 8, 2)   5.3 %: with two bands I - H_I is small around either band's dark pixel, r large   -> (2, 8, 12, 2): 0.02 %
#   bt_h  (4, 5, 7, 2)   2.2 %                                                                             -> (4, 7, 9, 2): 0.0 %
# Two cases more, for the first band counts at which a kernel's dynamic LDS passes 64 KiB: bt_h runs (12, 16, 8, 1) (k_hr_apply<bt_h> at C = 12) and hpm_h runs
# (15, 12, 12, 1) with per-band gains (k_hr_gram at C = F = 15); k_hr_moments's and k_hr_gram's with one plane never pass it.
SHAPES = {'fs': _swap(mr.SHAPES, {(4, 5, 7, 2): (4, 7, 9, 2)}), 'hpm_r': list(mr.SHAPES), 'hpm_h': list(HAZE_SHAPES) + [(15, 12, 12, 1)],
          'bt_h': _swap(HAZE_SHAPES, {(2, 8, 8, 2): (2, 8, 12, 2), (4, 5, 7, 2): (4, 7, 9, 2)}) + [(12, 16, 8, 1)]}
PER_BAND_SHAPES = {'fs': _swap(mr.PER_BAND_SHAPES, {(4, 5, 7, 2): (4, 7, 9, 2)}), 'hpm_r': list(mr.PER_BAND_SHAPES), 'hpm_h': list(HAZE_PER_BAND_SHAPES) + [(15, 12, 12, 1)],
                   'bt_h': []}
PROPERTY_SHAPES = [(4, 4, 4, 1), (4, 5, 7, 2), (8, 12, 8, 3)]
MIN_DENOMINATOR = 0.01
MAX_CONDITION = 1e4
CLIP_MARGIN = mr.CLIP_MARGIN


def make_haze_scene(C, h, w, seed):
    """(ms [C, h, w], pan [4h, 4w]) float32: per band a haze floor 0.04 + 0.01 k under a sinusoid of amplitude 0.12 that stays 0.12 above it, plus N(0, 0.01)
    at PAN resolution; pan = a random convex combination of the bands plus N(0, 0.005); ms = the 4 x 4 block means with ONE pixel per band set to the
    floor itself: the dark pixel the haze estimate finds"""
    rng = np.random.default_rng(seed)
    H, W = 4 * h, 4 * w
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing='ij')
    haze = 0.04 + 0.01 * np.arange(C)
    bands = np.stack([haze[k] + 0.12 + 0.12 * (1 + np.sin(2 * np.pi * ((k % 3 + 1) * yy + ((C - k) % 3 + 1) * xx) + rng.uniform(0, 2 * np.pi)))
                      + rng.normal(0, 0.01, (H, W)) for k in range(C)])
    wgt = rng.uniform(0.5, 1.5, C)
    wgt /= wgt.sum()
    pan = np.tensordot(wgt, bands, axes=1) + rng.normal(0, 0.005, (H, W))
    ms = bands.reshape(C, h, 4, w, 4).mean(axis=(2, 4))
    for k in range(C):
        ms[k].flat[(5 * k + 1 + seed) % (h * w)] = haze[k]
    return ms.astype(np.float32), pan.astype(np.float32)


def make_haze_batch(B, C, h, w, seed=HAZE_SEED):
    """B haze scenes stacked, seeds seed + b: ms [B, C, h, w], pan [B, 1, 4h, 4w]"""
    pairs = [make_haze_scene(C, h, w, seed + b) for b in range(B)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1][None] for p in pairs])


def make_inputs(rule, C, h, w, B):
    """the inputs of a GPU case: classical_ref.make_batch for 'fs' / 'hpm_r' (tests/test_gpu_mtf_glp.py's seeds), the haze scenes for 'hpm_h' / 'bt_h'"""
    return make_haze_batch(B, C, h, w) if rule in HAZE_RULES else cr.make_batch(B, C, h, w, seed=C * 100 + h)


def low_planes(pan, gains, n_taps, dtype):
    """-> (D [F, h, w], L [F, 4h, 4w]) of the raw pan, one pair per DISTINCT run of gains (F = 1 when all are equal), and the index of each band's pair.  PAN
    enters the filter minus its first pixel and the pivot is added back to D and to L = interp23(D - pivot) + pivot: a constant PAN has D = L = pan exactly"""
    pan = np.asarray(pan, dtype=dtype)
    gains = list(gains)
    uniq = gains[:1] if all(g == gains[0] for g in gains) else gains
    pv = pan[0, 0]
    Dc = np.stack([mr.lowpass(pan - pv, mr.taps(g, n_taps))[2::4, 2::4] for g in uniq]).astype(dtype)
    return (Dc + pv).astype(dtype), (cr.interp23(Dc, dtype) + pv).astype(dtype), [0 if len(uniq) == 1 else k for k in range(len(gains))]


def regress(ms, D, dtype=np.float64, pivot=0.0):
    """the direct form: lstsq of [ms_1 .. ms_C, 1] w = D over the h w pixels -> w [C + 1], the intercept last.  pivot: what D enters the fit without and the
    intercept gets back (the sample's first PAN pixel: the fit of a constant PAN has a right-hand side of zeros and slopes of exactly 0)"""
    C = ms.shape[0]
    A = np.concatenate([np.asarray(ms, dtype=dtype).reshape(C, -1).T, np.ones((ms[0].size, 1), dtype=dtype)], axis=1)
    wts = np.linalg.lstsq(A, (np.asarray(D, dtype=dtype) - dtype(pivot)).reshape(-1, 1), rcond=None)[0][:, 0].astype(dtype)
    wts[C] += dtype(pivot)
    return wts


def regress_closed(ms, D):
    """float64, the kernels' form: slopes = Sigma_ms^-1 cov(ms, D) from sums centred on each band's first pixel, the intercept from the means.  Also the
    condition number of the centred Gram matrix"""
    ms = np.asarray(ms, dtype=np.float64)
    C = ms.shape[0]
    n = ms[0].size
    x = ms.reshape(C, -1) - ms.reshape(C, -1)[:, :1]
    d = np.asarray(D, dtype=np.float64).reshape(-1)
    sx, sd = x.sum(axis=1), d.sum()
    G = x @ x.T - np.outer(sx, sx) / n
    slopes = np.linalg.solve(G, x @ d - sx * sd / n)
    means = ms.reshape(C, -1)[:, 0] + sx / n
    return np.concatenate([slopes, [sd / n - slopes @ means]]), float(np.linalg.cond(G))


def gains_closed(ms, pan, rule, gains, n_taps=41):
    """float64, the kernels' form of the gains of 'fs' / 'hpm_r': sums of u - m, L - mu, pan - mu and their products, corrected by the sums themselves"""
    u = cr.interp23(ms)
    pan = np.asarray(pan, dtype=np.float64)
    _, L, idx = low_planes(pan, gains, n_taps, np.float64)
    N, mu = pan.size, pan.mean()
    g, b = np.zeros(u.shape[0]), np.zeros(u.shape[0])
    for k in range(u.shape[0]):
        m = u[k].mean()
        uc, lc, pc = u[k] - m, L[idx[k]] - mu, pan - mu
        su, sl, sp = uc.sum(), lc.sum(), pc.sum()
        if rule == 'fs':
            g[k] = ((uc * pc).sum() - su * sp / N) / ((lc * pc).sum() - sl * sp / N)
        else:
            g[k] = ((uc * lc).sum() - su * sl / N) / ((lc * lc).sum() - sl * sl / N)
            b[k] = m - g[k] * (mu + sl / N)
    return g, b


def _ratio(num, den, dtype):
    """num / den, 1 where the denominator is not > 0 or the ratio is not finite"""
    with np.errstate(divide='ignore', invalid='ignore'):
        r = (num / den).astype(dtype)
    return np.where((den > 0) & np.isfinite(r), r, dtype(1))


def _gain(num, den, dtype):
    with np.errstate(divide='ignore', invalid='ignore'):
        g = dtype(num) / dtype(den)
    return g if den > 0 and np.isfinite(den) and np.isfinite(g) else dtype(0)


def mtf_hr(ms, pan, rule, gains=None, gain_pan=GAIN_PAN, n_taps=41, dtype=np.float64, return_stats=False, clip=True, return_den=False):
    """gains: one per band (None: EQUAL_GAIN each); 'bt_h' filters with gain_pan instead.  return_stats: also the 2C + 2 numbers of the device's stats;
    clip=False: the values before the clip; return_den: also the smallest ratio denominator of the case (inf for 'fs', which divides by none)"""
    ms = np.asarray(ms, dtype=dtype)
    pan = np.asarray(pan, dtype=dtype)
    C = ms.shape[0]
    u = cr.interp23(ms, dtype)
    gains = [EQUAL_GAIN] * C if gains is None else list(gains)
    stats = np.zeros(2 * C + 2, dtype=dtype)
    out = np.empty_like(u)
    den_min = np.inf
    if rule in ('fs', 'hpm_r'):
        _, L, idx = low_planes(pan, gains, n_taps, dtype)
        mu = pan.mean(dtype=dtype)
        pc = pan - mu
        for k in range(C):
            Lk = L[idx[k]]
            m, ell = u[k].mean(dtype=dtype), Lk.mean(dtype=dtype)
            if rule == 'fs':
                g = _gain(((u[k] - m) * pc).sum(dtype=dtype), ((Lk - ell) * pc).sum(dtype=dtype), dtype)
                out[k] = u[k] + g * (pan - Lk)
            else:
                g = _gain(((u[k] - m) * (Lk - ell)).sum(dtype=dtype), ((Lk - ell) * (Lk - ell)).sum(dtype=dtype), dtype)
                b = dtype(m - g * ell)
                den = g * Lk + b
                den_min = min(den_min, float(den.min()))
                out[k] = u[k] * _ratio(g * pan + b, den, dtype)
                stats[C + k] = b
            stats[k] = g
    elif rule == 'hpm_h':
        D, L, idx = low_planes(pan, gains, n_taps, dtype)
        H = ms.reshape(C, -1).min(axis=1)
        wts = [regress(ms, D[f], dtype, pan[0, 0]) for f in range(D.shape[0])]
        for k in range(C):
            wk = wts[idx[k]]
            HP = dtype(wk[C] + wk[:C] @ H)
            den = L[idx[k]] - HP
            den_min = min(den_min, float(den.min()))
            out[k] = (u[k] - H[k]) * _ratio(pan - HP, den, dtype) + H[k]
            stats[C + k] = HP
        stats[:C] = H
    elif rule == 'bt_h':
        D, _, _ = low_planes(pan, [gain_pan], n_taps, dtype)
        H = ms.reshape(C, -1).min(axis=1)
        wk = regress(ms, D[0], dtype, pan[0, 0])
        HI = dtype(wk[C] + wk[:C] @ H)
        den = np.tensordot(wk[:C], u - H[:, None, None], axes=1).astype(dtype)      # I - H_I, never a difference of two sums
        den_min = float(den.min())
        r = _ratio(pan - HI, den, dtype)
        out = (u - H[:, None, None]) * r[None] + H[:, None, None]
        stats[:C], stats[C:2 * C], stats[2 * C], stats[2 * C + 1] = H, wk[:C], wk[C], HI
    else:
        raise ValueError(rule)
    out = (np.clip(out, 0, 1) if clip else out).astype(dtype)
    res = (out,) + ((stats,) if return_stats else ()) + ((den_min,) if return_den else ())
    return res if len(res) > 1 else out
