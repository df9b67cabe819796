"""Helper, not a test: the yardstick of the MTF-GLP baselines (lgteun_amd/mtf_glp.py, the k_mg_* kernels of lgteun_amd/csrc/k_classical.hip).

A numpy / scipy restatement of the definitions in DESIGN.md 3.13, literally and one image at a time: the histogram-matched PAN p_k, correlate1d with a
replicate border along both axes, the samples [2::4, 2::4], classical_ref.interp23 of that plane, the rule.  Parametrised by dtype like classical_ref.py:
float64 is the yardstick, the distance of the float32 run to it sets the error bar of the GPU tests.  Arrays are CHW: ms [C, h, w], pan [4h, 4w], results
[C, 4h, 4w].  Also the low-pass as explicit sums over clamped indices (no scipy), and the inputs of the saturation test."""
import numpy as np
from scipy import ndimage

import classical_ref as cr

SHAPES = [(4, 4, 4, 1), (4, 8, 8, 2), (4, 5, 7, 2), (8, 12, 8, 3), (8, 32, 32, 3), (4, 40, 24, 2), (4, 136, 256, 1)]      # C, h, w, B
PER_BAND_SHAPES = [SHAPES[2], SHAPES[3], SHAPES[6]]
MODES = ('glp', 'hpm', 'cbd')
EQUAL_GAIN = 0.3
CLIP_SHAPE, CLIP_SEED = (4, 8, 8, 2), 9      # the saturation test's inputs (make_clip_batch)
CLIP_MARGIN = 1e-5                           # an element further than this outside [0, 1] in float64 must come out as exactly 0.0 or 1.0


def per_band_gains(C):
    return [0.22 + 0.02 * k for k in range(C)]


def taps(gain, n_taps=41):
    """lgteun_amd.wald.mtf_taps, restated: the Gaussian whose response at the MS grid's Nyquist frequency is `gain`, normalised to sum 1"""
    sigma = 4.0 * np.sqrt(-2.0 * np.log(float(gain))) / np.pi
    x = np.arange(n_taps, dtype=np.float64) - n_taps // 2
    t = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return t / t.sum()


def lowpass(p, t):
    """the separable filter on the whole plane, replicate border, in p's dtype"""
    t = np.asarray(t, dtype=p.dtype)
    return ndimage.correlate1d(ndimage.correlate1d(p, t, axis=1, mode='nearest'), t, axis=0, mode='nearest')


def lowpass_decimated_explicit(p, t):
    """float64: D(i, j) = sum_a sum_b t_a t_b p(clamp(4 i + 2 + a - r), clamp(4 j + 2 + b - r)), as written"""
    p = np.asarray(p, dtype=np.float64)
    H, W = p.shape
    r = len(t) // 2
    ys = np.clip(4 * np.arange(H // 4)[:, None] + 2 + np.arange(len(t))[None, :] - r, 0, H - 1)      # [h, n]
    xs = np.clip(4 * np.arange(W // 4)[:, None] + 2 + np.arange(len(t))[None, :] - r, 0, W - 1)      # [w, n]
    out = np.zeros((H // 4, W // 4))
    for a in range(len(t)):
        for b in range(len(t)):
            out += t[a] * t[b] * p[ys[:, a]][:, xs[:, b]]
    return out


def stats(ms, pan, dtype=np.float64):
    """-> (u [C, 4h, 4w], mu, s, m [C], a [C]): SFIM's numbers; a = 0 for a constant PAN"""
    u = cr.interp23(ms, dtype)
    pan = np.asarray(pan, dtype=dtype)
    mu, s = pan.mean(dtype=dtype), np.std(pan, ddof=1, dtype=dtype)
    m = np.array([u[k].mean(dtype=dtype) for k in range(u.shape[0])], dtype=dtype)
    a = np.array([np.std(u[k], ddof=1, dtype=dtype) / s if s > 0 else 0.0 for k in range(u.shape[0])], dtype=dtype)
    return u, dtype(mu), dtype(s), m, a


def mtf_glp(ms, pan, mode, gains, n_taps=41, dtype=np.float64, return_stats=False, clip=True):
    """gains: one per band.  return_stats: also a [C] and g [C] (1 for 'glp' and 'hpm').  clip=False: the values before the clip"""
    u, mu, _, m, a = stats(ms, pan, dtype)
    pan = np.asarray(pan, dtype=dtype)
    C = u.shape[0]
    out, g = np.empty_like(u), np.ones(C, dtype=dtype)
    for k in range(C):
        p = (a[k] * (pan - mu) + m[k]).astype(dtype)
        q = lowpass(p, taps(gains[k], n_taps))[2::4, 2::4]
        L = cr.interp23(q[None], dtype)[0]
        if mode == 'glp':
            out[k] = u[k] + (p - L)
        elif mode == 'hpm':
            out[k] = u[k] * p / (L + dtype(1e-8))
        else:
            Lc = L - L.mean(dtype=dtype)
            den = (Lc * Lc).sum(dtype=dtype)
            g[k] = ((u[k] - m[k]) * Lc).sum(dtype=dtype) / den if a[k] != 0 and den > 0 else 0.0
            if not np.isfinite(g[k]):
                g[k] = 0.0
            out[k] = u[k] + g[k] * (p - L)
    out = (np.clip(out, 0, 1) if clip else out).astype(dtype)
    return (out, a, g) if return_stats else out


def make_clip_batch(C, h, w, B, seed):
    """inputs whose results leave [0, 1] on both sides under every rule, in the manner of wavelet_ref.make_clip_batch: x' = 4 x - 1 in fp32 for PAN and for
    every band, clipped back into [0, 1] (the methods take normalised samples).  The bands then sit on 0 and on 1 over whole regions: the interpolation
    overshoots there, and the histogram-matched PAN, which has the band's spread, leaves the range with it"""
    ms, pan = cr.make_batch(B, C, h, w, seed)
    return tuple(np.clip(np.float32(4) * x - np.float32(1), 0, 1).astype(np.float32) for x in (ms, pan))
