"""Helper, not a test: the yardstick of the a trous baselines ATWT and AWLP (lgteun_amd/atrous.py, the k_at_* kernels of lgteun_amd/csrc/k_classical.hip).

A numpy / scipy restatement of the definitions in DESIGN.md 3.16, literally and one image at a time: classical_ref.interp23, the two-level B3-spline cascade
with correlate1d(mode='wrap') -- (1, 4, 6, 4, 1) / 16 along rows and columns, then the same five taps two apart -- the detail pan - P_L, the scale of each
band by std(pan) ('pan') or by the deviation of P_L about the mean of PAN ('lowpass'), the rule.  Parametrised by dtype like classical_ref.py: float64 is
the yardstick, the distance of the float32 run to it sets the error bar of the GPU tests.  Arrays are CHW: ms [C, h, w], pan [4h, 4w], results [C, 4h, 4w].
Also the cascade as one 13-tap filter, the same as explicit sums over modulo-indexed samples (no scipy), the shapes of the GPU tests and the inputs of the
saturation test."""
import numpy as np
from scipy import ndimage

import classical_ref as cr

RULES = ('atwt', 'awlp')
MATCHES = ('pan', 'lowpass')
B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
TAPS13 = np.array([1.0, 4.0, 10.0, 20.0, 31.0, 40.0, 44.0, 40.0, 31.0, 20.0, 10.0, 4.0, 1.0]) / 256.0      # by offset -6 .. 6
# C, h, w, B: the cases whose OUTPUT is compared, per match (at most 2 % of the float64 restatement may lie outside (0, 1): test_atrous_cpu.py re-derives it)
SHAPES = {
    'pan': [(4, 4, 4, 1), (4, 8, 8, 2), (4, 5, 7, 2), (8, 12, 8, 3), (8, 32, 32, 3), (4, 40, 24, 2), (4, 136, 256, 1), (2, 5, 7, 2), (3, 6, 9, 1), (16, 8, 8, 1)],
    'lowpass': [(4, 16, 16, 2), (4, 17, 33, 2), (4, 33, 17, 2), (4, 20, 12, 1), (8, 32, 32, 3), (4, 40, 24, 2), (4, 136, 256, 1), (3, 18, 26, 1), (2, 17, 33, 1)],
}
# 'lowpass' on the tiny shapes and at C = 16: this generator's low-passed PAN has so little variance there that 5 - 28 % of the restatement clips.  They are
# run for their STATISTICS only (a_k and s_L, which no clip touches)
STATS_ONLY_SHAPES = [(4, 4, 4, 1), (4, 8, 8, 2), (4, 5, 7, 2), (8, 12, 8, 3), (2, 5, 7, 2), (3, 6, 9, 1), (16, 8, 8, 1)]
CLIP_SHAPE, CLIP_SEED = (4, 8, 8, 2), 9      # the saturation test's inputs (make_clip_batch)
CLIP_MARGIN = 1e-5                           # an element further than this outside [0, 1] in float64 must come out as exactly 0.0 or 1.0
EPS = 1e-8                                   # SFIM's


def make_inputs(C, h, w, B):
    """the inputs of a case: classical_ref.make_batch with the seed every classical GPU test uses"""
    return cr.make_batch(B, C, h, w, seed=100 * C + h)


def lowpass(p, dtype=np.float64):
    """P_L: the two-level undecimated cascade, circular, in `dtype`"""
    p = np.asarray(p, dtype=dtype)
    b1 = B3.astype(dtype)
    b2 = np.zeros(9, dtype=dtype)
    b2[::2] = b1                             # the same five taps at offsets -4, -2, 0, 2, 4
    for b in (b1, b2):
        p = ndimage.correlate1d(ndimage.correlate1d(p, b, axis=1, mode='wrap'), b, axis=0, mode='wrap').astype(dtype)
    return p


def lowpass13(p, dtype=np.float64):
    """the cascade as ONE separable 13-tap circular filter"""
    p = np.asarray(p, dtype=dtype)
    t = TAPS13.astype(dtype)
    return ndimage.correlate1d(ndimage.correlate1d(p, t, axis=1, mode='wrap'), t, axis=0, mode='wrap').astype(dtype)


def lowpass_explicit(p):
    """float64: P_L(y, x) = sum_a sum_b t_a t_b p((y + a) mod H, (x + b) mod W), as written"""
    p = np.asarray(p, dtype=np.float64)
    H, W = p.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros((H, W))
    for a in range(-6, 7):
        for b in range(-6, 7):
            out += TAPS13[a + 6] * TAPS13[b + 6] * p[(ys + a) % H][:, (xs + b) % W]
    return out


def atrous(ms, pan, rule, match='pan', dtype=np.float64, return_stats=False, clip=True):
    """return_stats: also a [C] and the reference deviation (std(pan) or s_L).  clip=False: the values before the clip"""
    assert rule in RULES and match in MATCHES
    u = cr.interp23(ms, dtype)
    pan = np.asarray(pan, dtype=dtype)
    pan = pan - pan[0, 0]                    # the house rule: PAN enters every sum minus the sample's first pixel (a constant PAN is exactly zero)
    C, N = u.shape[0], pan.size
    mu = pan.mean(dtype=dtype)
    PL = lowpass(pan, dtype)
    d = (pan - PL).astype(dtype)
    if match == 'pan':
        ref = np.std(pan, ddof=1, dtype=dtype)
    else:
        ref = np.sqrt(((PL - mu) ** 2).sum(dtype=dtype) / dtype(N - 1))
    ref = dtype(ref)
    a = np.array([np.std(u[k], ddof=1, dtype=dtype) / ref if ref > 0 else 0.0 for k in range(C)], dtype=dtype)
    if rule == 'atwt':
        out = u + a[:, None, None] * d[None]
    else:
        den = (u.mean(axis=0, dtype=dtype) + dtype(EPS)).astype(dtype)
        ok = (den > 0) & np.isfinite(den)
        ratio = np.where(ok[None], u / np.where(ok, den, dtype(1))[None], dtype(0)).astype(dtype)
        out = u + a[:, None, None] * d[None] * ratio
    out = (np.clip(out, 0, 1) if clip else out).astype(dtype)
    return (out, a, ref) if return_stats else out


def make_clip_batch(C, h, w, B, seed):
    """mtf_glp_ref.make_clip_batch's recipe, restated: x' = 4 x - 1 in fp32 for PAN and for every band, clipped back into [0, 1].  The bands then sit on 0 and
    on 1 over whole regions: the interpolation overshoots there, and the detail of the stretched PAN carries the result further out"""
    ms, pan = cr.make_batch(B, C, h, w, seed)
    return tuple(np.clip(np.float32(4) * x - np.float32(1), 0, 1).astype(np.float32) for x in (ms, pan))
