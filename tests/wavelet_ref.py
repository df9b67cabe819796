"""Helper, not a test: the yardstick of the Wavelet baseline (lgteun_amd/classical.py:wavelet, k_cl_wavelet in lgteun_amd/csrc/k_classical.hip).

A numpy restatement of DESIGN.md 3.12's definition on top of tests/classical_ref.py, one image at a time, CHW like there: the explicit form
(interp23, two-level orthonormal Haar analysis of PAN and of every band, substitution of the level-2 approximation, synthesis, clip), parametrised by
dtype like cr.sfim; the closed form it collapses to; the 17 taps of the FIR that gives the block means of interp23(ms) from ms; and the inputs of
the GPU tests, the clip case among them."""
import numpy as np

import classical_ref as cr

SHAPES = [(4, 4, 4, 1), (4, 8, 8, 2), (4, 5, 7, 2), (8, 12, 8, 3), (8, 32, 32, 3), (4, 40, 24, 2), (4, 136, 256, 1)]      # tests/test_gpu_classical.py's seven
CLIP_SHAPES = [(4, 8, 8, 2), (8, 12, 8, 3)]


def _analysis(x):
    """one orthonormal Haar level, rows then columns: a = (x0 + x1) / sqrt 2, d = (x0 - x1) / sqrt 2 -> (aa, (ad, da, dd))"""
    s = x.dtype.type(np.sqrt(x.dtype.type(2)))
    lo, hi = (x[0::2] + x[1::2]) / s, (x[0::2] - x[1::2]) / s
    return (lo[:, 0::2] + lo[:, 1::2]) / s, ((lo[:, 0::2] - lo[:, 1::2]) / s, (hi[:, 0::2] + hi[:, 1::2]) / s, (hi[:, 0::2] - hi[:, 1::2]) / s)


def _synthesis(aa, details):
    ad, da, dd = details
    s = aa.dtype.type(np.sqrt(aa.dtype.type(2)))
    lo = np.empty((aa.shape[0], 2 * aa.shape[1]), dtype=aa.dtype)
    hi = np.empty_like(lo)
    lo[:, 0::2], lo[:, 1::2] = (aa + ad) / s, (aa - ad) / s
    hi[:, 0::2], hi[:, 1::2] = (da + dd) / s, (da - dd) / s
    x = np.empty((2 * lo.shape[0], lo.shape[1]), dtype=aa.dtype)
    x[0::2], x[1::2] = (lo + hi) / s, (lo - hi) / s
    return x


def wavelet(ms, pan, dtype=np.float64):
    """the explicit form: per band the two-level Haar decomposition of PAN with its level-2 approximation replaced by the band's, reconstructed"""
    u = cr.interp23(ms, dtype)
    pan = np.asarray(pan, dtype=dtype)
    a1, d1 = _analysis(pan)
    _, d2 = _analysis(a1)
    out = np.empty_like(u)
    for k in range(u.shape[0]):
        b2, _ = _analysis(_analysis(u[k])[0])
        out[k] = _synthesis(_synthesis(b2, d2), d1)
    return np.clip(out, 0, 1).astype(dtype)


def block_mean(x):
    """[..., 4m, 4n] -> [..., m, n]"""
    return x.reshape(x.shape[:-2] + (x.shape[-2] // 4, 4, x.shape[-1] // 4, 4)).mean(axis=(-3, -1))


def wavelet_closed_form(ms, pan):
    """float64, UNCLIPPED: pan - its 4 x 4 block mean + the block mean of interp23(ms)_k"""
    pan = np.asarray(pan, dtype=np.float64)
    up4 = lambda m: np.repeat(np.repeat(m, 4, axis=-2), 4, axis=-1)      # noqa: E731
    return (pan - up4(block_mean(pan)))[None] + up4(block_mean(cr.interp23(ms)))


def taps17():
    """the FIR's taps by offset -8 .. 8, by the 1-D chain from cr.taps23(): a unit impulse, level 1 (zero insertion at the odd positions, the 23 taps),
    level 2 (at the even positions, the 23 taps), the mean of groups of 4.  On a line of 64 ms samples nothing wraps."""
    n, t = 64, cr.taps23()
    x = np.zeros(n)
    x[n // 2] = 1.0
    for off in (1, 0):
        up = np.zeros(2 * x.size)
        up[off::2] = x
        x = np.array([sum(t[k + 11] * up[(i + k) % up.size] for k in range(-11, 12)) for i in range(up.size)])
    m = x.reshape(n, 4).mean(axis=1)
    assert not m[:n // 2 - 8].any() and not m[n // 2 + 9:].any()
    return m[n // 2 - 8:n // 2 + 9]


def fir_block_means(ms, taps):
    """M_k(i, j) = sum_a sum_b t_a t_b ms_k((i - a) mod h, (j - b) mod w), float64"""
    ms = np.asarray(ms, dtype=np.float64)
    rows = sum(taps[a + 8] * np.roll(ms, a, axis=1) for a in range(-8, 9))
    return sum(taps[b + 8] * np.roll(rows, b, axis=2) for b in range(-8, 9))


def make_batch(C, h, w, B):
    """the inputs of a shape in the GPU tests: ms [B, C, h, w], pan [B, 1, 4h, 4w]"""
    return cr.make_batch(B, C, h, w, seed=C * 100 + h)


def make_clip_batch(C, h, w, B):
    """inputs whose result leaves [0, 1] on both sides: pan' = 4 pan - 1 in fp32, ms' = ms with 0.45 added to the upper half of the bands"""
    ms, pan = make_batch(C, h, w, B)
    ms = ms.copy()
    ms[:, C // 2:] += np.float32(0.45)
    return ms, np.float32(4) * pan - np.float32(1)
