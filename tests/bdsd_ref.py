"""Helper, not a test: the yardstick of the BDSD baseline (lgteun_amd/bdsd.py, the k_bd_* kernels of lgteun_amd/csrc/k_classical.hip).

A numpy / scipy restatement of the definition in DESIGN.md 3.14, literally and one image at a time: classical_ref.interp23 of the bands, the bands
low-passed on their own grid (correlate1d, replicate border), the raw PAN low-passed and sampled at [2::4, 2::4], per block the least-squares fit of
ms_k - A_k on [A_1 .. A_C, D] with np.linalg.lstsq, the mix of the interpolated bands and PAN.  Parametrised by dtype like mtf_glp_ref.py: float64 is the
yardstick, the distance of the float32 run to it sets the error bar of the GPU tests.  A second route solves the explicit normal equations with
np.linalg.cholesky: the distance between the two routes sets the gate of the weights.  Arrays are CHW: ms [C, h, w], pan [4h, 4w], results [C, 4h, 4w],
weights [nby, nbx, C, C + 1].  Also the MS-grid low-pass as explicit sums over clamped indices (no scipy), a scene generator of smooth correlated fields
(classical_ref.make_scene's sinusoids are eigenfunctions of the low-pass: the fit then predicts their high-pass part from their low-pass part with huge
weights), and the inputs of the saturation test."""
import numpy as np
from scipy import ndimage

import classical_ref as cr
import mtf_glp_ref as mr

# C, h, w, B, block (None: global)
CASES = [(4, 8, 8, 2, None), (4, 5, 7, 2, None), (8, 12, 8, 3, None), (4, 8, 16, 2, 32), (2, 8, 8, 1, 32), (4, 40, 24, 2, 32), (8, 16, 24, 2, 32),
         (8, 32, 32, 3, 32), (8, 32, 32, 3, 64), (4, 24, 40, 2, 32), (4, 136, 256, 1, None), (4, 136, 256, 1, 32)]
PER_BAND_CASES = [(4, 5, 7, 2, None), (8, 32, 32, 3, 32), (4, 136, 256, 1, 32)]
EQUAL_GAIN, GAIN_PAN = 0.3, 0.15
PIVOT_TOL = 1e-12                            # a block whose Cholesky pivot d_j is at most this times G_jj is degenerate
CLIP_CASE, CLIP_SEED = (4, 8, 8, 2, None), 9      # the saturation test's inputs (make_clip_batch)
CLIP_MARGIN = mr.CLIP_MARGIN


def lowpass_ms(band, t):
    """A: the band low-passed on its own grid, replicate border, no decimation, in the band's dtype"""
    return mr.lowpass(band, t)


def lowpass_ms_explicit(band, t):
    """float64: A(i, j) = sum_a sum_b t_a t_b band(clamp(i + a - r), clamp(j + b - r)), as written"""
    band = np.asarray(band, dtype=np.float64)
    h, w = band.shape
    r = len(t) // 2
    ys = np.clip(np.arange(h)[:, None] + np.arange(len(t))[None, :] - r, 0, h - 1)      # [h, n]
    xs = np.clip(np.arange(w)[:, None] + np.arange(len(t))[None, :] - r, 0, w - 1)      # [w, n]
    out = np.zeros((h, w))
    for a in range(len(t)):
        for b in range(len(t)):
            out += t[a] * t[b] * band[ys[:, a]][:, xs[:, b]]
    return out


def regressors(ms, pan, gains, gain_pan=GAIN_PAN, n_taps=41, dtype=np.float64):
    """-> (x [C + 1, h, w]: A_1 .. A_C and D; y [C, h, w] = ms - A)"""
    ms = np.asarray(ms, dtype=dtype)
    pan = np.asarray(pan, dtype=dtype)
    A = np.stack([lowpass_ms(ms[k], mr.taps(gains[k], n_taps)) for k in range(ms.shape[0])])
    D = mr.lowpass(pan, mr.taps(gain_pan, n_taps))[2::4, 2::4]
    return np.concatenate([A, D[None]]).astype(dtype), (ms - A).astype(dtype)


def _solve_lstsq(X, Y):
    """a rank-deficient block gives zeros"""
    gam, _, rank, _ = np.linalg.lstsq(X, Y, rcond=None)
    return gam.T if rank == X.shape[1] else np.zeros((Y.shape[1], X.shape[1]), dtype=X.dtype)


def _solve_cholesky(X, Y):
    """the explicit normal equations G gamma_k = r_k; a pivot at or below PIVOT_TOL G_jj, or one that is not finite, gives zeros"""
    G, R = X.T @ X, X.T @ Y
    try:
        L = np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        return np.zeros((Y.shape[1], X.shape[1]), dtype=X.dtype)
    d = np.diag(L) ** 2
    if not np.all(np.isfinite(d)) or np.any(d <= PIVOT_TOL * np.diag(G)):
        return np.zeros((Y.shape[1], X.shape[1]), dtype=X.dtype)
    return np.linalg.solve(L.T, np.linalg.solve(L, R)).T


def weights(ms, pan, gains, block=None, gain_pan=GAIN_PAN, n_taps=41, dtype=np.float64, route='lstsq'):
    """gamma [nby, nbx, C, C + 1] per block of block x block PAN pixels (None: one block); a fit that is not finite gives zeros.  route: 'lstsq' or 'cholesky'"""
    x, y = regressors(ms, pan, gains, gain_pan, n_taps, dtype)
    C, h, w = y.shape
    sy, sx = (h, w) if block is None else (block // 4, block // 4)
    assert h % sy == 0 and w % sx == 0
    solve = {'lstsq': _solve_lstsq, 'cholesky': _solve_cholesky}[route]
    g = np.zeros((h // sy, w // sx, C, C + 1), dtype=dtype)
    for I in range(h // sy):
        for J in range(w // sx):
            X = x[:, I * sy:(I + 1) * sy, J * sx:(J + 1) * sx].reshape(C + 1, -1).T
            Y = y[:, I * sy:(I + 1) * sy, J * sx:(J + 1) * sx].reshape(C, -1).T
            gam = solve(X, Y).astype(dtype)
            g[I, J] = gam if np.all(np.isfinite(gam)) else 0
    return g


def bdsd(ms, pan, gains, block=None, gain_pan=GAIN_PAN, n_taps=41, dtype=np.float64, return_stats=False, clip=True, route='lstsq'):
    """gains: one per band.  return_stats: also gamma.  clip=False: the values before the clip"""
    g = weights(ms, pan, gains, block, gain_pan, n_taps, dtype, route)
    u = cr.interp23(ms, dtype)
    pan = np.asarray(pan, dtype=dtype)
    C, H, W = u.shape
    sy, sx = (H, W) if block is None else (block, block)
    out = np.empty_like(u)
    for I in range(H // sy):
        for J in range(W // sx):
            win = (slice(None), slice(I * sy, (I + 1) * sy), slice(J * sx, (J + 1) * sx))
            gam = g[I, J]
            out[win] = u[win] + np.tensordot(gam[:, :C], u[win], axes=1) + gam[:, C, None, None] * pan[win[1:]][None]
    out = (np.clip(out, 0, 1) if clip else out).astype(dtype)
    return (out, g) if return_stats else out


def gamma_distance(a, b):
    """the largest absolute difference of two sets of weights of one sample over that sample's largest |gamma| (b's)"""
    return float(np.abs(a - b).max() / np.abs(b).max())


def _field(rng, H, W, sigma):
    f = ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma, mode='wrap')
    return f / f.std()


def make_scene(C, h, w, seed):
    """(ms [C, h, w], pan [4h, 4w]) float32 in [0.02, 0.98]: smooth, correlated fields.  field(s) is unit-variance Gaussian-filtered (sigma s, wrap border)
    white noise at PAN size; a band is 0.5 + 0.04 (a field(6) + b field(2)) + 0.012 field(3) + 0.004 field(1) with the first two fields shared by the bands,
    a in U(0.6, 1), b in U(0.4, 0.8); pan = a random convex combination of the bands + 0.004 field(1); ms = the 4 x 4 block means"""
    rng = np.random.default_rng(seed)
    H, W = 4 * h, 4 * w
    s1, s2 = _field(rng, H, W, 6), _field(rng, H, W, 2)
    bands = np.stack([0.5 + 0.04 * (rng.uniform(0.6, 1.0) * s1 + rng.uniform(0.4, 0.8) * s2) + 0.012 * _field(rng, H, W, 3) + 0.004 * _field(rng, H, W, 1)
                      for _ in range(C)])
    wgt = rng.uniform(0.5, 1.5, C)
    wgt /= wgt.sum()
    pan = np.tensordot(wgt, bands, axes=1) + 0.004 * _field(rng, H, W, 1)
    ms = bands.reshape(C, h, 4, w, 4).mean(axis=(2, 4))
    return np.clip(ms, 0.02, 0.98).astype(np.float32), np.clip(pan, 0.02, 0.98).astype(np.float32)


def make_batch(B, C, h, w, seed):
    """B scenes stacked: ms [B, C, h, w], pan [B, 1, 4h, 4w]"""
    pairs = [make_scene(C, h, w, seed * 1000 + b) for b in range(B)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1][None] for p in pairs])


def make_clip_batch(C, h, w, B, seed):
    """inputs whose results leave [0, 1] on both sides, in the manner of mtf_glp_ref.make_clip_batch: x' = 0.5 + 12 (x - 0.5) in fp32 for PAN and for every
    band, clipped back into [0, 1].  The bands then sit on 0 and on 1 over whole regions: the interpolation overshoots there, and so does the mix"""
    ms, pan = make_batch(B, C, h, w, seed)
    return tuple(np.clip(np.float32(0.5) + np.float32(12) * (x - np.float32(0.5)), 0, 1).astype(np.float32) for x in (ms, pan))
