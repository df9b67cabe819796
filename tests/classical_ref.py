"""Helper, not a test: the yardstick of the classical baselines (lgteun_amd/classical.py, lgteun_amd/csrc/k_classical.hip).

A numpy / scipy restatement of the definitions in DESIGN.md 3.12, one image at a time, parametrised by dtype so that it runs in float64 (the
yardstick) and in float32 (whose distance to the float64 run sets the error bar of the GPU tests).  Arrays are CHW: ms [C, h, w], pan [4h, 4w],
results [C, 4h, 4w].  Also a seeded synthetic scene generator whose outputs stay off the clip boundaries."""
import numpy as np
from scipy import ndimage

HALF = (0.305334091185, -0.072698593239, 0.021809577942, -0.005192756653, 0.000807762146, -0.000060081482)     # taps at offsets 1, 3, .. 11, halved


def taps23(dtype=np.float64):
    """the 23 taps by offset -11 .. 11: 1 at the centre, 2 x HALF at the odd offsets, 0 at the even ones"""
    t = np.zeros(23, dtype=np.float64)
    t[11] = 1.0
    for i, v in enumerate(HALF):
        t[11 + 2 * i + 1] = t[11 - 2 * i - 1] = 2.0 * v
    return t.astype(dtype)


def interp23(ms, dtype=np.float64):
    """two x2 levels: zero insertion (level 1 at the odd positions, level 2 at the even ones), rows then columns, circular"""
    t = taps23(dtype)
    img = np.asarray(ms, dtype=dtype)
    for level in (1, 2):
        C, r, c = img.shape
        up = np.zeros((C, 2 * r, 2 * c), dtype=dtype)
        if level == 1:
            up[:, 1::2, 1::2] = img
        else:
            up[:, 0::2, 0::2] = img
        up = ndimage.correlate1d(up, t, axis=2, mode='wrap')
        up = ndimage.correlate1d(up, t, axis=1, mode='wrap')
        img = up.astype(dtype)
    return img


def interp23_explicit(ms):
    """the same in float64 as explicit sums over modulo-indexed samples (no scipy): checks the restatement's boundary handling"""
    t = taps23()
    img = np.asarray(ms, dtype=np.float64)
    for level in (1, 2):
        C, r, c = img.shape
        up = np.zeros((C, 2 * r, 2 * c))
        off = 1 if level == 1 else 0
        up[:, off::2, off::2] = img
        rows = np.zeros_like(up)
        for x in range(2 * c):
            for k in range(-11, 12):
                rows[:, :, x] += t[k + 11] * up[:, :, (x + k) % (2 * c)]
        cols = np.zeros_like(up)
        for y in range(2 * r):
            for k in range(-11, 12):
                cols[:, y, :] += t[k + 11] * rows[:, (y + k) % (2 * r), :]
        img = cols
    return img


def sfim(ms, pan, dtype=np.float64):
    u = interp23(ms, dtype)
    pan = np.asarray(pan, dtype=dtype)
    out = np.empty_like(u)
    for k in range(u.shape[0]):
        p = (pan - pan.mean(dtype=dtype)) * (np.std(u[k], ddof=1, dtype=dtype) / np.std(pan, ddof=1, dtype=dtype)) + u[k].mean(dtype=dtype)
        p = p.astype(dtype)
        lp = ndimage.uniform_filter(p, size=5, mode='wrap')
        out[k] = u[k] * p / (lp + dtype(1e-8))
    return np.clip(out, 0, 1).astype(dtype)


def low_pan(pc):
    """the mean of the four centre pixels of every 4 x 4 block: what a bilinear resize to exactly a quarter computes"""
    return (pc[1::4, 1::4] + pc[1::4, 2::4] + pc[2::4, 1::4] + pc[2::4, 2::4]) * pc.dtype.type(0.25)


def gsa(ms, pan, dtype=np.float64, return_stats=False):
    """the direct form: lstsq on [ms_k - mean, 1], np.cov(ddof=1) / np.var, and the final re-centering line"""
    ms = np.asarray(ms, dtype=dtype)
    pan = np.asarray(pan, dtype=dtype)
    C, h, w = ms.shape
    u = interp23(ms, dtype)
    means = u.mean(axis=(1, 2), dtype=dtype)
    lr = u - means[:, None, None]
    lr_lp = ms - ms.mean(axis=(1, 2), dtype=dtype)[:, None, None]
    hr = pan - pan.mean(dtype=dtype)
    hr0 = low_pan(hr)
    A = np.concatenate([lr_lp.reshape(C, -1).T, np.ones((h * w, 1), dtype=dtype)], axis=1)
    alpha = np.linalg.lstsq(A, hr0.reshape(-1, 1), rcond=None)[0][:, 0].astype(dtype)
    I = np.tensordot(alpha[:C], lr, axes=1) + alpha[C]
    I0 = (I - I.mean(dtype=dtype)).astype(dtype)
    g = np.array([np.cov(I0.reshape(-1), lr[k].reshape(-1), ddof=1)[0, 1] / np.var(I0) for k in range(C)], dtype=dtype)
    out = lr + g[:, None, None] * (hr - I0)[None]
    out = out - out.mean(axis=(1, 2), dtype=dtype)[:, None, None] + means[:, None, None]
    out = np.clip(out, 0, 1).astype(dtype)
    return (out, alpha, g) if return_stats else out


def gsa_closed_form(ms, pan):
    """float64: alpha from the C x C normal equations of the centred columns, the gains from the covariance of u"""
    ms = np.asarray(ms, dtype=np.float64)
    pan = np.asarray(pan, dtype=np.float64)
    C, h, w = ms.shape
    u = interp23(ms)
    N = u[0].size
    uc = (u - u.mean(axis=(1, 2))[:, None, None]).reshape(C, -1)
    mc = (ms - ms.mean(axis=(1, 2))[:, None, None]).reshape(C, -1)
    hr = pan - pan.mean()
    p0 = low_pan(hr).reshape(-1)
    a = np.linalg.solve(mc @ mc.T / (h * w), mc @ (p0 - p0.mean()) / (h * w))
    alpha = np.concatenate([a, [p0.mean()]])
    Su = uc @ uc.T / N
    g = N / (N - 1.0) * (Su @ a) / (a @ Su @ a)
    I0 = np.tensordot(a, uc.reshape(u.shape), axes=1)
    return np.clip(u + g[:, None, None] * (hr - I0)[None], 0, 1), alpha, g


def make_scene(C, h, w, seed):
    """(ms [C, h, w], pan [4h, 4w]) float32 in [0.02, 0.98]: per band a sinusoid of its own frequency around 0.35 plus N(0, 0.05) noise at PAN
    resolution, pan = a random convex combination of the bands plus N(0, 0.02), ms = the 4 x 4 block means"""
    rng = np.random.default_rng(seed)
    H, W = 4 * h, 4 * w
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing='ij')
    bands = np.stack([0.35 + 0.15 * np.sin(2 * np.pi * ((k + 1) * yy + (C - k) * xx) + rng.uniform(0, 2 * np.pi)) + rng.normal(0, 0.05, (H, W))
                      for k in range(C)])
    wgt = rng.uniform(0.5, 1.5, C)
    wgt /= wgt.sum()
    pan = np.tensordot(wgt, bands, axes=1) + rng.normal(0, 0.02, (H, W))
    ms = bands.reshape(C, h, 4, w, 4).mean(axis=(2, 4))
    return np.clip(ms, 0.02, 0.98).astype(np.float32), np.clip(pan, 0.02, 0.98).astype(np.float32)


def make_batch(B, C, h, w, seed):
    """B scenes stacked: ms [B, C, h, w], pan [B, 1, 4h, 4w]"""
    pairs = [make_scene(C, h, w, seed * 1000 + b) for b in range(B)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1][None] for p in pairs])
