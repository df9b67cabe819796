"""Helper, not a test: the seeded inputs of the reference-parity fixtures (tests/golden/parity_*.npz), shared by the generator
(tools/gen_goldens.py --only-parity) and by the tests that read them (tests/test_reference_parity_cpu.py, tests/test_gpu_reference_parity.py).
Images are in digital numbers (11 bit), float32, (H, W, bands) as the runner hands them to the metrics.  A fixture stores an input of up to
256 KB as an array; a larger one as its seed and the sha256 of its float32 bytes, and `load_input` rebuilds it here and checks the hash
before anything is compared with it."""
import hashlib

import numpy as np

MAX_STORED_BYTES = 256 * 1024


def sha256(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


def textured(H, W, C, seed, noise=60.0):
    """a smooth field of a few hundred DN per band plus N(0, noise): every Q window is textured and has a non-zero mean"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (900 + 500 * np.sin(yy / 7.0) * np.cos(xx / 5.0))[..., None] + 80 * np.arange(C)
    return np.clip(base + rng.normal(0, noise, (H, W, C)), 0, 2047).astype(np.float32)


def edge_images():
    """the images of tests/test_gpu_metrics.py::test_reduced_resolution_edge_cases, (48, 48, 4): img; the pair (p, g) with constant regions
    at 1234.567 and at fp32(0.99987 * 2047.5) in both; q = img with the bands 1 .. 3 negated"""
    H = W = 48
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (900 + 500 * np.sin(yy / 7.0) * np.cos(xx / 5.0))[None, None] + 80 * np.arange(4)[None, :, None, None]
    img = np.clip(base + rng.normal(0, 60, (1, 4, H, W)), 0, 2047).astype(np.float32)
    top = np.float32(0.99987 * 2047.5)
    p, g = img.copy(), np.clip(img + rng.normal(0, 30, img.shape), 0, 2047).astype(np.float32)
    for x in (p, g):
        x[..., :20, :24] = np.float32(1234.567)
        x[..., 28:, 30:] = top
    q = img.copy()
    q[:, 1:] *= -1.0
    hwc = lambda a: np.ascontiguousarray(a[0].transpose(1, 2, 0))      # noqa: E731
    return dict(img=hwc(img), p=hwc(p), g=hwc(g), q=hwc(q))


def ref_cases():
    """name -> (pred, gt) of the reference-based metric fixtures"""
    e = edge_images()
    return {
        'sq64_c4': (textured(64, 64, 4, 101), textured(64, 64, 4, 102)),
        'rect48x40_c8': (textured(48, 40, 8, 103), textured(48, 40, 8, 104)),
        'min16_c4': (textured(16, 16, 4, 105), textured(16, 16, 4, 106)),
        'flat48_c4': (e['p'], e['g']),
        'negdot48_c4': (e['q'], e['img']),
        'identical48_c4': (e['img'], e['img'].copy()),
    }


NOREF_CASES = {'c4_128': (4, 128, 201), 'c4_160': (4, 160, 202), 'c8_128': (8, 128, 203)}


def noref_case(C, H, seed):
    """-> pred (H, H, C), pan (H, H), ms (H/4, H/4, C): a scene at PAN resolution, the PAN a convex combination of its bands plus noise, the
    MS image the 4 x 4 block means of a smoothed scene plus noise, the fused image the scene plus an error"""
    rng = np.random.default_rng(seed)
    scene = textured(H, H, C, seed + 1000, noise=90.0).astype(np.float64)
    wgt = rng.uniform(0.5, 1.5, C)
    pan = scene @ (wgt / wgt.sum()) + rng.normal(0, 25, (H, H))
    ms = scene.reshape(H // 4, 4, H // 4, 4, C).mean(axis=(1, 3)) + rng.normal(0, 12, (H // 4, H // 4, C))
    pred = scene + rng.normal(0, 35, scene.shape)
    return tuple(np.clip(a, 0, 2047).astype(np.float32) for a in (pred, pan, ms))


def store_input(out, key, a, seed):
    """the generator's side: the array itself, or (above MAX_STORED_BYTES) its seed and hash"""
    if a.nbytes <= MAX_STORED_BYTES:
        out[key] = a
    else:
        assert seed is not None, f'{key}: {a.nbytes} bytes and no seed to rebuild it from'
        out[key + '__seed'] = np.array(seed)
        out[key + '__sha256'] = np.array(sha256(a))


def load_input(z, key, rebuild):
    """the test's side: `rebuild()` gives the array a fixture stored by seed; its hash is checked here"""
    if key in z.files:
        return z[key]
    a = rebuild()
    assert sha256(a) == str(z[key + '__sha256']), f'{key}: the rebuilt input is not the one the fixture was made from'
    return a
