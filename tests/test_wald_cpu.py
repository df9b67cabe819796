"""CPU: the geometry of training from a raw scene (lgteun_amd/wald.py) -- the MTF taps, the window grid, the random windows of an epoch and
their shares per rank -- and the boundary of its C ABI (lg_fir_decimate4 / lg_window_assemble of include/lgteun_hip.h: argument
validation before any HIP call).  The kernels themselves are tested on the GPU (tests/test_gpu_wald.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lgteun_amd import wald

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('lg_fir_decimate4', 'lg_window_assemble')


def _lib():
    from lgteun_amd import _lib
    return _lib, _lib.lib()


# ------------------------------------------------------------------------------------------------
# taps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gain', [0.3, 0.25, 0.2, 0.35, 0.15])
def test_mtf_taps_have_the_gain_at_the_decimated_nyquist(gain):
    t = wald.mtf_taps(gain)
    assert t.dtype == np.float64 and t.shape == (41,)
    assert np.array_equal(t, t[::-1]) and abs(t.sum() - 1.0) < 1e-15 and (t > 0).all() and t.argmax() == 20
    k = np.arange(41) - 20
    response = float((t * np.cos(2 * np.pi * k / 8.0)).sum())            # at 1 / (2 * 4) cycles per pixel (the taps are even: no sine part)
    assert abs(response - gain) < 1e-12, (gain, response)


def test_mtf_taps_documented_figures():
    t = wald.mtf_taps(0.3)
    sigma = 4 * np.sqrt(-2 * np.log(0.3)) / np.pi
    assert abs(sigma - 1.976) < 5e-4
    assert 1e-24 < t[0] < 1e-22 and t[0] == t[-1]
    assert np.allclose(t, np.exp(-(np.arange(-20, 21) ** 2) / (2 * sigma ** 2)) / np.exp(-(np.arange(-20, 21) ** 2) / (2 * sigma ** 2)).sum(), rtol=1e-15)
    assert wald.mtf_taps(0.3, n_taps=1).tolist() == [1.0]
    assert wald.DEFAULT_GAIN_MS == 0.3 and wald.DEFAULT_GAIN_PAN == 0.15
    assert 'NOT a sensor' in wald.__doc__                                # the defaults are documented as defaults


def test_bad_tap_requests_raise():
    for gain in (0.0, 1.0, -0.2, 1.5):
        with pytest.raises(ValueError, match='gain'):
            wald.mtf_taps(gain)
    for n in (40, 0, 65, 4):
        with pytest.raises(ValueError, match='n_taps'):
            wald.mtf_taps(0.3, n_taps=n)
    for phase in (-1, 4, 1.5):
        with pytest.raises(ValueError, match='phase'):
            wald._check_phase(phase)
    ms, pan = np.zeros((4, 8, 8), np.uint16), np.zeros((1, 32, 32), np.uint16)
    with pytest.raises(ValueError, match='GPU'):                          # before anything else: no quiet host path
        wald.degrade_scene(ms, pan, device='cpu')
    with pytest.raises(ValueError, match='sample type'):
        wald.degrade_scene(ms.astype(np.float64), pan.astype(np.float64), device='cpu')
    with pytest.raises(ValueError, match=r'\[1,4h,4w\]'):
        wald.degrade_scene(ms, pan[:, :28], device='cpu')


# ------------------------------------------------------------------------------------------------
# the window grid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step,ny,nx', [(4, 11, 6), (8, 6, 3), (20, 3, 2)])
def test_window_origins_of_72_by_52(step, ny, nx):
    org = wald.window_origins(72, 52, 32, step)
    assert org.dtype == np.int32 and org.shape == (ny * nx, 2)
    ys, xs = list(range(0, 41, step)), list(range(0, 21, step))
    assert (len(ys), len(xs)) == (ny, nx)
    assert org.tolist() == [[y, x] for y in ys for x in xs]              # row-major
    # flush with the border where the step divides the slack: 72 - 32 = 40 for every step here, 52 - 32 = 20 for 4 and 20; at step 8 the
    # `0, step, ...` that fit end at x = 16 (nothing is added or moved to reach the border)
    assert org[-1].tolist() == [40, 16 if step == 8 else 20]
    assert (org % 4 == 0).all() and (org[:, 0] + 32 <= 72).all() and (org[:, 1] + 32 <= 52).all()
    ids = [wald.window_id(y, x) for y, x in org]
    assert ids == sorted(ids) and len(set(ids)) == len(ids) and not any('_' in i for i in ids)


def test_window_origins_regions_and_rectangles():
    assert wald.window_origins(72, 52, 32, 12).tolist() == [[y, x] for y in (0, 12, 24, 36) for x in (0, 12)]     # the last does not reach 40: not flush
    train = wald.window_origins(72, 52, 32, 4, region=(0, 0, 40, 52))
    test = wald.window_origins(72, 52, 32, 4, region=(40, 0, 72, 52))
    assert train[:, 0].max() + 32 == 40 and test[:, 0].min() == 40 and test[:, 0].max() == 40      # the two parts share no row
    assert len(train) == 3 * 6 and len(test) == 6
    part = wald.window_origins(72, 52, (16, 32), 8, region=(8, 4, 48, 44))
    assert part[0].tolist() == [8, 4] and part[-1].tolist() == [32, 12] and len(part) == 4 * 2
    assert wald.window_origins(32, 32, 32, 4).tolist() == [[0, 0]]


def test_off_grid_values_raise_and_say_what_to_change():
    with pytest.raises(ValueError, match=r'step 6.*multiple of 4.*use 4'):
        wald.window_origins(72, 52, 32, 6)
    with pytest.raises(ValueError, match='step 0'):
        wald.window_origins(72, 52, 32, 0)
    with pytest.raises(ValueError, match=r'region x0 = 2.*4-pixel grid.*use 0 or 4'):
        wald.window_origins(72, 52, 32, 4, region=(0, 2, 72, 52))
    with pytest.raises(ValueError, match='inside the scene'):
        wald.window_origins(72, 52, 32, 4, region=(0, 0, 76, 52))
    with pytest.raises(ValueError, match=r'patch height 30.*multiple of 4'):
        wald.window_origins(72, 52, 30, 4)
    with pytest.raises(ValueError, match=r'patch width 32 exceeds the region width 28.*smaller patch'):
        wald.window_origins(72, 52, 32, 4, region=(0, 0, 72, 28))
    with pytest.raises(ValueError, match=r'scene width 50.*crop'):
        wald.window_origins(72, 50, 32, 4)
    shape = wald.SceneShape(72, 52)
    with pytest.raises(ValueError, match='needs step'):
        wald.SceneLoader(shape, 32, 4)
    with pytest.raises(ValueError, match='windows_per_epoch'):
        wald.SceneLoader(shape, 32, 4, mode='random')
    with pytest.raises(ValueError, match='mode'):
        wald.SceneLoader(shape, 32, 4, step=4, mode='spiral')
    with pytest.raises(ValueError, match='crop-resize'):                  # the ResidentLoader's rule
        wald.SceneLoader(shape, 32, 4, step=4, aug_dict=dict(r4_crop=0.5))
    with pytest.raises(TypeError, match='SceneStore'):                    # order and draws only: no batches without a GPU store
        next(iter(wald.SceneLoader(shape, 32, 4, step=4)))


# ------------------------------------------------------------------------------------------------
# random windows
# ------------------------------------------------------------------------------------------------
def test_random_origins_are_a_function_of_seed_and_epoch():
    region = (8, 4, 72, 48)
    a = wald.random_origins(72, 52, 32, 50, seed=3, epoch=0, region=region)
    assert a.dtype == np.int32 and a.shape == (50, 2)
    assert np.array_equal(a, wald.random_origins(72, 52, 32, 50, seed=3, epoch=0, region=region))
    b = wald.random_origins(72, 52, 32, 50, seed=3, epoch=1, region=region)
    assert not np.array_equal(a, b) and not np.array_equal(a, wald.random_origins(72, 52, 32, 50, seed=4, epoch=0, region=region))
    for org in (a, b):
        assert (org % 4 == 0).all()
        assert (org[:, 0] >= 8).all() and (org[:, 0] + 32 <= 72).all() and (org[:, 1] >= 4).all() and (org[:, 1] + 32 <= 48).all()
    assert set(a[:, 0]) == set(range(8, 41, 4)) and set(a[:, 1]) == set(range(4, 17, 4))       # 50 draws reach every row and column origin
    # the documented generator
    rng = np.random.default_rng([3, 0])
    oy = 8 + 4 * rng.integers(0, 9, size=50)
    assert np.array_equal(a[:, 0], oy)


def test_random_loader_epochs_and_rank_shares():
    shape = wald.SceneShape(72, 52)
    kw = dict(mode='random', windows_per_epoch=21, seed=5, shuffle=True, region=(0, 0, 72, 52))
    whole = wald.SceneLoader(shape, 32, 4, **kw)
    assert len(whole) == 6 and np.array_equal(whole.epoch_origins(0), wald.random_origins(72, 52, 32, 21, 5, 0))
    assert not np.array_equal(whole.epoch_origins(0), whole.epoch_origins(1))
    whole.set_epoch(1)
    assert np.array_equal(whole.epoch_origins(), whole.epoch_origins(1))
    for epoch in (0, 1):
        shares = []
        for r in (0, 1):
            ld = wald.SceneLoader(shape, 32, 4, rank=r, world=2, evaluation=True, **kw)
            assert np.array_equal(ld.epoch_origins(epoch), whole.epoch_origins(epoch))           # every rank draws the same list
            shares.append(ld.epoch_order(epoch))
        assert not set(shares[0]) & set(shares[1]) and sorted(shares[0] + shares[1]) == list(range(21))
        padded = [wald.SceneLoader(shape, 32, 4, rank=r, world=2, **kw).epoch_order(epoch) for r in (0, 1)]
        assert len(padded[0]) == len(padded[1]) == 11 and set(padded[0]) | set(padded[1]) == set(range(21))
        assert len(set(padded[0]) & set(padded[1])) == 1                                          # 21 padded to 22: one wraps around
    grid = wald.SceneLoader(shape, 32, 5, step=4, shuffle=True, seed=2, aug_dict=dict(ud_flip=0.5, lr_flip=0.5))
    assert len(grid.epoch_origins()) == 66 and len(grid) == 14 and sorted(grid.epoch_order(0)) == list(range(66))
    assert grid.epoch_order(0) != grid.epoch_order(1) and len(grid.flip_words(0)) == 14


# ------------------------------------------------------------------------------------------------
# configuration surface and C ABI
# ------------------------------------------------------------------------------------------------
def test_scene_dataset_is_registered():
    import lgteun_amd
    from lgteun_amd.dataset import DATASETS, SceneDataset, build_dataset, build_loader
    assert 'SceneDataset' in DATASETS and lgteun_amd.SceneLoader is wald.SceneLoader and lgteun_amd.mtf_taps is wald.mtf_taps
    cfg = dict(type='SceneDataset', ms_path='ms.tif', pan_path='pan.tif', bit_depth=11, patch=32, step=8, region=(0, 0, 40, 52),
               gains_ms=(0.3, 0.25, 0.2, 0.35), gain_pan=0.15)
    ds = build_dataset(cfg)
    assert isinstance(ds, SceneDataset) and ds.step == 8 and ds.windows_per_epoch is None and ds.degrade and ds.phase == 2
    with pytest.raises(ValueError, match='exactly one of step'):
        build_dataset(dict(cfg, windows_per_epoch=100))
    with pytest.raises(ValueError, match='exactly one of step'):
        build_dataset({k: v for k, v in cfg.items() if k != 'step'})
    with pytest.raises(ValueError, match='needs the device'):
        build_loader(dict(dataset=cfg, batch_size=4))


def test_wald_names_are_exported():
    lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    for name in NEW:
        assert name in lib_mod.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr), name
        assert hasattr(ctypes.CDLL(lib_mod.LIB_PATH), name), name
    assert 'k_wald.hip' in open(os.path.join(ROOT, 'Makefile')).read()
    assert lib_mod.LG_ABI_VERSION == L.lg_abi_version() == 2          # additions only
    assert 'wald' not in ' '.join(lib_mod.KERNEL_IDS) and L.lg_kernel_name(len(lib_mod.KERNEL_IDS)) == b'?'      # no profiler ids for the new kernels


def test_argument_validation_without_a_device():
    """every call here is rejected before any HIP call: the pointers are never dereferenced and nothing is launched"""
    _, L = _lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)
    off = lambda n: ctypes.c_void_p((1 << 20) + n)                                        # noqa: E731

    def fir(src=fake, dst=fake, taps=fake, planes=4, H=72, W=52, n_taps=41, phase=2, dtype=1, out_f32=0):
        rc = L.lg_fir_decimate4(src, dst, taps, planes, H, W, n_taps, phase, dtype, out_f32, null)
        return rc, L.lg_last_error().decode()

    for kw, msg in ((dict(src=null), 'null pointer'), (dict(dst=null), 'null pointer'), (dict(taps=null), 'null pointer'),
                    (dict(dtype=3), 'sample type'), (dict(dtype=-1), 'sample type'), (dict(out_f32=2), 'output flag'),
                    (dict(dtype=2, out_f32=0), 'float32 output'), (dict(H=70), 'multiples of 4'), (dict(W=4), 'multiples of 4'),
                    (dict(H=65540), 'multiples of 4'), (dict(n_taps=40), 'odd'), (dict(n_taps=0), 'odd'), (dict(n_taps=65), 'odd'),
                    (dict(phase=4), 'phase'), (dict(phase=-1), 'phase'), (dict(taps=off(4)), '8-byte'), (dict(src=off(1)), 'aligned to their sample'),
                    (dict(dst=off(2), out_f32=1), 'aligned to their sample'), (dict(planes=0), 'planes'), (dict(planes=1 << 40), 'planes')):
        rc, err = fir(**kw)
        assert rc == -1 and 'fir_decimate4' in err and msg in err, (kw, rc, err)

    def window(pan=fake, lr=fake, mul=fake, org=fake, n=10, first=0, flips=null, o_pan=fake, o_lr=fake, o_mul=fake, o_pl=fake, B=2, C=4,
               Hs=72, Ws=52, P=32, Q=32, dtype=1, divisor=2047.5, n_div=1, post=1.0):
        rc = L.lg_window_assemble(pan, lr, mul, org, n, first, flips, o_pan, o_lr, o_mul, o_pl, B, C, Hs, Ws, P, Q, dtype, divisor, n_div, post, null)
        return rc, L.lg_last_error().decode()

    for kw, msg in ((dict(pan=null), 'null pointer'), (dict(lr=null), 'null pointer'), (dict(org=null), 'null pointer'),
                    (dict(o_pl=null), 'null pointer'), (dict(mul=null), 'go together'), (dict(o_mul=null), 'go together'),
                    (dict(B=0), 'B must be'), (dict(B=70000, n=70000), 'B must be'), (dict(C=0), 'C must be'), (dict(C=17), 'C must be'),
                    (dict(Hs=70), 'scene Hs and Ws'), (dict(Ws=4), 'scene Hs and Ws'), (dict(Hs=1 << 17), 'scene Hs and Ws'),
                    (dict(P=30), 'window sides'), (dict(Q=4), 'window sides'), (dict(P=4100, Hs=8192), 'window sides'),
                    (dict(Q=56), 'exceed the scene'), (dict(dtype=3), 'sample type'), (dict(n_div=3), 'divide count'),
                    (dict(divisor=0.0), 'divisor'), (dict(post=float('inf')), 'scale'), (dict(n=0), 'origin list'), (dict(first=-1), 'origin list'),
                    (dict(first=9), 'origin list'), (dict(pan=off(8)), '16-byte'), (dict(o_lr=off(4)), '16-byte'), (dict(org=off(2)), '4-byte'),
                    (dict(flips=off(1)), '4-byte')):
        rc, err = window(**kw)
        assert rc == -1 and 'window_assemble' in err and msg in err, (kw, rc, err)
