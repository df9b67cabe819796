"""-m gpu: training from a raw scene (lgteun_amd/wald.py; kernels k_fir_decimate4, k_window_assemble, k_window_pyr).

Degradation: against an fp64 restatement in numpy that performs the kernel's operations in the kernel's order (row pass, then column
pass, each `acc = acc + taps[k] * x` from 0.0 in ascending k, every product and sum rounded on its own).  The fp32 output may differ from
the restatement's fp32 rounding by one ulp (the bound allows for double rounding); the integer output must be equal, after the test has
shown that no value of the restatement lies within 1e-9 of a rounding tie.

Window batches: every tensor torch.equal to the ResidentLoader batch over ResidentStore(HostPack(<the same windows cut with numpy>)).
End to end: the exported triplets reproduce the grid loader's batches, and three train_iter steps fed from a SceneDataset configuration
leave the losses and weights of three fed from the exported files."""
import ctypes
import logging

import numpy as np
import pytest
import torch

from helpers import state_shapes
from oracle import detweights as dw

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ('input_lr', 'input_pan', 'target', 'input_pan_l')
BIT_DEPTH = 11
GAINS_MS, GAIN_PAN = (0.3, 0.25, 0.2, 0.35), 0.15
ORIGINS = [(0, 0), (40, 20), (0, 4), (8, 12), (36, 4), (20, 20), (4, 16)]       # a corner, flush to the far border, x = 4 (8 bytes off as uint16)


# ------------------------------------------------------------------------------------------------------------------------
# the fp64 restatement
# ------------------------------------------------------------------------------------------------------------------------
def fir_ref(x, taps, phase):
    """[H, W] -> float64 [H/4, W/4]: separable FIR at (4 i + phase, 4 j + phase), replicate border, the kernel's order of operations"""
    n, r = len(taps), len(taps) // 2
    H, W = x.shape
    xp = np.pad(np.asarray(x, dtype=np.float64), r, mode='edge')
    rows = np.zeros((H + 2 * r, W // 4))
    for k in range(n):
        rows = rows + taps[k] * xp[:, phase + k::4][:, :W // 4]
    out = np.zeros((H // 4, W // 4))
    for k in range(n):
        out = out + taps[k] * rows[phase + k::4][:H // 4]
    return out


def fir_ref_columns_first(x, taps, phase):
    return fir_ref(np.asarray(x).T, taps, phase).T


def to_int(v, dtype):
    return np.clip(np.rint(v), 0, np.iinfo(dtype).max).astype(dtype)


def tie_distance(v):
    return float(np.abs(np.abs(v - np.floor(v)) - 0.5).min())


def fir_gpu(x, taps, phase, out_f32):
    """lg_fir_decimate4 on planes x [n, H, W] (numpy) with taps [n, n_taps] -> numpy [n, H/4, W/4]"""
    from lgteun_amd import _lib
    from lgteun_amd.wald import _as_numpy, _lib_code, _up
    kind = x.dtype.name
    d_x = _up(np.ascontiguousarray(x), DEV)
    d_t = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float64)).to(DEV)
    n, H, W = x.shape
    out = torch.empty(n, H // 4, W // 4, dtype=torch.float32 if out_f32 else d_x.dtype, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                                  # noqa: E731
    _lib.check(_lib.lib().lg_fir_decimate4(P(d_x), P(out), P(d_t), n, H, W, d_t.shape[1], phase, _lib_code(kind), int(out_f32),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'lg_fir_decimate4')
    return out.cpu().numpy() if out_f32 else _as_numpy(out, kind)


def ulps(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def raw_scene(dtype, seed=0, C=4, hs=72, ws=52):
    """raw MS [C,hs,ws] and raw PAN [1,4hs,4ws]: uint16 below 2048, uint8 over its range, float32 non-integers below 2048"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)

    def draw(shape):
        if dt.kind == 'f':
            return (rng.random(shape) * 2048).astype(np.float32)
        return rng.integers(0, 2048 if dt == np.uint16 else 256, size=shape).astype(dt)
    return draw((C, hs, ws)), draw((1, 4 * hs, 4 * ws))


# ------------------------------------------------------------------------------------------------------------------------
# degradation
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,phase', [('uint16', 0), ('uint16', 2), ('uint16', 3), ('uint8', 2), ('float32', 2)])
def test_degradation_against_the_fp64_restatement(dtype, phase):
    """raw PAN 288 x 208 under 41 taps and raw MS [4, 72, 52] -- a 52-wide plane under 41 taps is mostly border -- with one gain per band"""
    from lgteun_amd import wald
    ms, pan = raw_scene(dtype, seed=phase)
    taps_ms = np.stack([wald.mtf_taps(g) for g in GAINS_MS])
    taps_pan = wald.mtf_taps(GAIN_PAN)[np.newaxis]
    want_ms = np.stack([fir_ref(ms[c], taps_ms[c], phase) for c in range(4)])
    want_pan = fir_ref(pan[0], taps_pan[0], phase)[np.newaxis]
    assert want_ms.shape == (4, 18, 13) and want_pan.shape == (1, 72, 52)
    for x, taps, want in ((ms, taps_ms, want_ms), (pan, taps_pan, want_pan)):
        got = fir_gpu(x, taps, phase, True)
        d = ulps(got, want.astype(np.float32))
        print(f'{dtype} phase {phase} {x.shape}: fp32 output {d} ulp from the restatement, {int((got != want.astype(np.float32)).sum())} of {got.size} differ')
        assert got.dtype == np.float32 and d <= 1
    lr, pan_lr = wald.degrade_scene(ms, pan, GAINS_MS, GAIN_PAN, phase=phase, device=DEV)
    assert lr.dtype == ms.dtype and pan_lr.dtype == ms.dtype and lr.shape == (4, 18, 13) and pan_lr.shape == (1, 72, 52)
    if dtype == 'float32':
        assert ulps(lr, want_ms.astype(np.float32)) <= 1 and ulps(pan_lr, want_pan.astype(np.float32)) <= 1
        return
    for got, want, x, taps in ((lr, want_ms, ms, taps_ms), (pan_lr, want_pan, pan, taps_pan)):
        other = np.stack([fir_ref_columns_first(x[c], taps[c], phase) for c in range(len(x))])
        gap = tie_distance(want)
        print(f'{dtype} phase {phase} {x.shape}: closest rounding tie {gap:.2e} away, row-first against column-first {np.abs(want - other).max():.2e}')
        assert gap > 1e-9                                                  # first: the expected integers do not hang on the last bits
        assert np.array_equal(to_int(other, x.dtype), to_int(want, x.dtype))
        assert np.array_equal(got, to_int(want, x.dtype)), int((got != to_int(want, x.dtype)).sum())
    # a store built from the raw pair holds the same arrays, and the raw MS as the target
    store = wald.SceneStore.from_scene(ms, pan, DEV, gains_ms=GAINS_MS, gain_pan=GAIN_PAN, phase=phase)
    assert (store.Hs, store.Ws, store.C) == (72, 52, 4)
    for t, want in ((store.lr, lr), (store.pan, pan_lr), (store.mul, ms)):
        assert np.array_equal(wald._as_numpy(t, dtype), want)


def test_one_tap_is_plain_decimation():
    for dtype in ('uint8', 'uint16', 'float32'):
        ms, _ = raw_scene(dtype, seed=7, C=3)
        for phase in (0, 1, 3):
            got = fir_gpu(ms, np.ones((3, 1)), phase, dtype == 'float32')
            assert got.dtype == ms.dtype and np.array_equal(got, ms[:, phase::4, phase::4]), (dtype, phase)
    got = fir_gpu(ms, np.ones((3, 1)), 2, True)
    assert np.array_equal(got.view(np.int32), ms[:, 2::4, 2::4].view(np.int32))          # bitwise, float32 through fp64 and back


def test_binomial_taps_are_exact():
    """[1 4 6 4 1] / 16 on integers: every product and sum is exact in fp64, whatever the order, so both outputs equal the restatement"""
    taps = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    ties = 0
    for dtype in ('uint8', 'uint16'):
        ms, _ = raw_scene(dtype, seed=8, C=2)
        for phase in (0, 2):
            want = np.stack([fir_ref(ms[c], taps, phase) for c in range(2)])
            assert np.array_equal(want, np.stack([fir_ref_columns_first(ms[c], taps, phase) for c in range(2)]))
            assert np.array_equal(fir_gpu(ms, np.stack([taps, taps]), phase, True), want.astype(np.float32))
            # values ending in .5 are real ties here: half to even, like numpy.rint
            assert np.array_equal(fir_gpu(ms, np.stack([taps, taps]), phase, False), to_int(want, ms.dtype))
            ties += int((np.abs(want - np.floor(want)) == 0.5).sum())
    assert ties > 0


def test_integer_rounding_saturates_and_drops_nan():
    """taps that do not sum to 1 (the filter is separable: a single tap t scales by t * t); integers stay exact in fp64"""
    rng = np.random.default_rng(12)
    for dtype in (np.uint8, np.uint16):
        top = np.iinfo(dtype).max
        v = rng.integers(0, top + 1, size=(1, 8, 12)).astype(dtype)
        dec = v[:, 1::4, 1::4].astype(np.float64)
        assert np.array_equal(fir_gpu(v, np.array([[2.0]]), 1, False), np.minimum(4 * dec, top).astype(dtype)) and (4 * dec > top).any()
        assert np.array_equal(fir_gpu(v, np.array([[np.nan]]), 1, False), np.zeros_like(dec, dtype=dtype))
        taps = np.array([1.0, -2.0, 0.0])                                # x(-1,-1) - 2 x(-1,0) - 2 x(0,-1) + 4 x(0,0): both signs, above the range too
        want = fir_ref(v[0], taps, 1)[np.newaxis]
        assert (want < 0).any() and (want > top).any() and np.array_equal(want, np.rint(want))
        assert np.array_equal(fir_gpu(v, taps[np.newaxis], 1, False), to_int(want, dtype))
        assert np.array_equal(fir_gpu(v, taps[np.newaxis], 1, True), want.astype(np.float32))        # the fp32 output keeps them


def test_support_larger_than_the_plane():
    """16 x 16 under 41 taps: every output's support leaves the plane on both sides"""
    rng = np.random.default_rng(9)
    from lgteun_amd import wald
    x = rng.integers(0, 2048, size=(2, 16, 16)).astype(np.uint16)
    taps = np.stack([wald.mtf_taps(0.3), wald.mtf_taps(0.15)])
    for phase in (0, 3):
        want = np.stack([fir_ref(x[c], taps[c], phase) for c in range(2)])
        assert ulps(fir_gpu(x, taps, phase, True), want.astype(np.float32)) <= 1
        assert tie_distance(want) > 1e-9
        assert np.array_equal(fir_gpu(x, taps, phase, False), to_int(want, np.uint16))
    wide = rng.integers(0, 2048, size=(1, 8, 144)).astype(np.uint16)       # more than one tile across, fewer rows than taps
    want = fir_ref(wide[0], taps[0], 2)[np.newaxis]
    assert ulps(fir_gpu(wide, taps[:1], 2, True), want.astype(np.float32)) <= 1


def test_a_plane_alone_equals_the_plane_inside_a_larger_call():
    from lgteun_amd import wald
    rng = np.random.default_rng(10)
    x = (rng.random((5, 72, 52)) * 2048).astype(np.float32)
    taps = np.stack([wald.mtf_taps(g) for g in (0.3, 0.25, 0.2, 0.35, 0.15)])
    whole = fir_gpu(x, taps, 2, True)
    for c in (0, 3, 4):
        alone = fir_gpu(x[c:c + 1], taps[c:c + 1], 2, True)
        assert np.array_equal(alone.view(np.int32), whole[c:c + 1].view(np.int32)), c
    xi = x.astype(np.uint16)
    assert np.array_equal(fir_gpu(xi[2:3], taps[2:3], 2, False), fir_gpu(xi, taps, 2, False)[2:3])


# ------------------------------------------------------------------------------------------------------------------------
# window batches against the resident path
# ------------------------------------------------------------------------------------------------------------------------
def finished_scene(dtype, C, with_mul, seed=0, Hs=72, Ws=52):
    """a scene as the store holds it (samples over the whole range of the type) -> (pan, lr, mul or None)"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)

    def draw(shape):
        if dt.kind == 'f':
            return (rng.random(shape) * 2048).astype(np.float32)
        return rng.integers(0, np.iinfo(dt).max + 1, size=shape).astype(dt)
    return draw((1, Hs, Ws)), draw((C, Hs // 4, Ws // 4)), (draw((C, Hs, Ws)) if with_mul else None)


def cut(pan, lr, mul, origins, P=32):
    from lgteun_amd import wald
    from lgteun_amd.resident import HostPack
    c = lambda a, s: np.stack([a[:, y // s:(y + P) // s, x // s:(x + P) // s] for y, x in origins])       # noqa: E731
    return HostPack(c(pan, 1), c(lr, 4), None if mul is None else c(mul, 1), [wald.window_id(y, x) for y, x in origins])


def same(got, want, what):
    assert list(got) == list(want) and type(got) is type(want), (what, list(got), list(want))
    assert got['image_id'] == want['image_id'], what
    for k in got:
        if k != 'image_id':
            g, w = got[k].cpu(), want[k].cpu()
            assert g.dtype == torch.float32 and g.shape == w.shape and g.is_contiguous(), (what, k, g.shape, w.shape)
            assert torch.equal(g, w), (what, k, int((g != w).sum()))


@pytest.mark.parametrize('with_mul', [True, False])
@pytest.mark.parametrize('C', [4, 3])
@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'float32'])
def test_window_batches_equal_the_resident_path(dtype, C, with_mul):
    from lgteun_amd import wald
    from lgteun_amd.resident import ResidentLoader, ResidentStore
    pan, lr, mul = finished_scene(dtype, C, with_mul, seed=C)
    scene = wald.SceneStore(pan, lr, mul, DEV)
    items = ResidentStore(cut(pan, lr, mul, ORIGINS), DEV)
    runs = 0
    for word, (ud, lrf) in enumerate([(False, False), (True, False), (False, True)]):
        for norm_input in (False, True):
            for fold in (False, True):
                for bs in (1, 3, 5):                                     # 7 windows: 3 + 3 + 1 and 5 + 2
                    kw = dict(fold_normalize=fold, norm_input=norm_input, bit_depth=BIT_DEPTH, aug_dict=dict(ud_flip=0.5, lr_flip=0.5))
                    a = wald.SceneLoader(scene, 32, bs, origins=ORIGINS, **kw)
                    b = ResidentLoader(items, bs, **kw)
                    for ld in (a, b):
                        ld.aug_draws = lambda epoch, n=len(ld): [dict(ud_flip=ud, lr_flip=lrf)] * n
                    assert a.flip_words(0) == [word] * len(a)
                    got, want = list(a), list(b)
                    assert len(got) == len(want) == -(-7 // bs) and got[-1]['input_pan'].shape[0] == (7 - 1) % bs + 1
                    assert ('target' in got[0]) == with_mul and got[0]['input_pan_l'].shape == (min(bs, 7), 1, 8, 8)
                    for i, (g, w) in enumerate(zip(got, want)):
                        same(g, w, f'{dtype} C={C} flips={word} norm={norm_input} fold={fold} bs={bs} batch {i}')
                    runs += 1
    assert runs == 36


def test_shuffled_grid_epochs_and_a_rectangular_patch():
    """the grid loader with a sampler on top, two epochs, patch 16 x 32 at step 12 inside a region"""
    from lgteun_amd import wald
    from lgteun_amd.resident import ResidentLoader, ResidentStore
    pan, lr, mul = finished_scene('uint16', 4, True, seed=21)
    scene = wald.SceneStore(pan, lr, mul, DEV)
    region = (8, 4, 72, 52)
    org = wald.window_origins(72, 52, (16, 32), 12, region)
    assert len(org) == 5 * 2
    c = lambda a, s: np.stack([a[:, y // s:(y + 16) // s, x // s:(x + 32) // s] for y, x in org])       # noqa: E731
    from lgteun_amd.resident import HostPack
    items = ResidentStore(HostPack(c(pan, 1), c(lr, 4), c(mul, 1), [wald.window_id(y, x) for y, x in org]), DEV)
    kw = dict(shuffle=True, seed=4, bit_depth=BIT_DEPTH, fold_normalize=True, aug_dict=dict(ud_flip=0.5, lr_flip=0.5))
    a = wald.SceneLoader(scene, (16, 32), 4, step=12, region=region, **kw)
    b = ResidentLoader(items, 4, **kw)
    for epoch in (0, 1):
        assert a.epoch == b.epoch == epoch and a.epoch_order() == b.epoch_order()
        got, want = list(a), list(b)                     # complete passes: each loader's epoch counter advances
        assert len(got) == len(want) == 3
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, f'epoch {epoch} batch {i}')
    assert a.epoch_order(0) != a.epoch_order(1)


def test_random_windows_follow_the_epochs_origin_list():
    from lgteun_amd import wald
    from lgteun_amd.resident import ResidentLoader, ResidentStore
    pan, lr, mul = finished_scene('uint16', 4, True, seed=22)
    scene = wald.SceneStore(pan, lr, mul, DEV)
    a = wald.SceneLoader(scene, 32, 4, mode='random', windows_per_epoch=9, seed=6, bit_depth=BIT_DEPTH, norm_input=True)
    for epoch in (0, 1):
        org = wald.random_origins(72, 52, 32, 9, 6, epoch)
        b = ResidentLoader(ResidentStore(cut(pan, lr, mul, [tuple(o) for o in org]), DEV), 4, bit_depth=BIT_DEPTH, norm_input=True)
        got = list(a)
        assert len(got) == 3
        for i, (g, w) in enumerate(zip(got, b)):
            same(g, w, f'random epoch {epoch} batch {i}')


def test_out_of_range_origins_are_clamped_not_read():
    from lgteun_amd import wald
    pan, lr, mul = finished_scene('uint16', 4, True, seed=23)
    scene = wald.SceneStore(pan, lr, mul, DEV)
    wild = [(-8, -4), (100, 100), (41, 22), (6, 9), (-2 ** 31, 2 ** 31 - 1), (40, -1)]
    tame = [(0, 0), (40, 20), (40, 20), (4, 8), (0, 20), (40, 0)]
    got = list(wald.SceneLoader(scene, 32, 6, origins=wild))[0]
    want = list(wald.SceneLoader(scene, 32, 6, origins=tame))[0]
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got['input_pan'][1, 0].cpu(), torch.from_numpy(pan[0, 40:, 20:].astype(np.float32)))


def test_eight_batches_in_flight_keep_their_contents():
    """references to 8 consecutive batches, no synchronisation in between: an output buffer that is recycled would show"""
    from lgteun_amd import wald
    from lgteun_amd.resident import ResidentLoader, ResidentStore
    pan, lr, mul = finished_scene('uint16', 4, True, seed=24)
    scene = wald.SceneStore(pan, lr, mul, DEV)
    org = [tuple(o) for o in wald.window_origins(72, 52, 32, 8)[:16]]
    want = list(ResidentLoader(ResidentStore(cut(pan, lr, mul, org), DEV), 2, bit_depth=BIT_DEPTH, norm_input=True))
    torch.cuda.synchronize()
    it = iter(wald.SceneLoader(scene, 32, 2, origins=org, bit_depth=BIT_DEPTH, norm_input=True))
    held = [next(it) for _ in range(8)]
    torch.cuda.synchronize()
    assert len({b[k].data_ptr() for b in held for k in KEYS}) == 32
    for i, (g, w) in enumerate(zip(held, want)):
        same(g, w, f'held batch {i}')


# ------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------
T = torch.from_numpy


@pytest.fixture(scope='module')
def raw_files(tmp_path_factory):
    """a raw uint16 scene as two TIFFs: MS [72, 52, 4], PAN [288, 208]"""
    from lgteun_amd.dataset import write_tiff
    root = tmp_path_factory.mktemp('wald_scene')
    ms, pan = raw_scene('uint16', seed=31)
    write_tiff(str(root / 'ms.tif'), ms.transpose(1, 2, 0))
    write_tiff(str(root / 'pan.tif'), pan[0], compress=True)
    return str(root / 'ms.tif'), str(root / 'pan.tif'), ms, pan


def scene_cfg(raw_files, batch_size, **extra):
    ds = dict(type='SceneDataset', ms_path=raw_files[0], pan_path=raw_files[1], bit_depth=BIT_DEPTH, patch=32, gains_ms=GAINS_MS, gain_pan=GAIN_PAN)
    ds.update(extra)
    return dict(dataset=ds, batch_size=batch_size)


def test_exported_triplets_reproduce_the_grid_loader(raw_files, tmp_path):
    from lgteun_amd import wald
    from lgteun_amd.dataset import PSDataset, build_loader
    from lgteun_amd.resident import ResidentLoader, ResidentStore
    loader, sampler = build_loader(scene_cfg(raw_files, 4, step=20), device=DEV)
    assert sampler is None and isinstance(loader, wald.SceneLoader) and len(loader.origins) == 6
    want_lr, want_pan = wald.degrade_scene(raw_files[2], raw_files[3], GAINS_MS, GAIN_PAN, device=DEV)
    st = loader.store
    assert np.array_equal(wald._as_numpy(st.lr, 'uint16'), want_lr) and np.array_equal(wald._as_numpy(st.pan, 'uint16'), want_pan)
    ids = wald.export_triplets(st, loader.origins, str(tmp_path / 'set'), 32)
    ds = PSDataset([str(tmp_path / 'set')], BIT_DEPTH)
    assert ds.image_ids == ids and len(ids) == 6
    files = ResidentLoader(ResidentStore.from_dataset(ds, DEV), 4)
    got, want = list(loader), list(files)
    assert len(got) == len(want) == 2 and 'target' in got[0]
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, f'batch {i}')
    assert torch.equal(got[0]['target'][1].cpu(), T(raw_files[2][:, :32, 20:52].astype(np.float32)))       # the raw MS is the target


def _runner(tmp_path, tag, loaders, K=2, **extra):
    import lgteun_amd
    from lgteun_amd.compat import Config
    cfg = Config(dict(ms_chans=4, work_dir=str(tmp_path / tag), datas='GF-2', cuda=True, max_iter=3, bit_depth=BIT_DEPTH,
                      loss_cfg={'rec_loss': dict(type='l2', w=1.)}, optim_cfg={'core_module': dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3)},
                      sched_cfg=dict(step_size=1, gamma=0.85), model_cfg={'core_module': dict(stage=K)}, **extra))
    runner = lgteun_amd.build_model('UnlgFormer', cfg, logging.getLogger('t'), *loaders)
    sd = dw.fill_state_dict(state_shapes(4, K), salt=0)
    runner.module_dict['core_module'].load_state_dict({k: T(v) for k, v in sd.items()})
    runner.set_cuda()
    runner.module_dict['core_module'].eval()
    runner.set_optim()
    runner.optim_dict['core_module'].dropout = False
    runner.set_sched()
    return runner


def _train3(runner):
    losses = []
    runner.print_train_log = lambda it, res, freq=10: losses.append(res['full_loss'])
    for it, batch in runner._train_batches(runner._device()):
        runner.train_iter(it, batch, log_freq=1)
        runner.sched_dict['core_module'].step()
    torch.cuda.synchronize()
    assert len(losses) == 3
    return losses, {k: v.detach().cpu().clone() for k, v in runner.module_dict['core_module'].state_dict().items()}


@pytest.mark.parametrize('fold', [False, True])
def test_three_train_iterations_equal_the_exported_files(raw_files, tmp_path, fold):
    """A K = 2, C = 4 runner at patch 32, two pairs per batch, three steps: fed by a SceneDataset configuration in grid mode, and by the
    exported files through resident=True -- the same losses and the same weights, bit for bit.  The loss is the l2 one: its workgroups meet
    in fp64 before the one rounding to fp32, so the scalar is defined bitwise (the l1 scalar adds fp32 partial sums in arrival order:
    tests/test_gpu_resident.py)."""
    from lgteun_amd import wald
    from lgteun_amd.dataset import build_loader
    scene = build_loader(scene_cfg(raw_files, 2, step=20), device=DEV, fold_normalize=fold)[0]
    wald.export_triplets(scene.store, scene.origins, str(tmp_path / 'set'), 32)
    got_loss, got_sd = _train3(_runner(tmp_path, 'scene', (scene, None, None)))
    files_cfg = dict(dataset=dict(type='PSDataset', image_dirs=[str(tmp_path / 'set')], bit_depth=BIT_DEPTH), batch_size=2, num_workers=0)
    files = build_loader(files_cfg, device=DEV, resident=True, fold_normalize=fold)[0]
    want_loss, want_sd = _train3(_runner(tmp_path, 'files', (files, None, None)))
    print(f'fold={fold}: losses {got_loss} (scene) {want_loss} (files)')
    assert all(np.isfinite(x) and x > 0 for x in got_loss)
    assert got_loss == want_loss
    moved = sum(not torch.equal(want_sd[k], T(v)) for k, v in dw.fill_state_dict(state_shapes(4, 2), salt=0).items())
    assert moved > 0
    for k in want_sd:
        assert torch.equal(got_sd[k], want_sd[k]), k


def test_runner_evaluation_from_a_raw_scene(raw_files, tmp_path):
    """test(ref=False) from a degrade=False scene loader (the raw pair, no target), test(ref=True) from a degraded one"""
    from lgteun_amd.dataset import build_loader
    l0 = build_loader(scene_cfg(raw_files, 4, patch=64, step=64, degrade=False), device=DEV, evaluation=True, fold_normalize=True)[0]
    assert l0.store.mul is None and (l0.store.Hs, l0.store.Ws) == (288, 208) and len(l0.origins) == 4 * 3
    first = next(iter(l0))
    assert 'target' not in first and first['input_pan'].shape == (4, 1, 64, 64) and first['input_lr'].shape == (4, 4, 16, 16)
    l1 = build_loader(scene_cfg(raw_files, 3, step=20), device=DEV, evaluation=True)[0]
    runner = _runner(tmp_path, 'eval', (None, l0, l1))
    b = runner.test(iter_id=1, save=False, ref=False)
    a = runner.test(iter_id=1, save=False, ref=True)
    assert set(b) == {'D_lambda', 'D_s', 'QNR'} and set(a) == {'PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS'}
    assert np.all(np.isfinite(np.asarray(a['PSNR'], dtype=np.float64)))
