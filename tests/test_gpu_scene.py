"""-m gpu: tiled scene fusion (lgteun_amd/scene.py, kernels k_scene_gather / k_scene_blend / k_scene_to_u16): the gather bit for bit
against numpy's float32 arithmetic, the blend against its fp64 restatement (tests/test_scene_cpu.py) and its contract (a) - (d) of
include/lgteun_hip.h, the whole path against the oracle called per tile, and the exactness properties against the plain forward."""
import logging

import numpy as np
import pytest
import torch

from helpers import det_params, rel_l2, state_shapes
from lgteun_amd import scene as sc
from oracle import detweights as dw
from oracle import lgteun_oracle as orc
from test_scene_cpu import blend_fp64

pytestmark = pytest.mark.gpu

T = torch.from_numpy
DIV = 2047.5
POST = float(np.float32(1.0) / np.float32(DIV))


@pytest.fixture(autouse=True)
def canonical_real_bins(monkeypatch):
    """non-power-of-two tile sizes: pin the oracle's convention for the purely-real FFT bins (tests/test_gpu_anysize.py)"""
    monkeypatch.setattr(orc, 'CANONICAL_REAL_BINS', True)


def _api():
    from lgteun_amd import _lib
    from lgteun_amd.engine import _ptr, _stream_ptr
    return _lib, _lib.lib(), _ptr, _stream_ptr


def _scene_samples(kind, C, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == 'uint8':
        return rng.integers(0, 256, (C, H // 4, W // 4)).astype(np.uint8), rng.integers(0, 256, (1, H, W)).astype(np.uint8)
    if kind == 'uint16':
        return rng.integers(0, 65536, (C, H // 4, W // 4)).astype(np.uint16), rng.integers(0, 65536, (1, H, W)).astype(np.uint16)
    return (rng.uniform(0, 2047, (C, H // 4, W // 4)).astype(np.float32), rng.uniform(0, 2047, (1, H, W)).astype(np.float32))


def _scaled32(a, n_div, post):
    """ba_scale in numpy's float32 arithmetic (IEEE division and product are correctly rounded there too)"""
    x = a.astype(np.float32)
    for _ in range(n_div):
        x = x / np.float32(DIV)
    if post != 1.0:
        x = x * np.float32(post)
    assert x.dtype == np.float32
    return x


def _up(a):
    return T(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


# ------------------------------------------------------------------------------------------------
# 1. gather
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile', [32, (16, 48)])
@pytest.mark.parametrize('kind', ['uint8', 'uint16', 'float32'])
def test_gather_is_bitwise_the_scaled_numpy_slices(kind, tile):
    """PAN 56 x 108: the width and the origins 12 (MS 3), 72 and 76 give rows that are not 16-byte aligned; tile 32 at origin 0 takes the
    16-byte path"""
    lib_mod, L, P, S = _api()
    C, H, W, ov = 4, 56, 108, 8
    ms, pan = _scene_samples(kind, C, H, W, seed=7)
    ys, xs = sc.tile_grid(H, W, tile, ov)
    th, tw = sc.effective_tile(H, W, tile)
    org = [(y, x) for y in ys for x in xs] + [(12, 12), (20, 44)]          # the grid, then two more cuts on the 4-pixel grid
    n = len(org)
    d_org = T(np.array(org, dtype=np.int32)).cuda()
    d_ms, d_pan = _up(ms), _up(pan)
    code = {'uint8': lib_mod.LG_DT_U8, 'uint16': lib_mod.LG_DT_U16, 'float32': lib_mod.LG_DT_F32}[kind]
    for n_div in (0, 1, 2):
        for post in (1.0, POST):
            for first, B in ((0, n), (3, n - 3)):
                o_pan = torch.full((B, 1, th, tw), float('nan'), device='cuda')
                o_ms = torch.full((B, C, th // 4, tw // 4), float('nan'), device='cuda')
                lib_mod.check(L.lg_scene_gather(P(d_pan), P(d_ms), P(d_org), n, first, P(o_pan), P(o_ms), B, C, H, W, th, tw, code, DIV, n_div,
                                                post, S()), 'lg_scene_gather')
                g_pan, g_ms = o_pan.cpu().numpy(), o_ms.cpu().numpy()
                for b in range(B):
                    oy, ox = org[first + b]
                    want_pan = _scaled32(pan[:, oy:oy + th, ox:ox + tw], n_div, post)
                    want_ms = _scaled32(ms[:, oy // 4:(oy + th) // 4, ox // 4:(ox + tw) // 4], n_div, post)
                    assert np.array_equal(g_pan[b].view(np.uint32), want_pan.view(np.uint32)), (kind, tile, n_div, post, first, b)
                    assert np.array_equal(g_ms[b].view(np.uint32), want_ms.view(np.uint32)), (kind, tile, n_div, post, first, b)


# ------------------------------------------------------------------------------------------------
# 2. blend alone
# ------------------------------------------------------------------------------------------------
def _blend(tiles, H, W, th, tw, ov, cuts):
    """the scene after blending `tiles` [N,C,th,tw] in launches of the given sizes, into a buffer pre-filled with NaN"""
    lib_mod, L, P, S = _api()
    N, C = tiles.shape[:2]
    assert sum(cuts) == N
    scene = torch.full((C, H, W), float('nan'), device='cuda')
    first = 0
    for B in cuts:
        part = tiles[first:first + B].contiguous()
        lib_mod.check(L.lg_scene_blend(P(part), P(scene), first, B, C, H, W, th, tw, ov, S()), 'lg_scene_blend')
        first += B
    return scene.cpu().numpy()


@pytest.mark.parametrize('tile,ov', [(32, 8), ((16, 48), 8), (32, 16), (32, 0)])
def test_blend_contract_on_random_tiles(tile, ov):
    """no network: (a) against the fp64 restatement, (b) single-cover pixels are copies, (c) the cut into batches does not matter,
    (d) the NaN the scene starts with never shows.  Tile 32, overlap 8 on PAN 56 x 108 is the 2 x 5 grid with triple cover along x.
    The bound 16 * 2^-24 * max|v| is derived, not measured: at most 9 fma terms, the weights' roundings, one division."""
    C, H, W = 3, 56, 108
    ys, xs = sc.tile_grid(H, W, tile, ov)
    th, tw = sc.effective_tile(H, W, tile)
    N = len(ys) * len(xs)
    rng = np.random.default_rng(11)
    tiles_np = rng.standard_normal((N, C, th, tw)).astype(np.float32)
    tiles = T(tiles_np).cuda()
    want, cover = blend_fp64(tiles_np, H, W, tile, ov)
    if (tile, ov) == (32, 8):
        assert N == 10 and cover.max() == 6 and (cover[:, 76:80] % 3 == 0).all()
    whole = _blend(tiles, H, W, th, tw, ov, [N])
    assert np.isfinite(whole).all()                                                        # (d)
    err = float(np.abs(whole.astype(np.float64) - want).max())
    bound = 16 * 2.0 ** -24 * float(np.abs(tiles_np).max())
    print(f'blend tile {tile} overlap {ov}: max error {err:.3e}, bound {bound:.3e}')
    assert err <= bound, (err, bound)                                                      # (a)
    single = cover == 1
    assert single.any()
    k = 0
    for oy in ys:
        for ox in xs:
            m = single[oy:oy + th, ox:ox + tw]
            got = whole[:, oy:oy + th, ox:ox + tw][:, m]
            assert np.array_equal(got.view(np.uint32), tiles_np[k][:, m].view(np.uint32)), k          # (b)
            k += 1
    for cuts in ([1] * N, [3] * (N // 3) + ([N % 3] if N % 3 else []), [N - 1, 1]):
        again = _blend(tiles, H, W, th, tw, ov, cuts)
        assert np.array_equal(again.view(np.uint32), whole.view(np.uint32)), cuts          # (c)


# ------------------------------------------------------------------------------------------------
# 3. end to end against the oracle
# ------------------------------------------------------------------------------------------------
def _oracle_scene(C, K, ms, pan, tile, ov):
    """orc.forward on every tile crop, blended by the fp64 restatement"""
    H, W = pan.shape[1:]
    ys, xs = sc.tile_grid(H, W, tile, ov)
    th, tw = sc.effective_tile(H, W, tile)
    P = det_params(C, K)
    outs = []
    with torch.no_grad():
        for oy in ys:
            for ox in xs:
                m = T(np.ascontiguousarray(ms[None, :, oy // 4:(oy + th) // 4, ox // 4:(ox + tw) // 4]))
                p = T(np.ascontiguousarray(pan[None, :, oy:oy + th, ox:ox + tw]))
                outs.append(orc.forward(P, m, p, K, mode='live')[0].numpy())
    return blend_fp64(np.stack(outs), H, W, tile, ov)[0]


@pytest.mark.parametrize('C,K,H,W,tile,ov', [(4, 2, 56, 44, 32, 8), (8, 1, 48, 32, (32, 16), 4)])
def test_fused_scene_vs_oracle_per_tile(C, K, H, W, tile, ov):
    """gate: rel_l2 < 1e-3, the project's forward gate (the blend is a convex combination and cannot widen it); measured on the MI355X:
    5.5e-7 (C = 4) and 1.3e-6 (C = 8); the value is printed"""
    from gpu_helpers import make_module
    ms, pan, _ = dw.make_inputs(1, C, H // 4, W // 4, seed=300 + H, kind='smooth')
    ms, pan = ms[0], pan[0]
    net = make_module(C, K)
    got = net.fuse_scene(ms, pan, tile=tile, overlap=ov, batch=3).cpu().numpy()
    want = _oracle_scene(C, K, ms, pan, tile, ov)
    assert got.shape == (C, H, W)
    r = rel_l2(got, want)
    print(f'fuse_scene vs oracle C={C} K={K} PAN {H}x{W} tile {tile} overlap {ov}: rel_l2 {r:.3e}')
    assert r < 1e-3, r


# ------------------------------------------------------------------------------------------------
# 4. / 5. exactness against the plain forward
# ------------------------------------------------------------------------------------------------
def _crop_forward(net, ms, pan, oy, ox, th, tw):
    with torch.no_grad():
        return net(ms[None, :, oy // 4:(oy + th) // 4, ox // 4:(ox + tw) // 4].contiguous(), pan[None, :, oy:oy + th, ox:ox + tw].contiguous())[0]


def test_one_tile_and_zero_overlap_are_bitwise_the_plain_forward():
    from gpu_helpers import make_module
    net = make_module(4, 2)
    ms, pan, _ = dw.make_inputs(1, 4, 8, 12, seed=21, kind='smooth')                       # PAN 32 x 48, tile 64 >= scene
    ms, pan = T(ms[0]).cuda(), T(pan[0]).cuda()
    with torch.no_grad():
        want = net(ms[None], pan[None])[0]
    assert torch.equal(net.fuse_scene(ms, pan, tile=64, overlap=0), want)
    assert torch.equal(net.fuse_scene(ms[None], pan[None], tile=64, overlap=16), want)     # a batch axis of 1; the overlap plays no part
    ms, pan, _ = dw.make_inputs(1, 4, 16, 8, seed=22, kind='smooth')                       # PAN 64 x 32, tile 32, overlap 0: two halves
    ms, pan = T(ms[0]).cuda(), T(pan[0]).cuda()
    got = net.fuse_scene(ms, pan, tile=32, overlap=0)
    for oy in (0, 32):
        assert torch.equal(got[:, oy:oy + 32], _crop_forward(net, ms, pan, oy, 0, 32, 32)), oy
    for batch in (1, 2):
        assert torch.equal(net.fuse_scene(ms, pan, tile=32, overlap=0, batch=batch), got)


def test_scene_beyond_one_plan():
    """PAN 1040 x 272: the plain forward refuses it (1024 limit), the tiled path returns; on a corner, an edge and an interior tile the
    pixels no other tile covers are bitwise the plain forward of that crop"""
    from gpu_helpers import make_module
    C, K, H, W, t, ov = 4, 2, 1040, 272, 128, 32
    net = make_module(C, K)
    ms, pan, _ = dw.make_inputs(1, C, H // 4, W // 4, seed=9, kind='smooth')
    ms, pan = T(ms[0]).cuda(), T(pan[0]).cuda()
    with pytest.raises(RuntimeError, match='1024'):
        with torch.no_grad():
            net(ms[None], pan[None])
    got = net.fuse_scene(ms, pan, tile=t, overlap=ov)
    assert got.shape == (C, H, W) and bool(torch.isfinite(got).all())
    ys, xs = sc.tile_grid(H, W, t, ov)
    assert (len(ys), len(xs)) == (11, 3)
    cover = np.zeros((H, W), dtype=int)
    for oy in ys:
        for ox in xs:
            cover[oy:oy + t, ox:ox + t] += 1
    for iy, ix in ((0, 0), (5, 0), (5, 1)):                                                # corner, edge, interior
        oy, ox = ys[iy], xs[ix]
        m = torch.from_numpy(cover[oy:oy + t, ox:ox + t] == 1).cuda()
        assert int(m.sum()) > 0
        crop = _crop_forward(net, ms, pan, oy, ox, t, t)
        assert torch.equal(got[:, oy:oy + t, ox:ox + t][:, m], crop[:, m]), (iy, ix)


# ------------------------------------------------------------------------------------------------
# 6. digital numbers and the runner hook
# ------------------------------------------------------------------------------------------------
def test_uint16_output_and_integer_inputs():
    from gpu_helpers import make_module
    C, H, W = 4, 56, 44
    net = make_module(C, 1)
    ms, pan = _scene_samples('uint16', C, H, W, seed=3)
    ms, pan = ms >> 5, pan >> 5                                                            # 11-bit digital numbers
    x32 = net.fuse_scene(ms, pan, tile=32, overlap=8, bit_depth=11).cpu().numpy()
    u16 = net.fuse_scene(ms, pan, tile=32, overlap=8, bit_depth=11, out_dtype='uint16')
    assert u16.dtype == torch.uint16 and u16.shape == (C, H, W)
    want = np.clip(np.rint(x32 * np.float32(2 ** 11 - .5)), 0, 65535)
    assert want.dtype == np.float32
    assert np.array_equal(u16.cpu().numpy(), want.astype(np.uint16))
    # the same samples as float32 that are already normalised the way the resident loader's fold does it: the same scene, bit for bit
    f_ms, f_pan = _scaled32(ms, 0, POST), _scaled32(pan, 0, POST)
    assert np.array_equal(net.fuse_scene(f_ms, f_pan, tile=32, overlap=8).cpu().numpy().view(np.uint32), x32.view(np.uint32))
    # ... and from device tensors (uint16 as its int16 view), with the dataset's division on top
    a = net.fuse_scene(_up(ms), _up(pan), tile=32, overlap=8, bit_depth=11, norm_input=True)
    b = net.fuse_scene(_scaled32(ms, 1, POST), _scaled32(pan, 1, POST), tile=32, overlap=8)
    assert torch.equal(a, b)
    # the conversion alone, on values that pin rounding and clipping
    lib_mod, L, P, S = _api()
    v = np.array([0.5, 1.5, 2.5, -0.5, -3.0, 65534.5, 65535.5, 1e9, 0.49999997, 7.0, float('nan'), 65535.0], dtype=np.float32)
    src, dst = T(v).cuda(), torch.empty(v.size, dtype=torch.uint16, device='cuda')
    lib_mod.check(L.lg_scene_to_u16(P(src), P(dst), v.size, 1.0, S()), 'lg_scene_to_u16')
    assert dst.cpu().numpy().tolist() == [0, 2, 2, 0, 0, 65534, 65535, 65535, 0, 7, 0, 65535]


def test_runner_hook_is_opt_in(tmp_path):
    import lgteun_amd
    from lgteun_amd.compat import Config
    C, K = 4, 1
    base = dict(ms_chans=C, work_dir=str(tmp_path), datas='GF-2', cuda=True, max_iter=3, bit_depth=11,
                loss_cfg={'rec_loss': dict(type='l1', w=1.)}, model_cfg={'core_module': dict(stage=K)})
    sd = {k: T(v) for k, v in dw.fill_state_dict(state_shapes(C, K), dtype=np.float32).items()}
    ms, pan, _ = dw.make_inputs(2, C, 14, 11, seed=31, kind='smooth')                      # PAN 56 x 44: off the 16-pixel grid
    batch = dict(input_lr=T(ms).cuda(), input_pan=T(pan).cuda(), image_id=['a', 'b'])
    runner = lgteun_amd.build_model('UnlgFormer', Config(dict(base, scene_tile=32, scene_overlap=8)), logging.getLogger('t'), None, None, None)
    core = runner.module_dict['core_module']
    core.load_state_dict(sd)
    core.to('cuda').eval()
    got = runner.get_model_output(batch)
    assert got.shape == (2, C, 56, 44)
    for i in range(2):
        assert torch.equal(got[i], core.fuse_scene(batch['input_lr'][i], batch['input_pan'][i], tile=32, overlap=8)), i
    runner.cfg['scene_overlap'] = None                                                     # the default: a quarter of the tile
    assert torch.equal(runner.get_model_output(batch), got)
    with pytest.raises(RuntimeError, match='plan_create'):                                 # the plain call refuses this size
        with torch.no_grad():
            core(batch['input_lr'], batch['input_pan'])
    plain = lgteun_amd.build_model('UnlgFormer', Config(dict(base)), logging.getLogger('t'), None, None, None)
    core = plain.module_dict['core_module']
    core.load_state_dict(sd)
    core.to('cuda').eval()
    ms, pan, _ = dw.make_inputs(2, C, 8, 8, seed=32, kind='smooth')
    batch = dict(input_lr=T(ms).cuda(), input_pan=T(pan).cuda(), image_id=['a', 'b'])
    with torch.no_grad():
        assert torch.equal(plain.get_model_output(batch), core(batch['input_lr'], batch['input_pan']))


# ------------------------------------------------------------------------------------------------
# 7. a bad argument through the ABI
# ------------------------------------------------------------------------------------------------
def test_bad_tile_is_rejected_and_nothing_is_launched():
    lib_mod, L, P, S = _api()
    C, H, W = 4, 56, 108
    pan, ms = torch.zeros(1, H, W, device='cuda'), torch.zeros(C, H // 4, W // 4, device='cuda')
    org = torch.zeros(2, dtype=torch.int32, device='cuda')
    o_pan, o_ms = torch.full((1, 1, 24, 32), 5.0, device='cuda'), torch.full((1, C, 6, 8), 5.0, device='cuda')
    rc = L.lg_scene_gather(P(pan), P(ms), P(org), 1, 0, P(o_pan), P(o_ms), 1, C, H, W, 24, 32, lib_mod.LG_DT_F32, 1.0, 0, 1.0, S())
    assert rc == -1 and b'multiples of 16' in L.lg_last_error()
    scene, tiles = torch.full((C, H, W), 5.0, device='cuda'), torch.zeros(1, C, 24, 32, device='cuda')
    rc = L.lg_scene_blend(P(tiles), P(scene), 0, 1, C, H, W, 24, 32, 8, S())
    assert rc == -1 and b'multiples of 16' in L.lg_last_error()
    torch.cuda.synchronize()
    assert bool((o_pan == 5).all()) and bool((o_ms == 5).all()) and bool((scene == 5).all())
    with pytest.raises(lib_mod.LgteunHipError, match='scene_gather'):
        lib_mod.check(L.lg_scene_gather(P(pan), P(ms), P(org), 1, 0, P(o_pan), P(o_ms), 1, C, H, W, 24, 32, lib_mod.LG_DT_F32, 1.0, 0, 1.0, S()),
                      'lg_scene_gather')
