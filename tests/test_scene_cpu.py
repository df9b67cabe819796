"""CPU: the geometry of tiled scene fusion (lgteun_amd/scene.py), the boundary of its C ABI (lg_scene_gather / lg_scene_blend /
lg_scene_to_u16 of include/lgteun_hip.h: argument validation before any HIP call) and the fp64 restatement of the blend that the GPU tests
(tests/test_gpu_scene.py) compare the kernels with."""
import ctypes
import os
import re

import numpy as np
import pytest

from lgteun_amd import scene as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('lg_scene_gather', 'lg_scene_blend', 'lg_scene_to_u16')


def blend_fp64(tiles, H, W, tile, overlap):
    """the contract of lg_scene_blend in float64: tiles [N,C,th,tw] of the row-major grid -> (scene [C,H,W], cover count [H,W]).
    scene = sum_k w_k v_k / sum_k w_k with the exact window w(y) w(x) of scene.window."""
    tiles = np.asarray(tiles, dtype=np.float64)
    ys, xs = sc.tile_grid(H, W, tile, overlap)
    th, tw = tiles.shape[2:]
    w2 = np.outer(sc.window(th, overlap), sc.window(tw, overlap))
    num = np.zeros((tiles.shape[1], H, W))
    den = np.zeros((H, W))
    cover = np.zeros((H, W), dtype=np.int64)
    k = 0
    for oy in ys:
        for ox in xs:
            num[:, oy:oy + th, ox:ox + tw] += w2 * tiles[k]
            den[oy:oy + th, ox:ox + tw] += w2
            cover[oy:oy + th, ox:ox + tw] += 1
            k += 1
    assert k == tiles.shape[0]
    return num / den, cover


def test_grid_examples():
    axis = lambda L, t, ov: sc.tile_grid(L, L, t, ov)[0]                                  # noqa: E731
    assert axis(56, 32, 8) == [0, 24]
    assert axis(44, 32, 8) == [0, 12]
    assert axis(108, 32, 8) == [0, 24, 48, 72, 76]
    o = axis(1040, 128, 32)
    assert len(o) == 11 and o[-1] == 912 and o[:3] == [0, 96, 192]
    assert sc.tile_grid(56, 108, 32, 8) == ([0, 24], [0, 24, 48, 72, 76])
    assert sc.tile_grid(56, 108, (16, 48), 8) == ([0, 8, 16, 24, 32, 40], [0, 40, 60])
    assert sc.tile_grid(32, 48, 64, 0) == ([0], [0])                                      # the tile is cut down to the scene
    assert sc.tile_grid(64, 32, 32, 0) == ([0, 32], [0])
    cover = [sum(1 for a in axis(108, 32, 8) if a <= p < a + 32) for p in range(108)]
    assert cover[76:80] == [3] * 4 and max(cover) == 3


def test_cover_is_complete_and_at_most_three_per_axis():
    for t in (16, 32, 48, 128):
        for ov in range(0, t // 2 + 1, 4):
            for L in list(range(t, 3 * t + 20, 4)) + [5 * t + 4]:
                o = sc.tile_grid(L, L, t, ov)[0]
                assert o[0] == 0 and o[-1] == L - t and all(a % 4 == 0 for a in o) and o == sorted(set(o)), (L, t, ov, o)
                cover = np.zeros(L, dtype=int)
                for a in o:
                    cover[a:a + t] += 1
                assert cover.min() >= 1 and cover.max() <= 3, (L, t, ov)
                assert len(o) == (1 if L == t else -(-(L - t) // (t - ov)) + 1)
    # through the public function too (both axes, validation included)
    for H, W, tile, ov in ((20, 1040, (16, 128), 8), (400, 400, 128, 32), (4100, 36, (1024, 32), 16)):
        ys, xs = sc.tile_grid(H, W, tile, ov)
        th, tw = sc.effective_tile(H, W, tile)
        assert ys[-1] + th == H and xs[-1] + tw == W


@pytest.mark.parametrize('args,msg', [
    ((54, 64, 32, 8), 'multiples of 4'), ((64, 12, 32, 8), 'at least 16'), ((64, 66, 32, 8), 'multiples of 4'),
    ((64, 64, 24, 4), 'multiple of 16'), ((64, 64, (32, 40), 4), 'multiple of 16'), ((2048, 2048, 1040, 4), 'multiple of 16'),
    ((44, 64, 64, 4), 'crop the scene'),                                                  # scene below the tile: it is the tile, and 44 is off the grid
    ((64, 64, 8, 0), 'multiple of 16'),
    ((64, 64, 32, -4), 'overlap'), ((64, 64, 32, 6), 'overlap'), ((64, 64, 32, 20), 'overlap'), ((64, 64, (16, 32), 12), 'overlap'),
    ((64, 32, 64, 20), 'overlap'),                                                        # half the smaller EFFECTIVE side
])
def test_geometry_errors_say_what_to_change(args, msg):
    with pytest.raises(ValueError, match=msg):
        sc.tile_grid(*args)


def test_shape_errors():
    assert sc.check_shapes((4, 14, 27), (1, 56, 108)) == (4, 56, 108)
    assert sc.check_shapes((1, 8, 14, 27), (1, 1, 56, 108)) == (8, 56, 108)
    for ms, pan in (((4, 14, 27), (56, 108)), ((4, 14, 27), (1, 56, 104)), ((2, 4, 14, 27), (2, 1, 56, 108)), ((14, 27), (1, 56, 108)),
                    ((4, 14, 27), (2, 56, 108))):
        with pytest.raises(ValueError, match=r'\[C,h,w\]'):
            sc.check_shapes(ms, pan)


def test_window_values():
    assert np.array_equal(sc.window(32, 0), np.ones(32))
    w = sc.window(32, 16)                                                                 # overlap = t / 2: a triangle that reaches 16 / 17
    assert np.allclose(w[:16], np.arange(1, 17) / 17.0) and np.allclose(w[16:], w[:16][::-1]) and w.max() < 1
    w = sc.window(32, 8)
    assert np.allclose(w[:8], np.arange(1, 9) / 9.0) and np.all(w[8:24] == 1) and np.allclose(w, w[::-1])
    # two tiles at nominal overlap sum to 1: u in the right ramp of one tile is overlap - 1 - (t - 1 - u) in the left ramp of the next
    for t, ov in ((32, 8), (32, 16), (128, 32), (16, 4)):
        w = sc.window(t, ov)
        assert np.allclose(w[t - ov:] + w[:ov], 1.0, rtol=0, atol=1e-15), (t, ov)
    assert sc.default_overlap(1040, 272, 128) == 32 and sc.default_overlap(32, 400, 128) == 8


def test_fp64_restatement_of_the_blend():
    rng = np.random.default_rng(0)
    H, W, t, ov = 56, 108, 32, 8
    const = np.full((10, 2, t, t), 3.25)
    out, cover = blend_fp64(const, H, W, t, ov)
    assert np.allclose(out, 3.25, rtol=1e-15) and cover.max() == 6 and cover.min() == 1     # a convex combination; 2 x 3 covers at most
    tiles = rng.standard_normal((10, 2, t, t))
    out, cover = blend_fp64(tiles, H, W, t, ov)
    assert np.allclose(out[:, :24, :24], tiles[0][:, :24, :24], rtol=1e-15, atol=0)        # single cover: the tile itself (w v / w)
    assert (cover[:24, :24] == 1).all() and (cover[:, 76:80] >= 3).all()
    y, x = 30, 77                                                                          # rows 0 and 1, columns 2, 3 and 4
    ys, xs = sc.tile_grid(H, W, t, ov)
    wv = sc.window(t, ov)
    num = den = 0.0
    for iy in (0, 1):
        for ix in (2, 3, 4):
            w = wv[y - ys[iy]] * wv[x - xs[ix]]
            num += w * tiles[iy * 5 + ix][1, y - ys[iy], x - xs[ix]]
            den += w
    assert abs(out[1, y, x] - num / den) < 1e-15


# ------------------------------------------------------------------------------------------------
# the C ABI without a device
# ------------------------------------------------------------------------------------------------
def _lib():
    from lgteun_amd import _lib
    return _lib, _lib.lib()


def test_scene_names_are_exported():
    import lgteun_amd
    assert lgteun_amd.fuse_scene is sc.fuse_scene and lgteun_amd.tile_grid is sc.tile_grid
    assert callable(lgteun_amd.Pansharpening.fuse_scene)
    lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    for name in NEW:
        assert name in lib_mod.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr), name
        assert hasattr(ctypes.CDLL(lib_mod.LIB_PATH), name), name
    assert 'k_scene.hip' in open(os.path.join(ROOT, 'Makefile')).read()
    assert lib_mod.LG_ABI_VERSION == L.lg_abi_version() == 2          # additions only
    ids = lib_mod.KERNEL_IDS
    assert ids['scene_gather'] == ids['batch'] + 1 and ids['scene_blend'] == ids['batch'] + 2     # appended after the existing ids
    assert L.lg_kernel_name(ids['scene_gather']) == b'k_scene_gather' and L.lg_kernel_name(ids['scene_blend']) == b'k_scene_blend'
    assert L.lg_kernel_name(ids['batch']) == b'k_batch_assemble' and L.lg_kernel_name(ids['scene_blend'] + 1) == b'?'


def test_argument_validation_without_a_device():
    """every call here is rejected before any HIP call: the pointers are never dereferenced and nothing is launched"""
    _, L = _lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)
    off = lambda n: ctypes.c_void_p((1 << 20) + n)                                        # noqa: E731

    def gather(pan=fake, ms=fake, org=fake, n_tiles=10, first=0, o_pan=fake, o_ms=fake, B=2, C=4, H=56, W=108, th=32, tw=32, dtype=1,
               divisor=2047.5, n_div=1, post=1.0):
        rc = L.lg_scene_gather(pan, ms, org, n_tiles, first, o_pan, o_ms, B, C, H, W, th, tw, dtype, divisor, n_div, post, null)
        return rc, L.lg_last_error().decode()

    for kw, msg in ((dict(pan=null), 'null pointer'), (dict(ms=null), 'null pointer'), (dict(org=null), 'null pointer'),
                    (dict(o_pan=null), 'null pointer'), (dict(o_ms=null), 'null pointer'),
                    (dict(B=0), 'B must be'), (dict(B=70000), 'B must be'), (dict(C=0), 'C must be'), (dict(C=17), 'C must be'),
                    (dict(H=54), 'multiples of 4'), (dict(W=12), 'multiples of 4'), (dict(H=1 << 17), 'multiples of 4'),
                    (dict(th=24), 'multiples of 16'), (dict(tw=40), 'multiples of 16'), (dict(th=0), 'multiples of 16'),
                    (dict(tw=1040, W=2048), 'multiples of 16'), (dict(th=64), 'exceed the scene'),
                    (dict(dtype=3), 'sample type'), (dict(n_div=3), 'divide count'), (dict(divisor=0.0), 'divisor'),
                    (dict(post=float('nan')), 'scale'), (dict(n_tiles=0), 'origin list'), (dict(first=-1), 'origin list'),
                    (dict(first=9), 'origin list'), (dict(pan=off(4)), '16-byte'), (dict(o_ms=off(8)), '16-byte'), (dict(org=off(2)), '4-byte')):
        rc, err = gather(**kw)
        assert rc == -1 and 'scene_gather' in err and msg in err, (kw, rc, err)

    def blend(tiles=fake, scene=fake, first=0, B=2, C=4, H=56, W=108, th=32, tw=32, overlap=8):
        rc = L.lg_scene_blend(tiles, scene, first, B, C, H, W, th, tw, overlap, null)
        return rc, L.lg_last_error().decode()

    for kw, msg in ((dict(tiles=null), 'null pointer'), (dict(scene=null), 'null pointer'), (dict(B=0), 'B must be'), (dict(C=17), 'C must be'),
                    (dict(W=110), 'multiples of 4'), (dict(th=24), 'multiples of 16'), (dict(tw=128), 'exceed the scene'),
                    (dict(overlap=-4), 'overlap'), (dict(overlap=6), 'overlap'), (dict(overlap=20), 'overlap'), (dict(th=16, overlap=12), 'overlap'),
                    (dict(first=9), 'inside the grid'), (dict(first=-1), 'inside the grid'), (dict(B=11), 'inside the grid'),
                    (dict(scene=off(4)), '16-byte')):
        rc, err = blend(**kw)
        assert rc == -1 and 'scene_blend' in err and msg in err, (kw, rc, err)

    def to_u16(src=fake, dst=fake, n=64, scale=2047.5):
        rc = L.lg_scene_to_u16(src, dst, n, scale, null)
        return rc, L.lg_last_error().decode()

    for kw, msg in ((dict(src=null), 'null pointer'), (dict(dst=null), 'null pointer'), (dict(n=0), 'multiple of 4'), (dict(n=6), 'multiple of 4'),
                    (dict(scale=float('inf')), 'scale'), (dict(src=off(8)), 'aligned'), (dict(dst=off(4)), 'aligned')):
        rc, err = to_u16(**kw)
        assert rc == -1 and 'scene_to_u16' in err and msg in err, (kw, rc, err)


def test_fuse_scene_rejects_bad_requests_before_touching_a_device():
    ms, pan = np.zeros((4, 14, 27), np.uint16), np.zeros((1, 56, 108), np.uint16)
    with pytest.raises(ValueError, match='out_dtype'):
        sc.fuse_scene(None, ms, pan, out_dtype='int8')
    with pytest.raises(ValueError, match='bit_depth'):
        sc.fuse_scene(None, ms, pan, out_dtype='uint16')
    with pytest.raises(ValueError, match='bit_depth'):
        sc.fuse_scene(None, ms, pan, norm_input=True)
    with pytest.raises(ValueError, match=r'\[C,h,w\]'):
        sc.fuse_scene(None, ms, pan[0])
    with pytest.raises(ValueError, match='overlap'):
        sc.fuse_scene(None, ms, pan, tile=32, overlap=20)
