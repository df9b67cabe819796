"""-m gpu: the size limits include/lgteun_hip.h states for the satellite entries, exercised: tensors past 2^31 elements ("all indexing is
64-bit"), B = 65535 (also the hardware limit of gridDim.y / gridDim.z, where the launchers put B), and the per-sample maxima h = w = 4096.
lgteun_forward / lgteun_backward (tests/test_gpu_benchsize.py, test_gpu_fullsize.py), lg_l1_loss / lg_l2_loss / lg_optim_step* above 2^31
elements, the alignment of tensors whose entry states none, and non-default streams are out of scope.

How a wrong index would show.  No mis-indexed build is ever run here: a wrapped index reads or writes out of bounds.  The tests see one because
  - no two samples, items or regions of a large case hold the same bits (random integers drawn on the device; classical batches are a pool of 16
    host-made samples times 8200 or 65535 DISTINCT fp32 gains), and every probed unit is asserted to differ from the units whose offset differs
    from its own by 2^31 or 2^32 elements in any tensor of the call -- where a 32-bit product would land;
  - the probes are the first unit, the two units on either side of element offset 2^31 of the largest tensor, and the last unit;
  - a probe is compared bit for bit with the same unit run alone (the header promises those bits do not depend on the batch or the other planes)
    and with the fp64 / numpy restatement at the gate of that entry's own test file -- no tolerance is new here: classical outputs 8 x the error of
    the float32 run of the restatement, floor 2^-23, stats 1e-9, BDSD weights 8 x the distance of the two host routes (test_gpu_classical /
    _wavelet / _mtf_glp / _bdsd); FIR one ulp (test_gpu_wald); gather, window, store and blend copies bit for bit, blended pixels 16 x 2^-24 max|v|
    (test_gpu_scene, test_gpu_resident); indices 1e-9 and SAM 5e-8 (test_gpu_metrics, _ext); QNR 1e-11 and one rounding (test_gpu_qnr_loss); SAM /
    SSIM loss dout_ratio <= 1 and 1e-6 (test_gpu_recloss).
Every test allocates at most 16 GiB (asserted from torch's peak counter), frees everything before it returns and skips only when the device shows
less free memory than it needs plus 2 GiB, with the figures in the reason.

Every case prints its sizes, peak memory and seconds as `[limits] ...` lines.
Measured on an MI355X (288 GiB; the whole file 11.5 s, 36 passed, NONE skipped; seconds are pytest's per-test call time, input making and host
restatements included; peak = torch.cuda.max_memory_allocated over the case):
  case                                           largest tensors                                              peak GiB   s
  scene_to_u16, n = 2^31 + 2^22                  src 8.02 GiB fp32, dst 4.01 GiB u16                           14.27    1.17
  scene_blend, scene 4 x 23172^2                 scene 8.00 GiB fp32, 576 tiles of 4 x 1024^2 (<= 65 at once)  11.50    0.85
  scene_gather, PAN 46344^2                      pan 4.00 GiB u16, ms 4 x 11586^2 u16 1.00 GiB                  5.50    0.02
  fir_decimate4, 4 x 23172^2                     in 4.00 GiB u16, out 4 x 5793^2 fp32 0.50 GiB                  5.38    0.04
  window_assemble (a) PAN 46344^2, no mul        pan 4.00 GiB, lr 4 x 11586^2 1.00 GiB                          5.50    0.78
  window_assemble (b) 23172^2 with mul           mul 4.00 GiB, pan 1.00 GiB, lr 0.25 GiB                        5.75    0.01
  store N = 131 200 (pyr_down2, batch_assemble)  mul 4.00 GiB, pan 1.00 GiB, lr 0.25 GiB, pan_l 0.13 GiB        5.60    0.01
  classical B = 8200, C = 4, h = w = 64 (x 9)    out 8.01 GiB, pan 2.00 GiB, ms 0.50 GiB, workspace <= 1.47  12.26-12.34  0.10 - 1.02
      (interp23 0.30, sfim 0.92, gsa 0.10, wavelet 0.70, glp 0.18, hpm 0.18, cbd 1.02, bdsd 0.36, bdsd block 32 0.12 s)
  classical B = 65535, C = 2, h = w = 4 (x 8)    out 0.12 GiB                                                   0.42    0.01 - 0.02
  bdsd block 32, B = 65535, C = 2, h = w = 8     out 0.50 GiB                                                   1.66    0.02
  iqa_ref B = 65535, 4 x 16 x 16                 pred, gt 0.25 GiB each                                         0.75    0.07
  iqa_no_ref B = 65535, 4 x 32 x 32              pred 1.00 GiB                                                  3.00    0.05
  iqa_ref_ext + iqa_q2n B = 65535, 4 x 32 x 32   pred, gt 1.00 GiB each                                         3.00    0.01
  qnr_stats + qnr_grad B = 65535, 4 x 8 x 8      out 0.06 GiB                                                   0.21    0.91
  sam_loss 1 x 4 | ssim_loss 11 x 12, B = 65535  out 0.004 | 0.13 GiB                                        0.01 | 0.42  0.15 | 0.86
  batch_assemble | window_assemble | scene_gather | scene_blend at B = 65535 (65280)                          <= 0.38    <= 0.08
  maxima B = 1, C = 2, h = w = 4096 (3 methods)  out 2.00 GiB each, pan 1.00 GiB, two fp64 copies of 2 GiB     10.63    0.08
Probes and what they showed: every probe equals the unit run alone bit for bit.  Classical, B = 8200 and 65535, samples 0 / 8191 / 8192 / 8199 and
0 / 32768 / 65534: error 1.3e-8 - 1.5e-8 (3.0e-8 at the maxima), error / bar 0.001 - 0.097; GSA / MTF-GLP stats 3e-15 - 4e-14 relative, BDSD weights 9e-13 - 7e-11
against gates of 1.0e-9.  FIR crops 0 ulp.  Blend crops (covers 1 - 4) 1.8e-7 - 4.0e-7 against bounds of 3.7e-6 - 4.2e-6; copies, gathers, windows, store items
and lg_scene_to_u16 (all 2 151 677 952 elements) bit for bit.  QNR table 1.8e-15, dout 0.43 - 0.48 of its bound; SAM / SSIM dout 0.003 - 0.019 of the bar,
losses equal to the fp64 module's to 7 digits.  Maxima: lg_mtf_glp's a against float64 on the device 2.9e-11.
Found: no wrong offset, no launch error, no missing validator.  (tests/test_abi_limits_cpu.py found that 256-byte padding made four sizers grow
less than in proportion to B; they now reserve per-sample shares in 128-byte units, and this file ran again on that build.)"""
import functools

import numpy as np
import pytest
import torch

import bdsd_ref as br
import classical_ref as cr
import limits_helpers as lh
import mtf_glp_ref as mr
import qnr_helpers as qh
import recloss_helpers as rh
from limits_helpers import GIB, TWO31, Measured, memory_gate, ptr, same_bits, stream
from lgteun_amd import _lib
from lgteun_amd import device_metrics as dmt
from lgteun_amd import metrics as mtc
from lgteun_amd import scene as sc
from lgteun_amd import wald
from lgteun_amd.dataset import pyr_down
from test_gpu_wald import fir_ref, ulps

pytestmark = pytest.mark.gpu

DIV = 2047.5
POST = float(np.float32(1.0) / np.float32(DIV))
FLOOR = 2.0 ** -23
U = 2.0 ** -23
U16 = _lib.LG_DT_U16
DEV = 'cuda'


def L():
    return _lib.lib()


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """these cases run at sizes nothing ran at before: if the device reports an error behind one of them, the session ends there and nothing
    more is launched on a card that may have faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'the device reports an error behind this test; nothing more is launched: {e}', returncode=3)
    torch.cuda.empty_cache()


def i16(*shape):
    return torch.empty(*shape, dtype=torch.int16, device=DEV)


def f32(*shape):
    return torch.empty(*shape, dtype=torch.float32, device=DEV)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def as_u16_float(t):
    """an int16 device tensor holding uint16 bits -> the sample values as float32 (exact)"""
    return (t.to(torch.int32) & 0xFFFF).to(torch.float32)


# ========================================================================================================================
# 1. lg_scene_to_u16 past 2^31 floats
# ========================================================================================================================
def test_scene_to_u16_past_2_31_elements():
    """n = 2^31 + 2^22 floats in [-0.1, 1.1] with a few NaN, scale 2047.5: the quad index and both offsets cross 2^31 (the destination's byte
    offset crosses 2^32).  EVERY element against torch.round(src * scale).clamp(0, 65535) on the device in chunks of 2^28, and numpy's rint on
    three windows of 2^16: the first, the one straddling element 2^31, the last."""
    n, scale, chunk = TWO31 + (1 << 22), 2047.5, 1 << 28
    memory_gate(6 * n + 3 * 4 * chunk)
    with Measured(f'scene_to_u16 n = {n} (src {4 * n / GIB:.2f} GiB, dst {2 * n / GIB:.2f} GiB)'):
        src = lh.fill_uniform(f32(n), -0.1, 1.1, seed=1)
        nans = torch.tensor([5, (1 << 30) + 1, TWO31 - 3, TWO31, TWO31 + 2, n - 2], device=DEV)
        src[nans] = float('nan')
        assert not torch.equal(src[:1 << 16], src[TWO31:TWO31 + (1 << 16)]) and not torch.equal(src[:1 << 16], src[1 << 30:(1 << 30) + (1 << 16)])
        dst = i16(n)
        dst.fill_(-1)
        _lib.check(L().lg_scene_to_u16(ptr(src), ptr(dst), n, scale, stream()), 'lg_scene_to_u16')
        for o in range(0, n, chunk):
            t = src[o:o + chunk] * np.float32(scale)            # one fp32 product, as the kernel's
            t.round_()                                           # half to even
            torch.nan_to_num_(t, nan=0.0)
            t.clamp_(0, 65535)
            want = t.to(torch.int32)
            del t
            got = dst[o:o + chunk].to(torch.int32)
            got &= 0xFFFF
            assert torch.equal(got, want), (o, int((got != want).sum()))
            del got, want
        for o in (0, TWO31 - (1 << 15), n - (1 << 16)):
            x = src[o:o + (1 << 16)].cpu().numpy()
            want = np.clip(np.nan_to_num(np.rint(x * np.float32(scale)), nan=0.0), 0, 65535).astype(np.uint16)
            assert np.array_equal(lh.u16(dst[o:o + (1 << 16)]), want), o
        assert int(dst[TWO31].item()) == 0 and int(dst[n - 2].item()) == 0          # the NaNs
        del src, dst


# ========================================================================================================================
# 2. lg_scene_blend: a scene of 4 x 23172^2 floats
# ========================================================================================================================
def _blend(tiles, scene, first, C, H, W, t, ov):
    _lib.check(L().lg_scene_blend(ptr(tiles), ptr(scene), first, tiles.shape[0], C, H, W, t, t, ov, stream()), 'lg_scene_blend')


def _tile(k, C, t):
    """tile k of the big blend case: seeded by its index, so that any tile can be made again for a check"""
    g = torch.Generator(device=DEV).manual_seed(7000 + k)
    return torch.randn(C, t, t, generator=g, device=DEV)


def _blend_crop_ref(tile_of, H, W, t, ov, c, y0, y1, x0, x1):
    """the contract (a) in float64 on rows y0 .. y1, columns x0 .. x1 of plane c -> (values, cover count, max |v| of the tiles involved)"""
    ys, xs = sc.tile_grid(H, W, t, ov)
    wv = sc.window(t, ov)
    num, den = np.zeros((y1 - y0, x1 - x0)), np.zeros((y1 - y0, x1 - x0))
    cover = np.zeros((y1 - y0, x1 - x0), dtype=np.int64)
    top = 0.0
    for iy, oy in enumerate(ys):
        for ix, ox in enumerate(xs):
            a0, a1, b0, b1 = max(y0, oy), min(y1, oy + t), max(x0, ox), min(x1, ox + t)
            if a0 >= a1 or b0 >= b1:
                continue
            v = tile_of(iy * len(xs) + ix)[c, a0 - oy:a1 - oy, b0 - ox:b1 - ox].astype(np.float64)
            w2 = np.outer(wv[a0 - oy:a1 - oy], wv[b0 - ox:b1 - ox])
            num[a0 - y0:a1 - y0, b0 - x0:b1 - x0] += w2 * v
            den[a0 - y0:a1 - y0, b0 - x0:b1 - x0] += w2
            cover[a0 - y0:a1 - y0, b0 - x0:b1 - x0] += 1
            top = max(top, float(np.abs(v).max()))
    return num / den, cover, top


def test_scene_blend_scene_past_2_31_elements():
    """C = 4, H = W = 23172 (2.148e9 floats: plane 3 holds element 2^31, at row 23159), tiles 1024^2, overlap 32: 24 x 24 = 576 random tiles,
    blended in launches of 32, then again in launches of 65.  The contract (a) - (d) of test_blend_contract_on_random_tiles on crops of plane 0
    (a four-fold cover), of the rows of plane 3 around element 2^31 (across a two-fold cover), and of plane 3's bottom-right corner, whose last 324 rows and columns
    only tile 575 covers: they hold that tile's bits."""
    C, H, W, t, ov = 4, 23172, 23172, 1024, 32
    ys, xs = sc.tile_grid(H, W, t, ov)
    N = len(ys) * len(xs)
    assert N == 576 and C * H * W > TWO31
    p3, r31, c31 = lh.scene_offset(TWO31, H, W)
    assert (p3, r31) == (3, 23159)
    crops = [(0, 960, 1060, 960, 1060), (3, r31 - 4, r31 + 5, c31 - 200, c31 + 400), (3, H - 372, H, W - 372, W), (1, 11000, 11040, 0, 64)]
    memory_gate(4 * C * H * W + 65 * 4 * C * t * t + 2 * 4 * H * W)
    with Measured(f'scene_blend scene {C} x {H} x {W} ({4 * C * H * W / GIB:.2f} GiB), {N} tiles of {t}^2'):
        scene = f32(C, H, W)
        cache = {}

        def tile_of(k):
            if k not in cache:
                cache[k] = _tile(k, C, t).cpu().numpy()
            return cache[k]
        runs = []
        for cut in (32, 65):
            scene.fill_(float('nan'))
            for first in range(0, N, cut):
                tiles = torch.stack([_tile(k, C, t) for k in range(first, min(first + cut, N))])
                _blend(tiles, scene, first, C, H, W, t, ov)
                del tiles
            for c in range(C):
                assert bool(torch.isfinite(scene[c]).all()), (cut, c)                                   # (d): the NaN never shows
            runs.append([scene[c, y0:y1, x0:x1].cpu().numpy() for c, y0, y1, x0, x1 in crops])
        for (c, y0, y1, x0, x1), got, again in zip(crops, *runs):
            assert same_bits(got, again), ('(c): the cut into launches shows', c, y0, x0)
            want, cover, top = _blend_crop_ref(tile_of, H, W, t, ov, c, y0, y1, x0, x1)
            err, bound = float(np.abs(got.astype(np.float64) - want).max()), 16 * 2.0 ** -24 * top
            print(f'[limits] blend crop plane {c} rows {y0}..{y1} cols {x0}..{x1}: cover {cover.min()}..{cover.max()}, error {err:.3e}, bound {bound:.3e}')
            assert err <= bound, (c, y0, x0, err, bound)                                                # (a)
        assert not np.array_equal(tile_of(0)[0, :8, :8], tile_of(N - 1)[3, -8:, -8:])
        y_free = ys[-2] + t - ys[-1]                         # rows of the last tile that the tile before it still covers
        assert y_free == 700
        got = scene[3, ys[-1] + y_free:, xs[-1] + y_free:].cpu().numpy()
        assert got.shape == (324, 324) and same_bits(got, np.ascontiguousarray(tile_of(N - 1)[3, y_free:, y_free:]))      # (b)
        got0 = scene[0, :960, :960].cpu().numpy()            # tile 1 starts at 992
        assert same_bits(got0, np.ascontiguousarray(tile_of(0)[0, :960, :960]))                                            # (b), first unit
        del scene


# ========================================================================================================================
# 3. lg_scene_gather: a PAN scene of 46344^2 uint16
# ========================================================================================================================
def test_scene_gather_pan_past_2_31_elements():
    """uint16 PAN [1, 46344, 46344] (2.148e9 samples: row 46337 holds element 2^31), MS C = 4 at 11586^2, tile 256; origins at the four corners,
    over the row that holds element 2^31, in the middle, and two out of range (clamped): bitwise the scaled numpy slices, as in
    test_gather_is_bitwise_the_scaled_numpy_slices."""
    C, H, W, t = 4, 46344, 46344, 256
    _, r31, c31 = lh.scene_offset(TWO31, H, W)
    assert r31 == 46337 and H * W > TWO31
    org = [(0, 0), (0, W - t), (H - t, 0), (H - t, W - t), (H - t, (c31 - 128) & ~3), (r31 - 257 & ~3, c31 & ~3), (23000, 23000), (-8, 50000), (70000, -4)]
    clamped = [(min(max(y, 0), H - t) & ~3, min(max(x, 0), W - t) & ~3) for y, x in org]
    B = len(org)
    memory_gate(2 * H * W + 2 * C * (H // 4) * (W // 4) + 4 * (1 << 28))
    with Measured(f'scene_gather PAN {H}^2 uint16 ({2 * H * W / GIB:.2f} GiB), MS {C} x {H // 4}^2'):
        pan = lh.fill_randint16(i16(1, H, W), seed=3)
        ms = lh.fill_randint16(i16(C, H // 4, W // 4), seed=4)
        flat = pan.view(-1)
        assert not torch.equal(flat[:4096], flat[TWO31:TWO31 + 4096]) and not torch.equal(flat[:4096], flat[TWO31 - 4096:TWO31])
        d_org = dev_i32(org)
        o_pan, o_ms = torch.full((B, 1, t, t), float('nan'), device=DEV), torch.full((B, C, t // 4, t // 4), float('nan'), device=DEV)
        _lib.check(L().lg_scene_gather(ptr(pan), ptr(ms), ptr(d_org), B, 0, ptr(o_pan), ptr(o_ms), B, C, H, W, t, t, U16, DIV, 1, POST, stream()),
                   'lg_scene_gather')
        g_pan, g_ms = o_pan.cpu().numpy(), o_ms.cpu().numpy()
        for b, (oy, ox) in enumerate(clamped):
            want_pan = lh.scaled32(lh.u16(pan[:, oy:oy + t, ox:ox + t]), DIV, 1, POST)
            want_ms = lh.scaled32(lh.u16(ms[:, oy // 4:(oy + t) // 4, ox // 4:(ox + t) // 4]), DIV, 1, POST)
            assert same_bits(g_pan[b], want_pan), (b, org[b])
            assert same_bits(g_ms[b], want_ms), (b, org[b])
        one_pan, one_ms = f32(1, 1, t, t), f32(1, C, t // 4, t // 4)                  # the tile over element 2^31 in a call of its own
        _lib.check(L().lg_scene_gather(ptr(pan), ptr(ms), ptr(d_org), B, 4, ptr(one_pan), ptr(one_ms), 1, C, H, W, t, t, U16, DIV, 1, POST, stream()),
                   'lg_scene_gather')
        assert same_bits(one_pan[0], o_pan[4]) and same_bits(one_ms[0], o_ms[4])
        del pan, ms, flat, o_pan, o_ms


# ========================================================================================================================
# 4. lg_fir_decimate4: 4 planes of 23172^2 uint16
# ========================================================================================================================
def _fir(x, taps, phase=2):
    n, H, W = x.shape
    out = f32(n, H // 4, W // 4)
    _lib.check(L().lg_fir_decimate4(ptr(x), ptr(out), ptr(taps), n, H, W, taps.shape[1], phase, U16, 1, stream()), 'lg_fir_decimate4')
    return out


def test_fir_decimate4_planes_past_2_31_elements():
    """uint16, planes = 4, H = W = 23172, 41 taps per plane (four different gains), phase 2, fp32 output: the last plane, which holds element
    2^31, equals that plane run alone (planes = 1) bit for bit; the fp64 restatement of test_gpu_wald (one ulp) on the bottom-right 120 x 120
    outputs of the last plane, border included, and on the top-left 120 x 120 of the first."""
    P, H, W = 4, 23172, 23172
    assert lh.scene_offset(TWO31, H, W)[0] == P - 1
    taps_np = np.stack([wald.mtf_taps(g) for g in (0.3, 0.25, 0.2, 0.35)])
    memory_gate(2 * P * H * W + 4 * (P + 1) * (H // 4) * (W // 4) + 4 * (1 << 28))
    with Measured(f'fir_decimate4 {P} x {H}^2 uint16 ({2 * P * H * W / GIB:.2f} GiB)'):
        x = lh.fill_randint16(i16(P, H, W), seed=5)
        x &= 0x07FF                                                   # 11-bit digital numbers, as test_gpu_wald's raw scenes
        flat = x.view(-1)
        assert not torch.equal(flat[:4096], flat[TWO31:TWO31 + 4096])
        taps = torch.from_numpy(taps_np).to(DEV)
        out = _fir(x, taps)
        assert bool(torch.isfinite(out).all())
        alone = _fir(x[P - 1:], taps[P - 1:].contiguous())
        assert same_bits(alone[0], out[P - 1])
        first = _fir(x[:1], taps[:1].contiguous())
        assert same_bits(first[0], out[0])
        crop = lh.u16(x[P - 1, H - 512:, W - 512:])
        want = fir_ref(crop, taps_np[P - 1], 2)[8:, 8:]               # the crop's own top and left edges are not the plane's: 8 outputs in
        d = ulps(out[P - 1, -120:, -120:].cpu().numpy(), want.astype(np.float32))
        crop0 = lh.u16(x[0, :512, :512])
        d0 = ulps(out[0, :120, :120].cpu().numpy(), fir_ref(crop0, taps_np[0], 2)[:120, :120].astype(np.float32))
        print(f'[limits] fir: last plane bottom-right {d} ulp, first plane top-left {d0} ulp from the fp64 restatement')
        assert d <= 1 and d0 <= 1
        del x, flat, out, alone, first


# ========================================================================================================================
# 5. lg_window_assemble against lg_batch_assemble on big scenes; 6. the store of 131 200 items
# ========================================================================================================================
def _pyr(pan, planes, H, W):
    out = f32(planes, 1, H // 4, W // 4)
    _lib.check(L().lg_pyr_down2(ptr(pan), ptr(out), planes, H, W, U16, stream()), 'lg_pyr_down2')
    return out


def _batch(pan, lr, mul, pan_l, N, idx, B, C, H, W, flips, n_div, post, idx_offset=0):
    o_pan, o_lr, o_pl = (torch.full(s, float('nan'), device=DEV) for s in ((B, 1, H, W), (B, C, H // 4, W // 4), (B, 1, H // 4, W // 4)))
    o_mul = torch.full((B, C, H, W), float('nan'), device=DEV) if mul is not None else None
    _lib.check(L().lg_batch_assemble(ptr(pan), ptr(lr), ptr(mul), ptr(pan_l), N, ptr(idx), idx_offset, ptr(flips), ptr(o_pan), ptr(o_lr), ptr(o_mul),
                                     ptr(o_pl), B, C, H, W, H // 4, W // 4, U16, DIV, n_div, post, stream()), 'lg_batch_assemble')
    return o_pan, o_lr, o_mul, o_pl


def _windows(pan, lr, mul, org, first, B, C, Hs, Ws, P, flips, n_div, post):
    o_pan, o_lr, o_pl = (torch.full(s, float('nan'), device=DEV) for s in ((B, 1, P, P), (B, C, P // 4, P // 4), (B, 1, P // 4, P // 4)))
    o_mul = torch.full((B, C, P, P), float('nan'), device=DEV) if mul is not None else None
    _lib.check(L().lg_window_assemble(ptr(pan), ptr(lr), ptr(mul), ptr(org), org.shape[0], first, ptr(flips), ptr(o_pan), ptr(o_lr), ptr(o_mul), ptr(o_pl),
                                      B, C, Hs, Ws, P, P, U16, DIV, n_div, post, stream()), 'lg_window_assemble')
    return o_pan, o_lr, o_mul, o_pl


def _host_item(pan, lr, mul, flip, n_div, post):
    """what a batch holds for one stored item (numpy uint16 pan [1,H,W], lr [C,h,w], mul [C,H,W] or None): the samples as fp32, flipped, scaled;
    pan_l = pyr_down(pyr_down(pan)) in float64 rounded to fp32 (exact for integers), flipped and scaled the same way"""
    f = (lambda a: a[..., ::-1, :]) if flip & 1 else (lambda a: a)
    g = (lambda a: f(a)[..., ::-1]) if flip & 2 else f
    pl = pyr_down(pyr_down(pan[0].astype(np.float64))).astype(np.float32)[None]
    return [None if a is None else np.ascontiguousarray(lh.scaled32(g(a), DIV, n_div, post)) for a in (pan, lr, mul, pl)]


@pytest.mark.parametrize('with_mul', [False, True], ids=['pan46344', 'mul23172'])
def test_window_assemble_scene_past_2_31_elements(with_mul):
    """(a) PAN 46344^2 uint16 without mul: the PAN row offset crosses 2^31.  (b) a 23172^2 scene with mul [4, 23172, 23172]: mul's plane 3 does.
    64 x 64 windows at the four corners and over the row that holds element 2^31, flip word 3: bitwise what lg_batch_assemble writes for a store
    whose items are those windows (the header's promise), and the flipped, scaled numpy slices with the host pyramid."""
    C, P = 4, 64
    Hs = Ws = 23172 if with_mul else 46344
    big = (C, Hs, Ws) if with_mul else (1, Hs, Ws)
    p31, r31, c31 = lh.scene_offset(TWO31, Hs, Ws)
    assert p31 == big[0] - 1 and Hs - P <= r31 < Hs
    org = [(0, 0), (0, Ws - P), (Hs - P, 0), (Hs - P, Ws - P), (Hs - P, (c31 - 32) & ~3), (Hs - P, (c31 + 32) & ~3), ((r31 - 100) & ~3, c31 & ~3)]
    B = len(org)
    memory_gate(2 * (Hs * Ws * (1 + (C if with_mul else 0)) + C * Hs * Ws // 16) + 4 * (1 << 28))
    with Measured(f'window_assemble scene {Hs}^2 uint16, {"mul " + str(C) + " planes" if with_mul else "no mul"}'):
        pan = lh.fill_randint16(i16(1, Hs, Ws), seed=8)
        lr = lh.fill_randint16(i16(C, Hs // 4, Ws // 4), seed=9)
        mul = lh.fill_randint16(i16(C, Hs, Ws), seed=10) if with_mul else None
        flat = (mul if with_mul else pan).view(-1)
        assert not torch.equal(flat[:4096], flat[TWO31:TWO31 + 4096])
        flips = torch.tensor([3], dtype=torch.int32, device=DEV)
        d_org = dev_i32(org)
        got = _windows(pan, lr, mul, d_org, 0, B, C, Hs, Ws, P, flips, 1, POST)
        # the store whose items are those windows
        cut = lambda a, s: torch.stack([a[:, y // s:(y + P) // s, x // s:(x + P) // s] for y, x in org]).contiguous()       # noqa: E731
        s_pan, s_lr, s_mul = cut(pan, 1), cut(lr, 4), (cut(mul, 1) if with_mul else None)
        s_pl = _pyr(s_pan, B, P, P)
        want = _batch(s_pan, s_lr, s_mul, s_pl, B, torch.arange(B, dtype=torch.int32, device=DEV), B, C, P, P, flips, 1, POST)
        for name, g, w_ in zip(('pan', 'lr', 'mul', 'pan_l'), got, want):
            if g is not None:
                assert same_bits(g, w_), name
        for b in range(B):
            host = _host_item(lh.u16(s_pan[b]), lh.u16(s_lr[b]), lh.u16(s_mul[b]) if with_mul else None, 3, 1, POST)
            for name, g, h_ in zip(('pan', 'lr', 'mul', 'pan_l'), got, host):
                if g is not None:
                    assert same_bits(g[b].cpu().numpy(), h_), (name, b, org[b])
        one = _windows(pan, lr, mul, d_org, 4, 1, C, Hs, Ws, P, flips, 1, POST)                # the window at element 2^31 in a call of its own
        for g, o in zip(got, one):
            if g is not None:
                assert same_bits(g[4], o[0])
        del pan, lr, mul, flat, got, want, one


def test_store_of_131200_items_past_2_31_elements():
    """N = 131 200 items, C = 4, H = W = 64, uint16: mul 2.149e9 samples (item 131 072 starts at element 2^31), pan 5.4e8, pan_l by ONE
    lg_pyr_down2 over N planes (524 800 workgroups).  A batch of 8 -- items 0, 32767, 32768, 131071, 131072, N - 1 and two indices outside
    the store (clamped) -- against the host restatement on the downloaded items; pan_l of items 32768, 131072 and N - 1 equals lg_pyr_down2 of
    that plane alone."""
    N, C, H, W = 131200, 4, 64, 64
    assert N * C * H * W > TWO31 and 131072 * C * H * W == TWO31
    idx = [0, 32767, 32768, 131071, 131072, N - 1, -3, N + 5]
    items = [min(max(i, 0), N - 1) for i in idx]
    memory_gate(2 * N * (C * H * W + H * W + C * H * W // 16) + 4 * N * H * W // 16 + 4 * (1 << 28))
    with Measured(f'store N = {N}: mul {2 * N * C * H * W / GIB:.2f} GiB, pan {2 * N * H * W / GIB:.2f} GiB'):
        mul = lh.fill_randint16(i16(N, C, H, W), seed=11)
        pan = lh.fill_randint16(i16(N, 1, H, W), seed=12)
        lr = lh.fill_randint16(i16(N, C, H // 4, W // 4), seed=13)
        for a, b in ((0, 131072), (127, 131199), (131071, 131072)):
            assert not torch.equal(mul[a], mul[b]) and not torch.equal(pan[a], pan[b])
        pan_l = _pyr(pan, N, H, W)
        assert bool(torch.isfinite(pan_l).all())
        for i in (0, 32768, 131072, N - 1):
            assert same_bits(_pyr(pan[i:i + 1], 1, H, W)[0], pan_l[i]), i
        B = len(idx)
        got = _batch(pan, lr, mul, pan_l, N, dev_i32(idx), B, C, H, W, None, 1, POST)
        for b, i in enumerate(items):
            host = _host_item(lh.u16(pan[i]), lh.u16(lr[i]), lh.u16(mul[i]), 0, 1, POST)
            for name, g, h_ in zip(('pan', 'lr', 'mul', 'pan_l'), got, host):
                assert same_bits(g[b].cpu().numpy(), h_), (name, b, i)
        one = _batch(pan, lr, mul, pan_l, N, dev_i32(idx), 1, C, H, W, None, 1, POST, idx_offset=4)       # item 131072 in a call of its own
        for g, o in zip(got, one):
            assert same_bits(g[4], o[0])
        del mul, pan, lr, pan_l, got, one


# ========================================================================================================================
# 7. the nine classical calls: B = 8200 (out past 2^31 floats) and B = 65535
# ========================================================================================================================
@functools.lru_cache(maxsize=None)
def _pool(C, h, w, smooth):
    """16 host-made samples (a few MB): the only thing the classical cases share"""
    ms, pan = lh.classical_pool(C, h, w, smooth, seed=C * 100 + h)
    ms.setflags(write=False)
    pan.setflags(write=False)
    return ms, pan


def _classical_case(method, B, C, h, w, probes):
    smooth = method.startswith('bdsd')
    pool_ms, pool_pan = _pool(C, h, w, smooth)
    nw = lh.stats_width(method, C, h, w)
    need = 4 * B * (C * h * w + 16 * h * w + 16 * C * h * w) * (2 if B < 10000 else 3) // 2 + lh.classical_workspace_bytes(method, B, C, h, w) + 8 * B * nw
    memory_gate(need)
    with Measured(f'{method} B = {B}, C = {C}, h = w = {h}: out {4 * B * 16 * C * h * w / GIB:.2f} GiB, workspace '
                  f'{lh.classical_workspace_bytes(method, B, C, h, w) / GIB:.2f} GiB'):
        ms, pan, _ = lh.classical_batch(pool_ms, pool_pan, B, seed=h)
        units = [C * h * w, 16 * h * w, 16 * C * h * w, h * w]          # ms, pan, out, an fp64 workspace plane
        for b in probes:
            for p in lh.alias_partners(b, B, units) + [q for q in probes if q != b]:
                assert not torch.equal(ms[b], ms[p]) and not torch.equal(pan[b], pan[p]), (b, p)
        out, stats = lh.classical_call(method, ms, pan)
        assert lh.all_finite(out)
        if stats is not None:
            assert bool(torch.isfinite(stats).all())
        for b in probes:
            o1, s1 = lh.classical_call(method, ms[b:b + 1].contiguous(), pan[b:b + 1].contiguous())
            assert same_bits(o1[0], out[b]), (method, b, 'differs from the sample fused alone')
            if stats is not None:
                assert same_bits(s1[0], stats[b]), (method, b, 'stats differ from the sample fused alone')
            m, p = ms[b].cpu().numpy(), pan[b, 0].cpu().numpy()
            r64, s64 = lh.classical_restatement(method, m, p, np.float64)
            r32, _ = lh.classical_restatement(method, m, p, np.float32)
            assert r32.dtype == np.float32
            e32 = float(np.abs(r32.astype(np.float64) - r64).max())
            bar = max(8.0 * e32, FLOOR)
            err = float(np.abs(out[b].cpu().numpy().astype(np.float64) - r64).max())
            clip_share = float(((r64 <= 0) | (r64 >= 1)).mean())
            line = f'[limits] {method} B = {B} sample {b}: error {err:.3e}, float32 restatement {e32:.3e}, error / bar {err / bar:.3f}, clip share {clip_share:.4f}'
            assert clip_share <= 0.02, (method, b, clip_share)
            if stats is not None:
                got = stats[b].cpu().numpy()
                if smooth:
                    shape = (-1, C, C + 1)
                    chol = br.weights(m, p, [lh.EQUAL_GAIN] * C, 32 if method == 'bdsd32' else None, route='cholesky').reshape(shape)
                    routes = br.gamma_distance(chol, s64.reshape(shape))
                    dist, gate = br.gamma_distance(got.reshape(shape), s64.reshape(shape)), max(1e-9, 8.0 * routes)
                    line += f'; gamma distance {dist:.3e}, gate {gate:.3e}'
                else:
                    dist, gate = float(np.abs(got / s64 - 1.0).max()), 1e-9
                    line += f'; stats relative {dist:.3e}'
                    if method in ('glp', 'hpm'):
                        assert bool((got[C:] == 1).all())
            print(line)
            assert err <= bar, (method, b, err, bar)
            if stats is not None:
                assert dist <= gate, (method, b, dist, gate)
        del ms, pan, out, stats


@pytest.mark.parametrize('method', lh.CLASSICAL_METHODS)
def test_classical_batch_whose_output_passes_2_31_elements(method):
    """B = 8200, C = 4, h = w = 64: out is 8200 x 262144 = 2.1496e9 floats and sample 8192 starts exactly at element 2^31.  Samples 0, 8191, 8192
    and 8199: bitwise the sample fused alone, the float64 restatement at the method's own gate, their stats rows too."""
    B, C, h, w = 8200, 4, 64, 64
    probes = lh.probe_units(B, 16 * C * h * w)
    assert probes == [0, 8191, 8192, 8199] and 8192 * 16 * C * h * w == TWO31
    _classical_case(method, B, C, h, w, probes)


@pytest.mark.parametrize('method', lh.CLASSICAL_METHODS)
def test_classical_batch_of_65535(method):
    """B = 65535 at the smallest image the call takes: C = 2, h = w = 4 (block-wise BDSD: h = w = 8, the smallest sides a block of 32 PAN pixels
    divides).  Samples 0, 32768 and 65534."""
    s = 8 if method == 'bdsd32' else 4
    _classical_case(method, 65535, 2, s, s, [0, 32768, 65534])


# ========================================================================================================================
# 8. the evaluation indices and the training losses at B = 65535
# ========================================================================================================================
BIG_B = 65535
PROBES_B = (0, 32768, 65534)


def _image_batch(C, H, W, seed):
    """gt and pred [65535, C, H, W] on the device, every sample its own draw: gt = a smooth ramp times a per-sample gain plus noise, pred = gt + noise"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ramp = torch.linspace(0.3, 0.7, H * W, device=DEV).view(1, 1, H, W)
    gain = torch.linspace(0.6, 1.2, C, device=DEV).view(1, C, 1, 1) * torch.from_numpy(lh.distinct_gains(BIG_B, seed)).to(DEV).view(-1, 1, 1, 1)
    gt = (ramp * gain + 0.05 * torch.randn(BIG_B, C, H, W, generator=g, device=DEV)).clamp_(0.01, 0.99)
    pred = (gt + 0.02 * torch.randn(BIG_B, C, H, W, generator=g, device=DEV)).clamp_(0.0, 1.0)
    return pred.contiguous(), gt.contiguous()


def _host_np(t, scale):
    return (t * scale).permute(0, 2, 3, 1).cpu().numpy()


def _close(got, want, what, sam_col=None):
    for k, (g, w_) in enumerate(zip(got, want)):
        if k == sam_col:
            assert abs(g - w_) <= 5e-8, (what, k, g, w_)                       # test_gpu_metrics.SAM_ABS
        else:
            assert abs(g - w_) <= 1e-9 * max(1.0, abs(w_)), (what, k, g, w_)


def test_iqa_ref_batch_of_65535():
    C, H, W = 4, 16, 16
    memory_gate(6 * 4 * BIG_B * C * H * W + L().lg_iqa_workspace_bytes(BIG_B, C, H, W, 0))
    with Measured(f'iqa_ref B = {BIG_B}, C = {C}, {H} x {W}'):
        pred, gt = _image_batch(C, H, W, seed=21)
        rows = dmt.ref_evaluate_batch(pred, gt, DIV)
        assert bool(torch.isfinite(rows).all())
        for b in PROBES_B:
            assert all(not torch.equal(gt[b], gt[q]) for q in PROBES_B if q != b)
            assert same_bits(dmt.ref_evaluate_batch(pred[b:b + 1].contiguous(), gt[b:b + 1].contiguous(), DIV)[0], rows[b]), b
            _close(rows[b].cpu().numpy(), mtc.ref_evaluate(_host_np(pred[b:b + 1], DIV)[0], _host_np(gt[b:b + 1], DIV)[0]), f'image {b}', sam_col=3)
        del pred, gt, rows


def test_iqa_no_ref_batch_of_65535():
    C, H, W = 4, 32, 32
    memory_gate(8 * 4 * BIG_B * C * H * W + L().lg_iqa_workspace_bytes(BIG_B, C, H, W, 1))
    with Measured(f'iqa_no_ref B = {BIG_B}, C = {C}, {H} x {W} (pred {4 * BIG_B * C * H * W / GIB:.2f} GiB)'):
        pred, _ = _image_batch(C, H, W, seed=22)
        g = torch.Generator(device=DEV).manual_seed(23)
        pan = (pred.mean(dim=1, keepdim=True) + 0.02 * torch.randn(BIG_B, 1, H, W, generator=g, device=DEV)).clamp_(0, 1).contiguous()
        ms = (torch.nn.functional.avg_pool2d(pred, 4) + 0.01 * torch.randn(BIG_B, C, H // 4, W // 4, generator=g, device=DEV)).clamp_(0, 1).contiguous()
        rows = dmt.no_ref_evaluate_batch(pred, pan, ms, DIV)
        assert bool(torch.isfinite(rows).all())
        for b in PROBES_B:
            assert all(not torch.equal(pred[b], pred[q]) for q in PROBES_B if q != b)
            one = dmt.no_ref_evaluate_batch(pred[b:b + 1].contiguous(), pan[b:b + 1].contiguous(), ms[b:b + 1].contiguous(), DIV)
            assert same_bits(one[0], rows[b]), b
            want = mtc.no_ref_evaluate(_host_np(pred[b:b + 1], DIV)[0], _host_np(pan[b:b + 1], DIV)[0], _host_np(ms[b:b + 1], DIV)[0])
            _close(rows[b].cpu().numpy(), want, f'image {b}')
        del pred, pan, ms, rows


def test_iqa_ref_ext_and_q2n_batch_of_65535():
    C, H, W = 4, 32, 32
    memory_gate(6 * 4 * BIG_B * C * H * W + L().lg_iqa_ext_workspace_bytes(BIG_B, C, H, W))
    with Measured(f'iqa_ref_ext / iqa_q2n B = {BIG_B}, C = {C}, {H} x {W}'):
        pred, gt = _image_batch(C, H, W, seed=24)
        ext = dmt._call_ext(L().lg_iqa_ref_ext, 'lg_iqa_ref_ext', pred, gt, 3, DIV)
        q = dmt._call_ext(L().lg_iqa_q2n, 'lg_iqa_q2n', gt, pred, 1, DIV)
        assert bool(torch.isfinite(ext).all()) and same_bits(q[:, 0], ext[:, 0])
        for b in PROBES_B:
            assert all(not torch.equal(gt[b], gt[q_]) for q_ in PROBES_B if q_ != b)
            p1, g1 = pred[b:b + 1].contiguous(), gt[b:b + 1].contiguous()
            assert same_bits(dmt._call_ext(L().lg_iqa_ref_ext, 'lg_iqa_ref_ext', p1, g1, 3, DIV)[0], ext[b]), b
            assert same_bits(dmt._call_ext(L().lg_iqa_q2n, 'lg_iqa_q2n', g1, p1, 1, DIV)[0], q[b]), b
            hp, hg = _host_np(p1, DIV)[0], _host_np(g1, DIV)[0]
            _close(ext[b].cpu().numpy(), [mtc.q2n(hg, hp), mtc.scc(hg, hp), mtc.cc(hg, hp)], f'image {b}')
        del pred, gt, ext, q


def test_qnr_stats_and_grad_batch_of_65535():
    """C = 4, 8 x 8: q rows of samples 0, 32768, 65534 bitwise those of the sample alone and 1e-11 from the fp64 restatement, like the table over
    all 65535 samples; their dout rows bitwise those of the sample alone under the batch's table, within one rounding of the fp64 gradient."""
    C, H, W = 4, 8, 8
    host = qh.make_inputs(BIG_B, C, H, W, seed=31)
    q_ref, table_ref, dq = qh.stats_ref(*host)
    assert np.abs(table_ref / BIG_B).min() >= qh.MIN_ENTRY, 'the inputs do not meet the entry condition of qnr_helpers: pick another seed'
    Pn = qh.n_pairs(C)[1]
    need = int(L().lg_qnr_workspace_bytes(BIG_B, C, H, W))
    assert need > 0
    memory_gate(need + 4 * 4 * BIG_B * C * H * W)
    with Measured(f'qnr B = {BIG_B}, C = {C}, {H} x {W}'):
        x = tuple(t.to(DEV) for t in host)

        def run(xs, B, table=None):
            nb = int(L().lg_qnr_workspace_bytes(B, C, H, W))
            ws = torch.empty(nb // 8, dtype=torch.float64, device=DEV)
            q, tb = torch.empty(B, 2, Pn, dtype=torch.float64, device=DEV), torch.empty(Pn, dtype=torch.float64, device=DEV)
            _lib.check(L().lg_qnr_stats(*[ptr(t) for t in xs], ptr(q), ptr(tb), B, C, H, W, ptr(ws), nb, stream()), 'lg_qnr_stats')
            dout, loss, ind = f32(B, C, H, W), torch.zeros(1, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV)
            _lib.check(L().lg_qnr_grad(ptr(xs[0]), ptr(xs[1]), ptr(tb if table is None else table), ptr(dout), ptr(loss), ptr(ind), B, BIG_B, C, H, W, 1.0, 0,
                                       ptr(ws), nb, stream()), 'lg_qnr_grad')
            torch.cuda.synchronize()
            return q, tb, dout, float(loss.item()), ind.cpu().numpy()
        q, table, dout, loss, ind = run(x, BIG_B)
        rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))                # noqa: E731
        rt, ri = rel(table.cpu().numpy(), table_ref), rel(ind, np.array(qh.indices_ref(table_ref, BIG_B, C)))
        print(f'[limits] qnr B = {BIG_B}: table rel {rt:.2e}, indices rel {ri:.2e}, loss {loss:.6f}')
        assert rt <= 1e-11 and ri <= 1e-11 and abs(loss - ind[2]) <= U * ind[2]
        for b in PROBES_B:
            assert all(not torch.equal(x[0][b], x[0][p]) for p in PROBES_B if p != b)
            q1, _, d1, _, _ = run(tuple(t[b:b + 1].contiguous() for t in x), 1, table=table)
            assert same_bits(q1[0], q[b]) and same_bits(d1[0], dout[b]), b
            assert rel(q[b].cpu().numpy(), q_ref[b]) <= 1e-11, b
            g = qh.grad_ref(host[0][b:b + 1], host[1][b:b + 1], table_ref, BIG_B, dq[b:b + 1])[0]
            worst = float(np.max(np.abs(dout[b].double().cpu().numpy() - g) / (U * np.abs(g) + 1e-9 * np.abs(g).max())))
            print(f'[limits] qnr sample {b}: worst |dout - g| / bound {worst:.3f}')
            assert worst <= 1.0, (b, worst)
        del x, q, table, dout


@pytest.mark.parametrize('kind,H,W', [('sam', 1, 4), ('ssim', 11, 12)])
def test_sam_and_ssim_loss_batch_of_65535(kind, H, W):
    """the smallest images the calls take: SAM 1 x 4 (W is a multiple of 4), SSIM 11 x 12 (one window row).  dout of samples 0, 32768, 65534 bitwise
    that of the sample alone under B_global = 65535 and within test_gpu_recloss's bar of the fp64 module's gradient; the loss of the whole batch
    within its 1e-6 of the fp64 module's."""
    from lgteun_amd.losses import SAMLoss, SSIMLoss
    C = 4
    memory_gate(8 * 4 * BIG_B * C * H * W + int(L().lg_recloss_workspace_bytes(BIG_B, C, H, W)))
    with Measured(f'{kind}_loss B = {BIG_B}, C = {C}, {H} x {W}'):
        out, gt = _image_batch(C, H, W, seed=40 + H)

        def run(o, g_, B):
            nb = int(L().lg_recloss_workspace_bytes(B, C, H, W))
            ws = torch.empty(nb // 8, dtype=torch.float64, device=DEV)
            dout, loss = torch.full((B, C, H, W), float('nan'), device=DEV), torch.zeros(1, device=DEV)
            if kind == 'sam':
                rc = L().lg_sam_loss(ptr(o), ptr(g_), ptr(dout), ptr(loss), B, BIG_B, C, H, W, 1.0, 0, ptr(ws), nb, stream())
            else:
                rc = L().lg_ssim_loss(ptr(o), ptr(g_), ptr(dout), ptr(loss), B, BIG_B, C, H, W, 1.0, 1.0, 0, ptr(ws), nb, stream())
            _lib.check(rc, kind)
            torch.cuda.synchronize()
            return dout, float(loss.item())
        dout, loss = run(out, gt, BIG_B)
        assert not bool(torch.isnan(dout).any())
        module = SAMLoss() if kind == 'sam' else SSIMLoss(data_range=1.0)
        want = float(module(out.cpu().double(), gt.cpu().double()))
        print(f'[limits] {kind} B = {BIG_B}: loss {loss:.7f}, fp64 module {want:.7f}')
        assert abs(loss - want) <= 1e-6                                          # test_gpu_recloss.VALUE_TOL
        for b in PROBES_B:
            assert all(not torch.equal(out[b], out[p]) for p in PROBES_B if p != b)
            o1, g1 = out[b:b + 1].contiguous(), gt[b:b + 1].contiguous()
            d1, _ = run(o1, g1, 1)
            assert same_bits(d1[0], dout[b]), b
            ratio = rh.dout_ratio(dout[b:b + 1], rh.references(kind, o1.cpu(), g1.cpu()), scale=1.0 / BIG_B)
            print(f'[limits] {kind} sample {b}: dout error / bar {ratio:.3f}')
            assert ratio <= 1.0, (b, ratio)
        del out, gt, dout


# ========================================================================================================================
# 9. the gathers and the blend at B = 65535 (65280 for the blend: the tiles of its grid)
# ========================================================================================================================
def test_batch_assemble_batch_of_65535():
    """H = W = 8, C = 4, a store of 4099 items, 65535 random indices, raw digital numbers (no scaling): EVERY output element against torch's
    gather of the store on the device; rows 0, 32768, 65534 bitwise the one-item call."""
    N, C, H, W, B = 4099, 4, 8, 8, BIG_B
    with Measured(f'batch_assemble B = {B}, {H} x {W}'):
        pan, lr, mul = (lh.fill_randint16(i16(*s), seed=50 + k) for k, s in enumerate(((N, 1, H, W), (N, C, 2, 2), (N, C, H, W))))
        pan_l = _pyr(pan, N, H, W)
        g = torch.Generator(device=DEV).manual_seed(5)
        idx = torch.randint(0, N, (B,), generator=g, device=DEV, dtype=torch.int32)
        got = _batch(pan, lr, mul, pan_l, N, idx, B, C, H, W, None, 0, 1.0)
        li = idx.long()
        for name, g_, w_ in zip(('pan', 'lr', 'mul', 'pan_l'), got, (as_u16_float(pan[li]), as_u16_float(lr[li]), as_u16_float(mul[li]), pan_l[li])):
            assert same_bits(g_, w_), name
        for b in PROBES_B:
            one = _batch(pan, lr, mul, pan_l, N, idx, 1, C, H, W, None, 0, 1.0, idx_offset=b)
            for g_, o in zip(got, one):
                assert same_bits(g_[b], o[0]), b
            host = _host_item(lh.u16(pan[li[b]]), lh.u16(lr[li[b]]), lh.u16(mul[li[b]]), 0, 0, 1.0)
            for g_, h_ in zip(got, host):
                assert same_bits(g_[b].cpu().numpy(), h_), b


def _window_index(oy, ox, P):
    ar = torch.arange(P, device=DEV)
    return (oy.long().view(-1, 1, 1) + ar.view(1, P, 1)), (ox.long().view(-1, 1, 1) + ar.view(1, 1, P))


def test_window_assemble_batch_of_65535():
    """8 x 8 windows at 65535 random origins of a 512 x 512 scene with mul, raw digital numbers: EVERY element of pan, lr and mul against torch's
    indexing on the device; windows 0, 32768, 65534 (pan_l too) bitwise the one-window call and the host pyramid."""
    C, Hs, Ws, P, B = 4, 512, 512, 8, BIG_B
    with Measured(f'window_assemble B = {B}, windows {P} x {P}'):
        pan, lr, mul = (lh.fill_randint16(i16(*s), seed=60 + k) for k, s in enumerate(((1, Hs, Ws), (C, Hs // 4, Ws // 4), (C, Hs, Ws))))
        g = torch.Generator(device=DEV).manual_seed(6)
        org = torch.randint(0, (Hs - P) // 4 + 1, (B, 2), generator=g, device=DEV, dtype=torch.int32) * 4
        got = _windows(pan, lr, mul, org, 0, B, C, Hs, Ws, P, None, 0, 1.0)
        Y, X = _window_index(org[:, 0], org[:, 1], P)
        y, x_ = _window_index(org[:, 0] // 4, org[:, 1] // 4, P // 4)
        assert same_bits(got[0][:, 0], as_u16_float(pan[0][Y, X])), 'pan'
        assert same_bits(got[1], as_u16_float(lr[:, y, x_]).permute(1, 0, 2, 3).contiguous()), 'lr'
        assert same_bits(got[2], as_u16_float(mul[:, Y, X]).permute(1, 0, 2, 3).contiguous()), 'mul'
        assert bool(torch.isfinite(got[3]).all())
        for b in PROBES_B:
            one = _windows(pan, lr, mul, org, b, 1, C, Hs, Ws, P, None, 0, 1.0)
            for g_, o in zip(got, one):
                assert same_bits(g_[b], o[0]), b
            oy, ox = (int(v) for v in org[b].tolist())
            host = _host_item(lh.u16(pan[:, oy:oy + P, ox:ox + P]), lh.u16(lr[:, oy // 4:(oy + P) // 4, ox // 4:(ox + P) // 4]),
                              lh.u16(mul[:, oy:oy + P, ox:ox + P]), 0, 0, 1.0)
            for g_, h_ in zip(got, host):
                assert same_bits(g_[b].cpu().numpy(), h_), b


def test_scene_gather_batch_of_65535():
    """16 x 16 tiles at 65535 random origins of a 1024 x 1024 scene, raw digital numbers: EVERY element against torch's indexing on the device;
    tiles 0, 32768, 65534 bitwise the one-tile call."""
    C, H, W, t, B = 4, 1024, 1024, 16, BIG_B
    with Measured(f'scene_gather B = {B}, tiles {t} x {t}'):
        pan, ms = lh.fill_randint16(i16(1, H, W), seed=70), lh.fill_randint16(i16(C, H // 4, W // 4), seed=71)
        g = torch.Generator(device=DEV).manual_seed(7)
        org = torch.randint(0, (H - t) // 4 + 1, (B, 2), generator=g, device=DEV, dtype=torch.int32) * 4

        def gather(first, n):
            o_pan, o_ms = torch.full((n, 1, t, t), float('nan'), device=DEV), torch.full((n, C, t // 4, t // 4), float('nan'), device=DEV)
            _lib.check(L().lg_scene_gather(ptr(pan), ptr(ms), ptr(org), B, first, ptr(o_pan), ptr(o_ms), n, C, H, W, t, t, U16, DIV, 0, 1.0, stream()),
                       'lg_scene_gather')
            return o_pan, o_ms
        o_pan, o_ms = gather(0, B)
        Y, X = _window_index(org[:, 0], org[:, 1], t)
        y, x_ = _window_index(org[:, 0] // 4, org[:, 1] // 4, t // 4)
        assert same_bits(o_pan[:, 0], as_u16_float(pan[0][Y, X])), 'pan'
        assert same_bits(o_ms, as_u16_float(ms[:, y, x_]).permute(1, 0, 2, 3).contiguous()), 'ms'
        for b in PROBES_B:
            p1, m1 = gather(b, 1)
            assert same_bits(p1[0], o_pan[b]) and same_bits(m1[0], o_ms[b]), b


def test_scene_blend_batch_of_65280():
    """C = 1, scene 4096 x 4080, tile 16, overlap 0: 256 x 255 = 65280 tiles in ONE call (B on gridDim.z), then the same list in two calls.  With no
    overlap every pixel has one cover: the scene holds the tiles' bits, all of them."""
    C, H, W, t = 1, 4096, 4080, 16
    ny, nx = H // t, W // t
    N = ny * nx
    assert N == 65280
    with Measured(f'scene_blend B = {N}, scene {H} x {W}'):
        g = torch.Generator(device=DEV).manual_seed(8)
        tiles = torch.randn(N, C, t, t, generator=g, device=DEV)
        want = tiles.view(ny, nx, t, t).permute(0, 2, 1, 3).reshape(1, H, W).contiguous()
        scene = torch.full((C, H, W), float('nan'), device=DEV)
        _blend(tiles, scene, 0, C, H, W, t, 0)
        assert same_bits(scene, want)
        again = torch.full((C, H, W), float('nan'), device=DEV)
        _blend(tiles[:40000], again, 0, C, H, W, t, 0)
        _blend(tiles[40000:], again, 40000, C, H, W, t, 0)
        assert same_bits(again, want)


# ========================================================================================================================
# 10. the per-sample maxima: B = 1, C = 2, h = w = 4096
# ========================================================================================================================
def _wrap(lo, hi, n):
    return np.arange(lo, hi) % n


def _sfim_apply(u, pan_h, mu, a, m, dtype):
    """classical_ref.sfim's apply step on a crop: u [C, n, n], pan_h [n + 4, n + 4] (two pixels of circular halo), the global moments given"""
    from scipy import ndimage
    out = np.empty_like(u)
    for k in range(u.shape[0]):
        p = ((pan_h.astype(dtype) - dtype(mu)) * dtype(a[k]) + dtype(m[k])).astype(dtype)
        lp = ndimage.uniform_filter(p, size=5, mode='wrap')[2:-2, 2:-2]
        out[k] = u[k] * p[2:-2, 2:-2] / (lp + dtype(1e-8))
    return np.clip(out, 0, 1).astype(dtype)


def test_per_sample_maxima_h_w_4096():
    """B = 1, C = 2, h = w = 4096 (out 2 x 16384^2 floats, 2 GiB; 524 288 output tiles) through lg_interp23_up4, lg_sfim and lg_mtf_glp (GLP).
    The bottom-right 256 x 256 of each band against the restatement evaluated on a crop: interp23 on the MS crop with 16 samples of the
    interpolator's circular support on each side, taken modulo the sides (so the crop includes the wrap); SFIM's and GLP's apply steps on that
    crop with the GLOBAL moments, which are first checked -- lg_mtf_glp's stats a against std(u) / std(pan) in float64 on the device (1e-9, the
    gate of test_gpu_mtf_glp) -- and then taken from torch's float64 means.  GLP's low-pass D is restated on the crop's MS samples in float64 with
    clamped indices."""
    C, h, w, n, pad = 2, 4096, 4096, 64, 16
    H, W = 4 * h, 4 * w
    memory_gate(4 * (C * h * w + H * W + 3 * C * H * W) + 8 * H * W + int(L().lg_mtfglp_workspace_bytes(1, C, h, w, 1, 0)))
    with Measured(f'maxima C = {C}, h = w = {h}: out {4 * C * H * W / GIB:.2f} GiB per method'):
        g = torch.Generator(device=DEV).manual_seed(9)
        pan = torch.rand(1, 1, H, W, generator=g, device=DEV).mul_(0.4).add_(0.3)
        ms = torch.nn.functional.avg_pool2d(pan, 4) * torch.tensor([0.8, 1.0], device=DEV).view(1, C, 1, 1)
        ms = (ms + 0.02 * torch.rand(1, C, h, w, generator=g, device=DEV)).contiguous()
        u_dev, _ = lh.classical_call('interp23', ms, pan)
        # the global moments in float64 on the device
        pd = pan.double()
        mu, s_pan = float(pd.mean()), float(pd.std(unbiased=True))
        del pd
        m, a = [], []
        for k in range(C):
            ud = u_dev[0, k].double()
            m.append(float(ud.mean()))
            a.append(float(ud.std(unbiased=True)) / s_pan)
            del ud
        out_glp, stats = lh.classical_call('glp', ms, pan)
        got_a = stats[0, :C].cpu().numpy()
        rel = float(np.abs(got_a / np.array(a) - 1.0).max())
        print(f'[limits] maxima: stats a {got_a.tolist()}, float64 on the device {a}, relative {rel:.3e}')
        assert rel <= 1e-9 and bool((stats[0, C:] == 1).all())
        out_sfim, _ = lh.classical_call('sfim', ms, pan)
        for t_ in (u_dev, out_glp, out_sfim):
            assert bool(torch.isfinite(t_).all())
        # the crop: MS rows / columns h - n - pad .. h + pad (mod h), PAN rows / columns H - 4 n - 2 .. H + 2 (mod H)
        mi = torch.from_numpy(_wrap(h - n - pad, h + pad, h)).to(DEV)
        ms_c = ms[0][:, mi][:, :, mi].cpu().numpy()
        pi = torch.from_numpy(_wrap(H - 4 * n - 2, H + 2, H)).to(DEV)
        pan_h = pan[0, 0][pi][:, pi].cpu().numpy()
        # GLP's low-pass at the crop's MS samples, float64 on the device from clamped gathers
        taps = mr.taps(lh.EQUAL_GAIN)
        r = len(taps) // 2
        rows = np.clip(4 * _wrap(h - n - pad, h + pad, h)[:, None] + 2 + np.arange(len(taps))[None, :] - r, 0, H - 1).reshape(-1)
        ri = torch.from_numpy(rows).to(DEV)
        patch = pan[0, 0][ri][:, ri].double().view(n + 2 * pad, len(taps), n + 2 * pad, len(taps))
        td = torch.from_numpy(taps).to(DEV)
        D = ((patch * td.view(1, 1, 1, -1)).sum(3) * td.view(1, -1, 1)).sum(1).cpu().numpy()
        del patch
        c0, c1 = 4 * pad, 4 * (pad + n)
        res = {}
        for dtype in (np.float64, np.float32):
            u = cr.interp23(ms_c, dtype)[:, c0:c1, c0:c1]
            p = [((pan_h[2:-2, 2:-2].astype(dtype) - dtype(mu)) * dtype(a[k]) + dtype(m[k])).astype(dtype) for k in range(C)]
            Lk = [cr.interp23(((D.astype(dtype) - dtype(mu)) * dtype(a[k]) + dtype(m[k])).astype(dtype)[None], dtype)[0, c0:c1, c0:c1] for k in range(C)]
            res[dtype] = dict(interp23=u, sfim=_sfim_apply(u, pan_h, mu, a, m, dtype),
                              glp=np.clip(np.stack([u[k] + (p[k] - Lk[k]) for k in range(C)]), 0, 1).astype(dtype))
        for name, dev_out in (('interp23', u_dev), ('sfim', out_sfim), ('glp', out_glp)):
            r64, r32 = res[np.float64][name], res[np.float32][name]
            assert r32.dtype == np.float32
            e32 = float(np.abs(r32.astype(np.float64) - r64).max())
            bar = max(8.0 * e32, FLOOR)
            err = float(np.abs(dev_out[0, :, H - 4 * n:, W - 4 * n:].cpu().numpy().astype(np.float64) - r64).max())
            clip_share = float(((r64 <= 0) | (r64 >= 1)).mean())
            print(f'[limits] maxima {name}: bottom-right {4 * n} x {4 * n} error {err:.3e}, float32 restatement {e32:.3e}, error / bar {err / bar:.3f}, '
                  f'clip share {clip_share:.4f}')
            assert clip_share <= 0.02 and err <= bar, (name, err, bar, clip_share)
        del pan, ms, u_dev, out_glp, out_sfim, stats
