"""-m gpu: the BDSD baseline (lgteun_amd/bdsd.py, the k_bd_* kernels of lgteun_amd/csrc/k_classical.hip) against the float64 numpy restatement in
tests/bdsd_ref.py.

The bar of an output tensor is that of tests/test_gpu_classical.py: its largest absolute difference to the float64 restatement may be at most 8 x the
difference of the float32 run of the same restatement to its float64 run on that case, with a floor of 2^-23.  The weights gamma (`stats`) are compared
with the restatement's lstsq route: the largest absolute difference in a sample over that sample's largest |gamma| may be at most max(1e-9, 8 x the
distance between the restatement's own two routes -- lstsq and normal equations plus Cholesky -- on that case).  The measured figures are in DESIGN.md 3.14.

Which case covers what (16 x 32 output tiles; the low-passes work on 16 x 16 tiles of the MS grid; a Gram workgroup takes 256 MS pixels of a block at a
time, at most 128 workgroups per sample where a block is larger than that):
  (4, 8, 8, 2) global        two full tiles, one chunk of 64 pixels
  (4, 5, 7, 2) global        two ragged tiles, sides off every power-of-two grid, 35 pixels; also with per-band gains (one filter per band)
  (8, 12, 8, 3) global       three tiles, C = 8
  (4, 8, 16, 2) block 32     one row of two blocks
  (2, 8, 8, 1) block 32      C = 2, one block
  (4, 40, 24, 2) block 32    5 x 3 blocks; 3 x 2 tiles of the low-passes, ragged both ways
  (8, 16, 24, 2) block 32    C = 8, 2 x 3 blocks
  (8, 32, 32, 3) block 32/64 C = 8, 4 x 4 blocks and 2 x 2 blocks of one full chunk; block 32 also with per-band gains
  (4, 24, 40, 2) block 32    3 x 5 blocks
  (4, 136, 256, 1) global    136 chunks > 128: eight Gram workgroups walk a second chunk, the solve adds 128 partials
  (4, 136, 256, 1) block 32  34 x 64 blocks; also with per-band gains"""
import functools
import logging

import numpy as np
import pytest
import torch

import bdsd_ref as br
import classical_ref as cr
import mtf_glp_ref as mr
from gpu_helpers import GUARD, assert_guards_intact, guarded_empty
from lgteun_amd import _lib, bdsd, build_model, classical, device_metrics
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
CASES = [c + (False,) for c in br.CASES] + [c + (True,) for c in br.PER_BAND_CASES]      # C, h, w, B, block, per-band gains
SENTINEL = -1.2345e300


def gains_of(C, per_band):
    return mr.per_band_gains(C) if per_band else [br.EQUAL_GAIN] * C


@functools.lru_cache(maxsize=None)
def inputs(C, h, w, B):
    ms, pan = br.make_batch(B, C, h, w, seed=C * 100 + h)
    ms.setflags(write=False)
    pan.setflags(write=False)
    return ms, pan


def restate(ms, pan, gains, block):
    """-> dict(ref float64 [B, C, 4h, 4w], raw (unclipped), e32, bar, gamma [B, nby, nbx, C, C + 1], gate)"""
    B = ms.shape[0]
    r64 = [br.bdsd(ms[b], pan[b, 0], gains, block, return_stats=True, clip=False) for b in range(B)]
    r32 = np.stack([br.bdsd(ms[b], pan[b, 0], gains, block, dtype=np.float32) for b in range(B)])
    assert r32.dtype == np.float32
    raw, gamma = np.stack([r[0] for r in r64]), np.stack([r[1] for r in r64])
    ref = np.clip(raw, 0, 1)
    routes = max(br.gamma_distance(br.weights(ms[b], pan[b, 0], gains, block, route='cholesky'), gamma[b]) for b in range(B))
    e32 = float(np.abs(r32.astype(np.float64) - ref).max())
    res = dict(ref=ref, raw=raw, e32=e32, bar=max(8.0 * e32, FLOOR), gamma=gamma, routes=routes, gate=max(1e-9, 8.0 * routes))
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def case(C, h, w, B, block, per_band):
    """the float64 restatement of a case, its bar and the gate of its weights; computed once, never written to"""
    ms, pan = inputs(C, h, w, B)
    return restate(ms, pan, gains_of(C, per_band), block)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the cached arrays are read-only


def device_taps(gains, n_taps=41):
    return torch.from_numpy(np.stack([mr.taps(g, n_taps) for g in gains])).cuda()


def raw_call(ms, pan, gains, block, F=None, fill=SENTINEL):
    """the C ABI with the output and stats inside NaN guard bands and a caller-owned workspace, itself between guard bands, filled with `fill` (a finite
    sentinel or NaN); twice on the same workspace.  F: the number of MS filters (default: 1 when all gains are equal, else C).  -> (out, gamma)"""
    L = _lib.lib()
    B, C, h, w = ms.shape
    if F is None:
        F = 1 if len(set(gains)) == 1 else C
    taps_ms, taps_pan = device_taps(gains[:F]), device_taps([br.GAIN_PAN])
    blk = block or 0
    nby, nbx = (4 * h // blk, 4 * w // blk) if blk else (1, 1)
    need = int(L.lg_bdsd_workspace_bytes(B, C, h, w, blk))
    assert need > 0 and need % 8 == 0
    wbuf = torch.full((need // 8 + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    ws = wbuf[GUARD:GUARD + need // 8]
    ws.fill_(fill)
    ns = B * nby * nbx * C * (C + 1)
    outs = []
    for _ in range(2):
        buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')
        sbuf = torch.full((ns + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
        stats = sbuf[GUARD:GUARD + ns].view(B, nby, nbx, C, C + 1)
        _lib.check(L.lg_bdsd(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats), _ptr(taps_ms), F, _ptr(taps_pan), taps_ms.shape[1], blk, B, C, h, w, _ptr(ws), need,
                             _stream_ptr()), 'lg_bdsd')
        assert_guards_intact(buf, block)
        assert bool(torch.isnan(wbuf[:GUARD]).all()) and bool(torch.isnan(wbuf[-GUARD:]).all()), (block, 'written outside the workspace')
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[-GUARD:]).all()), (block, 'written outside stats')
        assert bool(torch.isfinite(out).all()), (block, 'an output element is missing or not finite')
        assert bool(torch.isfinite(stats).all()), (block, 'a weight is missing or not finite')
        outs.append((out, stats))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), (block, 'the second call on the same workspace differs')
    assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64)), (block, 'the weights of the second call differ')
    return outs[1]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))


@pytest.mark.parametrize('C,h,w,B,block,per_band', CASES)
def test_against_the_restatement(C, h, w, B, block, per_band):
    """element by element, the weights, every element written and nothing beside, a second call on the same workspace (raw_call)"""
    cs = case(C, h, w, B, block, per_band)
    ms, pan = inputs(C, h, w, B)
    ref, raw, bar = cs['ref'], cs['raw'], cs['bar']
    outside = float(((raw <= 0) | (raw >= 1)).mean())
    assert outside <= 0.02, f'{outside:.4f} of the unclipped restatement lies outside (0, 1): saturation could hide a wrong value'
    out, gamma = raw_call(dev(ms), dev(pan), gains_of(C, per_band), block)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    dist = max(br.gamma_distance(gamma[b].cpu().numpy(), cs['gamma'][b]) for b in range(B))
    print(f'C={C} h={h} w={w} B={B} block={block} {"per-band" if per_band else "equal"} gains: error {err:.3e}, float32 restatement {cs["e32"]:.3e}, '
          f'error / bar {err / bar:.3f}, share outside (0, 1) {outside:.4f}; gamma: distance to lstsq {dist:.3e}, the two routes {cs["routes"]:.3e}, '
          f'gate {cs["gate"]:.3e}, distance / gate {dist / cs["gate"]:.3f}')
    assert err <= bar, (err, bar)
    assert dist <= cs['gate'], (dist, cs['gate'])


@pytest.mark.parametrize('C,h,w,B,block,per_band', CASES)
def test_a_sample_has_the_same_bits_alone_and_in_a_batch_and_on_a_second_call(C, h, w, B, block, per_band):
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    ms = torch.cat([ms, ms.roll(1, dims=3)])              # 2 B samples: the shape's own and a variant of each
    pan = torch.cat([pan, pan.flip(2)])
    gains = gains_of(C, per_band)
    out, gamma = bdsd.bdsd(ms, pan, block, gains, br.GAIN_PAN, return_stats=True)
    assert gamma.shape == (2 * B,) + ((1, 1) if block is None else (4 * h // block, 4 * w // block)) + (C, C + 1) and gamma.dtype == torch.float64
    again, gamma2 = bdsd.bdsd(ms, pan, block, gains, br.GAIN_PAN, return_stats=True)
    assert same_bits(again, out) and same_bits(gamma2, gamma)
    assert same_bits(bdsd.bdsd(ms, pan, block, gains, br.GAIN_PAN), out)
    for b in range(2 * B):
        o1, g1 = bdsd.bdsd(ms[b:b + 1], pan[b:b + 1], block, gains, br.GAIN_PAN, return_stats=True)
        assert same_bits(o1[0], out[b]) and same_bits(g1[0], gamma[b]), b


@pytest.mark.parametrize('C,h,w,B,block,per_band', [CASES[1], CASES[7], CASES[10]])
def test_a_workspace_full_of_nan_changes_no_bit(C, h, w, B, block, per_band):
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    gains = gains_of(C, per_band)
    clean, g_clean = raw_call(ms, pan, gains, block)
    dirty, g_dirty = raw_call(ms, pan, gains, block, fill=float('nan'))
    assert same_bits(clean, dirty) and same_bits(g_clean, g_dirty)
    out, gamma = bdsd.bdsd(ms, pan, block, gains, br.GAIN_PAN, return_stats=True)      # ... and the function computes what the C ABI does
    assert same_bits(out, clean) and same_bits(gamma, g_clean)


def test_global_and_one_block_give_equal_bits():
    C, h, w, B = 8, 32, 32, 3
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    gains = gains_of(C, False)
    one, g_one = raw_call(ms, pan, gains, 128)
    glob, g_glob = raw_call(ms, pan, gains, None)
    assert g_one.shape == g_glob.shape == (B, 1, 1, C, C + 1)
    assert same_bits(one, glob) and same_bits(g_one, g_glob)


def test_one_filter_and_the_same_gain_per_band_give_equal_bits():
    C, h, w, B = 4, 5, 7, 2
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    gains = gains_of(C, False)
    one, g_one = raw_call(ms, pan, gains, None, F=1)
    per, g_per = raw_call(ms, pan, gains, None, F=C)
    assert same_bits(one, per) and same_bits(g_one, g_per)
    # ... and through the function: a scalar, a list of equal values, the defaults
    a = bdsd.bdsd(ms, pan, None, br.EQUAL_GAIN, br.GAIN_PAN)
    assert same_bits(a, one)
    assert same_bits(bdsd.bdsd(ms, pan, None, gains, br.GAIN_PAN), a)
    assert same_bits(bdsd.bdsd(ms, pan), a)               # wald.DEFAULT_GAIN_MS is 0.3, wald.DEFAULT_GAIN_PAN 0.15


@pytest.mark.parametrize('block', [None, 32])
def test_degenerate_sample_gives_clip_u_and_leaves_its_neighbour_alone(block):
    C, h, w, B = 4, 8, 16, 2
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    ms, pan = ms.clone(), pan.clone()
    for k in range(C):
        ms[0, k] = 0.25 + 0.125 * k                       # constant bands and a constant PAN, exactly representable: G has rank 1
    pan[0] = 0.5
    gains = gains_of(C, False)
    out, gamma = raw_call(ms, pan, gains, block)
    assert bool((gamma[0] == 0).all()) and bool((gamma[1] != 0).any(dim=-1).any(dim=-1).all())
    assert same_bits(out[0], classical.interp23(ms[:1])[0].clamp(0, 1))
    normal, g_normal = raw_call(ms[1:], pan[1:], gains, block)
    assert same_bits(normal[0], out[1]) and same_bits(g_normal[0], gamma[1])


def test_degenerate_blocks_beside_regular_ones():
    """tests/test_bdsd_cpu.py's sample: constant over the taps' reach of its first two blocks; blocks 2 and 3 are borderline and not asked about"""
    C, h, w = 4, 8, 64
    ms, pan = br.make_batch(1, C, h, w, seed=2)
    ms[0, :, :, :40], pan[0, 0, :, :160] = 0.25, 0.5
    gains = gains_of(C, False)
    out, gamma = raw_call(dev(ms), dev(pan), gains, 32)
    ref, want = br.bdsd(ms[0], pan[0, 0], gains, 32, return_stats=True)
    assert bool((gamma[0, 0, :2] == 0).all())
    assert same_bits(out[0, :, :, :64].contiguous(), classical.interp23(dev(ms))[0, :, :, :64].clamp(0, 1).contiguous())
    dist = br.gamma_distance(gamma[0, 0, 4:].cpu().numpy(), want[0, 4:])
    gate = max(1e-9, 8.0 * br.gamma_distance(br.weights(ms[0], pan[0, 0], gains, 32, route='cholesky')[0, 4:], want[0, 4:]))
    e32 = float(np.abs(br.bdsd(ms[0], pan[0, 0], gains, 32, dtype=np.float32).astype(np.float64) - ref)[:, :, 128:].max())
    err = float(np.abs(out[0].cpu().numpy().astype(np.float64) - ref)[:, :, 128:].max())
    print(f'regular blocks beside degenerate ones: error {err:.3e}, float32 restatement {e32:.3e}; gamma: distance to lstsq {dist:.3e}')
    assert err <= max(8.0 * e32, FLOOR) and dist <= gate


def test_saturation_gives_exactly_zero_and_one():
    C, h, w, B, block = br.CLIP_CASE
    ms, pan = br.make_clip_batch(C, h, w, B, seed=br.CLIP_SEED)
    gains = gains_of(C, False)
    cs = restate(ms, pan, gains, block)
    raw = cs['raw']
    below, above = raw < -br.CLIP_MARGIN, raw > 1 + br.CLIP_MARGIN
    assert below.mean() >= 0.02 and above.mean() >= 0.02 and cs['bar'] <= br.CLIP_MARGIN
    out, _ = raw_call(dev(ms), dev(pan), gains, block)
    got = out.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - cs['ref']).max())
    print(f'clip case: {100 * below.mean():.1f} % below 0, {100 * above.mean():.1f} % above 1; error {err:.3e}, error / bar {err / cs["bar"]:.3f}')
    assert np.array_equal(got[below], np.zeros(int(below.sum()), np.float32)) and np.array_equal(got[above], np.ones(int(above.sum()), np.float32))
    assert got.min() >= 0 and got.max() <= 1
    assert err <= cs['bar']


def test_rejected_calls_leave_the_output_alone():
    L = _lib.lib()
    B, C, h, w = 2, 4, 8, 16
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    taps_ms, taps_pan = device_taps([br.EQUAL_GAIN]), device_taps([br.GAIN_PAN])
    ws = torch.full((1 << 16,), SENTINEL, dtype=torch.float64, device='cuda')
    stats = torch.full((B * 2 * C * (C + 1),), SENTINEL, dtype=torch.float64, device='cuda')
    buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')

    def call(block=32, nbytes=ws.numel() * 8, ms=ms, pan=pan, C=C, h=h, w=w):
        return L.lg_bdsd(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats), _ptr(taps_ms), 1, _ptr(taps_pan), 41, block, B, C, h, w, _ptr(ws), nbytes, _stream_ptr())
    need = int(L.lg_bdsd_workspace_bytes(B, C, h, w, 32))
    m8, p8 = torch.zeros(B, 8, 4, 4, device='cuda'), torch.zeros(B, 1, 16, 16, device='cuda')
    for kw, text in ((dict(block=64), 'block must divide'), (dict(block=96), 'block must divide'), (dict(block=48), 'multiple of 32'),
                     (dict(nbytes=need - 8), 'workspace_bytes too small'), (dict(block=0, ms=m8, pan=p8, C=8, h=4, w=4), 'the global form needs')):
        assert call(**kw) < 0, text
        assert text in L.lg_last_error().decode(), (text, L.lg_last_error())
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()) and bool((ws == SENTINEL).all()) and bool((stats == SENTINEL).all()), text
    with pytest.raises(ValueError, match='does not divide'):
        bdsd.bdsd(ms, pan, 64)
    with pytest.raises(ValueError, match='multiple of 32'):
        bdsd.bdsd(ms, pan, 48)
    with pytest.raises(ValueError, match='global form needs'):
        bdsd.bdsd(m8, p8)
    assert call() == 0 and bool(torch.isfinite(out).all())                     # the same buffers, accepted


@pytest.mark.parametrize('block', [None, 32])
def test_runner(block, tmp_path):
    C, h, w, B = 4, 8, 8, 2
    rng = np.random.default_rng(5)
    peak = 2 ** 11 - .5
    batches = []
    for i in range(2):
        ms, pan = br.make_batch(B, C, h, w, seed=40 + i)
        target = np.clip(np.stack([cr.interp23(ms[b]) for b in range(B)]) + rng.normal(0, 0.02, (B, C, 4 * h, 4 * w)), 0.02, 0.98).astype(np.float32)
        batches.append(dict(input_lr=torch.from_numpy(ms * np.float32(peak)), input_pan=torch.from_numpy(pan * np.float32(peak)),
                            target=torch.from_numpy(target * np.float32(peak)), image_id=[f'im{i}_{b}' for b in range(B)]))
    gains = mr.per_band_gains(C)
    cfg = Config(dict(work_dir=str(tmp_path / 'w'), datas='synthetic', bit_depth=11, max_iter=10, eval_metrics='device', bdsd_block=block, mtf_gains_ms=gains,
                      mtf_gain_pan=0.12, mtf_taps=31))
    r = build_model('BDSD', cfg, logging.getLogger('t'), None, batches, batches)
    r.set_cuda()
    norm = [{k: (v.cuda() / peak if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    fused = [bdsd.bdsd(b['input_lr'], b['input_pan'], block, gains, 0.12, 31) for b in norm]
    for b, f in zip(norm, fused):
        got = r.get_model_output(b)
        assert got.is_cuda and same_bits(got, f)
    with_ref = r.test(iter_id=1, ref=True)
    no_ref = r.test(iter_id=1, ref=False)
    assert list(with_ref) == ['PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS'] and list(no_ref) == ['D_lambda', 'D_s', 'QNR']
    assert all(np.isfinite(v).all() for v in list(with_ref.values()) + list(no_ref.values()))
    rows = torch.cat([device_metrics.ref_evaluate_batch(f, b['target'].contiguous(), 1.0) for b, f in zip(norm, fused)]).cpu().numpy()
    for k, key in enumerate(with_ref):
        assert with_ref[key] == (float(rows[:, k].mean()), float(rows[:, k].std())), key


@pytest.mark.parametrize('block', [None, 32])
def test_whole_scene_in_one_call(block):
    """bdsd.fuse_scene on uint16 samples: the normalisation of scene.fuse_scene's gather, the method on the whole scene, lg_scene_to_u16"""
    C, h, w = 4, 16, 8
    ms, pan = br.make_scene(C, h, w, seed=77)
    ms16, pan16 = np.rint(ms * 2047.5).astype(np.uint16), np.rint(pan * 2047.5).astype(np.uint16)[None]
    post = float(np.float32(1.0) / np.float32(2047.5))
    gains = mr.per_band_gains(C)
    want = bdsd.bdsd(dev(ms16.astype(np.float32))[None] * post, dev(pan16.astype(np.float32))[None] * post, block, gains, 0.12)[0]
    got = bdsd.fuse_scene(ms16, pan16, block, gains_ms=gains, gain_pan=0.12, bit_depth=11)
    assert got.shape == (C, 4 * h, 4 * w) and same_bits(got, want)
    dn = bdsd.fuse_scene(torch.from_numpy(ms16.view(np.int16)).cuda(), torch.from_numpy(pan16.view(np.int16)).cuda(), block, gains_ms=gains, gain_pan=0.12,
                         bit_depth=11, out_dtype='uint16')
    assert dn.dtype == torch.uint16
    assert np.array_equal(dn.cpu().numpy(), np.clip(np.rint(want.cpu().numpy() * np.float32(2047.5)), 0, 65535).astype(np.uint16))
