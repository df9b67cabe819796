"""-m gpu: the MTF-GLP baselines (lgteun_amd/mtf_glp.py, the k_mg_* kernels of lgteun_amd/csrc/k_classical.hip) against the float64 numpy restatement
in tests/mtf_glp_ref.py.

The bar of an output tensor is that of tests/test_gpu_classical.py: its largest absolute difference to the float64 restatement may be at most 8 x the
difference of the float32 run of the same restatement to its float64 run on that case, with a floor of 2^-23.  The scales a and the gains g (`stats`)
must agree with numpy to 1e-9 relative.  The measured figures are in DESIGN.md 3.13.

Which shape covers what (16 x 32 output tiles; the low-pass works on 16 x 16 tiles of the MS grid; both moments passes run at most 768 workgroups per
sample at C = 4):
  (4, 4, 4, 1)      one ragged tile: the 41 taps clamp on every side of the 16 x 16 PAN, the 23 taps wrap three times
  (4, 8, 8, 2)      two full tiles
  (4, 5, 7, 2)      two ragged tiles, sides off every power-of-two grid; also with per-band gains (one filtered plane per band)
  (8, 12, 8, 3)     three tiles, C = 8; also with per-band gains
  (8, 32, 32, 3)    8 x 4 tiles; 2 x 2 tiles of the low-pass
  (4, 40, 24, 2)    10 x 3 tiles; 3 x 2 tiles of the low-pass, ragged both ways
  (4, 136, 256, 1)  1088 tiles > 768: workgroups of both moments passes walk a second tile; also with per-band gains"""
import functools
import logging

import numpy as np
import pytest
import torch

import classical_ref as cr
import mtf_glp_ref as mr
from gpu_helpers import GUARD, assert_guards_intact, guarded_empty
from lgteun_amd import _lib, build_model, classical, device_metrics, mtf_glp
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
CASES = [s + (False,) for s in mr.SHAPES] + [s + (True,) for s in mr.PER_BAND_SHAPES]      # C, h, w, B, per-band gains


def gains_of(C, per_band):
    return mr.per_band_gains(C) if per_band else [mr.EQUAL_GAIN] * C


@functools.lru_cache(maxsize=None)
def inputs(C, h, w, B):
    ms, pan = cr.make_batch(B, C, h, w, seed=C * 100 + h)
    ms.setflags(write=False)
    pan.setflags(write=False)
    return ms, pan


def restate(ms, pan, mode, gains):
    """-> dict(ref float64 [B, C, 4h, 4w], e32, bar, stats [B, 2C])"""
    B = ms.shape[0]
    r64 = [mr.mtf_glp(ms[b], pan[b, 0], mode, gains, return_stats=True) for b in range(B)]
    r32 = np.stack([mr.mtf_glp(ms[b], pan[b, 0], mode, gains, dtype=np.float32) for b in range(B)])
    assert r32.dtype == np.float32
    ref = np.stack([r[0] for r in r64])
    e32 = float(np.abs(r32.astype(np.float64) - ref).max())
    res = dict(ref=ref, e32=e32, bar=max(8.0 * e32, FLOOR), stats=np.stack([np.concatenate(r[1:]) for r in r64]))
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def case(C, h, w, B, per_band, mode):
    """the float64 restatement of a case and its bar; computed once, never written to"""
    ms, pan = inputs(C, h, w, B)
    return restate(ms, pan, mode, gains_of(C, per_band))


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the cached arrays are read-only


def device_taps(gains, n_taps=41):
    return torch.from_numpy(np.stack([mr.taps(g, n_taps) for g in gains])).cuda()


def raw_call(mode, ms, pan, gains, F=None):
    """the C ABI with the output inside NaN guard bands and the workspace, itself between guard bands, filled with a finite sentinel; twice on the same
    workspace.  F: the number of filtered planes (default: 1 when all gains are equal, else C).  -> (out, stats)"""
    L = _lib.lib()
    B, C, h, w = ms.shape
    if F is None:
        F = 1 if len(set(gains)) == 1 else C
    taps = device_taps(gains[:F])
    code = mtf_glp.MODES[mode]
    need = int(L.lg_mtfglp_workspace_bytes(B, C, h, w, F, code))
    assert need > 0 and need % 8 == 0
    wbuf = torch.full((need // 8 + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    ws = wbuf[GUARD:GUARD + need // 8]
    ws.fill_(-1.2345e300)
    outs = []
    for _ in range(2):
        buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')
        sbuf = torch.full((B * 2 * C + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
        stats = sbuf[GUARD:GUARD + B * 2 * C].view(B, 2 * C)
        _lib.check(L.lg_mtf_glp(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats), _ptr(taps), F, taps.shape[1], code, B, C, h, w, _ptr(ws), need, _stream_ptr()),
                   'lg_mtf_glp')
        assert_guards_intact(buf, mode)
        assert bool(torch.isnan(wbuf[:GUARD]).all()) and bool(torch.isnan(wbuf[-GUARD:]).all()), (mode, 'written outside the workspace')
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[-GUARD:]).all()), (mode, 'written outside stats')
        assert bool(torch.isfinite(out).all()), (mode, 'an output element is missing or not finite')
        assert bool(torch.isfinite(stats).all()), (mode, 'a statistic is missing or not finite')
        outs.append((out, stats))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), (mode, 'the second call on the same workspace differs')
    assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64)), (mode, 'stats of the second call differ')
    return outs[1]


@pytest.mark.parametrize('mode', mr.MODES)
@pytest.mark.parametrize('C,h,w,B,per_band', CASES)
def test_against_the_restatement(C, h, w, B, per_band, mode):
    cs = case(C, h, w, B, per_band, mode)
    ms, pan = inputs(C, h, w, B)
    ref, bar = cs['ref'], cs['bar']
    clip_share = float(((ref <= 0) | (ref >= 1)).mean())
    assert clip_share <= 0.02, f'{clip_share:.4f} of the restatement sits on a clip boundary: saturation could hide a wrong value'
    out, stats = raw_call(mode, dev(ms), dev(pan), gains_of(C, per_band))
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    rel = float(np.abs(stats.cpu().numpy() / cs['stats'] - 1.0).max())
    print(f'{mode} C={C} h={h} w={w} B={B} {"per-band" if per_band else "equal"} gains: error {err:.3e}, float32 restatement {cs["e32"]:.3e}, '
          f'error / bar {err / bar:.3f}, clip share {clip_share:.4f}; a and g, largest relative difference {rel:.3e}')
    assert err <= bar, (err, bar)
    assert rel <= 1e-9, rel
    if mode != 'cbd':
        assert bool((stats[:, C:] == 1).all())


@pytest.mark.parametrize('mode', mr.MODES)
@pytest.mark.parametrize('C,h,w,B,per_band', CASES)
def test_a_sample_has_the_same_bits_alone_and_in_a_batch(C, h, w, B, per_band, mode):
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    ms = torch.cat([ms, ms.roll(1, dims=3)])              # 2 B samples: the shape's own and a variant of each
    pan = torch.cat([pan, pan.flip(2)])
    gains = gains_of(C, per_band)
    out, stats = mtf_glp.mtf_glp(ms, pan, mode, gains, return_stats=True)
    for b in range(2 * B):
        o1, s1 = mtf_glp.mtf_glp(ms[b:b + 1], pan[b:b + 1], mode, gains, return_stats=True)
        assert torch.equal(o1[0].view(torch.int32), out[b].view(torch.int32)), (mode, b)
        assert torch.equal(s1[0].view(torch.int64), stats[b].view(torch.int64)), (mode, b)


@pytest.mark.parametrize('mode', mr.MODES)
def test_constant_pan_gives_clip_u_and_leaves_its_neighbour_alone(mode):
    C, h, w, B = 4, 8, 8, 2
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    pan = pan.clone()
    pan[0] = 0.3
    gains = gains_of(C, False)
    u64 = np.clip(cr.interp23(inputs(C, h, w, B)[0][0]), 0, 1)
    u32 = np.clip(cr.interp23(inputs(C, h, w, B)[0][0], np.float32), 0, 1)
    bar = max(8.0 * float(np.abs(u32.astype(np.float64) - u64).max()), FLOOR)           # interp23's bar on this sample
    out, stats = raw_call(mode, ms, pan, gains)
    err = float(np.abs(out[0].cpu().numpy().astype(np.float64) - u64).max())
    print(f'{mode}, constant PAN: distance to clip(u) {err:.3e}, bar {bar:.3e}')
    assert err <= bar
    assert bool((stats[0, :C] == 0).all())
    normal, nstats = raw_call(mode, ms[1:], pan[1:], gains)
    assert torch.equal(normal[0].view(torch.int32), out[1].view(torch.int32)), mode
    assert torch.equal(nstats[0].view(torch.int64), stats[1].view(torch.int64)), mode
    if mode == 'cbd':
        assert bool((stats[0, C:] == 0).all())
        assert torch.equal(out[0].view(torch.int32), classical.interp23(ms[:1])[0].clamp(0, 1).view(torch.int32))      # g = 0: exactly the clipped interpolation


@pytest.mark.parametrize('mode', mr.MODES)
def test_saturation_gives_exactly_zero_and_one(mode):
    C, h, w, B = mr.CLIP_SHAPE
    ms, pan = mr.make_clip_batch(C, h, w, B, seed=mr.CLIP_SEED)
    gains = gains_of(C, False)
    raw = np.stack([mr.mtf_glp(ms[b], pan[b, 0], mode, gains, clip=False) for b in range(B)])
    cs = restate(ms, pan, mode, gains)
    below, above = raw < -mr.CLIP_MARGIN, raw > 1 + mr.CLIP_MARGIN
    assert below.mean() >= 0.02 and above.mean() >= 0.02 and cs['bar'] <= mr.CLIP_MARGIN
    out, _ = raw_call(mode, dev(ms), dev(pan), gains)
    got = out.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - cs['ref']).max())
    print(f'{mode}, clip case: {100 * below.mean():.1f} % below 0, {100 * above.mean():.1f} % above 1; error {err:.3e}, error / bar {err / cs["bar"]:.3f}')
    assert np.array_equal(got[below], np.zeros(int(below.sum()), np.float32)) and np.array_equal(got[above], np.ones(int(above.sum()), np.float32))
    assert got.min() >= 0 and got.max() <= 1
    assert err <= cs['bar']


@pytest.mark.parametrize('mode', mr.MODES)
def test_one_filtered_plane_and_the_same_gain_per_band_give_equal_bits(mode):
    C, h, w, B = 4, 5, 7, 2
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    gains = gains_of(C, False)
    one, s_one = raw_call(mode, ms, pan, gains, F=1)
    per, s_per = raw_call(mode, ms, pan, gains, F=C)
    assert torch.equal(one.view(torch.int32), per.view(torch.int32)) and torch.equal(s_one.view(torch.int64), s_per.view(torch.int64))
    # ... and through the function: a scalar, a list of equal values, the default
    a = mtf_glp.mtf_glp(ms, pan, mode, mr.EQUAL_GAIN)
    assert torch.equal(a.view(torch.int32), one.view(torch.int32))
    assert torch.equal(mtf_glp.mtf_glp(ms, pan, mode, gains).view(torch.int32), a.view(torch.int32))
    assert torch.equal(mtf_glp.mtf_glp(ms, pan, mode).view(torch.int32), a.view(torch.int32))          # wald.DEFAULT_GAIN_MS is 0.3


@pytest.mark.parametrize('name', ['MTF_GLP', 'MTF_GLP_HPM', 'MTF_GLP_CBD'])
def test_runner(name, tmp_path):
    C, h, w, B = 4, 8, 8, 2
    rng = np.random.default_rng(5)
    peak = 2 ** 11 - .5
    batches = []
    for i in range(2):
        ms, pan = cr.make_batch(B, C, h, w, seed=40 + i)
        target = np.clip(np.stack([cr.interp23(ms[b]) for b in range(B)]) + rng.normal(0, 0.02, (B, C, 4 * h, 4 * w)), 0.02, 0.98).astype(np.float32)
        batches.append(dict(input_lr=torch.from_numpy(ms * np.float32(peak)), input_pan=torch.from_numpy(pan * np.float32(peak)),
                            target=torch.from_numpy(target * np.float32(peak)), image_id=[f'im{i}_{b}' for b in range(B)]))
    gains = mr.per_band_gains(C)
    mode = getattr(mtf_glp, name).mode

    def runner(metrics_on):
        cfg = Config(dict(work_dir=str(tmp_path / metrics_on), datas='synthetic', bit_depth=11, max_iter=10, eval_metrics=metrics_on, mtf_gains_ms=gains))
        r = build_model(name, cfg, logging.getLogger('t'), None, batches, batches)
        r.set_cuda()
        return r
    r = runner('device')
    norm = [{k: (v.cuda() / peak if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    fused = [mtf_glp.mtf_glp(b['input_lr'], b['input_pan'], mode, gains) for b in norm]
    for b, f in zip(norm, fused):
        got = r.get_model_output(b)
        assert got.is_cuda and torch.equal(got.view(torch.int32), f.view(torch.int32))
    with_ref = r.test(iter_id=1, ref=True)
    no_ref = r.test(iter_id=1, ref=False)
    assert list(with_ref) == ['PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS'] and list(no_ref) == ['D_lambda', 'D_s', 'QNR']
    assert all(np.isfinite(v).all() for v in list(with_ref.values()) + list(no_ref.values()))
    for key in ('PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS', 'D_lambda', 'D_s', 'QNR'):
        assert len(r.eval_results[key + '_mean']) == 1 and len(r.eval_results[key + '_std']) == 1
    rows = torch.cat([device_metrics.ref_evaluate_batch(f, b['target'].contiguous(), 1.0) for b, f in zip(norm, fused)]).cpu().numpy()
    for k, key in enumerate(with_ref):
        assert with_ref[key] == (float(rows[:, k].mean()), float(rows[:, k].std())), key
    host = runner('host').test(iter_id=1, ref=True)
    assert list(host) == list(with_ref) and all(np.isfinite(v).all() for v in host.values())


@pytest.mark.parametrize('mode', mr.MODES)
def test_whole_scene_in_one_call(mode):
    """mtf_glp.fuse_scene on uint16 samples: the normalisation of scene.fuse_scene's gather, the method on the whole scene, lg_scene_to_u16"""
    C, h, w = 4, 12, 8
    ms, pan = cr.make_scene(C, h, w, seed=77)
    ms16, pan16 = np.rint(ms * 2047.5).astype(np.uint16), np.rint(pan * 2047.5).astype(np.uint16)[None]
    post = float(np.float32(1.0) / np.float32(2047.5))
    gains = mr.per_band_gains(C)
    want = mtf_glp.mtf_glp(dev(ms16.astype(np.float32))[None] * post, dev(pan16.astype(np.float32))[None] * post, mode, gains)[0]
    got = mtf_glp.fuse_scene(mode, ms16, pan16, gains_ms=gains, bit_depth=11)
    assert got.shape == (C, 4 * h, 4 * w) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    dn = mtf_glp.fuse_scene(mode, torch.from_numpy(ms16.view(np.int16)).cuda(), torch.from_numpy(pan16.view(np.int16)).cuda(), gains_ms=gains, bit_depth=11,
                            out_dtype='uint16')
    assert dn.dtype == torch.uint16
    assert np.array_equal(dn.cpu().numpy(), np.clip(np.rint(want.cpu().numpy() * np.float32(2047.5)), 0, 65535).astype(np.uint16))
