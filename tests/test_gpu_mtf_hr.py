"""-m gpu: the regression-based and haze-corrected MTF baselines FS, HPM-R, HPM-H and BT-H (lgteun_amd/mtf_hr.py, the k_hr_* kernels of
lgteun_amd/csrc/k_classical.hip) against the float64 numpy restatement in tests/mtf_hr_ref.py.

The bar of an output tensor is that of tests/test_gpu_classical.py: its largest absolute difference to the float64 restatement may be at
most 8 x the difference of the float32 run of the same restatement to its float64 run on that case, with a floor of 2^-23 -- measured on the reference,
never on the kernels.  `stats` must agree with numpy to 1e-9 relative, element by element (a slot the rule leaves unused must be exactly 0).  The
preconditions of the cases -- denominators, conditioning, clip share -- are proven in tests/test_mtf_hr_cpu.py; the measured figures are in DESIGN.md 3.17.

Which shape covers what (16 x 32 output tiles; the Gram pass of the haze rules takes 256 MS pixels per chunk, at most 128 workgroups per sample):
  fs / hpm_r        tests/test_gpu_mtf_glp.py's shapes and inputs ((4, 7, 9, 2) for fs where hpm_r has (4, 5, 7, 2): tests/mtf_hr_ref.py says why)
  hpm_h / bt_h      the haze scenes of mtf_hr_ref.make_haze_batch: C = 2, 3, 5, 9, 16; (4, 5, 7, 2) / (4, 7, 9, 2) ragged and odd; (8, 32, 32, 3) four chunks,
                    (4, 136, 256, 1) 136 chunks against 128 workgroups: eight of them take a second chunk, and 1088 tiles against 768 walkers in k_hr_moments
  (15, 12, 12, 1)   hpm_h, per-band gains: C = F = 15 is the first count at which k_hr_gram's dynamic LDS passes 64 KiB (31 vectors of 256 doubles and the sums:
                    66 976 bytes; 62 296 at 14); (16, 16, 8, 1) is the maximum, 71 496 bytes
  (12, 16, 8, 1)    bt_h: C = 12 is the first count at which k_hr_apply<bt_h>'s C tiles of u pass 64 KiB ((2141 + 512 C) doubles: 62 184 bytes at 11, 66 280 at 12)
Properties (bits) run at (4, 4, 4, 1), (4, 5, 7, 2) and (8, 12, 8, 3) for every rule."""
import ctypes
import functools
import logging

import numpy as np
import pytest
import torch

import classical_ref as cr
import mtf_glp_ref as mr
import mtf_hr_ref as hr
from gpu_helpers import GUARD, assert_guards_intact, guarded_empty
from lgteun_amd import _lib, build_model, classical, mtf_hr
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
CASES = [(rule,) + s + (False,) for rule in hr.RULES for s in hr.SHAPES[rule]] + [(rule,) + s + (True,) for rule in hr.RULES for s in hr.PER_BAND_SHAPES[rule]]
PROPERTY_CASES = [(rule,) + s for rule in hr.RULES for s in hr.PROPERTY_SHAPES]


def gains_of(C, per_band):
    return mr.per_band_gains(C) if per_band else [hr.EQUAL_GAIN] * C


@functools.lru_cache(maxsize=None)
def inputs(rule_kind, C, h, w, B):
    ms, pan = hr.make_inputs('hpm_h' if rule_kind == 'haze' else 'fs', C, h, w, B)
    ms.setflags(write=False)
    pan.setflags(write=False)
    return ms, pan


def inputs_of(rule, C, h, w, B):
    return inputs('haze' if rule in hr.HAZE_RULES else 'full', C, h, w, B)


def restate(ms, pan, rule, gains):
    """-> dict(ref float64 [B, C, 4h, 4w], e32, bar, stats [B, 2C + 2])"""
    B = ms.shape[0]
    r64 = [hr.mtf_hr(ms[b], pan[b, 0], rule, gains, return_stats=True) for b in range(B)]
    r32 = np.stack([hr.mtf_hr(ms[b], pan[b, 0], rule, gains, dtype=np.float32) for b in range(B)])
    assert r32.dtype == np.float32
    ref = np.stack([r[0] for r in r64])
    e32 = float(np.abs(r32.astype(np.float64) - ref).max())
    res = dict(ref=ref, e32=e32, bar=max(8.0 * e32, FLOOR), stats=np.stack([r[1] for r in r64]))
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def case(rule, C, h, w, B, per_band):
    """the float64 restatement of a case and its bar; computed once, never written to"""
    ms, pan = inputs_of(rule, C, h, w, B)
    return restate(ms, pan, rule, gains_of(C, per_band))


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the cached arrays are read-only


def device_taps(gains, n_taps=41):
    return torch.from_numpy(np.stack([mr.taps(g, n_taps) for g in gains])).cuda()


def call(which, ms, pan, out, stats, taps_t, F, ws, need, **kw):
    """lg_mtf_hr with the rule `which` once -> its return code; kw: fields of the argument block to overwrite"""
    B, C, h, w = ms.shape
    d = dict(struct_bytes=ctypes.sizeof(_lib.LgMtfHrArgs), rule=mtf_hr.RULES[which], n_filters=F, n_taps=taps_t.shape[1], B=B, C=C, h=h, w=w, ms=_ptr(ms),
             pan=_ptr(pan), out=_ptr(out), stats=_ptr(stats) if stats is not None else None, taps=_ptr(taps_t), workspace=_ptr(ws), workspace_bytes=need,
             stream=_stream_ptr())
    d.update(kw)
    return _lib.lib().lg_mtf_hr(ctypes.byref(_lib.LgMtfHrArgs(**d)))


def raw_call(rule, ms, pan, gains, F=None, with_stats=True):
    """the C ABI with the output inside NaN guard bands and the workspace, itself between guard bands, filled with a finite sentinel; twice on the same
    workspace.  gains: the bands' (bt_h filters with hr.GAIN_PAN).  F: the number of filtered planes (default: 1 when all gains are equal, else C).
    -> (out, stats or None)"""
    L = _lib.lib()
    B, C, h, w = ms.shape
    if rule == 'bt_h':
        gains, F = [hr.GAIN_PAN], 1
    elif F is None:
        F = 1 if len(set(gains)) == 1 else C
    taps = device_taps(gains[:F])
    need = int(L.lg_mtf_hr_workspace_bytes(B, C, h, w, F, mtf_hr.RULES[rule]))
    assert need > 0 and need % 8 == 0
    wbuf = torch.full((need // 8 + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    ws = wbuf[GUARD:GUARD + need // 8]
    ws.fill_(-1.2345e300)
    ns = B * (2 * C + 2)
    outs = []
    for _ in range(2):
        buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')
        sbuf = torch.full((ns + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
        stats = sbuf[GUARD:GUARD + ns].view(B, 2 * C + 2) if with_stats else None
        _lib.check(call(rule, ms, pan, out, stats, taps, F, ws, need), 'lg_mtf_hr')
        assert_guards_intact(buf, rule)
        assert bool(torch.isnan(wbuf[:GUARD]).all()) and bool(torch.isnan(wbuf[-GUARD:]).all()), (rule, 'written outside the workspace')
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[-GUARD:]).all()), (rule, 'written outside stats')
        assert bool(torch.isfinite(out).all()), (rule, 'an output element is missing or not finite')
        if with_stats:
            assert bool(torch.isfinite(stats).all()), (rule, 'a statistic is missing or not finite')
        else:
            assert bool(torch.isnan(sbuf).all()), (rule, 'stats written although NULL was passed')
        outs.append((out, stats))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), (rule, 'the second call on the same workspace differs')
    if with_stats:
        assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64)), (rule, 'stats of the second call differ')
    return outs[1]


def stats_distance(got, want):
    """the largest |got - want| / |want| over the slots the rule fills; the others must be exactly 0"""
    used = want != 0
    assert np.array_equal(got[~used], np.zeros(int((~used).sum()))), 'an unused slot of stats is not 0'
    return float(np.abs(got[used] / want[used] - 1.0).max())


@pytest.mark.parametrize('rule,C,h,w,B,per_band', CASES)
def test_against_the_restatement(rule, C, h, w, B, per_band):
    cs = case(rule, C, h, w, B, per_band)
    ms, pan = inputs_of(rule, C, h, w, B)
    ref, bar = cs['ref'], cs['bar']
    out, stats = raw_call(rule, dev(ms), dev(pan), gains_of(C, per_band))
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    rel = stats_distance(stats.cpu().numpy(), cs['stats'])
    print(f'{rule} C={C} h={h} w={w} B={B} {"per-band" if per_band else "equal"} gains: error {err:.3e}, float32 restatement {cs["e32"]:.3e}, '
          f'error / bar {err / bar:.3f}; stats, largest relative difference {rel:.3e}')
    assert err <= bar, (err, bar)
    assert rel <= 1e-9, rel


@pytest.mark.parametrize('rule,C,h,w,B', PROPERTY_CASES)
def test_a_sample_has_the_same_bits_alone_and_in_a_batch(rule, C, h, w, B):
    ms, pan = (dev(a) for a in inputs_of(rule, C, h, w, B))
    ms = torch.cat([ms, ms.roll(1, dims=3)])              # 2 B samples: the shape's own and a variant of each
    pan = torch.cat([pan, pan.flip(2)])
    for gains in ([None] if rule == 'bt_h' else [None, mr.per_band_gains(C)]):
        out, stats = mtf_hr.fuse(ms, pan, rule, gains, return_stats=True)
        for b in range(2 * B):
            o1, s1 = mtf_hr.fuse(ms[b:b + 1].clone(), pan[b:b + 1].clone(), rule, gains, return_stats=True)
            assert torch.equal(o1[0].view(torch.int32), out[b].view(torch.int32)), (rule, b)
            assert torch.equal(s1[0].view(torch.int64), stats[b].view(torch.int64)), (rule, b)


@pytest.mark.parametrize('rule,C,h,w,B', PROPERTY_CASES)
def test_guards_workspace_planes_and_null_stats(rule, C, h, w, B):
    """raw_call itself: NaN guard bands around out, stats and the workspace, a sentinel-filled workspace, a second call.  Here also: one filtered plane and the
    same taps C times, stats = NULL, and the function, give the same bits"""
    ms, pan = (dev(a) for a in inputs_of(rule, C, h, w, B))
    gains = gains_of(C, False)
    one, s_one = raw_call(rule, ms, pan, gains, F=1)
    bare, none = raw_call(rule, ms, pan, gains, F=1, with_stats=False)
    assert none is None and torch.equal(bare.view(torch.int32), one.view(torch.int32)), (rule, 'stats = NULL changes the output')
    if rule != 'bt_h':
        per, s_per = raw_call(rule, ms, pan, gains, F=C)
        assert torch.equal(one.view(torch.int32), per.view(torch.int32)) and torch.equal(s_one.view(torch.int64), s_per.view(torch.int64))
    # ... and through the function: the default, a scalar, a list of equal values
    kw = dict(gain_pan=hr.GAIN_PAN) if rule == 'bt_h' else dict(gains_ms=hr.EQUAL_GAIN)
    a, s_a = mtf_hr.fuse(ms, pan, rule, return_stats=True)          # wald's defaults are 0.3 and 0.15
    assert torch.equal(a.view(torch.int32), one.view(torch.int32)) and torch.equal(s_a.view(torch.int64), s_one.view(torch.int64))
    assert torch.equal(mtf_hr.fuse(ms, pan, rule, **kw).view(torch.int32), a.view(torch.int32))
    assert torch.equal(getattr(mtf_hr, rule)(ms, pan).view(torch.int32), a.view(torch.int32))
    if rule != 'bt_h':
        assert torch.equal(mtf_hr.fuse(ms, pan, rule, gains).view(torch.int32), a.view(torch.int32))


@pytest.mark.parametrize('rule', hr.RULES)
def test_constant_pan_gives_clip_u_and_leaves_its_neighbour_alone(rule):
    C, h, w, B = 4, 8, 8, 2
    ms_np, pan_np = inputs_of(rule, C, h, w, B)
    ms, pan = dev(ms_np), dev(pan_np).clone()
    pan[0] = 0.3
    gains = gains_of(C, False)
    u64 = np.clip(cr.interp23(ms_np[0]), 0, 1)
    u32 = np.clip(cr.interp23(ms_np[0], np.float32), 0, 1)
    bar = max(8.0 * float(np.abs(u32.astype(np.float64) - u64).max()), FLOOR)           # interp23's bar on this sample
    out, stats = raw_call(rule, ms, pan, gains)
    err = float(np.abs(out[0].cpu().numpy().astype(np.float64) - u64).max())
    print(f'{rule}, constant PAN: distance to clip(u) {err:.3e}, bar {bar:.3e}')
    assert err <= bar
    if rule in ('fs', 'hpm_r'):
        assert bool((stats[0, :C] == 0).all())             # g = 0; hpm_r: b = m_k, r = m_k / m_k
        assert torch.equal(out[0].view(torch.int32), classical.interp23(ms[:1])[0].clamp(0, 1).view(torch.int32))      # exactly the clipped interpolation
    elif rule == 'bt_h':
        assert bool((stats[0, C:2 * C] == 0).all())        # the fit of a constant has slopes of exactly 0
    normal, nstats = raw_call(rule, ms[1:].clone(), pan[1:].clone(), gains)
    assert torch.equal(normal[0].view(torch.int32), out[1].view(torch.int32)), rule
    assert torch.equal(nstats[0].view(torch.int64), stats[1].view(torch.int64)), rule


@pytest.mark.parametrize('rule', hr.RULES)
def test_saturation_gives_exactly_zero_and_one(rule):
    C, h, w, B = mr.CLIP_SHAPE
    ms, pan = mr.make_clip_batch(C, h, w, B, seed=mr.CLIP_SEED)
    gains = gains_of(C, False)
    raw = np.stack([hr.mtf_hr(ms[b], pan[b, 0], rule, gains, clip=False) for b in range(B)])
    below, above = raw < -hr.CLIP_MARGIN, raw > 1 + hr.CLIP_MARGIN
    assert below.any() and above.any()
    out, _ = raw_call(rule, dev(ms), dev(pan), gains)      # (finite everywhere: raw_call checks)
    got = out.cpu().numpy()
    print(f'{rule}, clip case: {100 * below.mean():.1f} % below 0, {100 * above.mean():.1f} % above 1')
    assert np.array_equal(got[below], np.zeros(int(below.sum()), np.float32)) and np.array_equal(got[above], np.ones(int(above.sum()), np.float32))
    assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize('rule', hr.RULES)
def test_a_rejected_call_leaves_out_untouched(rule):
    C, h, w, B = 4, 5, 7, 2
    ms, pan = (dev(a) for a in inputs_of(rule, C, h, w, B))
    L = _lib.lib()
    taps = device_taps([hr.EQUAL_GAIN])
    need = int(L.lg_mtf_hr_workspace_bytes(B, C, h, w, 1, mtf_hr.RULES[rule]))
    ws = torch.full((need // 8,), 7.0, dtype=torch.float64, device='cuda')
    out = torch.full((B, C, 4 * h, 4 * w), -3.0, device='cuda')
    stats = torch.full((B, 2 * C + 2), -3.0, dtype=torch.float64, device='cuda')
    for kw, text in ((dict(workspace_bytes=need - 8), 'workspace_bytes too small'), (dict(n_taps=40), 'n_taps must be'), (dict(n_filters=2), 'n_filters must be'),
                     (dict(rule=7), 'rule must be'), (dict(struct_bytes=8), 'struct_bytes must be'), (dict(taps=None), 'taps is NULL')):
        assert call(rule, ms, pan, out, stats, taps, 1, ws, need, **kw) < 0
        msg = L.lg_last_error().decode()
        assert msg.startswith('mtf_hr:') and text in msg, msg
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((stats == -3.0).all()) and bool((ws == 7.0).all())
    assert call(rule, ms, pan, out, stats, taps, 1, ws, need) == 0           # and the same buffers are good for a valid call
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0


@pytest.mark.parametrize('name', ['MTF_GLP_FS', 'MTF_GLP_HPM_R', 'MTF_GLP_HPM_H', 'BT_H'])
def test_runner(name, tmp_path):
    C, h, w, B = 4, 8, 8, 2
    rule = getattr(mtf_hr, name).rule
    rng = np.random.default_rng(5)
    peak = 2 ** 11 - .5
    batches = []
    for i in range(2):
        ms, pan = hr.make_haze_batch(B, C, h, w, seed=7040 + 2 * i) if rule in hr.HAZE_RULES else cr.make_batch(B, C, h, w, seed=40 + i)
        target = np.clip(np.stack([cr.interp23(ms[b]) for b in range(B)]) + rng.normal(0, 0.02, (B, C, 4 * h, 4 * w)), 0.02, 0.98).astype(np.float32)
        batches.append(dict(input_lr=torch.from_numpy(ms * np.float32(peak)), input_pan=torch.from_numpy(pan * np.float32(peak)),
                            target=torch.from_numpy(target * np.float32(peak)), image_id=[f'im{i}_{b}' for b in range(B)]))
    gains, gain_pan = mr.per_band_gains(C), 0.17
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, max_iter=10, eval_metrics='device', mtf_gains_ms=gains,
                      mtf_gain_pan=gain_pan))
    r = build_model(name, cfg, logging.getLogger('t'), None, batches, batches)
    r.set_cuda()
    norm = [{k: (v.cuda() / peak if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    for b in norm:
        want = mtf_hr.fuse(b['input_lr'], b['input_pan'], rule, gains, gain_pan)
        got = r.get_model_output(b)
        assert got.is_cuda and torch.equal(got.view(torch.int32), want.view(torch.int32))
    with_ref = r.test(iter_id=1, ref=True)
    assert list(with_ref) == ['PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS'] and all(np.isfinite(v).all() for v in with_ref.values())


@pytest.mark.parametrize('rule', hr.RULES)
def test_whole_scene_in_one_call(rule):
    """mtf_hr.fuse_scene on uint16 samples: the normalisation of scene.fuse_scene's gather, the rule on the whole scene, lg_scene_to_u16"""
    C, h, w = 4, 12, 8
    ms, pan = hr.make_haze_scene(C, h, w, 7077) if rule in hr.HAZE_RULES else cr.make_scene(C, h, w, seed=77)
    ms16, pan16 = np.rint(ms * 2047.5).astype(np.uint16), np.rint(pan * 2047.5).astype(np.uint16)[None]
    post = float(np.float32(1.0) / np.float32(2047.5))
    gains, gain_pan = mr.per_band_gains(C), 0.17
    want = mtf_hr.fuse(dev(ms16.astype(np.float32))[None] * post, dev(pan16.astype(np.float32))[None] * post, rule, gains, gain_pan)[0]
    got = mtf_hr.fuse_scene(rule, ms16, pan16, gains_ms=gains, gain_pan=gain_pan, bit_depth=11)
    assert got.shape == (C, 4 * h, 4 * w) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    dn = mtf_hr.fuse_scene(rule, torch.from_numpy(ms16.view(np.int16)).cuda(), torch.from_numpy(pan16.view(np.int16)).cuda(), gains_ms=gains,
                           gain_pan=gain_pan, bit_depth=11, out_dtype='uint16')
    assert dn.dtype == torch.uint16
    assert np.array_equal(dn.cpu().numpy(), np.clip(np.rint(want.cpu().numpy() * np.float32(2047.5)), 0, 65535).astype(np.uint16))
