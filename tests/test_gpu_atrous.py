"""-m gpu: the a trous baselines ATWT and AWLP (lgteun_amd/atrous.py, the k_at_* kernels of lgteun_amd/csrc/k_classical.hip) against the float64 numpy
restatement in tests/atrous_ref.py.

The bar of an output tensor is that of tests/test_gpu_classical.py: its largest absolute difference to the float64 restatement may be at most 8 x the
difference of the float32 run of the same restatement to its float64 run on that case, with a floor of 2^-23.  The scales a and the reference deviation
(`stats`) must agree with numpy to 1e-9 relative.  The measured figures are in DESIGN.md 3.16.

Which shape covers what (16 x 32 output tiles, PAN staged with a circular halo of 6; the moments passes run at most 768 workgroups per sample at C = 4):
  (4, 4, 4, 1)      one ragged tile on a 16 x 16 PAN: the halo wraps on every side, the staged columns more than once
  (4, 8, 8, 2)      two full tiles
  (4, 5, 7, 2)      two ragged tiles, sides off every power-of-two grid; (2, 5, 7, 2), (3, 6, 9, 1), (16, 8, 8, 1): the ends of the band range and an odd count
  (8, 12, 8, 3)     three tiles, C = 8: AWLP's band mean takes two rounds of four bands
  (8, 32, 32, 3)    8 x 4 tiles
  (4, 40, 24, 2)    10 x 3 tiles
  (4, 136, 256, 1)  1088 tiles > 768: workgroups of both moments passes walk a second tile
  (4, 16, 16, 2), (4, 17, 33, 2), (4, 33, 17, 2), (4, 20, 12, 1), (3, 18, 26, 1), (2, 17, 33, 1)   match = 'lowpass': the smallest shapes at which this generator's
                    low-passed PAN keeps the restatement off the clip boundaries; ragged on either axis and on both
For match = 'lowpass' the shapes of atrous_ref.STATS_ONLY_SHAPES are compared by their statistics alone (5 - 28 % of their restatement clips)."""
import ctypes
import functools
import logging

import numpy as np
import pytest
import torch

import atrous_ref as ar
import classical_ref as cr
import stream_helpers as sh
from gpu_helpers import GUARD, assert_guards_intact, guarded_empty
from lgteun_amd import _lib, atrous, build_model, classical
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
OUTPUT_CASES = [s + (m,) for m in ar.MATCHES for s in ar.SHAPES[m]]      # C, h, w, B, match


@functools.lru_cache(maxsize=None)
def inputs(C, h, w, B):
    ms, pan = ar.make_inputs(C, h, w, B)
    ms.setflags(write=False)
    pan.setflags(write=False)
    return ms, pan


def restate(ms, pan, rule, match, outputs=True):
    """-> dict(stats [B, C + 1]; with outputs also ref float64 [B, C, 4h, 4w], e32, bar)"""
    B = ms.shape[0]
    r64 = [ar.atrous(ms[b], pan[b, 0], rule, match, return_stats=True) for b in range(B)]
    res = dict(stats=np.stack([np.concatenate([r[1], [r[2]]]) for r in r64]))
    if outputs:
        r32 = np.stack([ar.atrous(ms[b], pan[b, 0], rule, match, dtype=np.float32) for b in range(B)])
        assert r32.dtype == np.float32
        ref = np.stack([r[0] for r in r64])
        e32 = float(np.abs(r32.astype(np.float64) - ref).max())
        res.update(ref=ref, e32=e32, bar=max(8.0 * e32, FLOOR))
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def case(C, h, w, B, rule, match, outputs=True):
    """the float64 restatement of a case and its bar; computed once, never written to"""
    ms, pan = inputs(C, h, w, B)
    return restate(ms, pan, rule, match, outputs)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the cached arrays are read-only


def block(rule, match, ms, pan, out, stats, ws, nbytes, stream):
    B, C, h, w = ms.shape
    return _lib.LgAtrousArgs(ctypes.sizeof(_lib.LgAtrousArgs), atrous.RULES[rule], atrous.MATCHES[match], B, C, h, w, _ptr(ms), _ptr(pan), _ptr(out),
                             None if stats is None else _ptr(stats), _ptr(ws), nbytes, stream)


def raw_call(rule, match, ms, pan):
    """the C ABI with out, stats and the workspace inside NaN guard bands and the workspace itself filled with NaN; twice on the same workspace -> (out, stats)"""
    L = _lib.lib()
    B, C, h, w = ms.shape
    need = int(L.lg_atrous_workspace_bytes(B, C, h, w, atrous.MATCHES[match]))
    assert need > 0 and need % 8 == 0
    wbuf = torch.full((need // 8 + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    ws = wbuf[GUARD:GUARD + need // 8]
    outs = []
    for _ in range(2):
        buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')
        sbuf = torch.full((B * (C + 1) + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
        stats = sbuf[GUARD:GUARD + B * (C + 1)].view(B, C + 1)
        args = block(rule, match, ms, pan, out, stats, ws, need, _stream_ptr())
        _lib.check(L.lg_atrous(ctypes.byref(args)), 'lg_atrous')
        assert_guards_intact(buf, (rule, match))
        assert bool(torch.isnan(wbuf[:GUARD]).all()) and bool(torch.isnan(wbuf[-GUARD:]).all()), (rule, match, 'written outside the workspace')
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[-GUARD:]).all()), (rule, match, 'written outside stats')
        assert bool(torch.isfinite(out).all()), (rule, match, 'an output element is missing or not finite')
        assert bool(torch.isfinite(stats).all()), (rule, match, 'a statistic is missing or not finite')
        outs.append((out, stats))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), (rule, match, 'the second call on the same workspace differs')
    assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64)), (rule, match, 'stats of the second call differ')
    return outs[1]


@pytest.mark.parametrize('rule', ar.RULES)
@pytest.mark.parametrize('C,h,w,B,match', OUTPUT_CASES)
def test_against_the_restatement(C, h, w, B, match, rule):
    cs = case(C, h, w, B, rule, match)
    ms, pan = inputs(C, h, w, B)
    ref, bar = cs['ref'], cs['bar']
    clip_share = float(((ref <= 0) | (ref >= 1)).mean())
    assert clip_share <= 0.02, f'{clip_share:.4f} of the restatement sits on a clip boundary: saturation could hide a wrong value'
    out, stats = raw_call(rule, match, dev(ms), dev(pan))
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    rel = float(np.abs(stats.cpu().numpy() / cs['stats'] - 1.0).max())
    print(f'{rule} / {match} C={C} h={h} w={w} B={B}: error {err:.3e}, float32 restatement {cs["e32"]:.3e}, error / bar {err / bar:.3f}, '
          f'clip share {clip_share:.4f}; a and the reference deviation, largest relative difference {rel:.3e}')
    assert err <= bar, (err, bar)
    assert rel <= 1e-9, rel


@pytest.mark.parametrize('C,h,w,B', ar.STATS_ONLY_SHAPES)
def test_lowpass_statistics_where_the_outputs_clip(C, h, w, B):
    cs = case(C, h, w, B, 'atwt', 'lowpass', False)
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    for rule in ar.RULES:
        _, stats = raw_call(rule, 'lowpass', ms, pan)
        rel = float(np.abs(stats.cpu().numpy() / cs['stats'] - 1.0).max())
        print(f'{rule} / lowpass C={C} h={h} w={w} B={B}: a and s_L, largest relative difference {rel:.3e}')
        assert rel <= 1e-9, rel


@pytest.mark.parametrize('C,h,w,B,match', OUTPUT_CASES)
def test_a_sample_has_the_same_bits_alone_and_in_a_batch(C, h, w, B, match):
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    ms = torch.cat([ms, ms.roll(1, dims=3)])              # 2 B samples: the shape's own and a variant of each
    pan = torch.cat([pan, pan.flip(2)])
    for rule in ar.RULES:
        out, stats = atrous.atrous(ms, pan, rule, match, return_stats=True)
        for b in range(2 * B):
            o1, s1 = atrous.atrous(ms[b:b + 1].clone(), pan[b:b + 1].clone(), rule, match, return_stats=True)      # a copy: 16-byte aligned at any C h w
            assert torch.equal(o1[0].view(torch.int32), out[b].view(torch.int32)), (rule, b)
            assert torch.equal(s1[0].view(torch.int64), stats[b].view(torch.int64)), (rule, b)


@pytest.mark.parametrize('match', ar.MATCHES)
@pytest.mark.parametrize('rule', ar.RULES)
def test_constant_pan_gives_clip_u_and_leaves_its_neighbour_alone(rule, match):
    C, h, w, B = 4, 8, 8, 2
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    pan = pan.clone()
    pan[0] = 0.3
    out, stats = raw_call(rule, match, ms, pan)
    assert bool((stats[0] == 0).all())                    # a = 0 and the reference deviation is exactly 0
    assert torch.equal(out[0].view(torch.int32), classical.interp23(ms[:1])[0].clamp(0, 1).view(torch.int32))      # exactly the clipped interpolation
    normal, nstats = raw_call(rule, match, ms[1:], pan[1:])
    assert torch.equal(normal[0].view(torch.int32), out[1].view(torch.int32)), (rule, match)
    assert torch.equal(nstats[0].view(torch.int64), stats[1].view(torch.int64)), (rule, match)
    assert bool((stats[1] > 0).all())


@pytest.mark.parametrize('match', ar.MATCHES)
@pytest.mark.parametrize('rule', ar.RULES)
def test_saturation_gives_exactly_zero_and_one(rule, match):
    C, h, w, B = ar.CLIP_SHAPE
    ms, pan = ar.make_clip_batch(C, h, w, B, seed=ar.CLIP_SEED)
    raw = np.stack([ar.atrous(ms[b], pan[b, 0], rule, match, clip=False) for b in range(B)])
    below, above = raw < -ar.CLIP_MARGIN, raw > 1 + ar.CLIP_MARGIN
    assert below.mean() >= 0.02 and above.mean() >= 0.02
    out, _ = raw_call(rule, match, dev(ms), dev(pan))
    got = out.cpu().numpy()
    print(f'{rule} / {match}, clip case: {100 * below.mean():.1f} % below 0, {100 * above.mean():.1f} % above 1')
    assert np.array_equal(got[below], np.zeros(int(below.sum()), np.float32)) and np.array_equal(got[above], np.ones(int(above.sum()), np.float32))
    assert got.min() >= 0 and got.max() <= 1


def test_functions_are_the_general_one():
    C, h, w, B = 4, 5, 7, 2
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    for match in ar.MATCHES:
        raw = {rule: raw_call(rule, match, ms, pan) for rule in ar.RULES}
        for rule, fn in (('atwt', atrous.atwt), ('awlp', atrous.awlp)):
            out, stats = fn(ms, pan, match=match, return_stats=True)
            assert torch.equal(out.view(torch.int32), raw[rule][0].view(torch.int32)) and torch.equal(stats.view(torch.int64), raw[rule][1].view(torch.int64))
            assert torch.equal(atrous.atrous(ms, pan, rule, match).view(torch.int32), out.view(torch.int32))      # without stats: the same output
        assert torch.equal(raw['atwt'][1].view(torch.int64), raw['awlp'][1].view(torch.int64))                   # the statistics do not depend on the rule
    assert torch.equal(atrous.atrous(ms, pan).view(torch.int32), atrous.awlp(ms, pan, 'pan').view(torch.int32))  # the defaults


@pytest.mark.parametrize('name,match', [('ATWT', 'lowpass'), ('AWLP', None)])
def test_runner(name, match, tmp_path):
    C, h, w, B = 4, 8, 8, 2
    rng = np.random.default_rng(5)
    peak = 2 ** 11 - .5
    batches = []
    for i in range(2):
        ms, pan = cr.make_batch(B, C, h, w, seed=40 + i)
        target = np.clip(np.stack([cr.interp23(ms[b]) for b in range(B)]) + rng.normal(0, 0.02, (B, C, 4 * h, 4 * w)), 0.02, 0.98).astype(np.float32)
        batches.append(dict(input_lr=torch.from_numpy(ms * np.float32(peak)), input_pan=torch.from_numpy(pan * np.float32(peak)),
                            target=torch.from_numpy(target * np.float32(peak)), image_id=[f'im{i}_{b}' for b in range(B)]))
    extra = {} if match is None else dict(atrous_match=match)
    cfg = Config(dict(work_dir=str(tmp_path), datas='synthetic', bit_depth=11, max_iter=10, eval_metrics='device', **extra))
    r = build_model(name, cfg, logging.getLogger('t'), None, batches, batches)
    r.set_cuda()
    rule = getattr(atrous, name).rule
    norm = [{k: (v.cuda() / peak if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    for b in norm:
        got = r.get_model_output(b)
        want = atrous.atrous(b['input_lr'], b['input_pan'], rule, match or 'pan')
        assert got.is_cuda and torch.equal(got.view(torch.int32), want.view(torch.int32))
    with_ref = r.test(iter_id=1, ref=True)
    assert list(with_ref) == ['PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS'] and all(np.isfinite(v).all() for v in with_ref.values())


@pytest.mark.parametrize('match', ar.MATCHES)
@pytest.mark.parametrize('rule', ar.RULES)
def test_whole_scene_in_one_call(rule, match):
    """atrous.fuse_scene on uint16 samples: the normalisation of scene.fuse_scene's gather, the method on the whole scene, lg_scene_to_u16"""
    C, h, w = 4, 12, 8
    ms, pan = cr.make_scene(C, h, w, seed=77)
    ms16, pan16 = np.rint(ms * 2047.5).astype(np.uint16), np.rint(pan * 2047.5).astype(np.uint16)[None]
    post = float(np.float32(1.0) / np.float32(2047.5))
    want = atrous.atrous(dev(ms16.astype(np.float32))[None] * post, dev(pan16.astype(np.float32))[None] * post, rule, match)[0]
    got = atrous.fuse_scene(rule, ms16, pan16, match=match, bit_depth=11)
    assert got.shape == (C, 4 * h, 4 * w) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    dn = atrous.fuse_scene(rule, torch.from_numpy(ms16.view(np.int16)).cuda(), torch.from_numpy(pan16.view(np.int16)).cuda(), match=match, bit_depth=11,
                           out_dtype='uint16')
    assert dn.dtype == torch.uint16
    assert np.array_equal(dn.cpu().numpy(), np.clip(np.rint(want.cpu().numpy() * np.float32(2047.5)), 0, 65535).astype(np.uint16))


@pytest.mark.parametrize('match', ar.MATCHES)
def test_entry_runs_on_the_stream_in_its_argument_block(match):
    """the compute entry has no positional stream, so tests/test_gpu_streams.py's table does not count it: its late-input case is here"""
    B, C, h, w = 2, 4, 16, 16
    c, L = sh.Case(f'lg_atrous[awlp, {match}]'), _lib.lib()
    tms, tpan = sh.classical_scene(B, C, h, w, seed=21)
    dms, dpan = sh.classical_scene(B, C, h, w, seed=22)
    ms, pan = c.inp(tms, dms), c.inp(tpan, dpan)
    out = c.out(B, C, 4 * h, 4 * w)
    stats = c.out(B, C + 1, dtype=torch.float64)
    ws, nb = c.ws(L.lg_atrous_workspace_bytes(B, C, h, w, atrous.MATCHES[match]))
    c.call = lambda s: L.lg_atrous(ctypes.byref(block('awlp', match, ms, pan, out, stats, ws, nb, s)))
    sh.check_entry_runs_on_its_stream(c)
