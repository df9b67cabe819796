"""-m gpu: the component-substitution baselines IHS, Brovey, GS and PCA (lgteun_amd/cs.py, lgteun_amd/csrc/k_cs.hip) against the float64 numpy restatement in
tests/cs_ref.py, which is in the direct form (interp23 at full size, np.cov, np.linalg.eigh) and shares nothing with the kernels' MS-scale route.

The bar of an output tensor is that of tests/test_gpu_classical.py: its largest absolute difference to the float64 restatement may be at most 8 x the
difference of the float32 run of the same restatement to its float64 run on that case, with a floor of 2^-23.  `stats` (w, g, a, m_I) must agree with numpy
to 1e-9 of the largest entry of the sample's vector, GSA's gate.  The measured figures are in DESIGN.md 3.15.  The inputs are cs_ref.make_common's: bands
that share PAN's structure, so that PCA's first axis is well separated (tests/test_cs_cpu.py asserts the gap and the clip share per case).

Which shape covers what (the adjoint and the Gram pass work on 16 x 16 tiles of the MS grid, the Gram pass with at most 512 workgroups per sample; the apply
pass on 16 x 32 tiles of the output):
  (4, 4, 4, 1)      one ragged tile everywhere: t wraps four times over the 16 PAN pixels of a side, R eight times over the 4 MS pixels
  (4, 8, 8, 2)      one ragged MS tile, two full output tiles; the caller's weights, the degenerate and the saturation cases
  (4, 5, 7, 2)      sides off every power-of-two grid
  (8, 12, 8, 3)     C = 8
  (8, 32, 32, 3)    2 x 2 full MS tiles, 8 x 4 output tiles
  (4, 40, 24, 2)    3 x 2 MS tiles, ragged both ways; 10 x 3 output tiles
  (4, 136, 256, 1)  9 x 16 MS tiles; 1088 output tiles
  (3, 6, 9, 1)      an odd band count
  (16, 8, 8, 1)     the largest Jacobi, the most LDS
  (4, 264, 520, 1)  17 x 33 = 561 MS tiles > 512, ragged in both axes: the first 49 workgroups of the Gram pass walk a second tile"""
import functools
import logging

import numpy as np
import pytest
import torch

import classical_ref as cr
import cs_ref as cs
from gpu_helpers import GUARD, assert_guards_intact, guarded_empty
from lgteun_amd import _lib, build_model, device_metrics
from lgteun_amd import cs as pkg
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
SENTINEL = -1.2345e300


@functools.lru_cache(maxsize=None)
def inputs(C, h, w, B):
    ms, pan = cs.make_batch(B, C, h, w, seed=C * 100 + h)
    ms.setflags(write=False)
    pan.setflags(write=False)
    return ms, pan


def restate(ms, pan, weights=None):
    """-> {mode: dict(ref float64 [B, C, 4h, 4w], e32, bar, stats [B, 2C + 2])}; interp23 runs once per sample and dtype"""
    B = ms.shape[0]
    u64 = [cr.interp23(ms[b]) for b in range(B)]
    u32 = [cr.interp23(ms[b], np.float32) for b in range(B)]
    res = {}
    for mode in cs.MODES:
        wts = None if mode == 'pca' else weights
        r64 = [cs.fuse(ms[b], pan[b, 0], mode, wts, return_stats=True, u=u64[b]) for b in range(B)]
        r32 = np.stack([cs.fuse(ms[b], pan[b, 0], mode, wts, dtype=np.float32, u=u32[b]) for b in range(B)])
        assert r32.dtype == np.float32
        ref = np.stack([r[0] for r in r64])
        e32 = float(np.abs(r32.astype(np.float64) - ref).max())
        res[mode] = dict(ref=ref, e32=e32, bar=max(8.0 * e32, FLOOR), stats=np.stack([r[1] for r in r64]))
        for a in res[mode].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def case(C, h, w, B):
    """the float64 restatement of a shape, all four methods, and their bars; computed once, never written to"""
    return restate(*inputs(C, h, w, B))


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the cached arrays are read-only


def c_weights(weights):
    import ctypes
    return None if weights is None else (ctypes.c_double * len(weights))(*weights)


def raw_call(mode, ms, pan, weights=None):
    """the C ABI with the output and stats inside NaN guard bands and the workspace, itself between guard bands, filled with a finite sentinel; twice on the
    same workspace.  -> (out, stats)"""
    L = _lib.lib()
    B, C, h, w = ms.shape
    need = int(L.lg_cs_workspace_bytes(B, C, h, w))
    assert need > 0 and need % 8 == 0
    wbuf = torch.full((need // 8 + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    ws = wbuf[GUARD:GUARD + need // 8]
    ws.fill_(SENTINEL)
    ns = B * (2 * C + 2)
    outs = []
    for _ in range(2):
        buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')
        sbuf = torch.full((ns + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
        stats = sbuf[GUARD:GUARD + ns].view(B, 2 * C + 2)
        _lib.check(L.lg_cs(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats), c_weights(weights), pkg.MODES[mode], B, C, h, w, _ptr(ws), need, _stream_ptr()), 'lg_cs')
        assert_guards_intact(buf, mode)
        assert bool(torch.isnan(wbuf[:GUARD]).all()) and bool(torch.isnan(wbuf[-GUARD:]).all()), (mode, 'written outside the workspace')
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[-GUARD:]).all()), (mode, 'written outside stats')
        assert bool(torch.isfinite(out).all()), (mode, 'an output element is missing or not finite')
        assert bool(torch.isfinite(stats).all()), (mode, 'a statistic is missing or not finite')
        outs.append((out, stats))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), (mode, 'the second call on the same workspace differs')
    assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64)), (mode, 'stats of the second call differ')
    return outs[1]


def stats_distance(got, want):
    """per sample |difference| over the largest |entry| of the restatement's vector; the largest over the batch"""
    got = got.cpu().numpy()
    return float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())


@pytest.mark.parametrize('mode', cs.MODES)
@pytest.mark.parametrize('C,h,w,B', cs.SHAPES)
def test_against_the_restatement(C, h, w, B, mode):
    cse = case(C, h, w, B)[mode]
    ms, pan = inputs(C, h, w, B)
    ref, bar = cse['ref'], cse['bar']
    out, stats = raw_call(mode, dev(ms), dev(pan))
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    sd = stats_distance(stats, cse['stats'])
    print(f'{mode} C={C} h={h} w={w} B={B}: error {err:.3e}, float32 restatement {cse["e32"]:.3e}, error / bar {err / bar:.3f}; stats {sd:.3e}')
    assert err <= bar, (err, bar)
    assert sd <= 1e-9, sd
    if mode in ('ihs', 'brovey'):
        assert bool((stats[:, C:2 * C] == 1).all()) and bool((stats[:, :C] == 1.0 / C).all())


@pytest.mark.parametrize('mode', cs.MODES)
@pytest.mark.parametrize('C,h,w,B', cs.SHAPES)
def test_a_sample_has_the_same_bits_alone_and_in_a_batch(C, h, w, B, mode):
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    ms = torch.cat([ms, ms.roll(1, dims=3)])              # 2 B samples: the shape's own and a variant of each
    pan = torch.cat([pan, pan.flip(2)])
    out, stats = pkg.fuse(ms, pan, mode, return_stats=True)
    for b in range(2 * B):
        o1, s1 = pkg.fuse(ms[b:b + 1].clone(), pan[b:b + 1].clone(), mode, return_stats=True)      # a copy: a slice of [3, 6, 9] samples is not 16-byte aligned
        assert torch.equal(o1[0].view(torch.int32), out[b].view(torch.int32)), (mode, b)
        assert torch.equal(s1[0].view(torch.int64), stats[b].view(torch.int64)), (mode, b)


@pytest.mark.parametrize('mode', ['ihs', 'brovey', 'gs'])
def test_weights_of_the_caller(mode):
    C, h, w, B = 4, 8, 8, 2
    ms, pan = inputs(C, h, w, B)
    cse = restate(ms, pan, cs.USER_WEIGHTS)[mode]
    out, stats = raw_call(mode, dev(ms), dev(pan), cs.USER_WEIGHTS)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - cse['ref']).max())
    sd = stats_distance(stats, cse['stats'])
    print(f'{mode}, w = {cs.USER_WEIGHTS}: error {err:.3e}, error / bar {err / cse["bar"]:.3f}; stats {sd:.3e}')
    assert err <= cse['bar'] and sd <= 1e-9
    assert np.array_equal(stats[:, :C].cpu().numpy(), np.tile(np.array(cs.USER_WEIGHTS), (B, 1)))      # used as given
    assert float(np.abs(cse['ref'] - case(C, h, w, B)[mode]['ref']).max()) > 100 * cse['bar']         # the weights matter on this case
    # 1 / C each is what NULL means, bit for bit; and through the function
    none, s_none = raw_call(mode, dev(ms), dev(pan))
    quarter, s_quarter = raw_call(mode, dev(ms), dev(pan), (0.25, 0.25, 0.25, 0.25))
    assert torch.equal(none.view(torch.int32), quarter.view(torch.int32)) and torch.equal(s_none.view(torch.int64), s_quarter.view(torch.int64))
    assert torch.equal(pkg.fuse(dev(ms), dev(pan), mode, cs.USER_WEIGHTS).view(torch.int32), out.view(torch.int32))
    assert torch.equal(getattr(pkg, mode)(dev(ms), dev(pan)).view(torch.int32), none.view(torch.int32))


@pytest.mark.parametrize('what', ['constant PAN', 'constant bands'])
@pytest.mark.parametrize('mode', cs.MODES)
def test_degenerate_sample_gives_clip_u_and_leaves_its_neighbour_alone(mode, what):
    C, h, w, B = 4, 8, 8, 2
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    if what == 'constant PAN':
        pan = pan.clone()
        pan[0] = 0.3
    else:
        ms = ms.clone()
        ms[0] = torch.tensor([0.2, 0.4, 1.1, -0.1], device='cuda').view(C, 1, 1)      # two of the bands clip
    L = _lib.lib()
    u = torch.empty(1, C, 4 * h, 4 * w, device='cuda')
    _lib.check(L.lg_interp23_up4(_ptr(ms[:1].clone()), _ptr(u), 1, C, h, w, _stream_ptr()), 'lg_interp23_up4')
    out, stats = raw_call(mode, ms, pan)
    assert torch.equal(out[0].view(torch.int32), u[0].clamp(0, 1).view(torch.int32)), (mode, what)      # clip(interp23), bit for bit
    assert float(stats[0, 2 * C]) == 0 and bool((stats[0, C:2 * C] == 0).all())                         # a = 0, g = 0
    normal, nstats = raw_call(mode, ms[1:].clone(), pan[1:].clone())
    assert torch.equal(normal[0].view(torch.int32), out[1].view(torch.int32)), (mode, what)
    assert torch.equal(nstats[0].view(torch.int64), stats[1].view(torch.int64)), (mode, what)
    assert float(stats[1, 2 * C]) > 0


@pytest.mark.parametrize('mode', cs.MODES)
def test_saturation_gives_exactly_zero_and_one(mode):
    C, h, w, B = cs.CLIP_SHAPE
    ms, pan = cs.make_clip_batch(B, C, h, w, seed=9)
    raw = np.stack([cs.fuse(ms[b], pan[b, 0], mode, clip=False) for b in range(B)])
    cse = restate(ms, pan)[mode]
    below, above = raw < -cse['bar'], raw > 1 + cse['bar']
    for side in (raw < 0, raw > 1):
        assert 0.01 < side.mean() < 0.5
    out, _ = raw_call(mode, dev(ms), dev(pan))
    got = out.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - cse['ref']).max())
    print(f'{mode}, clip case: {100 * (raw < 0).mean():.1f} % below 0, {100 * (raw > 1).mean():.1f} % above 1; error {err:.3e}, error / bar {err / cse["bar"]:.3f}')
    assert np.array_equal(got[below], np.zeros(int(below.sum()), np.float32)) and np.array_equal(got[above], np.ones(int(above.sum()), np.float32))
    assert got.min() >= 0 and got.max() <= 1
    assert err <= cse['bar']


def test_rejected_calls_write_nothing():
    """each of the five kinds returns an error, names its reason and leaves a sentinel-filled output and workspace untouched"""
    import ctypes
    L = _lib.lib()
    C, h, w, B = 4, 8, 8, 2
    ms, pan = (dev(a) for a in inputs(C, h, w, B))
    need = int(L.lg_cs_workspace_bytes(B, C, h, w))
    out = torch.full((B, C, 4 * h, 4 * w), 7.25, device='cuda')
    ws = torch.full((need // 8,), SENTINEL, dtype=torch.float64, device='cuda')
    stats = torch.full((B, 2 * C + 2), SENTINEL, dtype=torch.float64, device='cuda')
    nan_w = (ctypes.c_double * C)(0.1, float('nan'), 0.4, 0.2)
    ok_w = (ctypes.c_double * C)(*cs.USER_WEIGHTS)

    def call(weights=None, mode=_lib.LG_CS_GS, C=C, h=h, ws_ptr=_ptr(ws), nbytes=need):
        return L.lg_cs(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats), weights, mode, B, C, h, w, ws_ptr, nbytes, _stream_ptr())
    for kw, text in ((dict(mode=4), 'mode must be'), (dict(weights=ok_w, mode=_lib.LG_CS_PCA), 'weights must be NULL for LG_CS_PCA'),
                     (dict(weights=nan_w), 'weights[1] must be finite'), (dict(nbytes=need - 8), 'workspace_bytes too small'),
                     (dict(ws_ptr=None), 'workspace is NULL'), (dict(C=17), 'C must be'), (dict(h=3), 'h must be')):
        assert call(**kw) < 0, text
        assert text in L.lg_last_error().decode(), (text, L.lg_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.25).all()) and bool((ws == SENTINEL).all()) and bool((stats == SENTINEL).all())
    assert call(weights=ok_w) == 0                             # ... and the same buffers are good for a call
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize('name', ['PCA', 'GS'])
def test_runner(name, tmp_path):
    C, h, w, B = 4, 8, 8, 2
    rng = np.random.default_rng(5)
    peak = 2 ** 11 - .5
    batches = []
    for i in range(2):
        ms, pan = cs.make_batch(B, C, h, w, seed=40 + i)
        target = np.clip(np.stack([cr.interp23(ms[b]) for b in range(B)]) + rng.normal(0, 0.02, (B, C, 4 * h, 4 * w)), 0.02, 0.98).astype(np.float32)
        batches.append(dict(input_lr=torch.from_numpy(ms * np.float32(peak)), input_pan=torch.from_numpy(pan * np.float32(peak)),
                            target=torch.from_numpy(target * np.float32(peak)), image_id=[f'im{i}_{b}' for b in range(B)]))
    weights = None if name == 'PCA' else list(cs.USER_WEIGHTS)
    fn = pkg.pca if name == 'PCA' else (lambda m, p: pkg.gs(m, p, weights))

    def runner(metrics_on):
        cfg = dict(work_dir=str(tmp_path / metrics_on), datas='synthetic', bit_depth=11, max_iter=10, eval_metrics=metrics_on)
        if weights is not None:
            cfg['cs_weights'] = weights
        r = build_model(name, Config(cfg), logging.getLogger('t'), None, batches, batches)
        r.set_cuda()
        return r
    r = runner('device')
    norm = [{k: (v.cuda() / peak if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    fused = [fn(b['input_lr'], b['input_pan']) for b in norm]
    for b, f in zip(norm, fused):
        got = r.get_model_output(b)
        assert got.is_cuda and torch.equal(got.view(torch.int32), f.view(torch.int32))
    with_ref = r.test(iter_id=1, ref=True)
    no_ref = r.test(iter_id=1, ref=False)
    assert list(with_ref) == ['PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS'] and list(no_ref) == ['D_lambda', 'D_s', 'QNR']
    assert all(np.isfinite(v).all() for v in list(with_ref.values()) + list(no_ref.values()))
    rows = torch.cat([device_metrics.ref_evaluate_batch(f, b['target'].contiguous(), 1.0) for b, f in zip(norm, fused)]).cpu().numpy()
    for k, key in enumerate(with_ref):
        assert with_ref[key] == (float(rows[:, k].mean()), float(rows[:, k].std())), key


@pytest.mark.parametrize('method', cs.MODES)
def test_whole_scene_in_one_call(method):
    """cs.fuse_scene on uint16 samples: the normalisation of scene.fuse_scene's gather, the method on the whole scene, lg_scene_to_u16"""
    C, h, w = 4, 36, 52
    ms, pan = cs.make_common(C, h, w, seed=77)
    ms16, pan16 = np.rint(ms * 2047.5).astype(np.uint16), np.rint(pan * 2047.5).astype(np.uint16)[None]
    post = float(np.float32(1.0) / np.float32(2047.5))
    want = pkg.fuse(dev(ms16.astype(np.float32))[None] * post, dev(pan16.astype(np.float32))[None] * post, method)[0]
    got = pkg.fuse_scene(method, ms16, pan16, bit_depth=11)
    assert got.shape == (C, 4 * h, 4 * w) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    dn = pkg.fuse_scene(method, torch.from_numpy(ms16.view(np.int16)).cuda(), torch.from_numpy(pan16.view(np.int16)).cuda(), bit_depth=11, out_dtype='uint16')
    assert dn.dtype == torch.uint16
    assert np.array_equal(dn.cpu().numpy(), np.clip(np.rint(want.cpu().numpy() * np.float32(2047.5)), 0, 65535).astype(np.uint16))
