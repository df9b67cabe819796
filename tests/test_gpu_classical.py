"""-m gpu: the classical baselines (lgteun_amd/classical.py, lgteun_amd/csrc/k_classical.hip) against the float64 numpy restatement in
tests/classical_ref.py.

The bar of an output tensor is that of tests/test_gpu_forward_shapes.py: its largest absolute difference to the float64 restatement may be
at most 8 x the difference of the float32 run of the same restatement to its float64 run on that case, with a floor of 2^-23.  Measured on an
MI355X, error / bar over all cases below: interp23 0.039 - 0.054, sfim 0.009 - 0.041, gsa 0.023 - 0.066 (the kernels' error is 1.5e-8 to 3.0e-8, one
rounding to fp32; the float32 run's own error is 0.4e-7 to 4.0e-7); alpha and g agree to 1.8e-14 - 4.6e-11 relative.

The kernels work on 16 x 32 tiles of the output; the moments pass runs min(tiles, 768) workgroups per sample at C = 4
(512 at C = 8).  Which shape covers what:
  (4, 4, 4, 1)      one ragged tile (16 x 16): the level-1 plane is 8 wide, the 23 taps wrap three times
  (4, 8, 8, 2)      two full tiles
  (4, 5, 7, 2)      two ragged tiles (20 x 28), sides off every power-of-two grid
  (8, 12, 8, 3)     three tiles, C = 8
  (8, 32, 32, 3)    8 x 4 tiles, C = 8: 32 workgroups per sample in the moments pass
  (4, 40, 24, 2)    10 x 3 tiles
  (4, 136, 256, 1)  34 x 32 = 1088 tiles > 768: the first 320 workgroups of the moments pass walk two tiles each"""
import functools
import logging

import numpy as np
import pytest
import torch

import classical_ref as cr
from gpu_helpers import GUARD, assert_guards_intact, guarded_empty
from lgteun_amd import _lib, build_model, classical, device_metrics
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4, 4, 1), (4, 8, 8, 2), (4, 5, 7, 2), (8, 12, 8, 3), (8, 32, 32, 3), (4, 40, 24, 2), (4, 136, 256, 1)]
METHODS = ('interp23', 'sfim', 'gsa')
FLOOR = 2.0 ** -23
REF = {'interp23': lambda ms, pan, dt: cr.interp23(ms, dt), 'sfim': cr.sfim, 'gsa': cr.gsa}


@functools.lru_cache(maxsize=None)
def case(C, h, w, B):
    """the inputs of a shape and, per method, the float64 restatement [B, C, 4h, 4w] and the bar; computed once, never written to"""
    ms, pan = cr.make_batch(B, C, h, w, seed=C * 100 + h)
    res = dict(ms=ms, pan=pan)
    for m in METHODS:
        r64 = np.stack([REF[m](ms[b], pan[b, 0], np.float64) for b in range(B)])
        r32 = np.stack([REF[m](ms[b], pan[b, 0], np.float32) for b in range(B)])
        assert r32.dtype == np.float32
        e32 = float(np.abs(r32.astype(np.float64) - r64).max())
        res[m] = dict(ref=r64, e32=e32, bar=max(8.0 * e32, FLOOR))
    res['stats'] = np.stack([np.concatenate(cr.gsa(ms[b], pan[b, 0], return_stats=True)[1:]) for b in range(B)])
    for v in res.values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return res


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the cached arrays are read-only


def raw_call(method, ms, pan):
    """the C ABI with the output inside NaN guard bands and the workspace, itself between guard bands, filled with a finite sentinel; twice on
    the same workspace.  -> (out, stats or None)"""
    L = _lib.lib()
    B, C, h, w = ms.shape
    outs = []
    need = int(L.lg_classical_workspace_bytes(B, C, h, w, _lib.LG_CLASSICAL_GSA if method == 'gsa' else _lib.LG_CLASSICAL_SFIM))
    assert need > 0 and need % 8 == 0
    wbuf = torch.full((need // 8 + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    ws = wbuf[GUARD:GUARD + need // 8]
    ws.fill_(-1.2345e300)
    for _ in range(2):
        buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')
        sbuf = torch.full((B * (2 * C + 1) + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
        stats = sbuf[GUARD:GUARD + B * (2 * C + 1)].view(B, 2 * C + 1)
        if method == 'interp23':
            rc = L.lg_interp23_up4(_ptr(ms), _ptr(out), B, C, h, w, _stream_ptr())
        elif method == 'sfim':
            rc = L.lg_sfim(_ptr(ms), _ptr(pan), _ptr(out), B, C, h, w, _ptr(ws), need, _stream_ptr())
        else:
            rc = L.lg_gsa(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats), B, C, h, w, _ptr(ws), need, _stream_ptr())
        _lib.check(rc, method)
        assert_guards_intact(buf, method)
        assert bool(torch.isnan(wbuf[:GUARD]).all()) and bool(torch.isnan(wbuf[-GUARD:]).all()), (method, 'written outside the workspace')
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[-GUARD:]).all()), (method, 'written outside stats')
        assert bool(torch.isfinite(out).all()), (method, 'an output element is missing or not finite')
        if method == 'gsa':
            assert bool(torch.isfinite(stats).all())
        outs.append((out, stats if method == 'gsa' else None))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), (method, 'the second call on the same workspace differs')
    if method == 'gsa':
        assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64))
    return outs[1]


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('C,h,w,B', SHAPES)
def test_against_the_restatement(C, h, w, B, method):
    cs = case(C, h, w, B)
    ref, bar = cs[method]['ref'], cs[method]['bar']
    clip_share = float(((ref <= 0) | (ref >= 1)).mean())
    assert clip_share <= 0.02, f'{clip_share:.4f} of the restatement sits on a clip boundary: saturation could hide a wrong value'
    out, stats = raw_call(method, dev(cs['ms']), dev(cs['pan']))
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print(f'{method} C={C} h={h} w={w} B={B}: error {err:.3e}, float32 restatement {cs[method]["e32"]:.3e}, error / bar {err / bar:.3f}, '
          f'clip share {clip_share:.4f}')
    assert err <= bar, (err, bar)
    if method == 'gsa':
        want = cs['stats']
        rel = float(np.abs(stats.cpu().numpy() / want - 1.0).max())
        print(f'gsa C={C} h={h} w={w} B={B}: alpha and g, largest relative difference {rel:.3e}')
        assert rel <= 1e-9, rel


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('C,h,w,B', SHAPES)
def test_a_sample_has_the_same_bits_alone_and_in_a_batch(C, h, w, B, method):
    cs = case(C, h, w, B)
    ms, pan = dev(cs['ms']), dev(cs['pan'])
    ms = torch.cat([ms, ms.roll(1, dims=3)])              # 2 B samples: the shape's own and a variant of each
    pan = torch.cat([pan, pan.flip(2)])
    run = {'interp23': lambda m, p: (classical.interp23(m), None), 'sfim': lambda m, p: (classical.sfim(m, p), None),
           'gsa': lambda m, p: classical.gsa(m, p, return_stats=True)}[method]
    out, stats = run(ms, pan)
    for b in range(2 * B):
        o1, s1 = run(ms[b:b + 1], pan[b:b + 1])
        assert torch.equal(o1[0].view(torch.int32), out[b].view(torch.int32)), (method, b)
        if stats is not None:
            assert torch.equal(s1[0].view(torch.int64), stats[b].view(torch.int64)), (method, b)


def test_constant_pan_gives_clip_u_and_leaves_its_neighbour_alone():
    C, h, w, B = 4, 8, 8, 2
    cs = case(C, h, w, B)
    ms, pan = dev(cs['ms']), dev(cs['pan']).clone()
    pan[0] = 0.3
    u = np.clip(cs['interp23']['ref'][0], 0, 1)
    for method in ('sfim', 'gsa'):
        out, stats = raw_call(method, ms, pan)
        assert bool(torch.isfinite(out).all())
        err = float(np.abs(out[0].cpu().numpy().astype(np.float64) - u).max())
        print(f'{method}, constant PAN: distance to clip(u) {err:.3e}, bar {cs["interp23"]["bar"]:.3e}')
        assert err <= cs['interp23']['bar']
        normal, _ = raw_call(method, ms[1:], pan[1:])
        assert torch.equal(normal[0].view(torch.int32), out[1].view(torch.int32)), method
        if method == 'gsa':
            assert bool((stats[0, :C] == 0).all()) and bool((stats[0, C + 1:] == 0).all())
            assert torch.equal(out[0], classical.interp23(ms[:1])[0].clamp(0, 1))       # g = 0: exactly the clipped interpolation


@pytest.mark.parametrize('name', ['GSA', 'SFIM'])
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
    fn = classical.gsa if name == 'GSA' else classical.sfim

    def runner(metrics_on):
        cfg = Config(dict(work_dir=str(tmp_path / metrics_on), datas='synthetic', bit_depth=11, max_iter=10, eval_metrics=metrics_on))
        r = build_model(name, cfg, logging.getLogger('t'), None, batches, batches)
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
    for key in ('PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS', 'D_lambda', 'D_s', 'QNR'):
        assert len(r.eval_results[key + '_mean']) == 1 and len(r.eval_results[key + '_std']) == 1
    rows = torch.cat([device_metrics.ref_evaluate_batch(f, b['target'].contiguous(), 1.0) for b, f in zip(norm, fused)]).cpu().numpy()
    for k, key in enumerate(with_ref):
        assert with_ref[key] == (float(rows[:, k].mean()), float(rows[:, k].std())), key
    host = runner('host').test(iter_id=1, ref=True)
    assert list(host) == list(with_ref) and all(np.isfinite(v).all() for v in host.values())


@pytest.mark.parametrize('method', ['gsa', 'sfim'])
def test_whole_scene_in_one_call(method):
    """classical.fuse_scene on uint16 samples: the normalisation of scene.fuse_scene's gather, the method on the whole scene, lg_scene_to_u16"""
    C, h, w = 4, 12, 8
    ms, pan = cr.make_scene(C, h, w, seed=77)
    ms16, pan16 = np.rint(ms * 2047.5).astype(np.uint16), np.rint(pan * 2047.5).astype(np.uint16)[None]
    post = float(np.float32(1.0) / np.float32(2047.5))
    want = (classical.gsa if method == 'gsa' else classical.sfim)(dev(ms16.astype(np.float32))[None] * post, dev(pan16.astype(np.float32))[None] * post)[0]
    got = classical.fuse_scene(method, ms16, pan16, bit_depth=11)
    assert got.shape == (C, 4 * h, 4 * w) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    dn = classical.fuse_scene(method, torch.from_numpy(ms16.view(np.int16)).cuda(), torch.from_numpy(pan16.view(np.int16)).cuda(), bit_depth=11,
                              out_dtype='uint16')
    assert dn.dtype == torch.uint16
    assert np.array_equal(dn.cpu().numpy(), np.clip(np.rint(want.cpu().numpy() * np.float32(2047.5)), 0, 65535).astype(np.uint16))
