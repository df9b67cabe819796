"""-m gpu: the Wavelet baseline (lgteun_amd/classical.py:wavelet, k_cl_wavelet in lgteun_amd/csrc/k_classical.hip) against the float64 numpy restatement
of the explicit two-level Haar form in tests/wavelet_ref.py.

The bar is that of tests/test_gpu_classical.py: the largest absolute difference to the float64 restatement may be at most 8 x the difference of the
float32 run of the same restatement to its float64 run on that case, with a floor of 2^-23.  Measured on an MI355X over all cases below: the kernel's error
2.9e-8 - 3.0e-8 (one rounding to fp32), the float32 run's own 1.7e-7 - 3.3e-7, error / bar 0.011 - 0.022; the clip case: bar 3.2e-6, error off the clipped elements 3.0e-8.

The kernel works on tiles of 8 x 64 blocks of 4 x 4 output pixels (32 x 256 of the output, 8 x 64 of ms); a workgroup has ONE tile and does not walk.
Which shape covers what:
  (4, 4, 4, 1)      the 17 taps over 4 samples: the halo wraps five times; one ragged tile
  (4, 8, 8, 2)      one tile, its 8 block rows full
  (4, 5, 7, 2)      sides off every grid
  (8, 12, 8, 3)     C = 8; two tiles in y, the second ragged
  (8, 32, 32, 3)    four full tiles in y
  (4, 40, 24, 2)    five tiles in y
  (4, 136, 256, 1)  17 x 4 tiles: the smallest of test_gpu_classical's shapes with more than one tile in x
  (4, 9, 72, 1)     this kernel's own: 2 x 2 tiles, the second ragged in y (1 of 8 block rows) AND in x (8 of 64 lanes), and w > 64 is no multiple of 64"""
import functools
import logging

import numpy as np
import pytest
import torch

import classical_ref as cr
import wavelet_ref as wr
from gpu_helpers import assert_guards_intact, guarded_empty
from lgteun_amd import _lib, build_model, classical, device_metrics
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

SHAPES = wr.SHAPES + [(4, 9, 72, 1)]
FLOOR = 2.0 ** -23


def _frozen(res):
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def _reference(ms, pan):
    """the float64 explicit form [B, C, 4h, 4w], the error of its float32 run and the bar"""
    B = ms.shape[0]
    r64 = np.stack([wr.wavelet(ms[b], pan[b, 0], np.float64) for b in range(B)])
    r32 = np.stack([wr.wavelet(ms[b], pan[b, 0], np.float32) for b in range(B)])
    assert r32.dtype == np.float32
    e32 = float(np.abs(r32.astype(np.float64) - r64).max())
    return dict(ms=ms, pan=pan, ref=r64, e32=e32, bar=max(8.0 * e32, FLOOR))


@functools.lru_cache(maxsize=None)
def case(C, h, w, B):
    """computed once, never written to"""
    return _frozen(_reference(*wr.make_batch(C, h, w, B)))


@functools.lru_cache(maxsize=None)
def clip_case(C, h, w, B):
    ms, pan = wr.make_clip_batch(C, h, w, B)
    res = _reference(ms, pan)
    res['raw'] = np.stack([wr.wavelet_closed_form(ms[b], pan[b, 0]) for b in range(B)])      # float64, unclipped
    return _frozen(res)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the cached arrays are read-only


def raw_call(ms, pan):
    """the C ABI with the output inside NaN guard bands, twice; the inputs keep their bits"""
    L = _lib.lib()
    B, C, h, w = ms.shape
    ms0, pan0 = ms.clone(), pan.clone()
    outs = []
    for _ in range(2):
        buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')
        _lib.check(L.lg_wavelet(_ptr(ms), _ptr(pan), _ptr(out), B, C, h, w, _stream_ptr()), 'lg_wavelet')
        assert_guards_intact(buf, 'wavelet')
        assert bool(torch.isfinite(out).all()), 'an output element is missing or not finite'
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), 'the second call differs'
    assert torch.equal(ms.view(torch.int32), ms0.view(torch.int32)) and torch.equal(pan.view(torch.int32), pan0.view(torch.int32)), 'an input was written'
    return outs[1]


@pytest.mark.parametrize('C,h,w,B', SHAPES)
def test_against_the_restatement(C, h, w, B):
    cs = case(C, h, w, B)
    ref, bar = cs['ref'], cs['bar']
    clip_share = float(((ref <= 0) | (ref >= 1)).mean())
    assert clip_share <= 0.02, f'{clip_share:.4f} of the restatement sits on a clip boundary: saturation could hide a wrong value'
    out = raw_call(dev(cs['ms']), dev(cs['pan']))
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print(f'wavelet C={C} h={h} w={w} B={B}: error {err:.3e}, float32 restatement {cs["e32"]:.3e}, error / bar {err / bar:.3f}, clip share {clip_share:.4f}')
    assert err <= bar, (err, bar)


@pytest.mark.parametrize('C,h,w,B', SHAPES)
def test_a_sample_has_the_same_bits_alone_and_in_a_batch(C, h, w, B):
    cs = case(C, h, w, B)
    ms, pan = dev(cs['ms']), dev(cs['pan'])
    ms = torch.cat([ms, ms.roll(1, dims=3)])              # 2 B samples: the shape's own and a variant of each
    pan = torch.cat([pan, pan.flip(2)])
    out = classical.wavelet(ms, pan)
    for b in range(2 * B):
        alone = classical.wavelet(ms[b:b + 1], pan[b:b + 1])
        assert torch.equal(alone[0].view(torch.int32), out[b].view(torch.int32)), b


@pytest.mark.parametrize('C,h,w,B', wr.CLIP_SHAPES)
def test_clip_case(C, h, w, B):
    cs = clip_case(C, h, w, B)
    raw, bar = cs['raw'], cs['bar']
    out = raw_call(dev(cs['ms']), dev(cs['pan'])).cpu().numpy()
    below, above = raw < -bar, raw > 1 + bar
    print(f'wavelet clip case C={C} h={h} w={w} B={B}: bar {bar:.3e}, {100 * below.mean():.1f} % below, {100 * above.mean():.1f} % above, '
          f'error elsewhere {np.abs(out.astype(np.float64) - np.clip(raw, 0, 1))[~below & ~above].max():.3e}')
    assert below.mean() >= 0.01 and above.mean() >= 0.05
    assert np.all(out[below] == 0.0) and np.all(out[above] == 1.0)
    assert np.abs(out.astype(np.float64) - np.clip(raw, 0, 1))[~below & ~above].max() <= bar
    assert np.abs(out.astype(np.float64) - cs['ref']).max() <= bar


def test_runner(tmp_path):
    C, h, w, B = 4, 8, 8, 2
    rng = np.random.default_rng(5)
    peak = 2 ** 11 - .5
    batches = []
    for i in range(2):
        ms, pan = cr.make_batch(B, C, h, w, seed=40 + i)
        target = np.clip(np.stack([cr.interp23(ms[b]) for b in range(B)]) + rng.normal(0, 0.02, (B, C, 4 * h, 4 * w)), 0.02, 0.98).astype(np.float32)
        batches.append(dict(input_lr=torch.from_numpy(ms * np.float32(peak)), input_pan=torch.from_numpy(pan * np.float32(peak)),
                            target=torch.from_numpy(target * np.float32(peak)), image_id=[f'im{i}_{b}' for b in range(B)]))

    def runner(metrics_on):
        cfg = Config(dict(work_dir=str(tmp_path / metrics_on), datas='synthetic', bit_depth=11, model_type='Wavelet', max_iter=0,
                          eval_metrics=metrics_on))
        r = build_model(cfg.model_type, cfg, logging.getLogger('t'), None, batches, batches)
        r.set_cuda()
        return r
    r = runner('device')
    norm = [{k: (v.cuda() / peak if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    fused = [classical.wavelet(b['input_lr'], b['input_pan']) for b in norm]
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


def test_whole_scene_in_one_call():
    """classical.fuse_scene on uint16 samples of a scene whose sides (PAN 148 x 88) are multiples of 4 and of nothing larger: the normalisation of
    scene.fuse_scene's gather, the method on the whole scene, lg_scene_to_u16 -- against the restatement on the same normalised samples"""
    C, h, w = 4, 37, 22
    ms, pan = cr.make_scene(C, h, w, seed=77)
    ms16, pan16 = np.rint(ms * 2047.5).astype(np.uint16), np.rint(pan * 2047.5).astype(np.uint16)[None]
    post = np.float32(1.0) / np.float32(2047.5)
    ms_n, pan_n = ms16.astype(np.float32) * post, pan16.astype(np.float32) * post
    ref = wr.wavelet(ms_n, pan_n[0])
    e32 = float(np.abs(wr.wavelet(ms_n, pan_n[0], np.float32).astype(np.float64) - ref).max())
    bar = max(8.0 * e32, FLOOR)
    got = classical.fuse_scene('wavelet', ms16, pan16, bit_depth=11)
    assert got.shape == (C, 4 * h, 4 * w) and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f'wavelet scene C={C} h={h} w={w}: error {err:.3e}, bar {bar:.3e}')
    assert err <= bar
    want = classical.wavelet(dev(ms_n)[None], dev(pan_n)[None])[0]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    dn = classical.fuse_scene('wavelet', torch.from_numpy(ms16.view(np.int16)).cuda(), torch.from_numpy(pan16.view(np.int16)).cuda(), bit_depth=11,
                              out_dtype='uint16')
    assert dn.dtype == torch.uint16 and dn.shape == (C, 4 * h, 4 * w)
    dn = dn.cpu().numpy().astype(np.float64)
    assert np.array_equal(dn, np.clip(np.rint(want.cpu().numpy() * np.float32(2047.5)), 0, 65535))
    # against the restatement: a digital number is rint(x * 2047.5); x is within bar of ref, so dn is within bar * 2047.5 + 0.5 (+ the fp32 product's rounding) of ref * 2047.5
    assert np.abs(dn - ref * 2047.5).max() <= 0.5 + 2047.5 * bar + 2047.5 * 2.0 ** -24
