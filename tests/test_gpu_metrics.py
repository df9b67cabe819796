"""-m gpu: the device evaluation indices (lgteun_amd/device_metrics.py, kernels in lgteun_amd/csrc/k_iqa.hip) against the host definitions
of lgteun_amd/metrics.py, which they reproduce in fp64 up to the order of summation; their determinism, batch independence and argument
checks; and the runner's cfg.eval_metrics = 'device' evaluation against its default host evaluation."""
import ctypes
import filecmp
import logging
import os

import numpy as np
import pytest
import torch

import lgteun_amd
from lgteun_amd import _lib
from lgteun_amd import device_metrics as dmt
from lgteun_amd import metrics as mtc
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr
from oracle import detweights as dw

pytestmark = pytest.mark.gpu
T = torch.from_numpy
PEAK = 2047.5
SAM_ABS = 5e-8      # arccos near 0: one ulp of a cosine near 1 is 1.5e-8 rad, so the order of the band products shows at that level


def host_np(t, scale=1.0):
    """what the runner's host path hands to metrics.py: the tensor scaled in fp32 on the device, as [b, h, w, c] numpy"""
    return (t * scale if scale != 1.0 else t).permute(0, 2, 3, 1).cpu().numpy()


def assert_close(got, want, what, sam_col=None):
    for k, (g, w) in enumerate(zip(got, want)):
        if np.isinf(w) or np.isinf(g):
            assert g == w, (what, k, g, w)
        elif k == sam_col:
            assert abs(g - w) <= SAM_ABS, (what, k, g, w)
        else:
            assert abs(g - w) <= 1e-9 * max(1.0, abs(w)), (what, k, g, w, g - w)


def check_ref(pred, gt, scale=1.0):
    got = dmt.ref_evaluate_batch(pred, gt, scale)
    assert got.dtype == torch.float64 and got.shape == (pred.shape[0], 5) and got.device == pred.device
    got = got.cpu().numpy()
    p, g = host_np(pred, scale), host_np(gt, scale)
    for i in range(p.shape[0]):
        assert_close(got[i], mtc.ref_evaluate(p[i], g[i]), f'image {i}', sam_col=3)
    return got


def check_no_ref(pred, pan, ms, scale=1.0):
    got = dmt.no_ref_evaluate_batch(pred, pan, ms, scale)
    assert got.dtype == torch.float64 and got.shape == (pred.shape[0], 3)
    got = got.cpu().numpy()
    p, pn, m = host_np(pred, scale), host_np(pan, scale), host_np(ms, scale)
    for i in range(p.shape[0]):
        assert_close(got[i], mtc.no_ref_evaluate(p[i], pn[i], m[i]), f'image {i}')
    return got


def fused_like(gt, seed, amp=0.02):
    """a stand-in for a fused image: the target plus a smooth-ish error"""
    rng = np.random.default_rng(seed)
    return np.clip(gt + amp * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('B,h,w', [(32, 32, 32), (2, 64, 64), (2, 52, 44), (3, 4, 4)])
def test_reduced_resolution_parity_on_network_output(C, B, h, w):
    """PAN 128^2 (B 32), 256^2, 208 x 176 and 16 x 16 (the smallest model size: 6 x 6 SSIM windows), K = 2, scale 2047.5"""
    from gpu_helpers import make_module
    net = make_module(C, K=2)
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(B, C, h, w, seed=40 + h + C, kind='smooth'))
    with torch.no_grad():
        out = net(ms, pan)
    rows = check_ref(out, gt, PEAK)
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 1] < 1.0) and np.all(rows[:, 3] > 0.0)


def test_reduced_resolution_edge_cases():
    H = W = 48
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (900 + 500 * np.sin(yy / 7.0) * np.cos(xx / 5.0))[None, None] + 80 * np.arange(4)[None, :, None, None]
    img = np.clip(base + rng.normal(0, 60, (1, 4, H, W)), 0, 2047).astype(np.float32)
    a = T(img).cuda()
    # identical images: the bounds tests/test_metrics_cpu.py holds the host to
    r = dmt.ref_evaluate_batch(a, a.clone()).cpu().numpy()[0]
    assert r[0] == np.inf and abs(r[1] - 1) <= 1e-12 and abs(r[2] - 1) <= 1e-10 and r[3] < 1e-7 and r[4] == 0.0, r
    check_ref(a, a.clone())
    # constant regions at 1234.567 and at fp32(0.99987 * 2047.5): flat windows must take the host's branch of Q
    top = np.float32(0.99987 * 2047.5)
    p, g = img.copy(), np.clip(img + rng.normal(0, 30, img.shape), 0, 2047).astype(np.float32)
    for x in (p, g):
        x[..., :20, :24] = np.float32(1234.567)
        x[..., 28:, 30:] = top
    check_ref(T(p).cuda(), T(g).cuda())
    # all-zero images; an image that is constant everywhere gives Q exactly 1, as on the host
    z = torch.zeros(1, 4, H, W, device='cuda')
    check_ref(z, z.clone())
    for v in (np.float32(1234.567), top):          # long rows and columns: direct window sums do not drift along them
        c = torch.full((1, 4, 1024, 48), float(v), device='cuda')
        r = check_ref(c, c.clone())
        assert np.all(r[:, 2] == 1.0)
        c = torch.full((1, 4, 48, 1024), float(v), device='cuda')
        r = check_ref(c, c.clone())
        assert np.all(r[:, 2] == 1.0) and mtc.qindex(host_np(c)[0], host_np(c)[0]) == 1.0
    # pixel vectors with negative dot products: the clip of the cosine to [0, 1]
    q = img.copy()
    q[:, 1:] *= -1.0
    r = check_ref(T(q).cuda(), a)
    assert r[0, 3] > 1.0


@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('H,W', [(128, 128), (256, 256), (400, 400), (208, 176)])
def test_no_reference_parity(C, H, W):
    B = 1 if H == 400 else 2
    ms, pan, gt = dw.make_inputs(B, C, H // 4, W // 4, seed=H + W + C, kind='smooth')
    check_no_ref(T(fused_like(gt, H + C)).cuda(), T(pan).cuda(), T(ms).cuda(), PEAK)


def test_no_reference_parity_with_clamped_ms_window():
    """64^2: the MS image is 16 x 16, so its Q window is clamped to 16 x 16 (metrics.d_lambda / d_s: min(block, min(shape)))"""
    ms, pan, gt = dw.make_inputs(2, 4, 16, 16, seed=11, kind='smooth')
    check_no_ref(T(fused_like(gt, 5)).cuda(), T(pan).cuda(), T(ms).cuda(), PEAK)


def test_scale_determinism_and_batch_independence():
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(32, 4, 32, 32, seed=9, kind='smooth'))
    pred = T(fused_like(gt.cpu().numpy(), 9)).cuda()
    a = dmt.ref_evaluate_batch(pred, gt, PEAK)
    assert torch.equal(a, dmt.ref_evaluate_batch((pred * PEAK).contiguous(), (gt * PEAK).contiguous(), 1.0))   # scale: bit-identical
    assert torch.equal(a, dmt.ref_evaluate_batch(pred, gt, PEAK))                                              # determinism
    for i in range(32):                                                                                       # batch independence
        assert torch.equal(a[i:i + 1], dmt.ref_evaluate_batch(pred[i:i + 1].contiguous(), gt[i:i + 1].contiguous(), PEAK)), i
    n = dmt.no_ref_evaluate_batch(pred[:4].contiguous(), pan[:4].contiguous(), ms[:4].contiguous(), PEAK)
    assert torch.equal(n, dmt.no_ref_evaluate_batch((pred[:4] * PEAK).contiguous(), (pan[:4] * PEAK).contiguous(),
                                                    (ms[:4] * PEAK).contiguous(), 1.0))
    assert torch.equal(n, dmt.no_ref_evaluate_batch(pred[:4].contiguous(), pan[:4].contiguous(), ms[:4].contiguous(), PEAK))
    for i in range(4):
        assert torch.equal(n[i:i + 1], dmt.no_ref_evaluate_batch(pred[i:i + 1].contiguous(), pan[i:i + 1].contiguous(),
                                                                 ms[i:i + 1].contiguous(), PEAK)), i


def test_rejections_raise_and_launch_nothing():
    L = _lib.lib()
    cu = lambda *s: torch.rand(*s, device='cuda')   # noqa: E731
    with pytest.raises(_lib.LgteunHipError, match='C must be'):
        dmt.ref_evaluate_batch(cu(1, 1, 32, 32), cu(1, 1, 32, 32))
    with pytest.raises(_lib.LgteunHipError, match='C must be'):
        dmt.ref_evaluate_batch(cu(1, 17, 32, 32), cu(1, 17, 32, 32))
    with pytest.raises(_lib.LgteunHipError, match='SSIM window'):
        dmt.ref_evaluate_batch(cu(1, 4, 10, 32), cu(1, 4, 10, 32))
    with pytest.raises(_lib.LgteunHipError, match='no-reference'):
        dmt.no_ref_evaluate_batch(cu(1, 4, 28, 28), cu(1, 1, 28, 28), cu(1, 4, 7, 7))
    with pytest.raises(_lib.LgteunHipError, match='no-reference'):
        dmt.no_ref_evaluate_batch(cu(1, 4, 34, 32), cu(1, 1, 34, 32), cu(1, 4, 8, 8))
    with pytest.raises(ValueError):
        dmt.no_ref_evaluate_batch(cu(1, 4, 32, 32), cu(1, 1, 32, 32), cu(1, 4, 16, 16))
    with pytest.raises(ValueError):
        dmt.ref_evaluate_batch(cu(1, 4, 32, 32).double(), cu(1, 4, 32, 32).double())
    # through the C ABI with real buffers: a rejected call leaves the output untouched
    pred, gt = cu(2, 4, 32, 32), cu(2, 4, 32, 32)
    out = torch.full((2, 5), -7.0, dtype=torch.float64, device='cuda')
    need = L.lg_iqa_workspace_bytes(2, 4, 32, 32, 0)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    null = ctypes.c_void_p(0)
    for args in ((_ptr(pred), _ptr(gt), _ptr(out), 2, 4, 32, 32, 1.0, _ptr(ws), need - 1),
                 (_ptr(pred), null, _ptr(out), 2, 4, 32, 32, 1.0, _ptr(ws), need),
                 (_ptr(pred), _ptr(gt), _ptr(out), 2, 1, 32, 32, 1.0, _ptr(ws), need)):
        assert L.lg_iqa_ref(*args, _stream_ptr()) < 0
    torch.cuda.synchronize()
    assert torch.all(out == -7.0)
    assert L.lg_iqa_ref(_ptr(pred), _ptr(gt), _ptr(out), 2, 4, 32, 32, 1.0, _ptr(ws), need, _stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.all(out != -7.0)


def test_runner_device_evaluation_matches_host(tmp_path, monkeypatch):
    """UnlgFormer built as in test_runner_train_eval_save_load_roundtrip, 128^2 C = 4 loaders: cfg.eval_metrics = 'device' gives the
    default mode's results and writes the same TIFFs, and never calls the host functions"""
    def batch(i):
        ms, pan, gt = dw.make_inputs(2, 4, 32, 32, seed=200 + i, kind='smooth')
        return dict(input_lr=T(ms) * 2047.5, input_pan=T(pan) * 2047.5, target=T(gt) * 2047.5, image_id=[f'a{i}', f'b{i}'])
    loader = [batch(i) for i in range(3)]
    cfg = Config(dict(ms_chans=4, work_dir=str(tmp_path), datas='GF-2', cuda=True, max_iter=6, bit_depth=11, norm_input=True,
                      save_freq=3, eval_freq=-1, test_freq=-1, loss_cfg={'rec_loss': dict(type='l1', w=1.)},
                      optim_cfg={'core_module': dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3)},
                      sched_cfg=dict(step_size=2, gamma=0.85), model_cfg={'core_module': dict(stage=2)}))
    torch.manual_seed(1)
    runner = lgteun_amd.build_model('UnlgFormer', cfg, logging.getLogger('runner'), loader, loader, loader)
    runner.set_cuda()
    host_ref = runner.test(iter_id=1, ref=True)
    host_full = runner.test(iter_id=1, ref=False, save=True)
    runner.cfg.eval_metrics = 'device'

    def no_host(*a, **k):
        raise AssertionError('the host metrics ran in device mode')
    monkeypatch.setattr(mtc, 'ref_evaluate', no_host)
    monkeypatch.setattr(mtc, 'no_ref_evaluate', no_host)
    dev_ref = runner.test(iter_id=2, ref=True)
    dev_full = runner.test(iter_id=2, ref=False, save=True)
    for host, dev in ((host_ref, dev_ref), (host_full, dev_full)):
        assert set(host) == set(dev) and host
        for name in host:
            for h, d in zip(host[name], dev[name]):
                assert abs(h - d) <= 1e-9 * max(1.0, abs(h)), (name, h, d)
    for key, vals in runner.eval_results.items():
        assert len(vals) == 2 and vals[0] == vals[1], (key, vals)
    d1, d2 = tmp_path / 'GF-2' / 'test_out0' / 'iter_1', tmp_path / 'GF-2' / 'test_out0' / 'iter_2'
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) and len(names) == 6
    assert all(filecmp.cmp(d1 / n, d2 / n, shallow=False) for n in names)
