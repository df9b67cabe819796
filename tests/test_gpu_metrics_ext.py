"""-m gpu: the extended device indices (lgteun_amd/device_metrics.py ref_evaluate_ext_batch / no_ref_evaluate_ext_batch, kernels in
lgteun_amd/csrc/k_iqa_ext.hip) against the host definitions of lgteun_amd/metrics.py (Q2n, SCC, CC, D_lambda_K, HQNR), to the bar of
tests/test_gpu_metrics.py: |got - want| <= 1e-9 max(1, |want|), NaN where the host has NaN.  Their branches on flat blocks and constant
bands, determinism, batch independence, the caller-owned buffers, the rejections, and the runner's cfg.eval_indices = 'extended' on both
eval_metrics routes."""
import ctypes
import logging

import numpy as np
import pytest
import torch

import lgteun_amd
from lgteun_amd import _lib
from lgteun_amd import device_metrics as dmt
from lgteun_amd import metrics as mtc
from lgteun_amd import wald
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr
from oracle import detweights as dw

pytestmark = pytest.mark.gpu
T = torch.from_numpy
PEAK = 2047.5
GUARD = 512        # doubles of NaN band on each side of a guarded output


def host_np(t, scale=1.0):
    """what the runner's host path hands to metrics.py: the tensor scaled in fp32 on the device, as [b, h, w, c] numpy"""
    return (t * scale if scale != 1.0 else t).permute(0, 2, 3, 1).cpu().numpy()


def assert_close(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if np.isnan(w) or np.isnan(g):
            assert np.isnan(w) and np.isnan(g), (what, k, g, w)
        else:
            assert abs(g - w) <= 1e-9 * max(1.0, abs(w)), (what, k, g, w, g - w)


def host_ext(pred, gt, scale=1.0):
    p, g = host_np(pred, scale), host_np(gt, scale)
    return [[mtc.q2n(g[i], p[i]), mtc.scc(g[i], p[i]), mtc.cc(g[i], p[i])] for i in range(p.shape[0])]


def check_ref_ext(pred, gt, scale=1.0):
    """the three new columns against the host, the first five against ref_evaluate_batch bit for bit -> the [B, 8] rows as numpy"""
    got = dmt.ref_evaluate_ext_batch(pred, gt, scale)
    assert got.dtype == torch.float64 and got.shape == (pred.shape[0], 8) and got.device == pred.device
    assert torch.equal(got[:, :5].contiguous().view(torch.int64), dmt.ref_evaluate_batch(pred, gt, scale).view(torch.int64))
    rows = got.cpu().numpy()
    for i, want in enumerate(host_ext(pred, gt, scale)):
        print(f'image {i}: device {rows[i, 5:].tolist()} host {want}')
        assert_close(rows[i, 5:], want, f'image {i}')
    return rows


def fused_like(gt, seed, amp=0.02):
    """a stand-in for a fused image: the target plus an error"""
    rng = np.random.default_rng(seed)
    return np.clip(gt + amp * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)


def raw_ref_ext(pred, gt, scale, out, ws, nbytes, B=None, C=None, H=None, W=None):
    b, c, h, w = pred.shape
    return _lib.lib().lg_iqa_ref_ext(_ptr(pred), _ptr(gt), _ptr(out), B or b, C or c, H or h, W or w, scale, _ptr(ws), nbytes, _stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------------------
# reduced resolution
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,H,W', [(3, 4, 32, 32),      # one block
                                     (2, 8, 48, 80),      # extension on both axes, octonions
                                     (2, 3, 64, 96),      # a zero-padded band
                                     (1, 5, 40, 32),      # C padded by three, extension by 24
                                     (2, 2, 32, 64)])     # N = 2
def test_parity_determinism_batch_independence_and_buffers(B, C, H, W):
    _, _, gt = dw.make_inputs(B, C, H // 4, W // 4, seed=H + W + C, kind='smooth')
    pred, gt = T(fused_like(gt, C + H)).cuda(), T(gt).cuda()
    rows = check_ref_ext(pred, gt, PEAK)
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 5:] < 1.0) and np.all(rows[:, 5:] > 0.0)
    ext = dmt.ref_evaluate_ext_batch(pred, gt, PEAK)
    assert torch.equal(ext, dmt.ref_evaluate_ext_batch(pred, gt, PEAK))                                              # two calls: the same bits
    assert torch.equal(ext[:, 5:], dmt.ref_evaluate_ext_batch((pred * PEAK).contiguous(), (gt * PEAK).contiguous(), 1.0)[:, 5:])
    for i in range(B):                                                                                               # row b alone
        assert torch.equal(ext[i:i + 1], dmt.ref_evaluate_ext_batch(pred[i:i + 1].contiguous(), gt[i:i + 1].contiguous(), PEAK)), i
    # through the C ABI: out inside NaN guard bands, a workspace that held a sentinel
    need = _lib.lib().lg_iqa_ext_workspace_bytes(B, C, H, W)
    assert need > 0
    for fill in (0x00, 0xFF, 0x5A):
        buf = torch.full((3 * B + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
        out = buf[GUARD:GUARD + 3 * B]
        ws = torch.full((need,), fill, dtype=torch.uint8, device='cuda')
        assert raw_ref_ext(pred, gt, PEAK, out, ws, need) == 0
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), 'written outside the output'
        assert torch.equal(out.view(B, 3), ext[:, 5:]), fill


def test_parity_on_network_output():
    """(4, 4, 128, 128): a K = 2 network output against its target, scale 2047.5"""
    from gpu_helpers import make_module
    net = make_module(4, K=2)
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(4, 4, 32, 32, seed=76, kind='smooth'))
    with torch.no_grad():
        out = net(ms, pan)
    rows = check_ref_ext(out, gt, PEAK)
    assert np.all(np.isfinite(rows))


def test_edge_cases():
    H, W = 64, 96
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (900 + 500 * np.sin(yy / 7.0) * np.cos(xx / 5.0))[None, None] + 80 * np.arange(4)[None, :, None, None]
    img = np.clip(base + rng.normal(0, 60, (1, 4, H, W)), 0, 2047).astype(np.float32)
    a = T(img).cuda()
    top = np.float32(0.99987 * 2047.5)
    # identical images
    r = check_ref_ext(a, a.clone())[0]
    assert abs(r[5] - 1) <= 1e-12 and abs(r[6] - 1) <= 1e-12 and abs(r[7] - 1) <= 1e-12, r
    # all-zero images: every block takes t3 == 0, no edges in either image, every band constant
    z = torch.zeros(2, 4, 40, 48, device='cuda')
    r = check_ref_ext(z, z.clone())
    assert np.all(r[:, 5] == 1.0) and np.all(r[:, 6] == 1.0) and np.all(np.isnan(r[:, 7]))
    # flat over whole blocks in both images (t3 == 0 there), the other blocks varying
    p, g = img.copy(), np.clip(img + rng.normal(0, 30, img.shape), 0, 2047).astype(np.float32)
    for x in (p, g):
        x[..., :32, :64] = np.float32(1234.567)
        x[..., 32:, 64:] = top
    assert list(mtc.q2n_blocks(g[0].transpose(1, 2, 0), p[0].transpose(1, 2, 0))[[0, 1, 5]]) == [1.0, 1.0, 1.0]
    check_ref_ext(T(p).cuda(), T(g).cuda())
    # flat in the ground truth only: c = 1
    g = img.copy()
    g[..., :32, 32:64] = np.float32(800.0)
    g[:, 2, 32:, :32] = 0.0                                       # one band of one block
    r = check_ref_ext(a, T(g).cuda())
    assert np.all(np.isfinite(r))
    # the two constants over long planes: Q2n exactly 1 in every block, as on the host
    for v in (np.float32(1234.567), top):
        for shape in ((1, 4, 1024, 32), (1, 4, 32, 1024)):
            c = torch.full(shape, float(v), device='cuda')
            r = check_ref_ext(c, c.clone())
            assert r[0, 5] == 1.0 and r[0, 6] == 1.0 and np.isnan(r[0, 7])
            assert mtc.q2n(host_np(c)[0], host_np(c)[0]) == 1.0
    # one constant band, in the fused image or in the ground truth: CC is NaN, Q2n and SCC are not
    for which in (0, 1):
        pair = [img.copy(), np.clip(img + rng.normal(0, 30, img.shape), 0, 2047).astype(np.float32)]
        pair[which][:, 1] = np.float32(77.0)
        r = check_ref_ext(T(pair[0]).cuda(), T(pair[1]).cuda())
        assert np.isnan(r[0, 7]) and np.isfinite(r[0, 5]) and np.isfinite(r[0, 6])
    # no edges in exactly one image: SCC 0
    r = check_ref_ext(torch.full((1, 4, H, W), 500.0, device='cuda'), a)
    assert r[0, 6] == 0.0


def test_rejected_calls_leave_the_output_untouched():
    L = _lib.lib()
    cu = lambda *s: torch.rand(*s, device='cuda')   # noqa: E731
    with pytest.raises(_lib.LgteunHipError, match='C must be'):
        dmt.ref_evaluate_ext_batch(cu(1, 9, 32, 32), cu(1, 9, 32, 32))
    with pytest.raises(_lib.LgteunHipError, match='Q2n block'):
        dmt.ref_evaluate_ext_batch(cu(1, 4, 31, 32), cu(1, 4, 31, 32))
    with pytest.raises(ValueError):
        dmt.ref_evaluate_ext_batch(cu(1, 4, 32, 32), cu(1, 4, 32, 64))
    with pytest.raises(_lib.LgteunHipError, match='Q2n block'):                      # MS sides below 32
        dmt.no_ref_evaluate_ext_batch(cu(1, 4, 64, 64), cu(1, 1, 64, 64), cu(1, 4, 16, 16))
    pred, gt = cu(2, 9, 32, 32), cu(2, 9, 32, 32)                                    # large enough for every shape tried below
    out = torch.full((2, 3), -7.0, dtype=torch.float64, device='cuda')
    need = L.lg_iqa_ext_workspace_bytes(2, 4, 32, 32)
    ws = torch.empty(L.lg_iqa_ext_workspace_bytes(2, 8, 32, 32), dtype=torch.uint8, device='cuda')
    for kw, nbytes in ((dict(C=9), ws.numel()), (dict(C=4, H=31), ws.numel()), (dict(C=4), need - 1)):
        assert raw_ref_ext(pred, gt, 1.0, out, ws, nbytes, **kw) < 0, kw
        assert L.lg_iqa_q2n(_ptr(gt), _ptr(pred), _ptr(out), 2, kw['C'], kw.get('H', 32), 32, 1.0, _ptr(ws), nbytes, _stream_ptr()) < 0, kw
    torch.cuda.synchronize()
    assert torch.all(out == -7.0)
    assert raw_ref_ext(pred, gt, 1.0, out, ws, need, C=4) == 0
    torch.cuda.synchronize()
    assert torch.all(out != -7.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# full resolution
# ---------------------------------------------------------------------------------------------------------------------------------
GAINS = {4: (0.3, 0.25, 0.2, 0.35), 8: (0.35, 0.3, 0.25, 0.2, 0.3, 0.35, 0.28, 0.22)}


@pytest.mark.parametrize('caller_gains', [False, True])
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('H,W', [(128, 128), (208, 176), (400, 400)])
def test_no_reference_parity(C, H, W, caller_gains):
    B = 1 if H == 400 else 2
    gains = GAINS[C] if caller_gains else None
    ms, pan, gt = dw.make_inputs(B, C, H // 4, W // 4, seed=H + W + C, kind='smooth')
    pred, pan, ms = T(fused_like(gt, H + C)).cuda(), T(pan).cuda(), T(ms).cuda()
    got = dmt.no_ref_evaluate_ext_batch(pred, pan, ms, PEAK, gains_ms=gains)
    assert got.dtype == torch.float64 and got.shape == (B, 5)
    assert torch.equal(got[:, :3].contiguous().view(torch.int64), dmt.no_ref_evaluate_batch(pred, pan, ms, PEAK).view(torch.int64))
    assert torch.equal(got, dmt.no_ref_evaluate_ext_batch(pred, pan, ms, PEAK, gains_ms=gains))
    rows = got.cpu().numpy()
    p, pn, m = host_np(pred, PEAK), host_np(pan, PEAK), host_np(ms, PEAK)
    for i in range(B):
        dk = mtc.d_lambda_k(p[i], m[i], gains)
        want = [dk, (1.0 - dk) * (1.0 - mtc.d_s(p[i], m[i], pn[i]))]
        print(f'image {i}: device {rows[i, 3:].tolist()} host {want}')
        assert_close(rows[i, 3:], want, f'image {i}')
        assert 0.0 < dk < 1.0
    if H == 128:
        # the two sides round at the same places: the degraded image is the same fp32 bits, and a sample's row does not depend on its batch
        g = wald._gain_rows(gains, C, wald.DEFAULT_GAIN_MS, 'gains_ms')
        taps = np.stack([wald.mtf_taps(v, wald.DEFAULT_TAPS) for v in g])
        dev = wald._fir((pred[0] * PEAK).contiguous(), taps, 2, 'float32').cpu().numpy()
        assert np.array_equal(dev.transpose(1, 2, 0), mtc.mtf_degrade_ms(p[0], gains))
        assert torch.equal(got[1:2], dmt.no_ref_evaluate_ext_batch(pred[1:2].contiguous(), pan[1:2].contiguous(), ms[1:2].contiguous(), PEAK, gains_ms=gains))
        assert_close(rows[0], mtc.no_ref_evaluate_ext(p[0], pn[0], m[0], gains), 'the whole row')


# ---------------------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------------------
def loader_128(n):
    def batch(i):
        ms, pan, gt = dw.make_inputs(2, 4, 32, 32, seed=300 + i, kind='smooth')
        return dict(input_lr=T(ms) * 2047.5, input_pan=T(pan) * 2047.5, target=T(gt) * 2047.5, image_id=[f'a{i}', f'b{i}'])
    return [batch(i) for i in range(n)]


def runner_cfg(tmp_path, **kw):
    return Config(dict(ms_chans=4, work_dir=str(tmp_path), datas='GF-2', cuda=True, max_iter=6, bit_depth=11, norm_input=True,
                       save_freq=3, eval_freq=-1, test_freq=-1, loss_cfg={'rec_loss': dict(type='l1', w=1.)},
                       optim_cfg={'core_module': dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3)},
                       sched_cfg=dict(step_size=2, gamma=0.85), model_cfg={'core_module': dict(stage=2)}, **kw))


@pytest.mark.parametrize('name,extra', [('UnlgFormer', {}), ('MTF_GLP_CBD', dict(mtf_gains_ms=GAINS[4]))])
def test_runner_extended_indices_on_both_routes(name, extra, tmp_path):
    loader = loader_128(2)
    torch.manual_seed(1)
    runner = lgteun_amd.build_model(name, runner_cfg(tmp_path, **extra), logging.getLogger('runner'), loader, loader, loader)
    runner.set_cuda()
    # the default configuration: five and three columns, as before
    std_ref, std_full = runner.test(iter_id=1, ref=True), runner.test(iter_id=1, ref=False)
    assert list(std_ref) == list(dmt.REF_NAMES) and list(std_full) == list(dmt.NO_REF_NAMES)
    assert not any(k.startswith(('Q2n', 'SCC', 'CC', 'D_lambda_K', 'HQNR')) for k in runner.eval_results)
    runner.cfg.eval_indices = 'extended'
    host_ref, host_full = runner.test(iter_id=2, ref=True), runner.test(iter_id=2, ref=False)
    runner.cfg.eval_metrics = 'device'
    dev_ref, dev_full = runner.test(iter_id=3, ref=True), runner.test(iter_id=3, ref=False)
    assert list(host_ref) == list(dev_ref) == list(dmt.REF_EXT_NAMES) and list(host_full) == list(dev_full) == list(dmt.NO_REF_EXT_NAMES)
    for std, host, dev in ((std_ref, host_ref, dev_ref), (std_full, host_full, dev_full)):
        for key in std:
            assert host[key] == std[key], key                       # the standard columns do not move when the set is extended
        for key in host:
            assert np.all(np.isfinite(host[key])), key
            assert_close(dev[key], host[key], key)
    for key in ('Q2n', 'SCC', 'CC', 'D_lambda_K', 'HQNR'):
        assert len(runner.eval_results[key + '_mean']) == 2 and len(runner.eval_results[key + '_std']) == 2
    assert len(runner.eval_results['PSNR_mean']) == 3
    if extra:   # cfg.mtf_gains_ms feeds D_lambda_K: the default gains give another value
        runner.cfg.mtf_gains_ms = None
        assert runner.test(iter_id=4, ref=False)['D_lambda_K'] != dev_full['D_lambda_K']


def test_runner_names_the_limit_for_small_images(tmp_path):
    def batch():
        ms, pan, gt = dw.make_inputs(2, 4, 4, 4, seed=5, kind='smooth')
        return dict(input_lr=T(ms) * 2047.5, input_pan=T(pan) * 2047.5, target=T(gt) * 2047.5, image_id=['a', 'b'])
    loader = [batch()]
    for metrics_on in ('host', 'device'):
        cfg = Config(dict(work_dir=str(tmp_path / metrics_on), datas='synthetic', bit_depth=11, max_iter=10, norm_input=True, eval_metrics=metrics_on,
                          eval_indices='extended'))
        r = lgteun_amd.build_model('SFIM', cfg, logging.getLogger('t'), None, loader, loader)
        r.set_cuda()
        with pytest.raises(ValueError, match='at least 32 x 32'):
            r.test(iter_id=1, ref=True)
        with pytest.raises(ValueError, match='at least 128 x 128'):
            r.test(iter_id=1, ref=False)
