"""-m gpu: the classical kernels (k_classical.hip), the device metrics (k_iqa.hip, k_iqa_ext.hip) and the QNR loss kernels (k_qnr.hip) against
what the REFERENCE ITSELF computes: tests/golden/parity_*.npz, written by tools/gen_goldens.py --only-parity from the reference's own functions
over three OpenCV stand-ins.  Fixtures only; tests/test_reference_parity_cpu.py holds the host functions and the yardsticks of the other GPU
tests to the same files, and derives the D_s / QNR gates used here (its module docstring).

Bars: classical outputs as in tests/test_gpu_classical.py (8 x the float32 restatement's distance to the fixture on that case, floor 2^-23);
device metrics as tests/test_gpu_metrics.py holds device to host (1e-9 relative, SAM 5e-8 absolute, infinity equal), D_s and QNR within the
derived gates 3.6e-6 and 4.5e-8 (both above 1e-9, so nothing is added); the QNR kernels as tests/test_gpu_qnr_loss.py holds them to
qnr_helpers (indices 1e-11 relative, loss_accum one fp32 rounding, dout one fp32 rounding of the gradient plus 1e-9 of its largest entry).

Measured on an MI355X: classical kernels 1.5e-8 .. 3.0e-8 from the reference, 0.026 .. 0.066 of the bar; SSIM within 3e-15, Q within 2e-14, CC within 4e-16
of the reference's values, PSNR / SAM / ERGAS to the last digits; D_s 4.3e-7 / 1.2e-7 / 8.9e-7 and QNR 8.8e-9 / 3.0e-9 / 1.1e-8 relative (the host's
distances: the device follows the host); the loss 2e-15 relative, loss_accum 1.4e-8."""
import functools

import numpy as np
import pytest
import torch

import classical_ref as cr
import parity_inputs as pin
import test_reference_parity_cpu as host
from gpu_helpers import assert_guards_intact, guarded_empty
from lgteun_amd import _lib, classical
from lgteun_amd import device_metrics as dmt
from lgteun_amd.engine import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -23
SAM_ABS = 5e-8
METHODS = ('interp23', 'sfim', 'gsa')
RESTATE = {'interp23': lambda ms, pan, dt: cr.interp23(ms, dt), 'sfim': cr.sfim, 'gsa': cr.gsa}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nchw(hwc):
    """(H, W, C) or (H, W) host image -> [1, C, H, W] device tensor"""
    a = np.asarray(hwc)
    a = a[..., None] if a.ndim == 2 else a
    return dev(a.transpose(2, 0, 1)[None])


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('C,h,w,B', host.CLASSICAL_CASES)
def test_classical_kernels_against_the_reference(C, h, w, B, method):
    z = host.classical_gold(C, h, w, B)
    ms, pan, want = z['ms'], z['pan'], z[method]
    share = float(((want <= 0) | (want >= 1)).mean())
    assert share <= 0.02, f'{share:.4f} of the reference\'s output sits on a clip boundary: saturation could hide a wrong value'
    r32 = np.stack([RESTATE[method](ms[b], pan[b, 0], np.float32) for b in range(B)])
    assert r32.dtype == np.float32
    e32 = float(np.abs(r32.astype(np.float64) - want).max())
    bar = max(8.0 * e32, FLOOR)
    L = _lib.lib()
    buf, out = guarded_empty((B, C, 4 * h, 4 * w), 'cuda')
    d_ms, d_pan = dev(ms), dev(pan)
    if method == 'interp23':
        rc = L.lg_interp23_up4(_ptr(d_ms), _ptr(out), B, C, h, w, _stream_ptr())
    else:
        code = _lib.LG_CLASSICAL_GSA if method == 'gsa' else _lib.LG_CLASSICAL_SFIM
        need = int(L.lg_classical_workspace_bytes(B, C, h, w, code))
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        if method == 'sfim':
            rc = L.lg_sfim(_ptr(d_ms), _ptr(d_pan), _ptr(out), B, C, h, w, _ptr(ws), need, _stream_ptr())
        else:
            rc = L.lg_gsa(_ptr(d_ms), _ptr(d_pan), _ptr(out), None, B, C, h, w, _ptr(ws), need, _stream_ptr())
    _lib.check(rc, method)
    assert_guards_intact(buf, method)
    assert bool(torch.isfinite(out).all()), (method, 'an output element is missing or not finite')
    fn = {'interp23': lambda: classical.interp23(d_ms), 'sfim': lambda: classical.sfim(d_ms, d_pan), 'gsa': lambda: classical.gsa(d_ms, d_pan)}[method]
    assert torch.equal(fn().view(torch.int32), out.view(torch.int32)), (method, 'the Python entry and the C ABI differ')
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    print(f'{method} C={C} h={h} w={w} B={B}: error against the reference {err:.3e}, float32 restatement {e32:.3e}, error / bar {err / bar:.3f}, '
          f'clip share {share:.4f}')
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------------------------
def assert_rows_close(got, want, what, sam_col=None, gates=None):
    for k, (g, w_) in enumerate(zip(got, want)):
        print(f'{what} column {k}: {g!r} against {w_!r}')
        if np.isinf(w_) or np.isinf(g):
            assert g == w_, (what, k, g, w_)
        elif k == sam_col:
            assert abs(g - w_) <= SAM_ABS, (what, k, g, w_)
        elif gates and k in gates:
            assert abs(g - w_) <= gates[k] * abs(w_), (what, k, g, w_, abs(g - w_) / abs(w_))
        else:
            assert abs(g - w_) <= 1e-9 * max(1.0, abs(w_)), (what, k, g, w_, g - w_)


@functools.lru_cache(maxsize=None)
def ref_pairs():
    z = host.gold('parity_metrics_ref')
    return {n: (z[n + '/pred'], z[n + '/gt']) for n in host.REF_CASES}


def ref_partner(name):
    """another case of the same shape, or (none left) the case's own pair with its images exchanged"""
    pairs = ref_pairs()
    same = [n for n in host.REF_CASES if n != name and pairs[n][0].shape == pairs[name][0].shape]
    return pairs[same[0]] if same else pairs[name][::-1]


@pytest.mark.parametrize('name', host.REF_CASES)
def test_device_reference_based_indices_against_the_reference(name):
    z = host.gold('parity_metrics_ref')
    pred, gt = ref_pairs()[name]
    p2, g2 = ref_partner(name)
    alone = dmt.ref_evaluate_batch(nchw(pred), nchw(gt))
    both = dmt.ref_evaluate_batch(torch.cat([nchw(p2), nchw(pred)]), torch.cat([nchw(g2), nchw(gt)]))
    assert torch.equal(alone[0].view(torch.int64), both[1].view(torch.int64)), 'the row differs inside a batch'
    assert_rows_close(alone[0].cpu().numpy(), z[name + '/ref_evaluate'], name, sam_col=3)
    if min(pred.shape[:2]) >= 32:          # the extended set is defined from one 32 x 32 Q2n block upwards: min16_c4 has no CC column
        ext1 = dmt.ref_evaluate_ext_batch(nchw(pred), nchw(gt))
        ext2 = dmt.ref_evaluate_ext_batch(torch.cat([nchw(p2), nchw(pred)]), torch.cat([nchw(g2), nchw(gt)]))
        assert torch.equal(ext1[0].view(torch.int64), ext2[1].view(torch.int64)), 'the extended row differs inside a batch'
        assert_rows_close([float(ext1[0, 7])], [float(z[name + '/scc'])], name + ' CC')
    else:
        assert name == 'min16_c4'


@pytest.mark.parametrize('name', list(pin.NOREF_CASES))
def test_device_no_reference_indices_against_the_reference(name):
    want = host.gold('parity_metrics_noref')[name + '/no_ref_evaluate']
    pred, pan, ms = (nchw(a) for a in host.noref_inputs(name))
    alone = dmt.no_ref_evaluate_batch(pred, pan, ms)
    flip = lambda t: t.flip(2).contiguous()      # noqa: E731  (the cases differ in shape: the partner is the case upside down)
    both = dmt.no_ref_evaluate_batch(torch.cat([flip(pred), pred]), torch.cat([flip(pan), pan]), torch.cat([flip(ms), ms]))
    assert torch.equal(alone[0].view(torch.int64), both[1].view(torch.int64)), 'the row differs inside a batch'
    assert_rows_close(alone[0].cpu().numpy(), want, name, gates={1: host.D_S_GATE, 2: host.QNR_GATE})


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', host.QNR_LOSS_CASES)
def test_qnr_loss_kernels_against_the_reference(name):
    import test_gpu_qnr_loss as k
    z = host.gold('parity_qnr_loss')
    x = tuple(dev(z[f'{name}/{key}']) for key in ('out', 'pan', 'ms', 'pan_l'))
    want_loss, want_grad = float(z[name + '/loss']), z[name + '/grad']
    B, C, H, W = x[0].shape
    wb, ws, need = k._workspace(B, C, H, W)
    _, table = k.qnr_stats(x, ws, need)
    dout, loss, idx = k.qnr_grad(x, table, ws, need)
    k._intact(wb, 'workspace')
    ri, rl = abs(idx[2] - want_loss) / want_loss, abs(float(loss) - want_loss) / want_loss
    print(f'{name}: indices[2] rel {ri:.2e}  loss_accum rel {rl:.2e}')
    assert ri <= 1e-11 and rl <= k.U
    assert abs((1 - idx[0]) * (1 - idx[1]) - (1 - want_loss)) <= 1e-11
    assert k._dout_ok(dout, want_grad)
