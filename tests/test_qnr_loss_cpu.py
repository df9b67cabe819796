"""The no-reference loss 1 - QNR without a device: losses.QNRLoss against the fp64 restatement of tests/qnr_helpers.py (value, and its
autograd gradient against the analytic alpha + beta x + gamma pan form the HIP kernel implements), the configuration surface, the C ABI
declarations and the argument validation of lg_qnr_*."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import qnr_helpers as qh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 4, 16, 16, 1), (3, 4, 48, 32, 2), (2, 8, 32, 80, 3), (5, 4, 16, 48, 4)]


@pytest.mark.parametrize('B,C,H,W,seed', SHAPES)
def test_qnr_loss_fp64_equals_the_restatement_and_its_gradient_the_analytic_form(B, C, H, W, seed):
    from lgteun_amd.losses import QNRLoss, qnr_table
    out, pan, ms, pan_l = qh.make_inputs(B, C, H, W, seed)
    ref = qh.reference(out, pan, ms, pan_l)                       # asserts the entry condition
    assert 0.0 < ref['indices'][2] < 1.0
    x = out.double().requires_grad_(True)
    loss = QNRLoss()(pan=pan.double(), ms=ms.double(), out=x, pan_l=pan_l.double())
    assert abs(loss.item() - ref['indices'][2]) <= 1e-12
    assert np.abs(qnr_table(pan.double(), ms.double(), x, pan_l.double()).detach().numpy() - ref['d']).max() <= 1e-12
    loss.backward()
    g = x.grad.numpy()
    assert np.abs(g - ref['grad']).max() <= 1e-10 * np.abs(ref['grad']).max()
    assert np.abs(ref['grad']).max() > 0


def test_reference_call_signature_and_the_bicubic_route():
    """forward(pan, ms, out, pan_l=None): without pan_l the PAN is down-sampled bicubically with align_corners=True"""
    from lgteun_amd.losses import QNRLoss
    out, pan, ms, pan_l = qh.make_inputs(2, 4, 32, 32, 7)
    m = QNRLoss(None, None)
    down = torch.nn.functional.interpolate(pan, size=[8, 8], mode='bicubic', align_corners=True)
    assert float(m(pan, ms, out)) == float(m(pan, ms, out, down))
    assert float(m(pan, ms, out)) != float(m(pan, ms, out, pan_l))
    assert float(m(pan, ms, out, pan_l)) == float(m(pan=pan, ms=ms, out=out, pan_l=pan_l)) and m.get_type() == 'qnr'


def test_get_loss_module_takes_noref_loss_and_keeps_rejecting_the_reference_key():
    from lgteun_amd.compat import Config
    from lgteun_amd.losses import QNRLoss, get_loss_module
    m = get_loss_module(Config(dict(loss_cfg={'noref_loss': dict(type='qnr', w=1.0)})), None)
    assert set(m) == {'noref_loss'} and isinstance(m['noref_loss'], QNRLoss)
    both = get_loss_module(Config(dict(loss_cfg={'rec_loss': dict(type='l1', w=1.0), 'noref_loss': dict(type='qnr', w=0.1)})), None)
    assert set(both) == {'rec_loss', 'noref_loss'}
    assert get_loss_module(Config(dict(loss_cfg={'noref_loss': dict(type='qnr', w=0.0)})), None) == {}
    with pytest.raises(SystemExit, match='noref_loss'):
        get_loss_module(Config(dict(loss_cfg={'noref_loss': dict(type='d_rho', w=1.0)})), None)
    with pytest.raises(SystemExit, match='noref_loss'):
        get_loss_module(Config(dict(loss_cfg={'QNR_loss': dict(w=1.0)})), None)


def test_symbols_are_declared_bound_and_built():
    from lgteun_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    for name in ('lg_qnr_workspace_bytes', 'lg_qnr_stats', 'lg_qnr_grad'):
        assert name in _lib.SIGNATURES and re.search(r'\b' + name + r'\s*\(', hdr), name
    assert 'losses.py:141-153' in hdr and 'metrics.py:336-397' in hdr
    assert _lib.LG_ABI_VERSION == 2 and re.search(r'#define\s+LG_ABI_VERSION\s+2\b', hdr)
    assert '$(CSRC)/k_qnr.hip' in open(os.path.join(ROOT, 'Makefile')).read()
    assert len(_lib.SIGNATURES['lg_qnr_stats'][1]) == 13 and len(_lib.SIGNATURES['lg_qnr_grad'][1]) == 16


def test_bad_arguments_are_rejected_without_a_device():
    """validation comes before any HIP call, so made-up addresses are never touched"""
    from lgteun_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('HIP library not built in this environment')
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('lg_qnr_workspace_bytes', 'lg_qnr_stats', 'lg_qnr_grad', 'lg_last_error'):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
    err = lambda: L.lg_last_error().decode()                                   # noqa: E731
    A = 0x100000                                                               # 16-byte aligned, never dereferenced
    need = L.lg_qnr_workspace_bytes(2, 4, 16, 16)
    assert need > 0 and need % 8 == 0
    assert L.lg_qnr_workspace_bytes(2, 5, 16, 16) == 0 and L.lg_qnr_workspace_bytes(2, 4, 18, 16) == 0
    assert L.lg_qnr_workspace_bytes(2, 4, 4, 16) == 0 and L.lg_qnr_workspace_bytes(0, 4, 16, 16) == 0
    assert L.lg_qnr_workspace_bytes(3, 4, 16, 16) > need                      # grows with B; the per-sample geometry does not
    stats = lambda C=4, H=16, W=16, out=A, pan_l=A, ws=A, nbytes=need: L.lg_qnr_stats(out, A, A, pan_l, None, A, 2, C, H, W, ws, nbytes, None)   # noqa: E731
    grad = lambda C=4, H=16, W=16, dout=A, ws=A, nbytes=need, bg=2, acc=0: L.lg_qnr_grad(A, A, A, dout, A, None, 2, bg, C, H, W, 1.0, acc, ws, nbytes, None)   # noqa: E731
    for call, who in ((stats, 'qnr_stats'), (grad, 'qnr_grad')):
        assert call(C=5) != 0 and who in err() and 'C must be 4 or 8' in err() and '5' in err()
        assert call(H=18) != 0 and 'H and W must be multiples of 4' in err() and '18 x 16' in err()
        assert call(W=4) != 0 and 'at least 8' in err()
        assert call(nbytes=need - 8) != 0 and 'workspace_bytes too small' in err() and str(need) in err()
        assert call(ws=A + 4) != 0 and 'workspace must be 8-byte aligned' in err()
        assert call(ws=None) != 0 and 'workspace is NULL' in err()
    assert stats(out=A + 4) != 0 and 'out must be 16-byte aligned' in err()
    assert stats(pan_l=A + 8) != 0 and 'pan_l must be 16-byte aligned' in err()
    assert stats(pan_l=None) != 0 and 'pan_l is NULL' in err()
    assert grad(dout=A + 4) != 0 and 'dout must be 16-byte aligned' in err()
    assert grad(bg=1) != 0 and 'B_global' in err()
    assert grad(acc=2) != 0 and 'accumulate' in err()
