"""No GPU: the definitions behind the fused SAM / SSIM training losses -- losses.SAMLoss and losses.SSIMLoss in fp64 against independent
restatements (tests/recloss_helpers.py) and against metrics.sam / metrics.ssim, and the loss factory's new entries."""
import logging
import math
import os

import numpy as np
import pytest
import torch

import recloss_helpers as rh
from lgteun_amd import metrics
from lgteun_amd.losses import QNRLoss, ReconstructionLoss, SAMLoss, SSIMLoss, get_loss_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = logging.getLogger('t')


def _modules(loss_cfg):
    return get_loss_module({'loss_cfg': loss_cfg}, LOG)


def test_factory_takes_the_new_entries_and_keeps_the_old_ones():
    from lgteun_amd.compat import Config
    m = _modules({'rec_loss': dict(type='l1', w=1.0), 'spectral_loss': dict(type='sam', w=0.1),
                  'struct_loss': dict(type='ssim', w=0.2, data_range=2.0), 'noref_loss': dict(type='qnr', w=0.3)})
    assert list(m) == ['rec_loss', 'spectral_loss', 'struct_loss', 'noref_loss']
    assert isinstance(m['rec_loss'], ReconstructionLoss) and isinstance(m['noref_loss'], QNRLoss)
    assert isinstance(m['spectral_loss'], SAMLoss) and m['spectral_loss'].get_type() == 'sam'
    assert isinstance(m['struct_loss'], SSIMLoss) and m['struct_loss'].get_type() == 'ssim' and m['struct_loss'].data_range == 2.0
    assert _modules({'struct_loss': dict(type='ssim', w=1.0)})['struct_loss'].data_range == 1.0
    # attribute-style entries, as a config file gives them
    cfg = Config(dict(loss_cfg={'spectral_loss': dict(type='sam', w=1.0), 'struct_loss': dict(type='ssim', w=1.0, data_range=0.5)}))
    m = get_loss_module(cfg, LOG)
    assert list(m) == ['spectral_loss', 'struct_loss'] and m['struct_loss'].data_range == 0.5
    # w = 0 drops the entry
    assert list(_modules({'rec_loss': dict(type='l2', w=1.0), 'spectral_loss': dict(type='sam', w=0), 'struct_loss': dict(type='ssim', w=0.0)})) \
        == ['rec_loss']
    # old behaviour
    assert list(_modules({'rec_loss': dict(type='l1', w=1.0)})) == ['rec_loss']
    for bad in ({'spectral_loss': dict(type='ergas', w=1.0)}, {'struct_loss': dict(type='ms-ssim', w=1.0)}, {'struct_loss': dict(type='sam', w=1.0)},
                {'spectral_loss': dict(type='ssim', w=0.0)}, {'noref_loss': dict(type='sam', w=1.0)}, {'QNR_loss': dict(w=1.0)},
                {'adv_loss': dict(type='gan', w=1.0)}, {'rec_loss': dict(type='sam', w=1.0)}):
        with pytest.raises(SystemExit):
            _modules(bad)


def test_the_sources_are_listed_for_the_build():
    assert '$(CSRC)/k_recloss.hip' in open(os.path.join(ROOT, 'Makefile')).read()
    from lgteun_amd import _lib
    for name in ('lg_recloss_workspace_bytes', 'lg_sam_loss', 'lg_ssim_loss'):
        assert name in _lib.SIGNATURES
        assert name + '(' in open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()


@pytest.mark.parametrize('C,H,W', [(4, 16, 16), (8, 12, 28)])
def test_sam_loss_against_acos_autograd(C, H, W):
    out, gt = (t.double() for t in rh.make_pair(2, C, H, W, seed=3))
    loss, grad = rh.module_run(SAMLoss(), out, gt, torch.float64)
    x = out.clone().requires_grad_(True)
    ref = rh.sam_acos(x, gt)
    ref.backward()
    assert abs(loss - float(ref.detach())) <= 1e-14
    assert np.abs(grad - x.grad.numpy()).max() <= 1e-12 * np.abs(x.grad.numpy()).max()
    # the gradient's norm at a pixel is 1 / (|o| pixels)
    n = np.sqrt((grad ** 2).sum(axis=1)) * out.norm(dim=1).numpy() * (2 * H * W)
    assert np.abs(n - 1).max() <= 1e-9


def test_sam_loss_at_the_planted_pixels():
    out, gt = (t.double() for t in rh.make_pair(2, 4, 16, 16, seed=4))
    out, gt, cols = rh.plant(out, gt)
    x = out.clone().requires_grad_(True)
    loss = SAMLoss()(x, gt)
    loss.backward()
    assert math.isfinite(float(loss)) and bool(torch.isfinite(x.grad).all())
    for col in cols:
        assert bool((x.grad[0, :, 0, col] == 0).all()), col
    assert int((x.grad.abs().sum(dim=1) == 0).sum()) == len(cols)          # ... and every other pixel has a gradient
    # their contributions: 0, 0, pi / 2, pi / 2
    theta = [float(SAMLoss()(out[:1, :, :1, c:c + 1], gt[:1, :, :1, c:c + 1])) for c in cols]
    assert theta[0] <= 1e-15 and theta[1] <= 1e-15 and theta[2] == math.pi / 2 and theta[3] == math.pi / 2


def test_sam_loss_is_the_mean_of_metrics_sam():
    out, gt = rh.make_pair(3, 4, 12, 20, seed=5)
    out, gt, _ = rh.plant(out, gt)
    want = np.mean([metrics.sam(out[n].permute(1, 2, 0).numpy(), gt[n].permute(1, 2, 0).numpy()) for n in range(3)])
    # acos near cosine 1 turns a rounding error of 1e-16 into an angle of 1e-8 at the two parallel pixels; atan2 does not
    assert abs(float(SAMLoss()(out.double(), gt.double())) - want) <= 1e-9


@pytest.mark.parametrize('C,H,W,kind,R', [(4, 16, 16, 'smooth', 1.0), (2, 12, 28, 'smooth', 1.0), (4, 11, 12, 'smooth', 2.0), (4, 16, 16, 'flat', 1.0)])
def test_ssim_loss_against_the_closed_form_gradient(C, H, W, kind, R):
    out, gt = rh.make_pair(2, C, H, W, seed=6, kind=kind)
    loss, grad = rh.module_run(SSIMLoss(data_range=R), out, gt, torch.float64)
    want, g = rh.ssim_closed_form(out, gt, R)
    assert abs(loss - float(want)) <= 1e-14
    # E[x^2] - mu^2 cancels: an absolute error of a few 2^-53 mu^2 = 1e-16 on B2 >= c2 = 9e-4 R^2 is 1e-13 relative in the derivative
    # maps, in either evaluation order; a factor of ten for the sums behind it
    assert np.abs(grad - g.numpy()).max() <= 1e-12 * np.abs(g.numpy()).max()


def test_ssim_loss_is_one_minus_the_mean_of_metrics_ssim():
    out, gt = rh.make_pair(2, 4, 16, 28, seed=7)
    s = metrics.PEAK
    want = np.mean([metrics.ssim(s * out[n].double().permute(1, 2, 0).numpy(), s * gt[n].double().permute(1, 2, 0).numpy()) for n in range(2)])
    got = 1.0 - float(SSIMLoss(data_range=1.0)(out.double(), gt.double()))
    assert abs(got - want) <= 1e-13
    with pytest.raises(ValueError, match='11 x 11'):
        SSIMLoss()(out[:, :, :10], gt[:, :, :10])
