"""Shared by tests/test_recloss_cpu.py, tests/test_gpu_recloss.py and tests/ddp_recloss_worker.py: the input recipe of the SAM / SSIM loss
tests, independent restatements of both losses (the spectral angle through acos of the clipped cosine, differentiated by autograd; the SSIM
gradient in the closed form T(dS/dm1) + 2 x T(dS/dm2) + y T(dS/dm3) with explicit sliding-window sums, no convolution call), and the fp64 /
fp32 runs of losses.SAMLoss / losses.SSIMLoss that the device kernels are held against."""
import numpy as np
import torch

from lgteun_amd import metrics
from lgteun_amd.losses import SAMLoss, SSIMLoss

U = 2.0 ** -23


def make_pair(B, C, H, W, seed, kind='smooth'):
    """(out, gt) float32 [B, C, H, W] in [0, 1].  'smooth': low-frequency waves with per-band gains plus noise, out = gt plus a smaller smooth
    error plus noise; 'flat': 0.5 + 1e-3 noise on both (the variances are far below c2 = 9e-4)."""
    g = torch.Generator().manual_seed(seed)
    nrm = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)           # noqa: E731
    if kind == 'flat':
        return tuple((0.5 + 1e-3 * nrm(B, C, H, W)).float().contiguous() for _ in range(2))
    r = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    c = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    ph = 6.28 * torch.rand(B, C, 1, 1, generator=g, dtype=torch.float64)
    gain = torch.linspace(0.7, 1.3, C, dtype=torch.float64).view(1, C, 1, 1)
    gt = 0.5 + 0.25 * gain * (torch.sin(0.31 * r + ph) * torch.cos(0.23 * c - ph)) + 0.04 * nrm(B, C, H, W)
    out = gt + 0.05 * torch.sin(0.17 * r + 0.29 * c + ph) + 0.03 * nrm(B, C, H, W)
    return tuple(t.clamp(0.0, 1.0).float().contiguous() for t in (out, gt))


def plant(out, gt):
    """copies with four planted pixels in sample 0, row 0: out == gt | out == 2 gt | out == 0 | out == -gt.  Returns (out, gt, columns)"""
    out, gt = out.clone(), gt.clone()
    cols = [1, 3, 6, 9]
    out[0, :, 0, cols[0]] = gt[0, :, 0, cols[0]]
    out[0, :, 0, cols[1]] = 2 * gt[0, :, 0, cols[1]]
    out[0, :, 0, cols[2]] = 0
    out[0, :, 0, cols[3]] = -gt[0, :, 0, cols[3]]
    return out, gt, cols


def sam_acos(out, gt):
    """the textbook form: mean acos(clip(<o, g> / (|o| |g|), 0, 1)); differentiable by autograd away from the clip's ends"""
    cs = (out * gt).sum(dim=1) / (out.norm(dim=1) * gt.norm(dim=1))
    return torch.acos(cs.clamp(0.0, 1.0)).mean()


def _windows(t, taps):
    """[..., H, W] -> [..., H - 10, W - 10]: explicit sliding-window sums, columns of the window then rows, like metrics._inside_windows"""
    n = taps.numel()
    rows = (t.unfold(-2, n, 1) * taps).sum(-1)
    return (rows.unfold(-1, n, 1) * taps).sum(-1)


def _transposed(d, taps, H, W):
    """T: [..., H - 10, W - 10] -> [..., H, W], every window's value spread back over its pixels with the window's weights"""
    n = taps.numel()
    full = d.new_zeros(d.shape[:-2] + (H, W))
    for a in range(n):
        for b in range(n):
            full[..., a:a + d.shape[-2], b:b + d.shape[-1]] += taps[a] * taps[b] * d
    return full


def ssim_closed_form(x, y, data_range=1.0):
    """fp64 (loss, gradient wrt x) of 1 - mean SSIM from the written-out derivatives; x, y [B, C, H, W]"""
    x, y = x.double(), y.double()
    H, W = x.shape[-2:]
    taps = torch.from_numpy(metrics.gaussian_taps())
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = _windows(x, taps), _windows(y, taps)
    m2, m3, m4 = _windows(x * x, taps), _windows(x * y, taps), _windows(y * y, taps)
    A1, B1 = 2 * mx * my + c1, mx * mx + my * my + c1
    A2, B2 = 2 * (m3 - mx * my) + c2, (m2 - mx * mx) + (m4 - my * my) + c2
    S = A1 * A2 / (B1 * B2)
    d3 = 2 * A1 / (B1 * B2)
    d2 = -A1 * A2 / (B1 * B2 ** 2)
    d1 = 2 * my * (A2 - A1) / (B1 * B2) - 2 * mx * A1 * A2 / (B1 ** 2 * B2) + 2 * mx * A1 * A2 / (B1 * B2 ** 2)
    grad = -(_transposed(d1, taps, H, W) + 2 * x * _transposed(d2, taps, H, W) + y * _transposed(d3, taps, H, W)) / S.numel()
    return 1 - S.mean(), grad


def module_run(module, out, gt, dtype):
    """(loss, d loss / d out) of a losses module on the CPU in `dtype`, as float64 numpy"""
    x = out.detach().cpu().to(dtype).requires_grad_(True)
    loss = module(x, gt.detach().cpu().to(dtype))
    loss.backward()
    return float(loss.detach()), x.grad.double().numpy()


def references(kind, out, gt, data_range=1.0):
    """dict(loss, grad: the module in fp64 | grad32: the same module in fp32, the route the kernel replaces)"""
    module = SAMLoss() if kind == 'sam' else SSIMLoss(data_range=data_range)
    loss, grad = module_run(module, out, gt, torch.float64)
    _, grad32 = module_run(module, out, gt, torch.float32)
    return dict(loss=loss, grad=grad, grad32=grad32)


def dout_ratio(dout, ref, scale=1.0):
    """largest error of a device dout against scale * the fp64 gradient, over the bar: the larger of twice the largest error of the fp32
    module (a different summation order may double it) and the one-rounding bound 2^-23 |g| + 1e-9 max |g|, taken at the worst element"""
    g, g32 = scale * ref['grad'], scale * ref['grad32']
    err = np.abs(dout.detach().double().cpu().numpy() - g)
    bar = np.maximum(2.0 * np.abs(g32 - g).max(), U * np.abs(g) + 1e-9 * np.abs(g).max())
    return float((err / bar).max())
