"""The loss surface the LGTEUN runner needs (reference models/base/losses.py: `ReconstructionLoss` :19-40 and the
`get_loss_module` factory :222-249, as used by configs/unlg_former.py:88-90 -- one `rec_loss` entry of type l1 / l2 with weight w).
`QNRLoss` (:141-153) is the no-reference term for full-resolution data, configured as `noref_loss`.  The adversarial / mutual-information
losses of the comparison methods are outside this build.  `SAMLoss` and `SSIMLoss` train on the spectral and the
structural index that lgteun_amd/metrics.py reports (`spectral_loss`, `struct_loss`); the reference has neither as a loss.
The fused train step does not call this module: it computes the loss + its gradient in `lg_l1_loss` / `lg_l2_loss` / `lg_sam_loss` /
`lg_ssim_loss` / `lg_qnr_stats` + `lg_qnr_grad`; this is the autograd-path / torch-optimizer route and what `get_type()` callers see."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

_CRITERIA = {'l1': nn.L1Loss, 'l2': nn.MSELoss}


class ReconstructionLoss(nn.Module):
    """mean |out - gt| (l1) or mean (out - gt)^2 (l2); unknown types end the run like the reference does (SystemExit)"""

    def __init__(self, cfg, logger, loss_type='l1'):
        super().__init__()
        if loss_type not in _CRITERIA:
            msg = f'No such type of ReconstructionLoss: "{loss_type}"'
            if logger is not None:
                logger.error(msg)
            raise SystemExit(msg)
        self.cfg, self.loss_type = cfg, loss_type
        self.loss = _CRITERIA[loss_type]()

    def get_type(self):
        return self.loss_type

    def forward(self, out, gt):
        return self.loss(out, gt)


def q_index(a, b, eps=1e-8):
    """Wang-Bovik Q of every sample over its WHOLE image (QIndex_torch, reference models/base/metrics.py:336-355, before its batch mean):
    a, b [N, H, W] -> [N]"""
    ea, eb = a.mean(dim=(1, 2)), b.mean(dim=(1, 2))
    var_a = (a * a).mean(dim=(1, 2)) - ea * ea
    var_b = (b * b).mean(dim=(1, 2)) - eb * eb
    cov = (a * b).mean(dim=(1, 2)) - ea * eb
    return 4 * cov * ea * eb / ((var_a + var_b) * (ea * ea + eb * eb) + eps)


def qnr_table(pan, ms, out, pan_l):
    """the C (C - 1) / 2 + C differences mean_n Q_n(fused pair) - mean_n Q_n(MS pair): band pairs i < j in row-major order, then the
    band-to-PAN pairs (the layout of lg_qnr_stats's table, there as sums over n)"""
    C = out.shape[1]
    d = [q_index(out[:, i], out[:, j]).mean() - q_index(ms[:, i], ms[:, j]).mean() for i in range(C) for j in range(i + 1, C)]
    d += [q_index(out[:, i], pan[:, 0]).mean() - q_index(ms[:, i], pan_l[:, 0]).mean() for i in range(C)]
    return torch.stack(d)


class QNRLoss(nn.Module):
    """1 - QNR = 1 - (1 - D_lambda)(1 - D_s) for data without a ground truth (reference models/base/losses.py:141-153 with
    D_lambda_torch / D_s_torch, metrics.py:358-397, p = q = 1): D_lambda the mean over band pairs of |Q(out_i, out_j) - Q(ms_i, ms_j)|,
    D_s the mean over bands of |Q(out_i, pan) - Q(ms_i, pan_l)|, every Q a batch mean of whole-image indices.  Q is symmetric, so the
    reference's sum over ordered pairs i != j divided by C (C - 1) is the mean over i < j taken here.  With pan_l=None the PAN is
    down-sampled bicubically with align_corners=True (the reference's down_sample, models/base/utils.py:127-138)."""

    def __init__(self, cfg=None, logger=None):
        super().__init__()
        self.cfg, self.logger = cfg, logger

    def get_type(self):
        return 'qnr'

    def forward(self, pan, ms, out, pan_l=None):
        if pan_l is None:
            pan_l = F.interpolate(pan, size=[pan.shape[2] // 4, pan.shape[3] // 4], mode='bicubic', align_corners=True)
        C = out.shape[1]
        d = qnr_table(pan, ms, out, pan_l).abs()
        n_pairs = C * (C - 1) // 2
        d_lambda, d_s = d[:n_pairs].mean(), d[n_pairs:].mean()
        return 1 - (1 - d_lambda) * (1 - d_s)


SAM_MIN_S = 1e-6      # below this |u| is rounding noise: the pixel keeps its angle and gets no gradient


class _SpectralAngle(torch.autograd.Function):
    """mean over pixels of theta = atan2(s, c) with o^ = o / |o|, g^ = g / |g|, c = <o^, g^>, u = g^ - c o^, s = |u|, and the gradient
    d theta / d o = -u / (s |o|) in closed form (its norm is exactly 1 / |o|): acos, whose derivative is unbounded at theta -> 0, is
    never differentiated.  gt gets no gradient."""

    @staticmethod
    def forward(ctx, out, gt):
        no, ng = out.norm(dim=1, keepdim=True), gt.norm(dim=1, keepdim=True)
        ok = (no > 0) & (ng > 0)
        one = torch.ones_like(no)
        oh, gh = out / torch.where(ok, no, one), gt / torch.where(ok, ng, one)
        c = (oh * gh).sum(dim=1, keepdim=True)
        ok = ok & (c > 0)
        u = gh - c * oh
        s = u.norm(dim=1, keepdim=True)
        theta = torch.where(ok, torch.atan2(s, c), torch.full_like(c, math.pi / 2))
        live = ok & (s >= SAM_MIN_S)
        grad = torch.where(live, -u / torch.where(live, s * no, one), torch.zeros_like(u)) / theta.numel()
        ctx.save_for_backward(grad)
        return theta.mean()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


class SAMLoss(nn.Module):
    """the mean over all B H W pixels of the spectral angle between out[n, :, p] and gt[n, :, p], in radians: the mean over the batch of
    metrics.sam.  As metrics.sam clips the cosine to [0, 1], a pixel with c <= 0, |out| = 0 or |gt| = 0 contributes pi / 2 and no gradient;
    a pixel with s < 1e-6 (out parallel to gt) contributes its angle and no gradient."""

    def __init__(self, cfg=None, logger=None):
        super().__init__()
        self.cfg, self.logger = cfg, logger

    def get_type(self):
        return 'sam'

    def forward(self, out, gt):
        return _SpectralAngle.apply(out, gt)


def _gaussian_taps(n, sigma, like):
    """metrics.gaussian_taps as a tensor"""
    t = torch.arange(n, dtype=torch.float64) - 0.5 * (n - 1)
    g = torch.exp(-0.5 * (t / sigma) ** 2)
    return (g / g.sum()).to(device=like.device, dtype=like.dtype)


class SSIMLoss(nn.Module):
    """1 - the mean of the SSIM map over every image, band and window: metrics._ssim_band exactly (11-tap Gaussian of sigma 1.5, only the
    windows that lie fully inside the image, c1 = (0.01 R)^2 and c2 = (0.03 R)^2 with R = data_range), differentiated by autograd."""

    TAPS, SIGMA = 11, 1.5

    def __init__(self, cfg=None, logger=None, data_range=1.0):
        super().__init__()
        self.cfg, self.logger, self.data_range = cfg, logger, float(data_range)

    def get_type(self):
        return 'ssim'

    def window_sums(self, t):
        """[B, C, H, W] -> [B, C, H - 10, W - 10]: the separable Gaussian over the inside windows, rows of the window first like the host"""
        B, C, H, W = t.shape
        g = _gaussian_taps(self.TAPS, self.SIGMA, t)
        t = F.conv2d(t.reshape(B * C, 1, H, W), g.view(1, 1, -1, 1))
        return F.conv2d(t, g.view(1, 1, 1, -1)).view(B, C, H - self.TAPS + 1, W - self.TAPS + 1)

    def ssim_map(self, out, gt):
        c1, c2 = (0.01 * self.data_range) ** 2, (0.03 * self.data_range) ** 2
        mx, my = self.window_sums(out), self.window_sums(gt)
        vx = self.window_sums(out * out) - mx * mx
        vy = self.window_sums(gt * gt) - my * my
        cxy = self.window_sums(out * gt) - mx * my
        return (2.0 * mx * my + c1) / (mx * mx + my * my + c1) * ((2.0 * cxy + c2) / (vx + vy + c2))

    def forward(self, out, gt):
        if out.shape[2] < self.TAPS or out.shape[3] < self.TAPS:
            raise ValueError(f'SSIMLoss needs images of at least {self.TAPS} x {self.TAPS} pixels (got {tuple(out.shape[2:])})')
        return 1.0 - self.ssim_map(out, gt).mean()


def _fatal(msg, logger):
    if logger is not None:
        logger.error(msg)
    raise SystemExit(msg)


def get_loss_module(full_cfg, logger):
    """{name: module} for every configured loss whose weight is non-zero: `rec_loss` entries (type l1 / l2), the spectral entry
    `spectral_loss` (type 'sam'), the structural entry `struct_loss` (type 'ssim', with an optional `data_range`, default 1) and the
    no-reference entry `noref_loss` (type 'qnr').  The reference spells the latter `QNR_loss`, without a type; that key keeps ending the run here, as it
    always has on this build (configurations and tests rely on unknown names being fatal), and its message points to `noref_loss` --
    a name that says what the term is for and leaves room for other no-reference types."""
    modules = {}
    table = full_cfg.get('loss_cfg') or {}
    for name in table:
        cfg = table[name]                 # attribute-style entry (mmcv Config / compat.Config) or a plain dict
        field = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
        if name == 'noref_loss':
            if field('type') != 'qnr':
                msg = f"No such type of noref_loss: {field('type')!r} (only 'qnr')"
                if logger is not None:
                    logger.error(msg)
                raise SystemExit(msg)
            if float(field('w')) != 0.0:
                modules[name] = QNRLoss(cfg, logger)
            continue
        if name == 'spectral_loss':
            if field('type') != 'sam':
                _fatal(f"No such type of spectral_loss: {field('type')!r} (only 'sam')", logger)
            if float(field('w')) != 0.0:
                modules[name] = SAMLoss(cfg, logger)
            continue
        if name == 'struct_loss':
            if field('type') != 'ssim':
                _fatal(f"No such type of struct_loss: {field('type')!r} (only 'ssim')", logger)
            if float(field('w')) != 0.0:
                has = ('data_range' in cfg) if isinstance(cfg, dict) else hasattr(cfg, 'data_range')
                modules[name] = SSIMLoss(cfg, logger, data_range=float(field('data_range')) if has else 1.0)
            continue
        if name == 'QNR_loss':
            raise SystemExit("loss 'QNR_loss' is configured on this build as loss_cfg['noref_loss'] = dict(type='qnr', w=...)")
        if 'rec_loss' not in name:
            raise SystemExit(f'loss "{name}" is outside the LGTEUN hot path of this build (only rec_loss, spectral_loss, struct_loss and noref_loss)')
        if float(field('w')) != 0.0:
            modules[name] = ReconstructionLoss(cfg, logger, loss_type=field('type'))
    return modules
