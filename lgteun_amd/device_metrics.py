"""The evaluation indices of lgteun_amd/metrics.py for whole batches on the GPU: `ref_evaluate_batch` (PSNR, SSIM, Q, SAM, ERGAS) and
`no_ref_evaluate_batch` (D_lambda, D_s, QNR).  The HIP kernels behind them (lgteun_amd/csrc/k_iqa.hip; C ABI lg_iqa_ref / lg_iqa_no_ref in
include/lgteun_hip.h) compute the host functions' definitions in fp64; only the order of summation differs.  The host functions stay the
definition and the yardstick (tests/test_gpu_metrics.py).

Inputs are contiguous float32 NCHW tensors on the GPU.  Every element is multiplied by `scale` in fp32 first: pass 2**bit_depth - 0.5 for
normalised tensors (the rounding data_denormalize applies) and 1 for digital numbers.  The rows come back as a float64 tensor on the
same device; nothing is copied to the host and nothing synchronises.

The extended set -- `ref_evaluate_ext_batch` (the five, then Q2n, SCC, CC) and `no_ref_evaluate_ext_batch` (the three, then D_lambda_K, HQNR) --
is metrics.ref_evaluate_ext / no_ref_evaluate_ext: kernels in lgteun_amd/csrc/k_iqa_ext.hip (C ABI lg_iqa_ref_ext / lg_iqa_q2n), yardstick
tests/test_gpu_metrics_ext.py.  Its images are 2 .. 8 bands and at least 32 x 32 (one Q2n block)."""
import numpy as np
import torch

from . import _lib
from .engine import _ptr, _stream_ptr

REF_NAMES = ('PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS')
NO_REF_NAMES = ('D_lambda', 'D_s', 'QNR')
REF_EXT_NAMES = REF_NAMES + ('Q2n', 'SCC', 'CC')
NO_REF_EXT_NAMES = NO_REF_NAMES + ('D_lambda_K', 'HQNR')


def _check(name, t):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
        what = f'{t.dtype} {tuple(t.shape)} on {t.device}' if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f'{name} must be a contiguous float32 NCHW tensor on the GPU (got {what})')


def _call(fn, what, tensors, k, B, C, H, W, no_ref, scale):
    dev = tensors[0].device
    if any(t.device != dev for t in tensors):
        raise ValueError(f'{what}: inputs are on different devices')
    L = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(L.lg_iqa_workspace_bytes(B, C, H, W, no_ref))      # 0 for a shape the library rejects: the call below says why
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        out = torch.empty(B, k, dtype=torch.float64, device=dev)
        _lib.check(fn(*[_ptr(t) for t in tensors], _ptr(out), B, C, H, W, float(scale), _ptr(ws), nbytes, _stream_ptr()), what)
    return out


def ref_evaluate_batch(pred, gt, scale=1.0):
    """metrics.ref_evaluate of every image of pred / gt [B, C, H, W]: a float64 [B, 5] device tensor, rows PSNR, SSIM, Q, SAM, ERGAS"""
    _check('pred', pred)
    _check('gt', gt)
    if pred.shape != gt.shape:
        raise ValueError(f'pred and gt differ in shape: {tuple(pred.shape)} vs {tuple(gt.shape)}')
    B, C, H, W = pred.shape
    return _call(_lib.lib().lg_iqa_ref, 'lg_iqa_ref', (pred, gt), len(REF_NAMES), B, C, H, W, 0, scale)


def no_ref_evaluate_batch(pred, pan, ms, scale=1.0):
    """metrics.no_ref_evaluate of every image: pred [B, C, H, W], pan [B, 1, H, W], ms [B, C, H/4, W/4] -> a float64 [B, 3] device
    tensor, rows D_lambda, D_s, QNR"""
    for name, t in (('pred', pred), ('pan', pan), ('ms', ms)):
        _check(name, t)
    B, C, H, W = pred.shape
    if tuple(pan.shape) != (B, 1, H, W) or tuple(ms.shape) != (B, C, H // 4, W // 4):
        raise ValueError(f'expected pan [B,1,H,W] and ms [B,C,H/4,W/4] for pred {tuple(pred.shape)}, got {tuple(pan.shape)} / {tuple(ms.shape)}')
    return _call(_lib.lib().lg_iqa_no_ref, 'lg_iqa_no_ref', (pred, pan, ms), len(NO_REF_NAMES), B, C, H, W, 1, scale)


def _call_ext(fn, what, a, b, k, scale):
    """lg_iqa_ref_ext / lg_iqa_q2n on the pair (a, b) -> float64 [B, k]"""
    B, C, H, W = a.shape
    L = _lib.lib()
    with torch.cuda.device(a.device):
        nbytes = int(L.lg_iqa_ext_workspace_bytes(B, C, H, W))          # 0 for a shape the library rejects: the call below says why
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=a.device)
        out = torch.empty(B, k, dtype=torch.float64, device=a.device)
        _lib.check(fn(_ptr(a), _ptr(b), _ptr(out), B, C, H, W, float(scale), _ptr(ws), nbytes, _stream_ptr()), what)
    return out


def ref_evaluate_ext_batch(pred, gt, scale=1.0):
    """metrics.ref_evaluate_ext of every image of pred / gt [B, C, H, W]: a float64 [B, 8] device tensor, rows REF_EXT_NAMES.  The first
    five columns are `ref_evaluate_batch`'s, bit for bit.  2 <= C <= 8; H, W >= 32"""
    std = ref_evaluate_batch(pred, gt, scale)
    if pred.device != gt.device:
        raise ValueError('lg_iqa_ref_ext: inputs are on different devices')
    return torch.cat([std, _call_ext(_lib.lib().lg_iqa_ref_ext, 'lg_iqa_ref_ext', pred, gt, 3, scale)], dim=1)


def no_ref_evaluate_ext_batch(pred, pan, ms, scale=1.0, gains_ms=None, n_taps=None, phase=2):
    """metrics.no_ref_evaluate_ext of every image: pred [B, C, H, W], pan [B, 1, H, W], ms [B, C, H/4, W/4] -> a float64 [B, 5] device
    tensor, rows NO_REF_EXT_NAMES; the first three columns are `no_ref_evaluate_batch`'s, bit for bit.  gains_ms: the sensor's MTF gains at
    Nyquist, one for all bands or one per band (None: wald.DEFAULT_GAIN_MS, a placeholder, as in mtf_glp); n_taps: None = wald.DEFAULT_TAPS.
    H, W >= 128 (MS sides >= 32).
    D_lambda_K rounds where the host does: pred * scale is ONE fp32 torch op, lg_fir_decimate4 rounds the degraded image to fp32 once,
    and Q2n takes (ms * scale, degraded) with scale 1"""
    from . import wald                      # (wald imports the loaders, which import base_model, which imports this module)
    std = no_ref_evaluate_batch(pred, pan, ms, scale)
    B, C, H, W = pred.shape
    n_taps = wald.DEFAULT_TAPS if n_taps is None else n_taps
    gains = wald._gain_rows(gains_ms, C, wald.DEFAULT_GAIN_MS, 'gains_ms')
    taps = np.stack([wald.mtf_taps(g, n_taps) for g in gains] * B)                      # one row per plane of [B * C, H, W]
    fine = pred * scale if scale != 1.0 else pred
    degraded = wald._fir(fine.reshape(B * C, H, W), taps, wald._check_phase(phase), 'float32').view(B, C, H // 4, W // 4)
    coarse = ms * scale if scale != 1.0 else ms
    q = _call_ext(_lib.lib().lg_iqa_q2n, 'lg_iqa_q2n', coarse, degraded, 1, 1.0)
    dk = 1.0 - q
    return torch.cat([std, dk, (1.0 - dk) * (1.0 - std[:, 1:2])], dim=1)
