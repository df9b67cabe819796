"""The evaluation indices of lgteun_amd/metrics.py for whole batches on the GPU: `ref_evaluate_batch` (PSNR, SSIM, Q, SAM, ERGAS) and
`no_ref_evaluate_batch` (D_lambda, D_s, QNR).  The HIP kernels behind them (lgteun_amd/csrc/k_iqa.hip; C ABI lg_iqa_ref / lg_iqa_no_ref in
include/lgteun_hip.h) compute the host functions' definitions in fp64; only the order of summation differs.  The host functions stay the
definition and the yardstick (tests/test_gpu_metrics.py).

Inputs are contiguous float32 NCHW tensors on the GPU.  Every element is multiplied by `scale` in fp32 first: pass 2**bit_depth - 0.5 for
normalised tensors (the rounding data_denormalize applies) and 1 for digital numbers.  The rows come back as a float64 tensor on the
same device; nothing is copied to the host and nothing synchronises."""
import torch

from . import _lib
from .engine import _ptr, _stream_ptr

REF_NAMES = ('PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS')
NO_REF_NAMES = ('D_lambda', 'D_s', 'QNR')


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
