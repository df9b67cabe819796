"""The component-substitution (CS) baselines, the four oldest rows of a pan-sharpening comparison, for whole batches on the GPU: generalised IHS, Brovey,
Gram-Schmidt (GS) and PCA.  Each replaces an intensity I = sum_k w_k (u_k - mean u_k) of u = interp23(ms) by PAN matched to I's mean and standard deviation
and injects the difference with a gain per band; they differ in w and in the gains only (GSA, classical.py, is the member that fits w by regression).  The
definitions are DESIGN.md 3.15; the HIP kernels are lgteun_amd/csrc/k_cs.hip (C ABI lg_cs, include/lgteun_hip.h): fp64 arithmetic, one rounding per output
element, no atomics.  There is no CPU path.

`fuse` and its shorthands `ihs`, `brovey`, `gs`, `pca` take normalised float32 NCHW tensors on the GPU -- ms [B, C, h, w], pan [B, 1, 4h, 4w] -- and return
[B, C, 4h, 4w] on the same device; a call copies nothing to or from the device and synchronises nothing.  `IHS`, `Brovey`, `GS` and `PCA` are runner classes like
classical.GSA: nothing to train, and `test()` scores them like any network."""
import ctypes
import math

import torch

from . import _lib
from .builder import MODELS
from .classical import _Classical, _fuse_scene, _prepare, _scratch
from .engine import _ptr, _stream_ptr

MODES = {'ihs': _lib.LG_CS_IHS, 'brovey': _lib.LG_CS_BROVEY, 'gs': _lib.LG_CS_GS, 'pca': _lib.LG_CS_PCA}
SCENE_METHODS = ('ihs', 'brovey', 'gs', 'pca')      # cs.fuse_scene, tools/fuse_scene.py --method


def _mode(mode):
    if mode not in MODES:
        raise ValueError(f"mode must be 'ihs', 'brovey', 'gs' or 'pca' (got {mode!r})")
    return MODES[mode]


def _weights(mode, weights, C):
    """-> None or a ctypes array of C doubles: the caller's intensity weights, used as given (not normalised)"""
    if weights is None:
        return None
    if mode == 'pca':
        raise ValueError("weights: 'pca' takes none, its weights are the first principal axis of the bands")
    try:
        ws = [float(v) for v in weights]
    except TypeError:
        raise ValueError(f'weights must be {C} numbers, one per band (got {weights!r})') from None
    if len(ws) != C:
        raise ValueError(f'weights: {len(ws)} weights for {C} bands')
    if not all(math.isfinite(v) for v in ws):
        raise ValueError(f'weights must be finite (got {ws})')
    return (ctypes.c_double * C)(*ws)


def _workspace(dev, shape):
    return _scratch(dev, 'lg_cs_workspace_bytes', *shape)      # q, the partial sums and the coefficients of lg_cs, for this call only


def fuse(ms, pan, mode, weights=None, return_stats=False):
    """The CS method `mode` ('ihs', 'brovey', 'gs' or 'pca') of every sample.  weights: the intensity weights of 'ihs', 'brovey' and 'gs', C finite numbers
    used as given (None: 1 / C each); 'pca' takes none.  return_stats: also a float64 [B, 2C + 2] device tensor, per sample the intensity weights w (C), the
    injection gains g (C), the scale a of PAN and the intensity's mean m_I"""
    code = _mode(mode)
    ms, pan, shape = _prepare(f'cs.{mode}', ms, pan)
    B, C, h, w = shape
    wts = _weights(mode, weights, C)
    with torch.cuda.device(ms.device):
        ws = _workspace(ms.device, shape)
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        stats = torch.empty(B, 2 * C + 2, dtype=torch.float64, device=ms.device) if return_stats else None
        _lib.check(_lib.lib().lg_cs(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats) if return_stats else None, wts, code, B, C, h, w, _ptr(ws), ws.numel() * 8,
                                    _stream_ptr()), 'lg_cs')
    return (out, stats) if return_stats else out


def ihs(ms, pan, weights=None, return_stats=False):
    """generalised IHS: out_k = clip(u_k + (P - I))"""
    return fuse(ms, pan, 'ihs', weights, return_stats)


def brovey(ms, pan, weights=None, return_stats=False):
    """Brovey: out_k = clip(u_k (P + m_I) / (I + m_I + 2^-52))"""
    return fuse(ms, pan, 'brovey', weights, return_stats)


def gs(ms, pan, weights=None, return_stats=False):
    """Gram-Schmidt: out_k = clip(u_k + g_k (P - I)), g_k = cov(u_k, I) / var(I)"""
    return fuse(ms, pan, 'gs', weights, return_stats)


def pca(ms, pan, return_stats=False):
    """PCA: the first principal component of the bands replaced by the matched PAN, out_k = clip(u_k + w_k (P - I)), w the first principal axis"""
    return fuse(ms, pan, 'pca', None, return_stats)


def fuse_scene(method, ms, pan, weights=None, bit_depth=None, norm_input=False, out_dtype='float32', device=None):
    """One whole scene through the CS method `method` in ONE call: MS [C, h, w], PAN [1, 4h, 4w] -> [C, 4h, 4w] on the device.  The samples, the
    normalisation and out_dtype are classical.fuse_scene's."""
    _mode(method)
    _weights(method, weights, ms.shape[0])
    return _fuse_scene(lambda m, p: fuse(m, p, method, weights), ms, pan, bit_depth, norm_input, out_dtype, device)


class _Cs(_Classical):
    """cfg.cs_weights (optional): the intensity weights of IHS, Brovey and GS, one per band"""
    mode = None

    def __init__(self, cfg, logger, train_data_loader, test_data_loader0, test_data_loader1):
        super().__init__(cfg, logger, train_data_loader, test_data_loader0, test_data_loader1)
        self.weights = cfg.get('cs_weights')
        if self.weights is not None and self.mode == 'pca':
            raise ValueError("cs_weights: 'PCA' takes none, its weights are the first principal axis of the bands")

    def get_model_output(self, input_batch):
        return fuse(input_batch['input_lr'], input_batch['input_pan'], self.mode, self.weights)


@MODELS.register_module()
class IHS(_Cs):
    mode = 'ihs'


@MODELS.register_module()
class Brovey(_Cs):
    mode = 'brovey'


@MODELS.register_module()
class GS(_Cs):
    mode = 'gs'


@MODELS.register_module()
class PCA(_Cs):
    mode = 'pca'
