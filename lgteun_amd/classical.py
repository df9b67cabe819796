"""The three non-learned rows of a pan-sharpening results table, for whole batches on the GPU: SFIM (smoothing-filter-based intensity
modulation), GSA (adaptive Gram-Schmidt with a global regression) and Wavelet (two-level Haar substitution), all defined on top of the 23-tap
interpolator x4 -- the reference's models/SFIM.py, models/GSA.py, models/Wavelet.py and models/common/model_based_utils.py:upsample_interp23.
The definitions, restated per sample of a batch, and the two deliberate deviations are in DESIGN.md 3.12; the HIP kernels are
lgteun_amd/csrc/k_classical.hip (C ABI lg_interp23_up4 / lg_sfim / lg_gsa / lg_wavelet in include/lgteun_hip.h): fp64 arithmetic, one rounding
per output element, no atomics.  There is no CPU path.

`interp23`, `sfim`, `gsa` and `wavelet` take normalised float32 NCHW tensors on the GPU -- ms [B, C, h, w], pan [B, 1, 4h, 4w] -- and return
[B, C, 4h, 4w] on the same device; nothing is copied to the host and nothing synchronises.  `GSA`, `SFIM` and `Wavelet` are the runner classes
the reference registers under those names: they have nothing to train, and `test()` scores them like any network."""
import functools

import numpy as np
import torch

from . import _lib
from .base_model import Base_model
from .builder import MODELS
from .engine import _ptr, _stream_ptr


def _prepare(what, ms, pan=None):
    for name, t in (('ms', ms), ('pan', pan))[:1 if pan is None else 2]:
        if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != torch.float32:
            got = f'{t.dtype} {tuple(t.shape)}' if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f'{what}: {name} must be a float32 NCHW tensor (got {got})')
        if not t.is_cuda:
            raise ValueError(f'{what}: {name} is on {t.device}; the classical methods run on the GPU only (there is no CPU path)')
    B, C, h, w = ms.shape
    if pan is not None:
        if pan.device != ms.device:
            raise ValueError(f'{what}: ms is on {ms.device}, pan on {pan.device}')
        if tuple(pan.shape) != (B, 1, 4 * h, 4 * w):
            raise ValueError(f'{what}: expected pan {(B, 1, 4 * h, 4 * w)} for ms {tuple(ms.shape)}, got {tuple(pan.shape)}')
        pan = pan.contiguous()
    return ms.contiguous(), pan, (B, C, h, w)


@functools.lru_cache(maxsize=256)
def _scratch_doubles(sizer, args):
    return max((int(getattr(_lib.lib(), sizer)(*args)) + 7) // 8, 1)      # 0 bytes for a shape the library rejects: the call says why


def _scratch(dev, sizer, *args):
    """the workspace of ONE call (partial sums and coefficients between a method's statistics pass and its apply pass), sized by the library's
    `sizer(*args)`, from torch's caching allocator: a block freed behind the call returns to the pool of the stream it was allocated on, so
    calls on different streams or from different threads never share one, and a second call on the same stream reuses it in stream order.
    Only the SIZE is remembered from call to call, never a buffer"""
    return torch.empty(_scratch_doubles(sizer, args), dtype=torch.float64, device=dev)


def _workspace(dev, method, shape):
    return _scratch(dev, 'lg_classical_workspace_bytes', *shape, method)


def interp23(ms):
    """ms [B, C, h, w] -> [B, C, 4h, 4w]: two x2 levels of zero insertion and the circular 23-tap half-band interpolator"""
    ms, _, (B, C, h, w) = _prepare('interp23', ms)
    with torch.cuda.device(ms.device):
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        _lib.check(_lib.lib().lg_interp23_up4(_ptr(ms), _ptr(out), B, C, h, w, _stream_ptr()), 'lg_interp23_up4')
    return out


def sfim(ms, pan):
    """SFIM of every sample: interp23(ms) modulated by the ratio of the histogram-matched PAN to its 5 x 5 circular box mean"""
    ms, pan, shape = _prepare('sfim', ms, pan)
    B, C, h, w = shape
    with torch.cuda.device(ms.device):
        ws = _workspace(ms.device, _lib.LG_CLASSICAL_SFIM, shape)
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        _lib.check(_lib.lib().lg_sfim(_ptr(ms), _ptr(pan), _ptr(out), B, C, h, w, _ptr(ws), ws.numel() * 8, _stream_ptr()), 'lg_sfim')
    return out


def gsa(ms, pan, return_stats=False):
    """GSA of every sample.  return_stats: also a float64 [B, 2C + 1] device tensor, per sample the regression weights alpha (C + 1, the
    intercept last) and the injection gains g (C)"""
    ms, pan, shape = _prepare('gsa', ms, pan)
    B, C, h, w = shape
    with torch.cuda.device(ms.device):
        ws = _workspace(ms.device, _lib.LG_CLASSICAL_GSA, shape)
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        stats = torch.empty(B, 2 * C + 1, dtype=torch.float64, device=ms.device) if return_stats else None
        _lib.check(_lib.lib().lg_gsa(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats) if return_stats else None, B, C, h, w, _ptr(ws),
                                     ws.numel() * 8, _stream_ptr()), 'lg_gsa')
    return (out, stats) if return_stats else out


def wavelet(ms, pan):
    """Wavelet of every sample: PAN with the level-2 Haar approximation (the 4 x 4 block means) of interp23(ms) in place of its own, clipped to
    [0, 1].  One launch: the block means of interp23(ms) are a 17-tap circular FIR on ms, so neither interp23(ms) nor a workspace is needed"""
    ms, pan, (B, C, h, w) = _prepare('wavelet', ms, pan)
    with torch.cuda.device(ms.device):
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        _lib.check(_lib.lib().lg_wavelet(_ptr(ms), _ptr(pan), _ptr(out), B, C, h, w, _stream_ptr()), 'lg_wavelet')
    return out


SCENE_METHODS = {'gsa': gsa, 'sfim': sfim, 'wavelet': wavelet}      # classical.fuse_scene, tools/fuse_scene.py --method


def fuse_scene(method, ms, pan, bit_depth=None, norm_input=False, out_dtype='float32', device=None):
    """One whole scene through `method` ('gsa', 'sfim' or 'wavelet') in ONE call -- no tiles, no checkpoint: MS [C, h, w], PAN [1, 4h, 4w] -> [C, 4h, 4w]
    on the device.  The arguments are scene.fuse_scene's: samples as numpy arrays or tensors (uint8, uint16 or its int16 view, float32);
    bit_depth / norm_input: the normalisation of the tile gather (norm_input: one correctly rounded fp32 division by 2**bit_depth - 0.5, then
    one multiplication by the fp32 reciprocal of that number); out_dtype 'uint16': digital numbers by lg_scene_to_u16 (needs bit_depth)."""
    if method not in SCENE_METHODS:
        raise ValueError(f"method must be 'gsa', 'sfim' or 'wavelet' (got {method!r})")
    return _fuse_scene(SCENE_METHODS[method], ms, pan, bit_depth, norm_input, out_dtype, device)


def _fuse_scene(fn, ms, pan, bit_depth, norm_input, out_dtype, device):
    """classical.fuse_scene and mtf_glp.fuse_scene: the normalisation, `fn(ms [1, C, h, w], pan [1, 1, 4h, 4w])` on the whole scene, the conversion"""
    from . import scene as sc
    if out_dtype not in ('float32', 'uint16'):
        raise ValueError(f"out_dtype must be 'float32' or 'uint16' (got {out_dtype!r})")
    if (norm_input or out_dtype == 'uint16') and bit_depth is None:
        raise ValueError("norm_input and out_dtype='uint16' need bit_depth")
    C, H, W = sc.check_shapes(ms.shape, pan.shape)
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    ms_t, kind = sc._to_device(ms, dev, 'ms')
    pan_t, kind_p = sc._to_device(pan, dev, 'pan')
    if kind != kind_p:
        raise ValueError(f'ms ({kind}) and pan ({kind_p}) must have the same sample type')
    divisor = float(2 ** bit_depth - .5) if bit_depth is not None else 1.0

    def normalised(t):
        if t.dtype == torch.int16:                        # the int16 view of uint16 samples
            t = t.to(torch.int32) & 0xFFFF
        t = t.to(torch.float32)
        if norm_input:
            t = torch.div(t, torch.tensor(divisor, dtype=torch.float32, device=dev))
        if bit_depth is not None:
            t = t * float(np.float32(1.0) / np.float32(divisor))        # scene.fuse_scene's post_scale
        return t
    with torch.cuda.device(dev):
        fused = fn(normalised(ms_t).view(1, C, H // 4, W // 4), normalised(pan_t).view(1, 1, H, W))[0]
        if out_dtype == 'float32':
            return fused
        out = torch.empty(C, H, W, dtype=torch.uint16, device=dev)
        _lib.check(_lib.lib().lg_scene_to_u16(_ptr(fused), _ptr(out), fused.numel(), divisor, _stream_ptr()), 'lg_scene_to_u16')
        return out


class _Classical(Base_model):
    """a runner without modules: `get_model_output` is the method itself, on the whole batch (the reference squeezes the batch to one image
    and returns an HWC numpy array; models/GSA.py:49-52)"""
    method = None

    def _device(self):
        return torch.device('cuda', torch.cuda.current_device())

    def get_model_output(self, input_batch):
        return type(self).method(input_batch['input_lr'], input_batch['input_pan'])

    def train(self):
        if self.logger is not None:
            self.logger.info(f'{type(self).__name__} has nothing to train')

    def train_iter(self, iter_id, input_batch, log_freq=10):
        raise RuntimeError(f'{type(self).__name__} is a classical method: it has nothing to train')

    def save(self, iter_id):
        if self.logger is not None:
            self.logger.info(f'{type(self).__name__} has no weights: nothing to save')
        return None


@MODELS.register_module()
class GSA(_Classical):
    method = staticmethod(gsa)


@MODELS.register_module()
class SFIM(_Classical):
    method = staticmethod(sfim)


@MODELS.register_module()
class Wavelet(_Classical):
    method = staticmethod(wavelet)
