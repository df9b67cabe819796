"""MTF-GLP, the multiresolution baselines a pan-sharpening comparison asks for first, for whole batches on the GPU: the generalised Laplacian pyramid
with the sensor's MTF-matched Gaussian at the MS scale, and three injection rules -- additive (GLP), high-pass modulation (HPM) and context-based
decision with a global regression gain (CBD).  SFIM (classical.py) is the crude member of this family: it takes the detail from a 5 x 5 box mean.
The definitions are DESIGN.md 3.13; the HIP kernels are in lgteun_amd/csrc/k_classical.hip (C ABI lg_mtf_glp, include/lgteun_hip.h): fp64 arithmetic,
one rounding per output element, no atomics.  There is no CPU path.

`mtf_glp` takes normalised float32 NCHW tensors on the GPU -- ms [B, C, h, w], pan [B, 1, 4h, 4w] -- and returns [B, C, 4h, 4w] on the same device; a
call copies nothing to or from the host and synchronises nothing.  The MTF gains at Nyquist are per band and per sensor and are the CALLER's: without
them every band takes wald.DEFAULT_GAIN_MS, a common placeholder and NOT a sensor's measured value.  `MTF_GLP`, `MTF_GLP_HPM` and `MTF_GLP_CBD` are
runner classes like classical.GSA: nothing to train, and `test()` scores them like any network."""
import numpy as np
import torch

from . import _lib, wald
from .builder import MODELS
from .classical import _Classical, _fuse_scene, _prepare, _scratch
from .engine import _ptr, _stream_ptr

MODES = {'glp': _lib.LG_MTFGLP_GLP, 'hpm': _lib.LG_MTFGLP_HPM, 'cbd': _lib.LG_MTFGLP_CBD}
SCENE_METHODS = {'mtf_glp': 'glp', 'mtf_glp_hpm': 'hpm', 'mtf_glp_cbd': 'cbd'}      # tools/fuse_scene.py --method -> mode

_taps = {}              # (device, gains, n_taps) -> float64 [F, n_taps] on the device: written once, in _device_taps, then only read


def _gains(gains_ms, C):
    """-> the tuple of gains that is the cache key: one value when all bands share it (one filtered plane then serves every band), else C"""
    g = tuple(wald._gain_rows(gains_ms, C, wald.DEFAULT_GAIN_MS, 'gains_ms'))
    return g[:1] if all(v == g[0] for v in g) else g


def _device_taps(dev, gains, n_taps):
    key = (dev, gains, int(n_taps))
    t = _taps.get(key)
    if t is None:
        t = _taps[key] = torch.from_numpy(np.stack([wald.mtf_taps(g, n_taps) for g in gains])).to(dev)
    return t


def mtf_glp(ms, pan, mode='glp', gains_ms=None, n_taps=wald.DEFAULT_TAPS, return_stats=False):
    """MTF-GLP of every sample with the injection rule `mode` ('glp', 'hpm' or 'cbd').  gains_ms: the sensor's MTF gain at Nyquist, one for all bands or
    one per band (None: wald.DEFAULT_GAIN_MS); n_taps: odd, in 1 .. 63.  return_stats: also a float64 [B, 2C] device tensor, per sample the
    histogram-matching scales a (C) and the injection gains g (C; 1 for 'glp' and 'hpm')"""
    if mode not in MODES:
        raise ValueError(f"mode must be 'glp', 'hpm' or 'cbd' (got {mode!r})")
    ms, pan, shape = _prepare('mtf_glp', ms, pan)
    B, C, h, w = shape
    taps = _device_taps(ms.device, _gains(gains_ms, C), n_taps)
    F, L = taps.shape[0], _lib.lib()
    with torch.cuda.device(ms.device):
        ws = _scratch(ms.device, 'lg_mtfglp_workspace_bytes', B, C, h, w, F, MODES[mode])
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        stats = torch.empty(B, 2 * C, dtype=torch.float64, device=ms.device) if return_stats else None
        _lib.check(L.lg_mtf_glp(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats) if return_stats else None, _ptr(taps), F, taps.shape[1], MODES[mode], B, C, h, w,
                                _ptr(ws), ws.numel() * 8, _stream_ptr()), 'lg_mtf_glp')
    return (out, stats) if return_stats else out


def fuse_scene(mode, ms, pan, gains_ms=None, n_taps=wald.DEFAULT_TAPS, bit_depth=None, norm_input=False, out_dtype='float32', device=None):
    """One whole scene through MTF-GLP with the rule `mode` in ONE call: MS [C, h, w], PAN [1, 4h, 4w] -> [C, 4h, 4w] on the device.  The samples, the
    normalisation and out_dtype are classical.fuse_scene's."""
    if mode not in MODES:
        raise ValueError(f"mode must be 'glp', 'hpm' or 'cbd' (got {mode!r})")
    return _fuse_scene(lambda m, p: mtf_glp(m, p, mode, gains_ms, n_taps), ms, pan, bit_depth, norm_input, out_dtype, device)


class _MtfGlp(_Classical):
    """cfg.mtf_gains_ms: the sensor's gains (a scalar or one per band); cfg.mtf_taps: the tap count (41)"""
    mode = None

    def __init__(self, cfg, logger, train_data_loader, test_data_loader0, test_data_loader1):
        super().__init__(cfg, logger, train_data_loader, test_data_loader0, test_data_loader1)
        self.gains_ms, self.n_taps = cfg.get('mtf_gains_ms'), cfg.get('mtf_taps', wald.DEFAULT_TAPS)
        if self.gains_ms is None and logger is not None:
            logger.info(f'{type(self).__name__}: no mtf_gains_ms in the config: every band takes the MTF gain {wald.DEFAULT_GAIN_MS}, '
                        "a placeholder and not a sensor's value")

    def get_model_output(self, input_batch):
        return mtf_glp(input_batch['input_lr'], input_batch['input_pan'], self.mode, self.gains_ms, self.n_taps)


@MODELS.register_module()
class MTF_GLP(_MtfGlp):
    mode = 'glp'


@MODELS.register_module()
class MTF_GLP_HPM(_MtfGlp):
    mode = 'hpm'


@MODELS.register_module()
class MTF_GLP_CBD(_MtfGlp):
    mode = 'cbd'
