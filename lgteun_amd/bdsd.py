"""BDSD, the band-dependent spatial detail method (Garzelli, Nencini, Capobianco, 2008), for whole batches on the GPU, in its global form and its block-wise
("local") form.  It is the one classical baseline whose injection weights come from a joint least-squares fit over all bands and PAN together: per block
and band a (C + 1)-vector gamma, fitted at the MS scale, mixes the C interpolated bands and PAN into the detail of that band.  The definition is DESIGN.md
3.14; the HIP kernels are the k_bd_* of lgteun_amd/csrc/k_classical.hip (C ABI lg_bdsd, include/lgteun_hip.h): fp64 arithmetic, a Cholesky solve per block,
one rounding per output element, no atomics.  There is no CPU path.

`bdsd` takes normalised float32 NCHW tensors on the GPU -- ms [B, C, h, w], pan [B, 1, 4h, 4w] -- and returns [B, C, 4h, 4w] on the same device; a call
copies nothing to or from the host and synchronises nothing.  The MTF gains at Nyquist are per band and per sensor and are the CALLER's: without them the
bands take wald.DEFAULT_GAIN_MS and PAN wald.DEFAULT_GAIN_PAN, common placeholders and NOT a sensor's measured values.  `BDSD` is a runner class like
classical.GSA: nothing to train, and `test()` scores it like any network."""
import numpy as np
import torch

from . import _lib, wald
from .builder import MODELS
from .classical import _Classical, _fuse_scene, _prepare, _scratch
from .engine import _ptr, _stream_ptr
from .mtf_glp import _device_taps, _gains


def _block(block, C, h, w):
    """-> lg_bdsd's block argument: 0 for the global form (None), else the side of a block in PAN pixels"""
    if block is None:
        if h * w < 2 * (C + 1):
            raise ValueError(f'bdsd: the global form needs h * w >= 2 (C + 1) = {2 * (C + 1)} equations (got ms {h} x {w})')
        return 0
    if isinstance(block, bool) or int(block) != block or block < 32 or block % 32:
        raise ValueError(f'bdsd: block must be None (global) or a multiple of 32 PAN pixels (got {block!r})')
    if (4 * h) % block or (4 * w) % block:
        raise ValueError(f'bdsd: block {block} does not divide the sides {4 * h} x {4 * w} of pan')
    return int(block)


def bdsd(ms, pan, block=None, gains_ms=None, gain_pan=None, n_taps=wald.DEFAULT_TAPS, return_stats=False):
    """BDSD of every sample.  block: None fits one set of weights per sample; else the side of a block in PAN pixels, a multiple of 32 that divides 4h and
    4w, and every block has its own.  gains_ms: the sensor's MTF gain at Nyquist, one for all bands or one per band (None: wald.DEFAULT_GAIN_MS); gain_pan:
    that of PAN (None: wald.DEFAULT_GAIN_PAN); n_taps: odd, in 1 .. 63.  return_stats: also the weights gamma, a float64 [B, nby, nbx, C, C + 1] device
    tensor (column C weighs PAN); a degenerate block has zeros"""
    if isinstance(n_taps, bool) or int(n_taps) != n_taps or n_taps < 1 or n_taps > 63 or n_taps % 2 == 0:
        raise ValueError(f'bdsd: n_taps must be odd, in 1 .. 63 (got {n_taps!r})')
    if torch.is_tensor(ms) and ms.dim() == 4:
        blk = _block(block, *ms.shape[1:])
    ms, pan, shape = _prepare('bdsd', ms, pan)
    B, C, h, w = shape
    taps_ms = _device_taps(ms.device, _gains(gains_ms, C), n_taps)
    taps_pan = _device_taps(ms.device, (float(wald.DEFAULT_GAIN_PAN if gain_pan is None else gain_pan),), n_taps)
    F, L = taps_ms.shape[0], _lib.lib()
    nby, nbx = (4 * h // blk, 4 * w // blk) if blk else (1, 1)
    with torch.cuda.device(ms.device):
        ws = _scratch(ms.device, 'lg_bdsd_workspace_bytes', B, C, h, w, blk)
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        stats = torch.empty(B, nby, nbx, C, C + 1, dtype=torch.float64, device=ms.device) if return_stats else None
        _lib.check(L.lg_bdsd(_ptr(ms), _ptr(pan), _ptr(out), _ptr(stats) if return_stats else None, _ptr(taps_ms), F, _ptr(taps_pan), int(n_taps), blk, B, C, h,
                             w, _ptr(ws), ws.numel() * 8, _stream_ptr()), 'lg_bdsd')
    return (out, stats) if return_stats else out


def fuse_scene(ms, pan, block=None, gains_ms=None, gain_pan=None, n_taps=wald.DEFAULT_TAPS, bit_depth=None, norm_input=False, out_dtype='float32',
               device=None):
    """One whole scene through BDSD in ONE call: MS [C, h, w], PAN [1, 4h, 4w] -> [C, 4h, 4w] on the device.  The samples, the normalisation and out_dtype
    are classical.fuse_scene's."""
    return _fuse_scene(lambda m, p: bdsd(m, p, block, gains_ms, gain_pan, n_taps), ms, pan, bit_depth, norm_input, out_dtype, device)


@MODELS.register_module()
class BDSD(_Classical):
    """cfg.bdsd_block: the side of a block in PAN pixels (None: the global form); cfg.mtf_gains_ms, cfg.mtf_gain_pan: the sensor's gains; cfg.mtf_taps: the
    tap count (41)"""

    def __init__(self, cfg, logger, train_data_loader, test_data_loader0, test_data_loader1):
        super().__init__(cfg, logger, train_data_loader, test_data_loader0, test_data_loader1)
        self.block, self.gains_ms, self.gain_pan = cfg.get('bdsd_block'), cfg.get('mtf_gains_ms'), cfg.get('mtf_gain_pan')
        self.n_taps = cfg.get('mtf_taps', wald.DEFAULT_TAPS)
        if (self.gains_ms is None or self.gain_pan is None) and logger is not None:
            logger.info(f'BDSD: no mtf_gains_ms / mtf_gain_pan in the config: the bands take the MTF gain {wald.DEFAULT_GAIN_MS}, PAN {wald.DEFAULT_GAIN_PAN}, '
                        "placeholders and not a sensor's values")

    def get_model_output(self, input_batch):
        return bdsd(input_batch['input_lr'], input_batch['input_pan'], self.block, self.gains_ms, self.gain_pan, self.n_taps)
