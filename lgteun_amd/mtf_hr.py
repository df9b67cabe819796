"""FS, HPM-R, HPM-H and BT-H, the regression-based and haze-corrected members of the MTF-GLP family, for whole batches on the GPU: the rows recent
comparisons report first among the classical methods.  All four take the low-pass of the RAW PAN under the sensor's MTF at the MS scale (no histogram
matching): FS injects the detail with a full-scale regression gain, HPM-R modulates by a regression-matched ratio, HPM-H and BT-H subtract a dark-pixel
haze estimate before they modulate.  The definitions are DESIGN.md 3.17; the HIP kernels are the k_hr_* of lgteun_amd/csrc/k_classical.hip (C ABI
lg_mtf_hr, include/lgteun_hip.h): fp64 arithmetic, one rounding per output element, no atomics.  There is no CPU path.

`fuse` and its shorthands `fs`, `hpm_r`, `hpm_h`, `bt_h` take normalised float32 NCHW tensors on the GPU -- ms [B, C, h, w], pan [B, 1, 4h, 4w] -- and
return [B, C, 4h, 4w] on the same device; a call copies nothing to or from the host and synchronises nothing.  The MTF gains at Nyquist are per band
and per sensor and are the CALLER's: without them the bands take wald.DEFAULT_GAIN_MS and PAN (bt_h) wald.DEFAULT_GAIN_PAN, common placeholders and NOT
a sensor's measured values.  `MTF_GLP_FS`, `MTF_GLP_HPM_R`, `MTF_GLP_HPM_H` and `BT_H` are runner classes like classical.GSA: nothing to train, and
`test()` scores them like any network."""
import ctypes

import torch

from . import _lib, wald
from .builder import MODELS
from .classical import _Classical, _fuse_scene, _prepare, _scratch
from .engine import _ptr, _stream_ptr
from .mtf_glp import _device_taps, _gains

RULES = {'fs': _lib.LG_MTFHR_FS, 'hpm_r': _lib.LG_MTFHR_HPM_R, 'hpm_h': _lib.LG_MTFHR_HPM_H, 'bt_h': _lib.LG_MTFHR_BT_H}
SCENE_METHODS = {'fs', 'hpm_r', 'hpm_h', 'bt_h'}      # tools/fuse_scene.py --method: the rule's own name


def _check_rule(rule):
    if rule not in RULES:
        raise ValueError(f"rule must be 'fs', 'hpm_r', 'hpm_h' or 'bt_h' (got {rule!r})")


def fuse(ms, pan, rule, gains_ms=None, gain_pan=None, n_taps=wald.DEFAULT_TAPS, return_stats=False):
    """The rule `rule` ('fs', 'hpm_r', 'hpm_h' or 'bt_h') on every sample.  gains_ms: the sensor's MTF gain at Nyquist, one for all bands or one per band
    (None: wald.DEFAULT_GAIN_MS); gain_pan: that of PAN, which 'bt_h' filters with in place of gains_ms (None: wald.DEFAULT_GAIN_PAN); n_taps: odd, in
    1 .. 63.  return_stats: also a float64 [B, 2C + 2] device tensor, unused slots 0 -- fs: g; hpm_r: g, b; hpm_h: H, H_P; bt_h: H, w_1 .. w_C, w_0, H_I"""
    _check_rule(rule)
    ms, pan, shape = _prepare('mtf_hr', ms, pan)
    B, C, h, w = shape
    if rule == 'bt_h':
        taps = _device_taps(ms.device, (float(wald.DEFAULT_GAIN_PAN if gain_pan is None else gain_pan),), n_taps)
    else:
        taps = _device_taps(ms.device, _gains(gains_ms, C), n_taps)
    F = taps.shape[0]
    with torch.cuda.device(ms.device):
        ws = _scratch(ms.device, 'lg_mtf_hr_workspace_bytes', B, C, h, w, F, RULES[rule])
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        stats = torch.empty(B, 2 * C + 2, dtype=torch.float64, device=ms.device) if return_stats else None
        args = _lib.LgMtfHrArgs(ctypes.sizeof(_lib.LgMtfHrArgs), RULES[rule], F, taps.shape[1], B, C, h, w, _ptr(ms), _ptr(pan), _ptr(out),
                                _ptr(stats) if return_stats else None, _ptr(taps), _ptr(ws), ws.numel() * 8, _stream_ptr())
        _lib.check(_lib.lib().lg_mtf_hr(ctypes.byref(args)), 'lg_mtf_hr')
    return (out, stats) if return_stats else out


def fs(ms, pan, gains_ms=None, n_taps=wald.DEFAULT_TAPS, return_stats=False):
    """out_k = clip(u_k + g_k (pan - L_k)), g_k = cov(u_k, pan) / cov(L_k, pan)"""
    return fuse(ms, pan, 'fs', gains_ms, None, n_taps, return_stats)


def hpm_r(ms, pan, gains_ms=None, n_taps=wald.DEFAULT_TAPS, return_stats=False):
    """out_k = clip(u_k (g_k pan + b_k) / (g_k L_k + b_k)), g_k = cov(u_k, L_k) / var(L_k), b_k = mean u_k - g_k mean L_k"""
    return fuse(ms, pan, 'hpm_r', gains_ms, None, n_taps, return_stats)


def hpm_h(ms, pan, gains_ms=None, n_taps=wald.DEFAULT_TAPS, return_stats=False):
    """out_k = clip((u_k - H_k) (pan - H_P,k) / (L_k - H_P,k) + H_k), H the dark-pixel haze of ms, H_P its image under the regression of D_k on ms"""
    return fuse(ms, pan, 'hpm_h', gains_ms, None, n_taps, return_stats)


def bt_h(ms, pan, gain_pan=None, n_taps=wald.DEFAULT_TAPS, return_stats=False):
    """out_k = clip((u_k - H_k) (pan - H_I) / (I - H_I) + H_k), I = w_0 + sum_j w_j u_j the regression of the low-passed PAN on ms"""
    return fuse(ms, pan, 'bt_h', None, gain_pan, n_taps, return_stats)


def fuse_scene(rule, ms, pan, gains_ms=None, gain_pan=None, n_taps=wald.DEFAULT_TAPS, bit_depth=None, norm_input=False, out_dtype='float32', device=None):
    """One whole scene through the rule `rule` in ONE call: MS [C, h, w], PAN [1, 4h, 4w] -> [C, 4h, 4w] on the device.  The samples, the normalisation and
    out_dtype are classical.fuse_scene's."""
    _check_rule(rule)
    return _fuse_scene(lambda m, p: fuse(m, p, rule, gains_ms, gain_pan, n_taps), ms, pan, bit_depth, norm_input, out_dtype, device)


class _MtfHr(_Classical):
    """cfg.mtf_gains_ms, cfg.mtf_gain_pan: the sensor's gains (the bands': a scalar or one per band); cfg.mtf_taps: the tap count (41)"""
    rule = None

    def __init__(self, cfg, logger, train_data_loader, test_data_loader0, test_data_loader1):
        super().__init__(cfg, logger, train_data_loader, test_data_loader0, test_data_loader1)
        self.gains_ms, self.gain_pan = cfg.get('mtf_gains_ms'), cfg.get('mtf_gain_pan')
        self.n_taps = cfg.get('mtf_taps', wald.DEFAULT_TAPS)
        missing = self.gain_pan is None if self.rule == 'bt_h' else self.gains_ms is None
        if missing and logger is not None:
            what = f'PAN takes the MTF gain {wald.DEFAULT_GAIN_PAN}' if self.rule == 'bt_h' else f'every band takes the MTF gain {wald.DEFAULT_GAIN_MS}'
            logger.info(f'{type(self).__name__}: no {"mtf_gain_pan" if self.rule == "bt_h" else "mtf_gains_ms"} in the config: {what}, '
                        "a placeholder and not a sensor's value")

    def get_model_output(self, input_batch):
        return fuse(input_batch['input_lr'], input_batch['input_pan'], self.rule, self.gains_ms, self.gain_pan, self.n_taps)


@MODELS.register_module()
class MTF_GLP_FS(_MtfHr):
    rule = 'fs'


@MODELS.register_module()
class MTF_GLP_HPM_R(_MtfHr):
    rule = 'hpm_r'


@MODELS.register_module()
class MTF_GLP_HPM_H(_MtfHr):
    rule = 'hpm_h'


@MODELS.register_module()
class BT_H(_MtfHr):
    rule = 'bt_h'
