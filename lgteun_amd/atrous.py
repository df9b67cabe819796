"""ATWT and AWLP, the a trous members of the multiresolution family, for whole batches on the GPU: the detail of PAN against its two-level undecimated
B3-spline low-pass (one separable 13-tap circular filter), injected additively (ATWT) or in proportion to each band's share of the band mean (AWLP).
MTF-GLP (mtf_glp.py) takes its low-pass from the sensor's MTF at the MS scale; these two take it from a fixed spline at the PAN scale and need no gains.
The definitions are DESIGN.md 3.16; the HIP kernels are in lgteun_amd/csrc/k_classical.hip (C ABI lg_atrous, include/lgteun_hip.h): fp64 arithmetic,
one rounding per output element, no atomics.  There is no CPU path.

`atrous`, `atwt` and `awlp` take normalised float32 NCHW tensors on the GPU -- ms [B, C, h, w], pan [B, 1, 4h, 4w] -- and return [B, C, 4h, 4w] on the same
device; a call copies nothing to or from the host and synchronises nothing.  match: which deviation scales the detail to a band -- 'pan' (std(u_k) /
std(pan), SFIM's scale) or 'lowpass' (std(u_k) / std(P_L), the rule of the current toolbox AWLP).  `ATWT` and `AWLP` are runner classes like
classical.GSA: nothing to train, and `test()` scores them like any network."""
import ctypes

import torch

from . import _lib
from .builder import MODELS
from .classical import _Classical, _fuse_scene, _prepare, _scratch
from .engine import _ptr, _stream_ptr

RULES = {'atwt': _lib.LG_ATROUS_ATWT, 'awlp': _lib.LG_ATROUS_AWLP}
MATCHES = {'pan': _lib.LG_ATROUS_MATCH_PAN, 'lowpass': _lib.LG_ATROUS_MATCH_LOWPASS}
SCENE_METHODS = {'atwt': 'atwt', 'awlp': 'awlp'}      # tools/fuse_scene.py --method -> rule


def _check_words(rule, match):
    if rule not in RULES:
        raise ValueError(f"rule must be 'atwt' or 'awlp' (got {rule!r})")
    if match not in MATCHES:
        raise ValueError(f"match must be 'pan' or 'lowpass' (got {match!r})")


def atrous(ms, pan, rule='awlp', match='pan', return_stats=False):
    """ATWT or AWLP of every sample.  return_stats: also a float64 [B, C + 1] device tensor, per sample the scales a (C) and the deviation they were
    matched to (std(pan) or std(P_L))"""
    _check_words(rule, match)
    ms, pan, shape = _prepare('atrous', ms, pan)
    B, C, h, w = shape
    with torch.cuda.device(ms.device):
        ws = _scratch(ms.device, 'lg_atrous_workspace_bytes', B, C, h, w, MATCHES[match])
        out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
        stats = torch.empty(B, C + 1, dtype=torch.float64, device=ms.device) if return_stats else None
        args = _lib.LgAtrousArgs(ctypes.sizeof(_lib.LgAtrousArgs), RULES[rule], MATCHES[match], B, C, h, w, _ptr(ms), _ptr(pan), _ptr(out),
                                 _ptr(stats) if return_stats else None, _ptr(ws), ws.numel() * 8, _stream_ptr())
        _lib.check(_lib.lib().lg_atrous(ctypes.byref(args)), 'lg_atrous')
    return (out, stats) if return_stats else out


def atwt(ms, pan, match='pan', return_stats=False):
    """out_k = clip(u_k + a_k (pan - P_L))"""
    return atrous(ms, pan, 'atwt', match, return_stats)


def awlp(ms, pan, match='pan', return_stats=False):
    """out_k = clip(u_k + a_k (pan - P_L) u_k / (mean over the bands of u + 1e-8))"""
    return atrous(ms, pan, 'awlp', match, return_stats)


def fuse_scene(rule, ms, pan, match='pan', bit_depth=None, norm_input=False, out_dtype='float32', device=None):
    """One whole scene through ATWT or AWLP in ONE call: MS [C, h, w], PAN [1, 4h, 4w] -> [C, 4h, 4w] on the device.  The samples, the normalisation and
    out_dtype are classical.fuse_scene's."""
    _check_words(rule, match)
    return _fuse_scene(lambda m, p: atrous(m, p, rule, match), ms, pan, bit_depth, norm_input, out_dtype, device)


class _Atrous(_Classical):
    """cfg.atrous_match: 'pan' (the default) or 'lowpass'"""
    rule = None

    def __init__(self, cfg, logger, train_data_loader, test_data_loader0, test_data_loader1):
        super().__init__(cfg, logger, train_data_loader, test_data_loader0, test_data_loader1)
        self.match = cfg.get('atrous_match', 'pan')
        _check_words(self.rule, self.match)

    def get_model_output(self, input_batch):
        return atrous(input_batch['input_lr'], input_batch['input_pan'], self.rule, self.match)


@MODELS.register_module()
class ATWT(_Atrous):
    rule = 'atwt'


@MODELS.register_module()
class AWLP(_Atrous):
    rule = 'awlp'
