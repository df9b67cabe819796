"""CPU: the boundary of the device evaluation indices (lgteun_amd/device_metrics.py; C ABI lg_iqa_* of include/lgteun_hip.h, kernels in
lgteun_amd/csrc/k_iqa.hip): the exported names, argument validation before any HIP call, workspace sizes, the header's constants against
metrics.py, and the runner's cfg.eval_metrics switch.  The values themselves are tested on the GPU (tests/test_gpu_metrics.py)."""
import ctypes
import os
import re

import pytest

from lgteun_amd import metrics as mtc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('lg_iqa_workspace_bytes', 'lg_iqa_ref', 'lg_iqa_no_ref')


def _lib():
    from lgteun_amd import _lib
    return _lib, _lib.lib()


def test_device_metric_names_are_exported():
    import lgteun_amd
    from lgteun_amd import device_metrics
    assert lgteun_amd.ref_evaluate_batch is device_metrics.ref_evaluate_batch
    assert lgteun_amd.no_ref_evaluate_batch is device_metrics.no_ref_evaluate_batch
    assert device_metrics.REF_NAMES == ('PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS')
    assert device_metrics.NO_REF_NAMES == ('D_lambda', 'D_s', 'QNR')
    lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    for name in NEW:
        assert name in lib_mod.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr), name
        assert hasattr(ctypes.CDLL(lib_mod.LIB_PATH), name), name


def test_header_constants_equal_the_metrics_constants():
    hdr = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()

    def define(name):
        return float(re.search(rf'#define {name} ([0-9.]+)', hdr).group(1))
    assert define('LG_IQA_PEAK') == mtc.PEAK
    assert define('LG_IQA_SSIM_TAPS') == mtc.SSIM_TAPS
    assert define('LG_IQA_SSIM_SIGMA') == mtc.SSIM_SIGMA
    assert define('LG_IQA_Q_BLOCK') == mtc.Q_BLOCK
    assert define('LG_IQA_RATIO') == mtc.ERGAS_RATIO
    assert define('LG_IQA_QNR_BLOCK') == mtc.QNR_BLOCK
    assert define('LG_IQA_MTF_TAPS') == mtc.MTF_TAPS
    assert define('LG_IQA_MTF_GAIN') == mtc.MTF_GAIN_PAN


def test_workspace_bytes_is_zero_for_shapes_without_indices():
    _, L = _lib()
    ws = L.lg_iqa_workspace_bytes
    assert ws(1, 4, 128, 128, 0) > 0 and ws(1, 4, 128, 128, 1) > 0
    assert ws(32, 4, 128, 128, 0) > ws(1, 4, 128, 128, 0) and ws(1, 8, 400, 400, 1) > ws(1, 4, 400, 400, 1)
    assert ws(3, 4, 16, 16, 0) > 0 and ws(1, 4, 11, 11, 0) > 0
    for B, C, H, W in ((0, 4, 64, 64), (1, 1, 64, 64), (1, 17, 64, 64), (1, 4, 10, 64), (1, 4, 64, 10)):
        assert ws(B, C, H, W, 0) == 0 and ws(B, C, H, W, 1) == 0, (B, C, H, W)
    for H, W in ((28, 64), (64, 28), (66, 64), (64, 62)):       # no-reference: >= 32 and multiples of 4
        assert ws(1, 4, H, W, 1) == 0 and ws(1, 4, H, W, 0) > 0, (H, W)


def test_argument_validation_without_a_device():
    """every call here is rejected before any HIP call: the pointers are never dereferenced and nothing is launched"""
    lib_mod, L = _lib()
    fake = ctypes.c_void_p(1 << 20)           # never dereferenced: each call below fails validation first
    null = ctypes.c_void_p(0)

    def ref(pred=fake, gt=fake, out=fake, B=1, C=4, H=64, W=64, scale=1.0, ws=fake, nbytes=None):
        nbytes = L.lg_iqa_workspace_bytes(max(B, 1), 4, 64, 64, 0) if nbytes is None else nbytes
        rc = L.lg_iqa_ref(pred, gt, out, B, C, H, W, scale, ws, nbytes, null)
        return rc, L.lg_last_error().decode()

    def no_ref(pred=fake, pan=fake, ms=fake, out=fake, B=1, C=4, H=64, W=64, scale=1.0, ws=fake, nbytes=None):
        nbytes = L.lg_iqa_workspace_bytes(1, 4, 64, 64, 1) if nbytes is None else nbytes
        rc = L.lg_iqa_no_ref(pred, pan, ms, out, B, C, H, W, scale, ws, nbytes, null)
        return rc, L.lg_last_error().decode()

    for kw, msg in ((dict(C=1), 'C must be'), (dict(C=17), 'C must be'), (dict(H=10), 'SSIM window'), (dict(W=8), 'SSIM window'),
                    (dict(B=0), 'B must be'), (dict(B=70000), 'B must be'), (dict(pred=null), 'null pointer'), (dict(gt=null), 'null pointer'),
                    (dict(out=null), 'null pointer'), (dict(ws=null), 'null pointer'), (dict(ws=ctypes.c_void_p((1 << 20) + 4)), 'aligned'),
                    (dict(scale=float('inf')), 'finite')):
        rc, err = ref(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)
    need = L.lg_iqa_workspace_bytes(1, 4, 64, 64, 0)
    rc, err = ref(nbytes=need - 1)
    assert rc < 0 and 'workspace too small' in err, err
    for kw, msg in ((dict(H=28), 'no-reference'), (dict(W=66), 'no-reference'), (dict(C=1), 'C must be'), (dict(pan=null), 'null pointer'),
                    (dict(ms=null), 'null pointer'), (dict(pred=null), 'null pointer'), (dict(out=null), 'null pointer'),
                    (dict(nbytes=L.lg_iqa_workspace_bytes(1, 4, 64, 64, 1) - 1), 'workspace too small')):
        rc, err = no_ref(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)
    assert lib_mod.LG_ABI_VERSION == L.lg_abi_version() == 2          # additions only


def test_unknown_eval_metrics_value_is_rejected(tmp_path):
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    cfg = Config(dict(work_dir=str(tmp_path), datas='GF-2', bit_depth=11, eval_metrics='gpu', loss_cfg={'rec_loss': dict(type='l1', w=1.)}))
    runner = Base_model(cfg, None, None, None, None)
    with pytest.raises(ValueError, match='eval_metrics'):
        runner.test(iter_id=0, ref=True)
    with pytest.raises(ValueError, match='eval_metrics'):
        runner.test(iter_id=0, ref=False)
