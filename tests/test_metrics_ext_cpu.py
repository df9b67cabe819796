"""CPU: the extended evaluation indices of lgteun_amd/metrics.py -- the hypercomplex product, Q2n, SCC, CC, D_lambda_K and HQNR -- against
the properties their definitions give them, and the boundary of their device versions (C ABI lg_iqa_ext_workspace_bytes /
lg_iqa_ref_ext / lg_iqa_q2n of include/lgteun_hip.h, lgteun_amd/device_metrics.py): exported names, argtypes, validation before any HIP
call.  The device values are tested on the GPU (tests/test_gpu_metrics_ext.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lgteun_amd import metrics as mtc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('lg_iqa_ext_workspace_bytes', 'lg_iqa_ref_ext', 'lg_iqa_q2n')


def image(C, H, W, seed):
    """11-bit data with correlated bands: a smooth scene plus band offsets and noise, as float32 (H, W, C)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 900 + 500 * np.sin(yy / 7.0) * np.cos(xx / 5.0) + 200 * np.sin((yy + 2 * xx) / 11.0)
    img = base[..., None] * (0.6 + 0.1 * np.arange(C)) + 60 * np.arange(C) + rng.normal(0, 40, (H, W, C))
    return np.clip(img, 0, 2047).astype(np.float32)


def noisy(img, sigma, seed):
    return np.clip(img + np.random.default_rng(seed).normal(0, sigma, img.shape), 0, 2047).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [2, 4, 8])
def test_hypercomplex_product_is_norm_multiplicative_and_x_conj_x_is_real(N):
    rng = np.random.default_rng(N)
    x, y = rng.standard_normal((2, 500, N)) * 10.0
    p = mtc.hmul(x, y)
    nx, ny = np.linalg.norm(x, axis=-1), np.linalg.norm(y, axis=-1)
    assert np.max(np.abs(np.linalg.norm(p, axis=-1) - nx * ny) / (nx * ny)) <= 1e-14
    s = mtc.hmul(x, mtc.hconj(x))
    assert np.all(s[:, 1:] == 0.0) and np.max(np.abs(s[:, 0] - nx * nx) / (nx * nx)) <= 1e-14
    assert np.array_equal(mtc.hconj(x)[:, 0], x[:, 0]) and np.array_equal(mtc.hconj(x)[:, 1:], -x[:, 1:])
    with pytest.raises(ValueError):
        mtc.hmul(np.ones(3), np.ones(3))


def test_hypercomplex_product_at_n2_is_the_complex_product():
    x, y = np.array([1.5, -2.0]), np.array([0.25, 3.0])
    assert np.array_equal(mtc.hmul(x, y), [1.5 * 0.25 + 2.0 * 3.0, 1.5 * 3.0 - 2.0 * 0.25])


@pytest.mark.parametrize('C,H,W', [(4, 32, 32), (8, 48, 80), (3, 64, 96)])
def test_q2n_of_identical_images_is_one(C, H, W):
    img = image(C, H, W, seed=H + C)
    assert abs(1.0 - mtc.q2n(img, img)) <= 1e-12
    assert len(mtc.q2n_blocks(img, img)) == -(-H // 32) * -(-W // 32)


def test_q2n_pads_bands_with_zero_planes():
    gt = image(3, 64, 96, seed=1)
    fu = noisy(gt, 60, 2)
    z = np.zeros((64, 96, 1), np.float32)
    assert mtc.q2n(gt, fu) == mtc.q2n(np.concatenate([gt, z], 2), np.concatenate([fu, z], 2))
    gt5, fu5 = image(5, 40, 32, seed=3), noisy(image(5, 40, 32, seed=3), 60, 4)
    z3 = np.zeros((40, 32, 3), np.float32)
    assert mtc.q2n(gt5, fu5) == mtc.q2n(np.concatenate([gt5, z3], 2), np.concatenate([fu5, z3], 2))


def test_q2n_extension_mirrors_with_the_edge():
    gt, fu = image(4, 40, 48, seed=5), noisy(image(4, 40, 48, seed=5), 60, 6)

    def extend(v):
        v = np.concatenate([v, v[39:15:-1]], axis=0)            # 24 rows: 39, 38, ..., 16
        return np.concatenate([v, v[:, 47:31:-1]], axis=1)      # 16 columns: 47, ..., 32
    assert extend(gt).shape == (64, 64, 4)
    assert mtc.q2n(gt, fu) == mtc.q2n(extend(gt), extend(fu))


def test_q2n_falls_with_noise_and_sees_swapped_bands():
    for C, H, W in ((4, 64, 64), (8, 48, 80)):
        gt = image(C, H, W, seed=7)
        q30, q120 = mtc.q2n(gt, noisy(gt, 30, 8)), mtc.q2n(gt, noisy(gt, 120, 9))
        assert 1.0 > q30 > q120 > 0.0, (q30, q120)
        assert mtc.q2n(gt, gt[..., ::-1].copy()) < q120
        assert mtc.q2n(gt, 0.5 * gt + 100.0) < 1.0                  # a change of gain and offset: contrast and bias terms


def test_q2n_flat_blocks():
    flat = np.full((32, 64, 4), np.float32(1234.567))
    assert mtc.q2n(flat, flat) == 1.0                                                   # t3 == 0: |bias| of equal means
    assert np.array_equal(mtc.q2n_blocks(np.zeros((32, 32, 4)), np.zeros((32, 32, 4))), [1.0])
    # one flat block beside a varying one: the flat block alone takes the branch
    gt = image(4, 32, 64, seed=10)
    gt[:, :32] = np.float32(0.99987 * 2047.5)
    blocks = mtc.q2n_blocks(gt, gt)
    assert blocks[0] == 1.0 and abs(blocks[1] - 1.0) <= 1e-12
    # the tree of halvings is what makes the branch reachable: P2 equals M2 to the last bit for any constant
    for v in (3.0, 0.1, 1234.567, 2047.0):
        assert mtc.q2n(np.full((32, 32, 3), np.float32(v)), np.full((32, 32, 3), np.float32(v))) == 1.0
    # a flat ground-truth block under a varying fused block: c = 1 instead of a division by eps; finite and far from 1
    fu = image(4, 32, 32, seed=11)
    q = mtc.q2n(np.full((32, 32, 4), np.float32(800.0)), fu)
    assert np.isfinite(q) and 0.0 <= q < 0.5
    with pytest.raises(ValueError, match='>= 32'):
        mtc.q2n(np.zeros((31, 40, 4)), np.zeros((31, 40, 4)))
    with pytest.raises(ValueError, match='bands'):
        mtc.q2n(np.zeros((32, 32, 9)), np.zeros((32, 32, 9)))
    with pytest.raises(ValueError, match='block'):
        mtc.q2n(flat, flat, block=16)


def test_scc():
    gt = image(4, 40, 33, seed=12)
    assert abs(mtc.scc(gt, 2.5 * gt.astype(np.float64) + 7.0) - 1.0) <= 1e-12
    assert abs(mtc.scc(gt, gt) - 1.0) <= 1e-12
    assert 0.0 < mtc.scc(gt, noisy(gt, 120, 13)) < 1.0
    flat, other = np.full((40, 33, 4), 5.0), np.full((40, 33, 4), 9.0)
    assert mtc.scc(flat, other) == 1.0 and mtc.scc(flat, gt) == 0.0 and mtc.scc(gt, flat) == 0.0
    # brute force at one pixel: the Sobel pair, no padding
    x = gt[..., 0].astype(np.float64)
    k = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float64)
    win = x[4:7, 9:12]
    want = np.hypot((k * win).sum(), (k.T * win).sum())
    assert abs(mtc._sobel_magnitude(gt.astype(np.float64))[4, 9, 0] - want) <= 1e-9 * want
    assert mtc._sobel_magnitude(gt.astype(np.float64)).shape == (38, 31, 4)


def test_cc_is_the_mean_of_pearsons_r_and_nan_for_a_constant_band():
    gt = image(4, 36, 44, seed=14)
    fu = noisy(gt, 90, 15)
    want = np.mean([np.corrcoef(gt[..., k].ravel().astype(np.float64), fu[..., k].ravel().astype(np.float64))[0, 1] for k in range(4)])
    assert mtc.cc(gt, fu) == want and 0.5 < want < 1.0
    fu[..., 2] = 100.0
    assert np.isnan(mtc.cc(gt, fu)) and np.isnan(mtc.cc(fu, gt))


@pytest.mark.parametrize('gains', [None, 0.25, (0.3, 0.25, 0.2, 0.35)])
def test_d_lambda_k_and_hqnr_are_composed_of_their_parts(gains):
    from lgteun_amd import wald
    assert mtc.MTF_TAPS == wald.DEFAULT_TAPS
    fused = image(4, 128, 160, seed=16)
    ms = noisy(fused[1::4, 1::4], 20, 17)
    pan = fused.mean(axis=2).astype(np.float32)
    g = wald._gain_rows(gains, 4, wald.DEFAULT_GAIN_MS, 'gains_ms')
    assert gains is not None or g == [0.3] * 4
    degraded = np.stack([mtc.fir_decimate4(fused[..., k], wald.mtf_taps(g[k], 41), 2) for k in range(4)], axis=-1)
    assert degraded.dtype == np.float32 and degraded.shape == (32, 40, 4)
    dk = mtc.d_lambda_k(fused, ms, gains)
    assert dk == 1.0 - mtc.q2n(ms, degraded) and 0.0 < dk < 1.0
    assert mtc.hqnr(fused, ms, pan, gains) == (1.0 - dk) * (1.0 - mtc.d_s(fused, ms, pan))
    row = mtc.no_ref_evaluate_ext(fused, pan, ms, gains)
    assert row[:3] == mtc.no_ref_evaluate(fused, pan, ms) and row[3] == dk and row[4] == (1.0 - dk) * (1.0 - row[1])
    with pytest.raises(ValueError, match='128'):
        mtc.d_lambda_k(fused[:124], ms[:31], gains)


def test_fir_decimate4_is_the_documented_arithmetic():
    """the sample (i, j) by hand: the pass along the row, then along the column, clamped indices, ascending k, one rounding to fp32"""
    from lgteun_amd import wald
    x = image(1, 16, 24, seed=18)[..., 0]
    taps = wald.mtf_taps(0.3, 9)
    got = mtc.fir_decimate4(x, taps, phase=2)
    for i, j in ((0, 0), (3, 5), (1, 2)):
        col = 0.0
        for k in range(9):
            r = min(max(4 * i + 2 + k - 4, 0), 15)
            row = 0.0
            for l in range(9):
                row = row + taps[l] * float(x[r, min(max(4 * j + 2 + l - 4, 0), 23)])
            col = col + taps[k] * row
        assert got[i, j] == np.float32(col), (i, j)


def test_ref_evaluate_ext_appends_to_the_five():
    gt = image(4, 48, 40, seed=19)
    fu = noisy(gt, 50, 20)
    row = mtc.ref_evaluate_ext(fu, gt)
    assert row[:5] == mtc.ref_evaluate(fu, gt) and row[5:] == [mtc.q2n(gt, fu), mtc.scc(gt, fu), mtc.cc(gt, fu)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the boundary of the device versions
# ---------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from lgteun_amd import _lib
    return _lib, _lib.lib()


def test_new_symbols_are_bound_declared_and_exported():
    import lgteun_amd
    from ctypes import c_float, c_int32, c_size_t, c_void_p
    from lgteun_amd import device_metrics as dmt
    lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    for name in NEW:
        assert name in lib_mod.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr), name
        assert hasattr(ctypes.CDLL(lib_mod.LIB_PATH), name), name
    call = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_size_t, c_void_p]
    assert lib_mod.SIGNATURES['lg_iqa_ext_workspace_bytes'] == (c_size_t, [c_int32] * 4)
    assert lib_mod.SIGNATURES['lg_iqa_ref_ext'] == (c_int32, call) and lib_mod.SIGNATURES['lg_iqa_q2n'] == (c_int32, call)
    assert L.lg_iqa_ref_ext.argtypes == call and L.lg_iqa_ext_workspace_bytes.restype is c_size_t
    assert re.search(r'size_t lg_iqa_ext_workspace_bytes\(int32_t B, int32_t C, int32_t H, int32_t W\);', hdr)
    assert re.search(r'int lg_iqa_ref_ext\(const float\* pred, const float\* gt, double\* out, int32_t B, int32_t C, int32_t H, int32_t W, float scale,\s+'
                     r'void\* workspace, size_t workspace_bytes, void\* stream\);', hdr)
    assert '#define LG_ABI_VERSION 2' in hdr and lib_mod.LG_ABI_VERSION == L.lg_abi_version() == 2          # additions only
    assert float(re.search(r'#define LG_IQA_Q2N_BLOCK ([0-9]+)', hdr).group(1)) == mtc.Q2N_BLOCK
    assert float(re.search(r'#define LG_IQA_Q2N_MAX_BANDS ([0-9]+)', hdr).group(1)) == mtc.Q2N_MAX_BANDS
    assert dmt.REF_EXT_NAMES == ('PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS', 'Q2n', 'SCC', 'CC')
    assert dmt.NO_REF_EXT_NAMES == ('D_lambda', 'D_s', 'QNR', 'D_lambda_K', 'HQNR')
    assert lgteun_amd.ref_evaluate_ext_batch is dmt.ref_evaluate_ext_batch
    assert lgteun_amd.no_ref_evaluate_ext_batch is dmt.no_ref_evaluate_ext_batch


def test_ext_workspace_bytes_is_zero_for_rejected_shapes():
    _, L = _lib()
    ws = L.lg_iqa_ext_workspace_bytes
    assert ws(1, 4, 32, 32) > 0 and ws(1, 2, 32, 32) > 0 and ws(1, 8, 48, 80) > 0
    assert ws(32, 4, 128, 128) > ws(1, 4, 128, 128) and ws(1, 8, 128, 128) > ws(1, 4, 128, 128)
    for B, C, H, W in ((1, 1, 64, 64), (1, 9, 64, 64), (1, 4, 31, 64), (1, 4, 64, 31), (0, 4, 64, 64), (70000, 4, 64, 64), (1, 4, 8200, 64)):
        assert ws(B, C, H, W) == 0, (B, C, H, W)


def test_ext_argument_validation_without_a_device():
    """every call here is rejected before any HIP call: the pointers are never dereferenced and nothing is launched"""
    _, L = _lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)
    need = L.lg_iqa_ext_workspace_bytes(1, 4, 64, 64)

    def call(fn, a=fake, b=fake, out=fake, B=1, C=4, H=64, W=64, scale=1.0, ws=fake, nbytes=need):
        rc = fn(a, b, out, B, C, H, W, scale, ws, nbytes, null)
        return rc, L.lg_last_error().decode()

    for fn, who in ((L.lg_iqa_ref_ext, 'lg_iqa_ref_ext'), (L.lg_iqa_q2n, 'lg_iqa_q2n')):
        for kw, msg in ((dict(C=1), 'C must be'), (dict(C=9), 'C must be'), (dict(H=31), 'Q2n block'), (dict(W=31), 'Q2n block'), (dict(B=0), 'B must be'),
                        (dict(a=null), 'null pointer'), (dict(b=null), 'null pointer'), (dict(out=null), 'null pointer'), (dict(ws=null), 'null pointer'),
                        (dict(ws=ctypes.c_void_p((1 << 20) + 4)), 'aligned'), (dict(scale=float('nan')), 'finite'),
                        (dict(nbytes=need - 1), 'workspace too small')):
            rc, err = call(fn, **kw)
            assert rc < 0 and msg in err and err.startswith(who), (who, kw, rc, err)


def test_cpu_tensors_raise_value_error():
    import torch
    from lgteun_amd import device_metrics as dmt
    a = torch.rand(1, 4, 32, 32)
    with pytest.raises(ValueError, match='on the GPU'):
        dmt.ref_evaluate_ext_batch(a, a)
    b = torch.rand(1, 4, 128, 128)
    with pytest.raises(ValueError, match='on the GPU'):
        dmt.no_ref_evaluate_ext_batch(b, torch.rand(1, 1, 128, 128), a)


def test_unknown_eval_indices_value_is_rejected(tmp_path):
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    cfg = Config(dict(work_dir=str(tmp_path), datas='GF-2', bit_depth=11, eval_indices='all', loss_cfg={'rec_loss': dict(type='l1', w=1.)}))
    runner = Base_model(cfg, None, None, None, None)
    for ref in (True, False):
        with pytest.raises(ValueError, match='eval_indices'):
            runner.test(iter_id=0, ref=ref)
