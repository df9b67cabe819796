"""No GPU: the surface of the component-substitution baselines (lgteun_amd/cs.py: IHS, Brovey, GS, PCA) -- the registry entries, the C ABI names, the argument
checks of the library (lg_cs returns before it touches a device), the command line -- and the arithmetic the kernels rest on, in numpy: the exported taps
against the impulse response of classical_ref.interp23, the MS-scale identities (lgteun_amd/csrc/k_cs.hip forms every moment from ms itself and one adjoint
pass over PAN) against the direct moments of u, the closed forms of DESIGN.md 3.15 against the direct forms of tests/cs_ref.py, PCA's sign rule, and the
inputs of the GPU tests.

Measured: taps against numpy 1.1e-16 (t), 5.6e-17 (R); MS-scale moments against the direct ones at most 4.2e-14 relative; over the GPU cases the eigen gap
(lambda_1 - lambda_2) / lambda_1 is 0.81 - 0.91, the float32 restatement errs by 4.2e-8 - 3.7e-7 and no element sits on a clip boundary."""
import ctypes
import importlib.util
import logging
import os

import numpy as np
import pytest

import classical_ref as cr
import cs_ref as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lg_cs_workspace_bytes', 'lg_cs', 'lg_cs_taps')
RUNNERS = {'IHS': 'ihs', 'Brovey': 'brovey', 'GS': 'gs', 'PCA': 'pca'}
ISSUE_SHAPES = [(4, 4, 4, 1), (4, 8, 8, 2), (4, 5, 7, 2), (8, 12, 8, 3), (8, 32, 32, 3), (4, 40, 24, 2), (4, 136, 256, 1), (3, 6, 9, 1), (16, 8, 8, 1)]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_exported_taps_are_those_of_interp23():
    from lgteun_amd import _lib
    L = _lib.lib()
    t, R, st = cs.taps()
    a, b = (ctypes.c_double * 67)(), (ctypes.c_double * 33)()
    assert L.lg_cs_taps(a, b) == 0
    a, b = np.array(a), np.array(b)
    print(f'lg_cs_taps against numpy: t {np.abs(a - t).max():.3e}, R {np.abs(b - R).max():.3e}; sum t = {a.sum():.12f}')
    assert len(t) == 67 and len(R) == 33
    assert np.abs(a - t).max() <= 1e-15 and np.abs(b - R).max() <= 1e-15
    assert np.array_equal(b, b[::-1]) and a[33] == 1.0
    assert f'{a.sum():.11f}' == '3.99999999838' and f'{st:.11f}' == '3.99999999838'
    assert L.lg_cs_taps(None, b.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) < 0 and b't67 is NULL' in L.lg_last_error()
    assert L.lg_cs_taps(a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None) < 0 and b'r33 is NULL' in L.lg_last_error()


@pytest.mark.parametrize('C,h,w', [(4, 4, 4), (4, 5, 7), (8, 12, 8)])
def test_ms_scale_moments_equal_the_direct_moments(C, h, w):
    """(4, 4, 4): t wraps four times over the 16 PAN pixels of a side, R eight times over the 4 MS pixels"""
    ms, pan = cs.make_common(C, h, w, seed=3)
    direct = cs.stats_of(cr.interp23(ms), pan.astype(np.float64), 'ihs', None, np.float64)
    route = cs.ms_scale_moments(ms, pan)
    for key in ('m', 'mp', 'S', 'r', 'vp'):
        e = rel(route[key], direct[key])
        print(f'C={C} h={h} w={w}: {key} by the MS-scale route against np.cov of u: {e:.3e}')
        assert e <= 1e-12, key


def test_constant_inputs_have_exactly_zero_moments_by_the_ms_scale_route():
    ms, pan = cs.make_common(4, 8, 8, seed=4)
    flat = cs.ms_scale_moments(ms, np.full_like(pan, 0.3))
    assert flat['vp'] == 0 and not flat['r'].any()
    const = cs.ms_scale_moments(np.full_like(ms, 0.4) * np.arange(1, 5, dtype=np.float32)[:, None, None] / 4, pan)
    assert not const['S'].any()


@pytest.mark.parametrize('mode', cs.MODES)
def test_closed_forms_equal_the_direct_forms(mode):
    """out_k = clip(u_k + g_k (P - I)) with the moments of the MS-scale route against the restatement (GS with its re-centring line)"""
    for C, h, w in ((4, 5, 7), (8, 12, 8), (3, 6, 9)):
        ms, pan = cs.make_common(C, h, w, seed=5)
        want, stats, _ = cs.fuse(ms, pan, mode, return_stats=True)
        mo = cs.ms_scale_moments(ms, pan)
        u, p = cr.interp23(ms), pan.astype(np.float64)
        if mode == 'pca':
            wv = np.linalg.eigh(mo['S'])[1][:, -1]
            wv = -wv if wv @ mo['r'] < 0 else wv
        else:
            wv = np.full(C, 1.0 / C)
        vI, mI = wv @ mo['S'] @ wv, wv @ mo['m']
        a = np.sqrt(vI / mo['vp'])
        g = {'ihs': np.ones(C), 'brovey': np.ones(C), 'gs': mo['S'] @ wv / vI, 'pca': wv}[mode]
        P, I = a * (p - mo['mp']), np.tensordot(wv, u - mo['m'][:, None, None], axes=1)
        got = u * ((P + mI) / (I + mI + cs.EPS)) if mode == 'brovey' else u + g[:, None, None] * (P - I)
        e_out, e_st = float(np.abs(np.clip(got, 0, 1) - want).max()), rel(np.concatenate([wv, g, [a, mI]]), stats)
        print(f'{mode} C={C} h={h} w={w}: closed form against the restatement: output {e_out:.3e}, stats {e_st:.3e}')
        assert e_out <= 1e-12 and e_st <= 1e-12


def test_sign_rule_makes_pca_a_function_of_its_input():
    ms, pan = cs.make_common(4, 8, 8, seed=6)
    a, sa, _ = cs.fuse(ms, pan, 'pca', return_stats=True)
    b, sb, _ = cs.fuse(ms, pan, 'pca', return_stats=True, flip=True)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    assert sa[:4] @ cs.stats_of(cr.interp23(ms), pan.astype(np.float64), 'pca', None, np.float64)['r'] > 0
    with pytest.raises(ValueError, match='no weights'):
        cs.fuse(ms, pan, 'pca', weights=[0.25] * 4)


def test_names_are_declared_bound_and_exported():
    import lgteun_amd
    from lgteun_amd import _lib, cs as pkg
    header = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + '(' in header
        assert hasattr(L, name)
    for code, name in enumerate(('LG_CS_IHS', 'LG_CS_BROVEY', 'LG_CS_GS', 'LG_CS_PCA')):
        assert getattr(_lib, name) == code and f'#define {name} {code}' in header
    assert _lib.LG_ABI_VERSION == 2 and L.lg_abi_version() == 2 and '#define LG_ABI_VERSION 2' in header      # additions only
    assert pkg.MODES == {'ihs': 0, 'brovey': 1, 'gs': 2, 'pca': 3} and pkg.SCENE_METHODS == ('ihs', 'brovey', 'gs', 'pca')
    assert all(callable(getattr(pkg, f)) for f in ('fuse', 'ihs', 'brovey', 'gs', 'pca', 'fuse_scene'))
    for name in RUNNERS:
        assert getattr(lgteun_amd, name) is getattr(pkg, name)
    assert '$(CSRC)/k_cs.hip' in open(os.path.join(ROOT, 'Makefile')).read()


def test_size_function():
    from lgteun_amd import _lib
    L = _lib.lib()
    n1, n2 = L.lg_cs_workspace_bytes(1, 4, 8, 8), L.lg_cs_workspace_bytes(2, 4, 8, 8)
    assert n1 > 0 and n1 % 8 == 0 and n2 > n1
    assert L.lg_cs_workspace_bytes(1, 4, 4096, 4096) >= 8 * 4096 * 4096          # q: one fp64 plane [h, w] per sample
    assert L.lg_cs_workspace_bytes(1, 16, 8, 8) > L.lg_cs_workspace_bytes(1, 2, 8, 8)
    for bad in ((0, 4, 8, 8), (65536, 4, 8, 8), (2, 1, 8, 8), (2, 17, 8, 8), (2, 4, 3, 8), (2, 4, 8, 3), (2, 4, 4097, 8), (2, 4, 8, 4097), (-1, 4, 8, 8)):
        assert L.lg_cs_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_named_before_any_device_call():
    """the pointers are made-up addresses: a call that got past its checks would fault here"""
    from lgteun_amd import _lib
    L = _lib.lib()
    ms, pan, out, ws = 0x10000, 0x20000, 0x30000, 0x50000
    need = L.lg_cs_workspace_bytes(2, 4, 8, 8)
    good = (ctypes.c_double * 4)(0.1, 0.3, 0.4, 0.2)

    def call(ms=ms, pan=pan, out=out, stats=None, weights=None, mode=2, B=2, C=4, h=8, w=8, ws=ws, nbytes=need):
        return L.lg_cs(ms, pan, out, stats, weights, mode, B, C, h, w, ws, nbytes, None)
    cases = [(dict(ms=None), 'ms is NULL'), (dict(pan=None), 'pan is NULL'), (dict(out=None), 'out is NULL'), (dict(ws=None), 'workspace is NULL'),
             (dict(ms=ms + 4), 'ms must be 16-byte aligned'), (dict(pan=pan + 8), 'pan must be 16-byte aligned'), (dict(out=out + 4), 'out must be 16-byte aligned'),
             (dict(stats=0x60004), 'stats must be 8-byte aligned'), (dict(ws=ws + 4), 'workspace must be 8-byte aligned'),
             (dict(C=1), 'C must be'), (dict(C=17), 'C must be'), (dict(h=3), 'h must be'), (dict(w=4097), 'w must be'), (dict(B=0), 'B must be'),
             (dict(B=65536), 'B must be'), (dict(mode=4), 'mode must be'), (dict(mode=-1), 'mode must be'),
             (dict(mode=3, weights=good), 'weights must be NULL for LG_CS_PCA'),
             (dict(weights=(ctypes.c_double * 4)(0.1, float('nan'), 0.4, 0.2)), 'weights[1] must be finite'),
             (dict(weights=(ctypes.c_double * 4)(0.1, 0.2, 0.4, float('inf'))), 'weights[3] must be finite'),
             (dict(nbytes=need - 8), 'workspace_bytes too small'), (dict(B=3), 'workspace_bytes too small')]
    for kw, text in cases:
        assert call(**kw) < 0, text
        assert text in L.lg_last_error().decode() and L.lg_last_error().decode().startswith('cs: '), (text, L.lg_last_error())
    with pytest.raises(_lib.LgteunHipError, match='out is NULL'):
        _lib.check(call(out=None), 'lg_cs')


def test_functions_refuse_bad_arguments_before_any_device_call():
    import torch
    from lgteun_amd import cs as pkg
    ms, pan = torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 32, 32)
    for mode in cs.MODES:
        with pytest.raises(ValueError, match='no CPU path'):
            pkg.fuse(ms, pan, mode)
        with pytest.raises(ValueError, match='no CPU path'):
            getattr(pkg, mode)(ms, pan)
    with pytest.raises(ValueError, match="'ihs', 'brovey', 'gs' or 'pca'"):
        pkg.fuse(ms, pan, 'nope')
    with pytest.raises(ValueError, match="'ihs', 'brovey', 'gs' or 'pca'"):
        pkg.fuse_scene('nope', np.zeros((4, 8, 8), np.uint16), np.zeros((1, 32, 32), np.uint16), bit_depth=11)
    with pytest.raises(ValueError, match='float32 NCHW'):
        pkg.ihs(ms.double(), pan)
    # the weights are checked on the host, in front of the call
    assert pkg._weights('gs', None, 4) is None and list(pkg._weights('ihs', (0.1, 0.3, 0.4, 0.2), 4)) == [0.1, 0.3, 0.4, 0.2]
    with pytest.raises(ValueError, match='3 weights for 4 bands'):
        pkg._weights('ihs', [0.2, 0.3, 0.5], 4)
    with pytest.raises(ValueError, match='must be finite'):
        pkg._weights('brovey', [0.2, 0.3, float('nan'), 0.1], 4)
    with pytest.raises(ValueError, match="'pca' takes none"):
        pkg._weights('pca', [0.25] * 4, 4)
    with pytest.raises(ValueError, match='one per band'):
        pkg._weights('gs', 0.25, 4)
    with pytest.raises(ValueError, match="'pca' takes none"):
        pkg.fuse_scene('pca', np.zeros((4, 8, 8), np.uint16), np.zeros((1, 32, 32), np.uint16), weights=[0.25] * 4, bit_depth=11)


@pytest.mark.parametrize('name', sorted(RUNNERS))
def test_registry_builds_the_runner(name, tmp_path):
    from lgteun_amd import MODELS, build_model, cs as pkg
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    assert MODELS.get(name) is getattr(pkg, name) and getattr(pkg, name).mode == RUNNERS[name]
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0))
    runner = build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)
    assert isinstance(runner, Base_model) and runner.module_dict == {} and runner.weights is None
    assert runner.print_total_params() == 0
    runner.train()                                         # nothing to train: returns
    assert runner.save(iter_id=1) is None and not os.path.exists(runner.train_out)
    with pytest.raises(RuntimeError, match='nothing to train'):
        runner.train_iter(1, {})
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0, cs_weights=[0.1, 0.3, 0.4, 0.2]))
    if name == 'PCA':
        with pytest.raises(ValueError, match='takes none'):
            build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)
    else:
        assert list(build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None).weights) == [0.1, 0.3, 0.4, 0.2]


def test_tool_accepts_the_new_methods(capsys):
    from lgteun_amd import classical, cs as pkg, mtf_glp
    assert set(classical.SCENE_METHODS) == {'gsa', 'sfim', 'wavelet'} and set(mtf_glp.SCENE_METHODS) == {'mtf_glp', 'mtf_glp_hpm', 'mtf_glp_cbd'}
    spec = importlib.util.spec_from_file_location('fuse_scene_tool', os.path.join(ROOT, 'tools', 'fuse_scene.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for m in pkg.SCENE_METHODS:
        a = tool.parser().parse_args(['scene', '--method', m])
        assert a.method == m and a.cs_weights is None
    a = tool.parser().parse_args(['scene', '--method', 'gs', '--cs-weights', '0.1', '0.3', '0.4', '0.2'])
    assert a.cs_weights == [0.1, 0.3, 0.4, 0.2]
    with pytest.raises(SystemExit):
        tool.parser().parse_args(['scene', '--method', 'nope'])
    err = capsys.readouterr().err
    assert all(m in err for m in ('gsa', 'mtf_glp_cbd', 'bdsd', 'ihs', 'brovey', 'gs', 'pca'))


@pytest.mark.parametrize('C,h,w,B', cs.SHAPES)
def test_inputs_of_the_gpu_tests(C, h, w, B):
    """per case, on the restatement: clip share at most 2 %, PCA's eigen gap at least 0.5; the float32 run's own error is printed"""
    ms, pan = cs.make_batch(B, C, h, w, seed=C * 100 + h)
    assert ms.dtype == np.float32 and pan.dtype == np.float32 and ms.shape == (B, C, h, w) and pan.shape == (B, 1, 4 * h, 4 * w)
    for b in range(B):
        u64, u32 = cr.interp23(ms[b]), cr.interp23(ms[b], np.float32)
        for mode in cs.MODES:
            raw = cs.fuse(ms[b], pan[b, 0], mode, clip=False, u=u64)
            _, _, st = cs.fuse(ms[b], pan[b, 0], mode, return_stats=True, u=u64)
            e32 = float(np.abs(cs.fuse(ms[b], pan[b, 0], mode, dtype=np.float32, u=u32).astype(np.float64) - np.clip(raw, 0, 1)).max())
            share = float(((raw <= 0) | (raw >= 1)).mean())
            gap = float((st['lam'][-1] - st['lam'][-2]) / st['lam'][-1]) if mode == 'pca' else 1.0
            print(f'{mode} C={C} h={h} w={w} sample {b}: clip share {share:.4f}, float32 restatement {e32:.3e}' + (f', eigen gap {gap:.3f}' if mode == 'pca' else ''))
            assert share <= 0.02 and gap >= 0.5 and not st['degenerate'], (mode, b)


def test_the_cases_are_those_of_the_issue():
    assert cs.SHAPES[:len(ISSUE_SHAPES)] == ISSUE_SHAPES and len(cs.SHAPES) == len(ISSUE_SHAPES) + 1
    C, h, w, B = cs.SHAPES[-1]                             # the Gram pass's own: ragged 16 x 16 tiles in both axes, more tiles than workgroups
    assert h % 16 and w % 16 and -(-h // 16) * -(-w // 16) > 512


@pytest.mark.parametrize('mode', cs.MODES)
def test_clip_case_leaves_the_range_on_both_sides(mode):
    C, h, w, B = cs.CLIP_SHAPE
    ms, pan = cs.make_clip_batch(B, C, h, w, seed=9)
    assert ms.dtype == np.float32 and pan.dtype == np.float32 and ms.min() >= 0 and ms.max() <= 1 and pan.min() >= 0 and pan.max() <= 1
    for b in range(B):
        raw = cs.fuse(ms[b], pan[b, 0], mode, clip=False)
        below, above = float((raw < 0).mean()), float((raw > 1).mean())
        print(f'{mode} sample {b}: {100 * below:.1f} % below 0, {100 * above:.1f} % above 1')
        assert 0.01 < below < 0.5 and 0.01 < above < 0.5, (mode, b, below, above)
