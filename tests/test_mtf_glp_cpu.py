"""No GPU: the surface of the MTF-GLP baselines -- the registry entries, the C ABI names, the argument checks of the library (lg_mtf_glp returns before it
touches a device), the command line -- and self-checks of the numpy restatement the GPU tests compare with (tests/mtf_glp_ref.py): the explicit low-pass
against the scipy form, and the inputs of the GPU tests.

Measured: explicit against scipy low-pass 2.3e-15; clip share of the GPU cases at most 0.45 % (cbd at (4, 5, 7, 2) with per-band gains; glp and hpm 0);
the clip case leaves [0, 1] below on 4.7 - 19.4 % and above on 3.7 - 10.3 % of a sample, per rule."""
import importlib.util
import logging
import os

import numpy as np
import pytest

import classical_ref as cr
import mtf_glp_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lg_mtfglp_workspace_bytes', 'lg_mtf_glp')
RUNNERS = {'MTF_GLP': 'glp', 'MTF_GLP_HPM': 'hpm', 'MTF_GLP_CBD': 'cbd'}


def test_explicit_lowpass_equals_the_scipy_form():
    p = np.random.default_rng(3).uniform(0, 1, (16, 28))
    for gain, n in ((0.3, 41), (0.22, 41), (0.3, 63), (0.15, 5), (0.3, 1)):
        t = mr.taps(gain, n)
        err = float(np.abs(mr.lowpass_decimated_explicit(p, t) - mr.lowpass(p, t)[2::4, 2::4]).max())
        print(f'gain {gain}, {n} taps: explicit against scipy {err:.3e}')
        assert abs(t.sum() - 1.0) <= 1e-15 and err <= 1e-14


def test_restatement_uses_the_taps_of_the_package():
    from lgteun_amd import wald
    for gain, n in ((0.3, 41), (0.22, 41), (0.28, 63), (0.3, 1)):
        assert np.array_equal(mr.taps(gain, n), wald.mtf_taps(gain, n))


def test_names_are_declared_bound_and_exported():
    import lgteun_amd
    from lgteun_amd import _lib, mtf_glp
    header = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + '(' in header
        assert hasattr(L, name)
    for code, name in enumerate(('LG_MTFGLP_GLP', 'LG_MTFGLP_HPM', 'LG_MTFGLP_CBD')):
        assert getattr(_lib, name) == code and f'#define {name} {code}' in header
    assert _lib.LG_ABI_VERSION == 2 and L.lg_abi_version() == 2 and '#define LG_ABI_VERSION 2' in header
    assert L.lg_classical_workspace_bytes(2, 4, 8, 8, 2) == 0           # the new methods have their own size function
    assert lgteun_amd.mtf_glp is mtf_glp and callable(mtf_glp.mtf_glp) and callable(mtf_glp.fuse_scene)
    for name in RUNNERS:
        assert getattr(lgteun_amd, name) is getattr(mtf_glp, name)


def test_size_function():
    from lgteun_amd import _lib
    L = _lib.lib()
    sizes = {}
    for mode in range(3):
        for F in (1, 4):
            sizes[mode, F] = n = L.lg_mtfglp_workspace_bytes(2, 4, 8, 8, F, mode)
            assert n > 0 and n % 8 == 0
    assert sizes[0, 4] - sizes[0, 1] >= 2 * 3 * 8 * 8 * 8              # C - 1 more fp64 planes [h, w] per sample
    assert sizes[2, 1] > sizes[0, 1] == sizes[1, 1]                    # cbd: the partials of the second moments pass
    for bad in ((0, 4, 8, 8, 1, 0), (65536, 4, 8, 8, 1, 0), (2, 1, 8, 8, 1, 0), (2, 17, 8, 8, 1, 0), (2, 4, 3, 8, 1, 0), (2, 4, 8, 4097, 1, 0),
                (2, 4, 8, 8, 0, 0), (2, 4, 8, 8, 2, 0), (2, 4, 8, 8, 5, 0), (2, 4, 8, 8, 1, -1), (2, 4, 8, 8, 1, 3)):
        assert L.lg_mtfglp_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_named_before_any_device_call():
    """the pointers are made-up addresses: a call that got past its checks would fault here"""
    from lgteun_amd import _lib
    L = _lib.lib()
    ms, pan, out, taps, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    need = L.lg_mtfglp_workspace_bytes(2, 4, 8, 8, 1, 2)

    def call(ms=ms, pan=pan, out=out, stats=None, taps=taps, F=1, n=41, mode=2, B=2, C=4, h=8, w=8, ws=ws, nbytes=need):
        return L.lg_mtf_glp(ms, pan, out, stats, taps, F, n, mode, B, C, h, w, ws, nbytes, None)
    cases = [(dict(ms=None), 'ms is NULL'), (dict(pan=None), 'pan is NULL'), (dict(out=None), 'out is NULL'), (dict(taps=None), 'taps is NULL'),
             (dict(ws=None), 'workspace is NULL'), (dict(ms=ms + 4), 'ms must be 16-byte aligned'), (dict(pan=pan + 8), 'pan must be 16-byte aligned'),
             (dict(out=out + 4), 'out must be 16-byte aligned'), (dict(taps=taps + 4), 'taps must be 8-byte aligned'),
             (dict(stats=0x60004), 'stats must be 8-byte aligned'), (dict(ws=ws + 4), 'workspace must be 8-byte aligned'),
             (dict(C=1), 'C must be'), (dict(C=17), 'C must be'), (dict(h=3), 'h must be'), (dict(w=4097), 'w must be'), (dict(B=0), 'B must be'),
             (dict(B=65536), 'B must be'), (dict(F=0), 'n_filters must be'), (dict(F=2), 'n_filters must be'), (dict(F=5), 'n_filters must be'),
             (dict(n=40), 'n_taps must be'), (dict(n=65), 'n_taps must be'), (dict(n=0), 'n_taps must be'), (dict(mode=3), 'mode must be'),
             (dict(mode=-1), 'mode must be'), (dict(nbytes=need - 8), 'workspace_bytes too small'),
             (dict(mode=2, nbytes=L.lg_mtfglp_workspace_bytes(2, 4, 8, 8, 1, 0)), 'workspace_bytes too small'),
             (dict(F=4, nbytes=need), 'workspace_bytes too small')]
    for kw, text in cases:
        assert call(**kw) < 0, text
        assert text in L.lg_last_error().decode() and 'mtf_glp' in L.lg_last_error().decode(), (text, L.lg_last_error())
    with pytest.raises(_lib.LgteunHipError, match='out is NULL'):
        _lib.check(call(out=None), 'lg_mtf_glp')


@pytest.mark.parametrize('name', sorted(RUNNERS))
def test_registry_builds_the_runner(name, tmp_path, caplog):
    from lgteun_amd import MODELS, build_model, mtf_glp
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    assert MODELS.get(name) is getattr(mtf_glp, name) and getattr(mtf_glp, name).mode == RUNNERS[name]
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0))
    with caplog.at_level(logging.INFO, logger='t'):
        runner = build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)
    assert sum('placeholder' in r.getMessage() for r in caplog.records) == 1          # no gains in the config: said once
    assert isinstance(runner, Base_model) and runner.module_dict == {}
    assert runner.gains_ms is None and runner.n_taps == 41
    assert runner.print_total_params() == 0
    runner.train()                                         # nothing to train: returns
    assert runner.save(iter_id=1) is None and not os.path.exists(runner.train_out)
    with pytest.raises(RuntimeError, match='nothing to train'):
        runner.train_iter(1, {})
    caplog.clear()
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0, mtf_gains_ms=[0.3, 0.28, 0.26, 0.24],
                      mtf_taps=31))
    with caplog.at_level(logging.INFO, logger='t'):
        runner = build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)
    assert list(runner.gains_ms) == [0.3, 0.28, 0.26, 0.24] and runner.n_taps == 31
    assert not any('placeholder' in r.getMessage() for r in caplog.records)


def test_functions_refuse_cpu_tensors_and_unknown_modes():
    import torch
    from lgteun_amd import mtf_glp
    for mode in mr.MODES:
        with pytest.raises(ValueError, match='no CPU path'):
            mtf_glp.mtf_glp(torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 32, 32), mode)
    with pytest.raises(ValueError, match="'glp', 'hpm' or 'cbd'"):
        mtf_glp.mtf_glp(torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 32, 32), 'nope')
    with pytest.raises(ValueError, match="'glp', 'hpm' or 'cbd'"):
        mtf_glp.fuse_scene('nope', np.zeros((4, 8, 8), np.uint16), np.zeros((1, 32, 32), np.uint16), bit_depth=11)
    assert mtf_glp._gains(None, 4) == (0.3,) and mtf_glp._gains(0.25, 8) == (0.25,) and mtf_glp._gains([0.2] * 4, 4) == (0.2,)
    assert mtf_glp._gains([0.2, 0.3, 0.2, 0.3], 4) == (0.2, 0.3, 0.2, 0.3)
    with pytest.raises(ValueError, match='3 gains for 4 bands'):
        mtf_glp._gains([0.2, 0.3, 0.2], 4)


def test_tool_accepts_the_new_methods_and_scene_methods_of_classical_stay(capsys):
    from lgteun_amd import classical, mtf_glp
    assert set(classical.SCENE_METHODS) == {'gsa', 'sfim', 'wavelet'}
    assert mtf_glp.SCENE_METHODS == {'mtf_glp': 'glp', 'mtf_glp_hpm': 'hpm', 'mtf_glp_cbd': 'cbd'}
    spec = importlib.util.spec_from_file_location('fuse_scene_tool', os.path.join(ROOT, 'tools', 'fuse_scene.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for m in mtf_glp.SCENE_METHODS:
        a = tool.parser().parse_args(['scene', '--method', m])
        assert a.method == m and a.mtf_gains is None
    a = tool.parser().parse_args(['scene', '--method', 'mtf_glp_cbd', '--mtf-gains', '0.3', '0.28', '0.26', '0.24'])
    assert a.mtf_gains == [0.3, 0.28, 0.26, 0.24]
    assert tool.parser().parse_args(['scene', '--method', 'mtf_glp', '--mtf-gains', '0.25']).mtf_gains == [0.25]
    with pytest.raises(SystemExit):
        tool.parser().parse_args(['scene', '--method', 'nope'])
    err = capsys.readouterr().err
    assert all(m in err for m in ('gsa', 'sfim', 'wavelet', 'mtf_glp', 'mtf_glp_hpm', 'mtf_glp_cbd'))


def gpu_cases():
    for C, h, w, B in mr.SHAPES:
        yield C, h, w, B, [mr.EQUAL_GAIN] * C
        if (C, h, w, B) in mr.PER_BAND_SHAPES:
            yield C, h, w, B, mr.per_band_gains(C)


def test_inputs_of_the_gpu_tests_stay_off_the_clip_boundaries():
    assert len(mr.SHAPES) == 7 and len(list(gpu_cases())) == 10
    for C, h, w, B, gains in gpu_cases():
        ms, pan = cr.make_batch(B, C, h, w, seed=C * 100 + h)
        for mode in mr.MODES:
            raw = np.stack([mr.mtf_glp(ms[b], pan[b, 0], mode, gains, clip=False) for b in range(B)])
            share = float(((raw <= 0) | (raw >= 1)).mean())
            print(f'{mode} C={C} h={h} w={w} B={B} gains {gains[0]:.2f} .. {gains[-1]:.2f}: clip share {share:.4f}')
            assert share <= 0.02, (mode, C, h, w, B)


@pytest.mark.parametrize('mode', mr.MODES)
def test_clip_case_leaves_the_range_on_both_sides(mode):
    C, h, w, B = mr.CLIP_SHAPE
    ms, pan = mr.make_clip_batch(C, h, w, B, seed=mr.CLIP_SEED)
    assert ms.dtype == np.float32 and pan.dtype == np.float32 and ms.min() >= 0 and ms.max() <= 1 and pan.min() >= 0 and pan.max() <= 1
    for b in range(B):
        raw = mr.mtf_glp(ms[b], pan[b, 0], mode, [mr.EQUAL_GAIN] * C, clip=False)
        below, above = float((raw < -mr.CLIP_MARGIN).mean()), float((raw > 1 + mr.CLIP_MARGIN).mean())
        print(f'{mode} sample {b}: {100 * below:.1f} % below 0, {100 * above:.1f} % above 1 by more than {mr.CLIP_MARGIN}')
        assert below >= 0.02 and above >= 0.02
