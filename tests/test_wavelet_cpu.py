"""No GPU: the Wavelet baseline's surface -- the registry entry, the C ABI names, the argument checks of the library (lg_wavelet returns before it
touches a device, lg_wavelet_taps is host code) -- and self-checks of the numpy restatement the GPU tests compare with (tests/wavelet_ref.py): the
explicit two-level Haar form against the closed form, the 17-tap FIR against the block means of the interpolation, and the inputs of the GPU tests.

Measured: explicit against closed form 4.4e-16 - 5.6e-16; lg_wavelet_taps against the numpy chain 0 (every tap the same bits); the FIR against the block means
3.3e-16; clip share of the seven shapes 0; the clip case 1.2 - 2.3 % below 0 and 6.7 - 8.7 % above 1 per sample, nothing within 3e-6 of a bound."""
import ctypes
import importlib.util
import logging
import os

import numpy as np
import pytest

import classical_ref as cr
import wavelet_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lg_wavelet', 'lg_wavelet_taps')


@pytest.mark.parametrize('C,h,w', [(4, 4, 4), (4, 5, 7), (8, 12, 8)])
def test_explicit_form_equals_the_closed_form(C, h, w):
    ms, pan = cr.make_scene(C, h, w, seed=12)
    closed = wr.wavelet_closed_form(ms, pan)
    err = float(np.abs(wr.wavelet(ms, pan) - np.clip(closed, 0, 1)).max())
    print(f'C={C} h={h} w={w}: explicit against closed form {err:.3e}')
    assert err <= 1e-14
    # neither input comes back: the result is a thousand test bars (~ 2e-6) away from the interpolation and from PAN
    assert np.abs(closed - cr.interp23(ms)).max() > 2e-3 and np.abs(closed - pan[None]).max() > 2e-3


def library_taps():
    from lgteun_amd import _lib
    got = (ctypes.c_double * 17)()
    assert _lib.lib().lg_wavelet_taps(got) == 0
    return np.array(got)


def test_the_library_uses_the_taps_of_the_chain():
    want, got = wr.taps17(), library_taps()
    err = float(np.abs(got - want).max())
    print(f'lg_wavelet_taps against taps17: {err:.3e}; sum {got.sum():.12f}')
    assert want.shape == (17,) and err <= 1e-15
    assert abs(want[8] - 0.847680807599) < 1e-12 and abs(want[9] - 0.186719662878) < 1e-12 and abs(want[0] + 4.49217623559e-08) < 1e-18
    assert abs(want.sum() - 0.999999999596) < 1e-12
    assert np.abs(want - want[::-1]).max() > 0.1            # asymmetric: ms(i) sits at u(4 i + 2), the block's centre at 4 i + 1.5


@pytest.mark.parametrize('h,w', [(4, 4), (5, 7)])
def test_fir_on_ms_equals_the_block_means_of_the_interpolation(h, w):
    ms = np.random.default_rng(h * 10 + w).uniform(0, 1, (4, h, w))
    want = wr.block_mean(cr.interp23_explicit(ms))
    for name, taps in (('taps17', wr.taps17()), ('lg_wavelet_taps', library_taps())):
        err = float(np.abs(wr.fir_block_means(ms, taps) - want).max())
        print(f'h={h} w={w}: FIR with {name} against the block means {err:.3e}')
        assert err <= 1e-14


def test_registry_builds_the_runner(tmp_path):
    import lgteun_amd
    from lgteun_amd import MODELS, build_model, classical
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    assert MODELS.get('Wavelet') is classical.Wavelet
    assert lgteun_amd.wavelet is classical.wavelet and lgteun_amd.Wavelet is classical.Wavelet
    cfg = Config(dict(work_dir=str(tmp_path / 'Wavelet'), datas='synthetic', bit_depth=11, model_type='Wavelet', max_iter=0))
    runner = build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)
    assert isinstance(runner, Base_model) and runner.module_dict == {}
    assert runner.print_total_params() == 0
    runner.train()                                         # nothing to train: returns
    assert runner.save(iter_id=1) is None and not os.path.exists(runner.train_out)
    with pytest.raises(RuntimeError, match='nothing to train'):
        runner.train_iter(1, {})


def test_function_refuses_cpu_tensors():
    import torch
    from lgteun_amd import classical
    with pytest.raises(ValueError, match='no CPU path'):
        classical.wavelet(torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 32, 32))


def test_names_are_declared_bound_and_exported():
    from lgteun_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + '(' in header
        assert hasattr(L, name)
    assert L.lg_classical_workspace_bytes(2, 4, 8, 8, 2) == 0          # no third method code: the method has no workspace


def test_bad_arguments_are_named_before_any_device_call():
    """the pointers are made-up addresses: a call that got past its checks would fault here"""
    from lgteun_amd import _lib
    L = _lib.lib()
    ms, pan, out = 0x10000, 0x20000, 0x30000
    cases = [((None, pan, out, 2, 4, 8, 8), 'ms is NULL'), ((ms, None, out, 2, 4, 8, 8), 'pan is NULL'), ((ms, pan, None, 2, 4, 8, 8), 'out is NULL'),
             ((ms + 4, pan, out, 2, 4, 8, 8), 'ms must be 16-byte aligned'), ((ms, pan + 8, out, 2, 4, 8, 8), 'pan must be 16-byte aligned'),
             ((ms, pan, out, 2, 1, 8, 8), 'C must be'), ((ms, pan, out, 2, 17, 8, 8), 'C must be'), ((ms, pan, out, 2, 4, 3, 8), 'h must be'),
             ((ms, pan, out, 2, 4, 8, 4097), 'w must be'), ((ms, pan, out, 0, 4, 8, 8), 'B must be'), ((ms, pan, out, 65536, 4, 8, 8), 'B must be')]
    for args, text in cases:
        assert L.lg_wavelet(*args, None) < 0, text
        assert text in L.lg_last_error().decode() and 'wavelet' in L.lg_last_error().decode(), (text, L.lg_last_error())
    assert L.lg_wavelet_taps(None) < 0 and 'out17 is NULL' in L.lg_last_error().decode()
    with pytest.raises(_lib.LgteunHipError, match='out is NULL'):
        _lib.check(L.lg_wavelet(ms, pan, None, 2, 4, 8, 8, None), 'lg_wavelet')


def test_inputs_of_the_gpu_tests_stay_off_the_clip_boundaries():
    assert len(wr.SHAPES) == 7
    for C, h, w, B in wr.SHAPES:
        ms, pan = wr.make_batch(C, h, w, B)
        raw = np.stack([wr.wavelet_closed_form(ms[b], pan[b, 0]) for b in range(B)])
        share = float(((raw <= 0) | (raw >= 1)).mean())
        print(f'C={C} h={h} w={w} B={B}: clip share {share:.4f}')
        assert share <= 0.02, (C, h, w, B)


@pytest.mark.parametrize('C,h,w,B', wr.CLIP_SHAPES)
def test_clip_case_leaves_the_range_on_both_sides_and_keeps_off_the_bounds(C, h, w, B):
    ms, pan = wr.make_clip_batch(C, h, w, B)
    assert ms.dtype == np.float32 and pan.dtype == np.float32
    for b in range(B):
        raw = wr.wavelet_closed_form(ms[b], pan[b, 0])
        below, above = float((raw < 0).mean()), float((raw > 1).mean())
        near = int((np.minimum(np.abs(raw), np.abs(raw - 1)) <= 3e-6).sum())
        print(f'C={C} h={h} w={w} sample {b}: {100 * below:.1f} % below 0, {100 * above:.1f} % above 1, {near} within 3e-6 of a bound')
        assert below >= 0.01 and above >= 0.05 and near == 0


def test_scene_entry_and_tool_accept_wavelet_and_name_all_three(capsys):
    from lgteun_amd import classical
    assert set(classical.SCENE_METHODS) == {'gsa', 'sfim', 'wavelet'} and classical.SCENE_METHODS['wavelet'] is classical.wavelet
    with pytest.raises(ValueError) as e:
        classical.fuse_scene('nope', np.zeros((4, 8, 8), np.uint16), np.zeros((1, 32, 32), np.uint16), bit_depth=11)
    assert all(repr(m) in str(e.value) for m in ('gsa', 'sfim', 'wavelet'))
    spec = importlib.util.spec_from_file_location('fuse_scene_tool', os.path.join(ROOT, 'tools', 'fuse_scene.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parser().parse_args(['scene', '--method', 'wavelet']).method == 'wavelet'
    with pytest.raises(SystemExit):
        tool.parser().parse_args(['scene', '--method', 'nope'])
    err = capsys.readouterr().err
    assert all(m in err for m in ('gsa', 'sfim', 'wavelet'))
