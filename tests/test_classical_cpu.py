"""No GPU: the classical baselines' surface -- the registry entries, the C ABI names, the argument checks of the library (every entry returns
before it touches a device) -- and self-checks of the numpy restatement the GPU tests compare with (tests/classical_ref.py)."""
import ctypes
import logging
import os

import numpy as np
import pytest

import classical_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lg_classical_workspace_bytes', 'lg_interp23_up4', 'lg_sfim', 'lg_gsa')


def test_registry_builds_both_runners(tmp_path):
    import lgteun_amd
    from lgteun_amd import MODELS, build_model, classical
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    assert MODELS.get('GSA') is classical.GSA and MODELS.get('SFIM') is classical.SFIM
    assert lgteun_amd.gsa is classical.gsa and lgteun_amd.sfim is classical.sfim and lgteun_amd.interp23 is classical.interp23
    for name in ('GSA', 'SFIM'):
        cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, max_iter=10))
        runner = build_model(name, cfg, logging.getLogger('t'), None, None, None)
        assert isinstance(runner, Base_model) and runner.module_dict == {}
        assert runner.print_total_params() == 0
        runner.train()                                     # nothing to train: returns
        assert runner.save(iter_id=1) is None and not os.path.exists(runner.train_out)
        with pytest.raises(RuntimeError, match='nothing to train'):
            runner.train_iter(1, {})


def test_functions_refuse_cpu_tensors():
    import torch
    from lgteun_amd import classical
    ms, pan = torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 32, 32)
    for call in (lambda: classical.interp23(ms), lambda: classical.sfim(ms, pan), lambda: classical.gsa(ms, pan)):
        with pytest.raises(ValueError, match='no CPU path'):
            call()


def test_names_are_declared_bound_and_exported():
    from lgteun_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    assert '$(CSRC)/k_classical.hip' in open(os.path.join(ROOT, 'Makefile')).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + '(' in header
        assert hasattr(L, name)


def test_workspace_bytes():
    from lgteun_amd import _lib
    L = _lib.lib()
    for method in (_lib.LG_CLASSICAL_SFIM, _lib.LG_CLASSICAL_GSA):
        assert L.lg_classical_workspace_bytes(2, 4, 8, 8, method) > 0
        assert L.lg_classical_workspace_bytes(1, 8, 5, 7, method) > 0
        for B, C, h, w in ((1, 1, 8, 8), (1, 4, 3, 8), (1, 4, 8, 4097), (0, 4, 8, 8), (1, 17, 8, 8), (65536, 4, 8, 8)):
            assert L.lg_classical_workspace_bytes(B, C, h, w, method) == 0, (B, C, h, w)
    assert L.lg_classical_workspace_bytes(2, 4, 8, 8, 2) == 0


def _entries(L):
    """name -> call(ms, pan, out, C, workspace, workspace_bytes) at B = 2, h = w = 8"""
    return {
        'lg_interp23_up4': lambda ms, pan, out, C, ws, nb: L.lg_interp23_up4(ms, out, 2, C, 8, 8, None),
        'lg_sfim': lambda ms, pan, out, C, ws, nb: L.lg_sfim(ms, pan, out, 2, C, 8, 8, ws, nb, None),
        'lg_gsa': lambda ms, pan, out, C, ws, nb: L.lg_gsa(ms, pan, out, None, 2, C, 8, 8, ws, nb, None),
    }


def test_bad_arguments_are_named_before_any_device_call():
    """the pointers are made-up addresses: a call that got past its checks would fault here"""
    from lgteun_amd import _lib
    L = _lib.lib()
    ms, pan, out, ws = 0x10000, 0x20000, 0x30000, 0x40000
    for name, call in _entries(L).items():
        need = int(L.lg_classical_workspace_bytes(2, 4, 8, 8, _lib.LG_CLASSICAL_GSA if name == 'lg_gsa' else _lib.LG_CLASSICAL_SFIM))
        cases = [((ms + 4, pan, out, 4, ws, need), 'ms must be 16-byte aligned'), ((ms, pan, None, 4, ws, need), 'out is NULL'),
                 ((ms, pan, out, 17, ws, need), 'C must be')]
        if name != 'lg_interp23_up4':
            cases += [((ms, pan + 8, out, 4, ws, need), 'pan must be 16-byte aligned'), ((ms, pan, out, 4, ws, need - 1), 'workspace_bytes too small'),
                      ((ms, pan, out, 4, None, need), 'workspace is NULL'), ((ms, pan, out, 4, ws + 4, need), 'workspace must be 8-byte aligned')]
        for args, text in cases:
            assert call(*args) < 0, (name, text)
            assert text in L.lg_last_error().decode(), (name, text, L.lg_last_error())
    assert L.lg_gsa(ms, pan, out, 0x50004, 2, 4, 8, 8, ws, 1 << 20, None) < 0 and 'stats' in L.lg_last_error().decode()
    with pytest.raises(_lib.LgteunHipError, match='out is NULL'):
        _lib.check(L.lg_sfim(ms, pan, None, 2, 4, 8, 8, ws, 1 << 20, None), 'lg_sfim')


@pytest.mark.parametrize('h,w', [(4, 4), (5, 7)])
def test_interp23_through_scipy_equals_the_explicit_modulo_sum(h, w):
    ms, _ = cr.make_scene(4, h, w, seed=11)
    assert np.abs(cr.interp23(ms) - cr.interp23_explicit(ms)).max() <= 1e-14
    # the placement: ms sample (i, j) sits at u(4 i + 2, 4 j + 2), because both levels keep the inserted samples
    assert np.array_equal(cr.interp23(ms)[:, 2::4, 2::4], ms.astype(np.float64))
    t = cr.taps23()
    assert t[11] == 1.0 and np.all(t[1::2][np.arange(11) != 5] == 0) and abs(t.sum() - 2.0) < 1e-9


@pytest.mark.parametrize('C,h,w', [(4, 4, 4), (4, 5, 7), (8, 12, 8)])
def test_closed_form_gsa_equals_the_direct_form(C, h, w):
    ms, pan = cr.make_scene(C, h, w, seed=12)
    out, alpha, g = cr.gsa(ms, pan, return_stats=True)
    out2, alpha2, g2 = cr.gsa_closed_form(ms, pan)
    assert np.abs(out - out2).max() <= 1e-12
    assert np.abs(alpha - alpha2).max() <= 1e-12 * np.abs(alpha).max() and np.abs(g - g2).max() <= 1e-12 * np.abs(g).max()


def test_generator_keeps_the_outputs_off_the_clip_boundaries():
    ms, pan = cr.make_scene(4, 8, 8, seed=13)
    assert ms.dtype == np.float32 and pan.dtype == np.float32 and ms.shape == (4, 8, 8) and pan.shape == (32, 32)
    u = cr.interp23(ms)
    for res in (cr.sfim(ms, pan), cr.gsa(ms, pan)):
        assert ((res <= 0) | (res >= 1)).mean() <= 0.02
        assert np.abs(res - u).max() > 0.05                # the methods do inject detail: a test against them is not one against u
