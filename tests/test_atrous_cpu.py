"""No GPU: the surface of the a trous baselines ATWT and AWLP -- the C ABI names and the argument block, the argument checks of the library (lg_atrous returns
before it touches a device), the registry entries, the command line -- and self-checks of the numpy restatement the GPU tests compare with
(tests/atrous_ref.py): the cascade against its 13-tap form and against explicit modulo-indexed sums, the taps of the kernel, and the inputs of the GPU tests.

Measured: cascade against the 13-tap form 2.2e-16, against the explicit sums 6.7e-16; clip share of the output cases at most 0.004 % for match 'pan' and
0.79 % for 'lowpass' ((4, 20, 12, 1), atwt); the clip case leaves [0, 1] below on 8.9 - 37.9 % and above on 4.5 - 30.5 % of its elements."""
import ctypes
import importlib.util
import logging
import os

import numpy as np
import pytest

import atrous_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lg_atrous_workspace_bytes', 'lg_atrous', 'lg_atrous_taps')
RUNNERS = {'ATWT': 'atwt', 'AWLP': 'awlp'}


def test_taps_of_the_kernel_are_the_cascade_exactly():
    from lgteun_amd import _lib
    L = _lib.lib()
    t = (ctypes.c_double * 13)()
    assert L.lg_atrous_taps(t) == 0
    assert list(t) == [v / 256.0 for v in (1, 4, 10, 20, 31, 40, 44, 40, 31, 20, 10, 4, 1)] == list(ar.TAPS13)
    full = np.convolve(ar.B3, np.kron(ar.B3, [1.0, 0.0])[:-1])          # level 1 against level 2's taps two apart
    assert np.array_equal(full, ar.TAPS13) and ar.TAPS13.sum() == 1.0
    assert L.lg_atrous_taps(None) < 0 and b'out13 is NULL' in L.lg_last_error()


def test_cascade_equals_its_13_tap_form_and_the_explicit_sums():
    p = np.random.default_rng(3).uniform(0, 1, (20, 28))
    e13 = float(np.abs(ar.lowpass(p) - ar.lowpass13(p)).max())
    eex = float(np.abs(ar.lowpass(p) - ar.lowpass_explicit(p)).max())
    small = np.random.default_rng(4).uniform(0, 1, (16, 16))            # the smallest PAN: the 13 taps wrap on both sides
    esm = float(np.abs(ar.lowpass(small) - ar.lowpass_explicit(small)).max())
    print(f'cascade against the 13-tap form {e13:.3e}, against the explicit sums {eex:.3e} (20 x 28) and {esm:.3e} (16 x 16)')
    assert e13 <= 1e-15 and eex <= 2e-15 and esm <= 2e-15
    const = np.full((16, 20), 0.3)
    assert np.array_equal(ar.lowpass(const - const[0, 0]), np.zeros((16, 20)))      # minus its first pixel a constant PAN has exactly zero detail


def test_names_are_declared_bound_and_exported():
    import lgteun_amd
    from lgteun_amd import _lib, atrous
    header = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + '(' in header
        assert hasattr(L, name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [5, 1, 1]      # no positional stream: the stream rides in the argument block
    for name, code in (('LG_ATROUS_ATWT', 0), ('LG_ATROUS_AWLP', 1), ('LG_ATROUS_MATCH_PAN', 0), ('LG_ATROUS_MATCH_LOWPASS', 1)):
        assert getattr(_lib, name) == code and f'#define {name} {code}' in header
    assert _lib.LG_ABI_VERSION == 2 and L.lg_abi_version() == 2 and '#define LG_ABI_VERSION 2' in header
    assert 'lg_atrous_workspace_bytes, lg_atrous, lg_atrous_taps' in header.split('came without a bump')[0]
    assert lgteun_amd.atrous is atrous and callable(atrous.atrous) and callable(atrous.fuse_scene)
    assert lgteun_amd.atwt is atrous.atwt and lgteun_amd.awlp is atrous.awlp
    for name in RUNNERS:
        assert getattr(lgteun_amd, name) is getattr(atrous, name)
    assert atrous.RULES == {'atwt': 0, 'awlp': 1} and atrous.MATCHES == {'pan': 0, 'lowpass': 1}


def _args(**kw):
    from lgteun_amd import _lib
    L = _lib.lib()
    d = dict(struct_bytes=ctypes.sizeof(_lib.LgAtrousArgs), rule=1, match=0, B=2, C=4, h=8, w=8, ms=0x10000, pan=0x20000, out=0x30000, stats=None,
             workspace=0x50000, workspace_bytes=None, stream=None)
    d.update(kw)
    if d['workspace_bytes'] is None:
        d['workspace_bytes'] = L.lg_atrous_workspace_bytes(2, 4, 8, 8, d['match'] if d['match'] in (0, 1) else 0)
    return _lib.LgAtrousArgs(**d)


def test_the_argument_block_has_the_size_the_library_accepts():
    """the pointers are made-up addresses: a call that got past its checks would fault here.  With everything valid but a NULL `out`, the right struct_bytes
    gets as far as that check and every other value stops at the first"""
    from lgteun_amd import _lib
    L = _lib.lib()
    n = ctypes.sizeof(_lib.LgAtrousArgs)
    assert n == 88          # 7 x 4 bytes and 4 of padding, four pointers, pointer, size_t, pointer
    assert L.lg_atrous(ctypes.byref(_args(out=None))) < 0 and b'atrous: out is NULL' in L.lg_last_error()
    for bad in (0, n - 8, n - 1, n + 1, n + 8):
        assert L.lg_atrous(ctypes.byref(_args(out=None, struct_bytes=bad))) < 0
        msg = L.lg_last_error().decode()
        assert msg.startswith('atrous: struct_bytes must be') and f'{n}' in msg and f'got {bad}' in msg, msg
    assert L.lg_atrous(None) < 0 and L.lg_last_error().decode().startswith('atrous: args is NULL')


def test_bad_arguments_are_named_before_any_device_call():
    from lgteun_amd import _lib
    L = _lib.lib()
    need_pan, need_low = L.lg_atrous_workspace_bytes(2, 4, 8, 8, 0), L.lg_atrous_workspace_bytes(2, 4, 8, 8, 1)
    assert 0 < need_pan < need_low
    cases = [(dict(struct_bytes=0), 'struct_bytes must be'), (dict(rule=2), 'rule must be'), (dict(rule=-1), 'rule must be'),
             (dict(match=2), 'match must be'), (dict(match=-1), 'match must be'),
             (dict(B=0), 'B must be'), (dict(B=65536), 'B must be'), (dict(C=1), 'C must be'), (dict(C=17), 'C must be'),
             (dict(h=3), 'h must be'), (dict(h=4097), 'h must be'), (dict(w=3), 'w must be'), (dict(w=4097), 'w must be'),
             (dict(ms=None), 'ms is NULL'), (dict(pan=None), 'pan is NULL'), (dict(out=None), 'out is NULL'), (dict(workspace=None), 'workspace is NULL'),
             (dict(ms=0x10004), 'ms must be 16-byte aligned'), (dict(pan=0x20008), 'pan must be 16-byte aligned'),
             (dict(out=0x30004), 'out must be 16-byte aligned'), (dict(stats=0x60004), 'stats must be 8-byte aligned'),
             (dict(workspace=0x50004), 'workspace must be 8-byte aligned'),
             (dict(workspace_bytes=need_pan - 8), 'workspace_bytes too small'), (dict(match=1, workspace_bytes=need_low - 8), 'workspace_bytes too small'),
             (dict(match=1, workspace_bytes=need_pan), 'workspace_bytes too small')]
    for kw, text in cases:
        assert L.lg_atrous(ctypes.byref(_args(**kw))) < 0, text
        msg = L.lg_last_error().decode()
        assert msg.startswith('atrous:') and text in msg, (text, msg)
    with pytest.raises(_lib.LgteunHipError, match='out is NULL'):
        _lib.check(L.lg_atrous(ctypes.byref(_args(out=None))), 'lg_atrous')


def test_size_function():
    from lgteun_amd import _lib
    L = _lib.lib()
    for match in (0, 1):
        for ok in ((1, 2, 4, 4), (65535, 16, 4, 4), (1, 16, 4096, 4096), (2, 4, 8, 8)):       # the last values inside the ranges
            n = L.lg_atrous_workspace_bytes(*ok, match)
            assert n > 0 and n % 8 == 0, (ok, match)
        for bad in ((0, 4, 8, 8), (65536, 4, 8, 8), (2, 1, 8, 8), (2, 17, 8, 8), (2, 4, 3, 8), (2, 4, 4097, 8), (2, 4, 8, 3), (2, 4, 8, 4097)):
            assert L.lg_atrous_workspace_bytes(*bad, match) == 0, (bad, match)
    assert L.lg_atrous_workspace_bytes(2, 4, 8, 8, 2) == 0 and L.lg_atrous_workspace_bytes(2, 4, 8, 8, -1) == 0
    assert L.lg_atrous_workspace_bytes(2, 4, 8, 8, 0) == L.lg_classical_workspace_bytes(2, 4, 8, 8, _lib.LG_CLASSICAL_SFIM)      # SFIM's two arrays
    # lowpass: [B, gx] partials more, gx = min(tiles, 768); (4, 136, 256, 1) has 1088 tiles
    extra = L.lg_atrous_workspace_bytes(1, 4, 136, 256, 1) - L.lg_atrous_workspace_bytes(1, 4, 136, 256, 0)
    assert 768 * 8 <= extra <= 768 * 8 + 256


@pytest.mark.parametrize('name', sorted(RUNNERS))
def test_registry_builds_the_runner(name, tmp_path):
    from lgteun_amd import MODELS, atrous, build_model
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    assert MODELS.get(name) is getattr(atrous, name) and getattr(atrous, name).rule == RUNNERS[name]
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0))
    runner = build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)
    assert isinstance(runner, Base_model) and runner.module_dict == {} and runner.match == 'pan'
    assert runner.print_total_params() == 0
    runner.train()                                         # nothing to train: returns
    assert runner.save(iter_id=1) is None and not os.path.exists(runner.train_out)
    with pytest.raises(RuntimeError, match='nothing to train'):
        runner.train_iter(1, {})
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0, atrous_match='lowpass'))
    assert build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None).match == 'lowpass'
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0, atrous_match='nope'))
    with pytest.raises(ValueError, match="'pan' or 'lowpass'"):
        build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)


def test_functions_refuse_cpu_tensors_and_unknown_words():
    import torch
    from lgteun_amd import atrous
    ms, pan = torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 32, 32)
    for rule in ar.RULES:
        for match in ar.MATCHES:
            with pytest.raises(ValueError, match='no CPU path'):
                atrous.atrous(ms, pan, rule, match)
    for fn in (atrous.atwt, atrous.awlp):
        with pytest.raises(ValueError, match='no CPU path'):
            fn(ms, pan)
        with pytest.raises(ValueError, match="'pan' or 'lowpass'"):
            fn(ms, pan, match='nope')
    with pytest.raises(ValueError, match="'atwt' or 'awlp'"):
        atrous.atrous(ms, pan, 'nope')
    with pytest.raises(ValueError, match="'atwt' or 'awlp'"):
        atrous.fuse_scene('nope', np.zeros((4, 8, 8), np.uint16), np.zeros((1, 32, 32), np.uint16), bit_depth=11)
    with pytest.raises(ValueError, match="'pan' or 'lowpass'"):
        atrous.fuse_scene('awlp', np.zeros((4, 8, 8), np.uint16), np.zeros((1, 32, 32), np.uint16), match='nope', bit_depth=11)


def test_tool_accepts_the_new_methods(capsys):
    from lgteun_amd import atrous
    assert atrous.SCENE_METHODS == {'atwt': 'atwt', 'awlp': 'awlp'}
    spec = importlib.util.spec_from_file_location('fuse_scene_tool', os.path.join(ROOT, 'tools', 'fuse_scene.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for m in atrous.SCENE_METHODS:
        a = tool.parser().parse_args(['scene', '--method', m])
        assert a.method == m and a.atrous_match == 'pan'
        assert tool.parser().parse_args(['scene', '--method', m, '--atrous-match', 'lowpass']).atrous_match == 'lowpass'
    with pytest.raises(SystemExit):
        tool.parser().parse_args(['scene', '--method', 'awlp', '--atrous-match', 'nope'])
    with pytest.raises(SystemExit):
        tool.parser().parse_args(['scene', '--method', 'nope'])
    err = capsys.readouterr().err
    assert all(m in err for m in ('atwt', 'awlp', 'sfim', 'mtf_glp'))


def test_shape_lists_are_the_stated_ones():
    assert len(ar.SHAPES['pan']) == 10 and len(ar.SHAPES['lowpass']) == 9 and len(ar.STATS_ONLY_SHAPES) == 7
    assert not set(ar.STATS_ONLY_SHAPES) & set(ar.SHAPES['lowpass']) and set(ar.STATS_ONLY_SHAPES) <= set(ar.SHAPES['pan'])
    for shapes in ar.SHAPES.values():
        assert (4, 136, 256, 1) in shapes                  # 1088 tiles against 768 workgroups: a workgroup of the moments passes walks a second tile
    assert {s[0] for s in ar.SHAPES['pan']} >= {2, 3, 16}  # both ends of the band range


@pytest.mark.parametrize('match', ar.MATCHES)
def test_inputs_of_the_gpu_tests_stay_off_the_clip_boundaries(match):
    for C, h, w, B in ar.SHAPES[match]:
        ms, pan = ar.make_inputs(C, h, w, B)
        for rule in ar.RULES:
            raw = np.stack([ar.atrous(ms[b], pan[b, 0], rule, match, clip=False) for b in range(B)])
            share = float(((raw <= 0) | (raw >= 1)).mean())
            print(f'{rule} / {match} C={C} h={h} w={w} B={B}: clip share {share:.5f}')
            assert share <= 0.02, (rule, match, C, h, w, B)


@pytest.mark.parametrize('match', ar.MATCHES)
@pytest.mark.parametrize('rule', ar.RULES)
def test_clip_case_leaves_the_range_on_both_sides(rule, match):
    C, h, w, B = ar.CLIP_SHAPE
    ms, pan = ar.make_clip_batch(C, h, w, B, seed=ar.CLIP_SEED)
    assert ms.dtype == np.float32 and pan.dtype == np.float32 and ms.min() >= 0 and ms.max() <= 1 and pan.min() >= 0 and pan.max() <= 1
    raw = np.stack([ar.atrous(ms[b], pan[b, 0], rule, match, clip=False) for b in range(B)])
    below, above = float((raw < -ar.CLIP_MARGIN).mean()), float((raw > 1 + ar.CLIP_MARGIN).mean())
    print(f'{rule} / {match}: {100 * below:.1f} % below 0, {100 * above:.1f} % above 1 by more than {ar.CLIP_MARGIN}')
    assert below >= 0.02 and above >= 0.02


def test_constant_pan_restates_to_clip_u():
    import classical_ref as cr
    ms, pan = ar.make_inputs(4, 8, 8, 1)
    flat = np.full_like(pan[0, 0], 0.3)
    for rule in ar.RULES:
        for match in ar.MATCHES:
            out, a, ref = ar.atrous(ms[0], flat, rule, match, return_stats=True)
            assert np.array_equal(out, np.clip(cr.interp23(ms[0]), 0, 1)) and not a.any() and ref == 0
