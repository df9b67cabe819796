"""No GPU: the surface of the regression-based and haze-corrected MTF baselines FS, HPM-R, HPM-H and BT-H -- the C ABI names and the argument block, the
argument checks of the library (lg_mtf_hr returns before it touches a device), the registry entries, the command line -- self-checks of the numpy restatement
the GPU tests compare with (tests/mtf_hr_ref.py): its closed forms (the kernels' route) against its direct forms, the degenerate cases -- and the
preconditions of the GPU cases, proven per case in float64: every ratio denominator at least 0.01, the centred Gram matrix of ms conditioned at most 1e4, at
most 2 % of a result within CLIP_MARGIN of 0 or 1.

Measured (float64): closed against direct forms at most 2.5e-13 relative (slopes, (8, 32, 32, 3)); smallest denominator 0.0168 (bt_h, I - H_I at
(8, 12, 8, 3)), 0.0249 (hpm_h, per-band gains at (8, 12, 8, 3)), 0.171 (hpm_r, (4, 40, 24, 2)); largest condition 7.4e2 ((8, 32, 32, 3)); largest clip share
1.5 % (bt_h, (3, 8, 8, 2)).  The three listed cases that miss the clip share, and what replaces them, are in tests/mtf_hr_ref.py."""
import ctypes
import importlib.util
import logging
import os

import numpy as np
import pytest

import classical_ref as cr
import mtf_glp_ref as mr
import mtf_hr_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lg_mtf_hr_workspace_bytes', 'lg_mtf_hr')
RUNNERS = {'MTF_GLP_FS': 'fs', 'MTF_GLP_HPM_R': 'hpm_r', 'MTF_GLP_HPM_H': 'hpm_h', 'BT_H': 'bt_h'}
CODES = {'fs': 0, 'hpm_r': 1, 'hpm_h': 2, 'bt_h': 3}


def test_names_are_declared_bound_and_exported():
    import lgteun_amd
    from lgteun_amd import _lib, atrous, classical, cs, mtf_glp, mtf_hr
    header = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + '(' in header
        assert hasattr(L, name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [6, 1]         # no positional stream: the stream rides in the argument block
    for name, code in (('LG_MTFHR_FS', 0), ('LG_MTFHR_HPM_R', 1), ('LG_MTFHR_HPM_H', 2), ('LG_MTFHR_BT_H', 3)):
        assert getattr(_lib, name) == code and f'#define {name} {code}' in header
    assert _lib.LG_ABI_VERSION == 2 and L.lg_abi_version() == 2 and '#define LG_ABI_VERSION 2' in header
    assert 'lg_mtf_hr_workspace_bytes, lg_mtf_hr' in header.split('came without a bump')[0]
    assert lgteun_amd.mtf_hr is mtf_hr and mtf_hr.RULES == CODES
    for fn in ('fuse', 'fs', 'hpm_r', 'hpm_h', 'bt_h', 'fuse_scene'):
        assert callable(getattr(mtf_hr, fn))
    for name in RUNNERS:
        assert getattr(lgteun_amd, name) is getattr(mtf_hr, name)
    # a table of its own: the siblings' tables are as they were
    assert mtf_hr.SCENE_METHODS == {'fs', 'hpm_r', 'hpm_h', 'bt_h'} and not any(m.startswith('mtf_glp') for m in mtf_hr.SCENE_METHODS)
    assert set(mtf_glp.MODES) == {'glp', 'hpm', 'cbd'} and set(mtf_glp.SCENE_METHODS) == {'mtf_glp', 'mtf_glp_hpm', 'mtf_glp_cbd'}
    assert set(classical.SCENE_METHODS) == {'gsa', 'sfim', 'wavelet'} and set(atrous.SCENE_METHODS) == {'atwt', 'awlp'}
    assert not mtf_hr.SCENE_METHODS & set(cs.SCENE_METHODS)


def _args(**kw):
    from lgteun_amd import _lib
    L = _lib.lib()
    d = dict(struct_bytes=ctypes.sizeof(_lib.LgMtfHrArgs), rule=0, n_filters=1, n_taps=41, B=2, C=4, h=8, w=8, ms=0x10000, pan=0x20000, out=0x30000,
             stats=None, taps=0x40000, workspace=0x50000, workspace_bytes=None, stream=None)
    d.update(kw)
    if d['workspace_bytes'] is None:
        ok = d['rule'] in (0, 1, 2, 3) and d['n_filters'] in (1, 4)
        d['workspace_bytes'] = L.lg_mtf_hr_workspace_bytes(2, 4, 8, 8, d['n_filters'] if ok else 1, d['rule'] if ok else 0)
    return _lib.LgMtfHrArgs(**d)


def test_the_argument_block_has_the_size_the_library_accepts():
    """the pointers are made-up addresses: a call that got past its checks would fault here.  With everything valid but a NULL `out`, the right struct_bytes
    gets as far as that check and every other value stops at the first"""
    from lgteun_amd import _lib
    L = _lib.lib()
    n = ctypes.sizeof(_lib.LgMtfHrArgs)
    assert n == 96          # 8 x 4 bytes, five pointers, pointer, size_t, pointer
    assert L.lg_mtf_hr(ctypes.byref(_args(out=None))) < 0 and b'mtf_hr: out is NULL' in L.lg_last_error()
    for bad in (0, n - 8, n - 1, n + 1, n + 8):
        assert L.lg_mtf_hr(ctypes.byref(_args(out=None, struct_bytes=bad))) < 0
        msg = L.lg_last_error().decode()
        assert msg.startswith('mtf_hr: struct_bytes must be') and f'{n}' in msg and f'got {bad}' in msg, msg
    assert L.lg_mtf_hr(None) < 0 and L.lg_last_error().decode().startswith('mtf_hr: args is NULL')


@pytest.mark.parametrize('rule', sorted(CODES.values()))
def test_bad_arguments_are_named_before_any_device_call(rule):
    from lgteun_amd import _lib
    L = _lib.lib()
    need = L.lg_mtf_hr_workspace_bytes(2, 4, 8, 8, 1, rule)
    assert need > 0
    cases = [(dict(struct_bytes=0), 'struct_bytes must be'), (dict(rule=4), 'rule must be'), (dict(rule=-1), 'rule must be'),
             (dict(n_filters=0), 'n_filters must be'), (dict(n_filters=2), 'n_filters must be'), (dict(n_filters=5), 'n_filters must be'),
             (dict(n_taps=0), 'n_taps must be'), (dict(n_taps=40), 'n_taps must be'), (dict(n_taps=65), 'n_taps must be'),
             (dict(B=0), 'B must be'), (dict(B=65536), 'B must be'), (dict(C=1), 'C must be'), (dict(C=17), 'C must be'),
             (dict(h=3), 'h must be'), (dict(h=4097), 'h must be'), (dict(w=3), 'w must be'), (dict(w=4097), 'w must be'),
             (dict(ms=None), 'ms is NULL'), (dict(pan=None), 'pan is NULL'), (dict(out=None), 'out is NULL'), (dict(taps=None), 'taps is NULL'),
             (dict(workspace=None), 'workspace is NULL'),
             (dict(ms=0x10004), 'ms must be 16-byte aligned'), (dict(pan=0x20008), 'pan must be 16-byte aligned'),
             (dict(out=0x30004), 'out must be 16-byte aligned'), (dict(taps=0x40004), 'taps must be 8-byte aligned'),
             (dict(stats=0x60004), 'stats must be 8-byte aligned'), (dict(workspace=0x50004), 'workspace must be 8-byte aligned'),
             (dict(workspace_bytes=need - 8), 'workspace_bytes too small'), (dict(workspace_bytes=0), 'workspace_bytes too small')]
    if rule == 3:
        cases.append((dict(n_filters=4), 'n_filters must be 1 for LG_MTFHR_BT_H'))
    else:
        cases.append((dict(n_filters=4, workspace_bytes=need), 'workspace_bytes too small'))        # one plane per band: a larger D
    for kw, text in cases:
        kw = dict(dict(rule=rule), **kw)
        assert L.lg_mtf_hr(ctypes.byref(_args(**kw))) < 0, text
        msg = L.lg_last_error().decode()
        assert msg.startswith('mtf_hr:') and text in msg, (text, msg)
    with pytest.raises(_lib.LgteunHipError, match='out is NULL'):
        _lib.check(L.lg_mtf_hr(ctypes.byref(_args(rule=rule, out=None))), 'lg_mtf_hr')


def test_size_function():
    from lgteun_amd import _lib
    L = _lib.lib()
    for rule in range(4):
        for ok in ((1, 2, 4, 4), (65535, 16, 4, 4), (1, 16, 4096, 4096), (2, 4, 8, 8)):       # the last values inside the ranges
            for F in (1, ok[1]) if rule != 3 else (1,):
                n = L.lg_mtf_hr_workspace_bytes(*ok, F, rule)
                assert n > 0 and n % 8 == 0, (ok, F, rule)
        for bad in ((0, 4, 8, 8), (65536, 4, 8, 8), (2, 1, 8, 8), (2, 17, 8, 8), (2, 4, 3, 8), (2, 4, 4097, 8), (2, 4, 8, 3), (2, 4, 8, 4097)):
            assert L.lg_mtf_hr_workspace_bytes(*bad, 1, rule) == 0, (bad, rule)
        for F in (0, 2, 3, 5, -1):
            assert L.lg_mtf_hr_workspace_bytes(2, 4, 8, 8, F, rule) == 0, (F, rule)
    assert L.lg_mtf_hr_workspace_bytes(2, 4, 8, 8, 4, 3) == 0                                  # bt_h: one plane only
    assert L.lg_mtf_hr_workspace_bytes(2, 4, 8, 8, 1, 4) == 0 and L.lg_mtf_hr_workspace_bytes(2, 4, 8, 8, 1, -1) == 0
    # one plane per band: C - 1 more planes of h w doubles per sample, and for hpm_h their right-hand sides
    for rule in (0, 1, 2):
        extra = L.lg_mtf_hr_workspace_bytes(1, 4, 136, 256, 4, rule) - L.lg_mtf_hr_workspace_bytes(1, 4, 136, 256, 1, rule)
        assert 3 * 136 * 256 * 8 <= extra <= 3 * 136 * 256 * 8 + 128 * 3 * 5 * 8 + 1024, (rule, extra)
    # the haze rules need neither SFIM's partials nor a full-scale moments pass
    assert L.lg_mtf_hr_workspace_bytes(1, 4, 136, 256, 1, 2) < L.lg_mtf_hr_workspace_bytes(1, 4, 136, 256, 1, 0)
    assert L.lg_mtf_hr_workspace_bytes(1, 4, 136, 256, 1, 0) == L.lg_mtf_hr_workspace_bytes(1, 4, 136, 256, 1, 1)


class _Notes(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.mark.parametrize('name', sorted(RUNNERS))
def test_registry_builds_the_runner(name, tmp_path):
    from lgteun_amd import MODELS, build_model, mtf_hr
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    assert MODELS.get(name) is getattr(mtf_hr, name) and getattr(mtf_hr, name).rule == RUNNERS[name]
    log, notes = logging.getLogger(f'mtf_hr_{name}'), _Notes()
    log.addHandler(notes)
    log.setLevel(logging.INFO)
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0))
    runner = build_model(cfg.model_type, cfg, log, None, None, None)
    assert isinstance(runner, Base_model) and runner.module_dict == {}
    assert runner.gains_ms is None and runner.gain_pan is None and runner.n_taps == 41
    assert sum('placeholder' in line for line in notes.lines) == 1                            # the note, once
    assert runner.print_total_params() == 0
    runner.train()                                         # nothing to train: returns
    assert runner.save(iter_id=1) is None and not os.path.exists(runner.train_out)
    with pytest.raises(RuntimeError, match='nothing to train'):
        runner.train_iter(1, {})
    notes.lines.clear()
    cfg = Config(dict(work_dir=str(tmp_path / name), datas='synthetic', bit_depth=11, model_type=name, max_iter=0, mtf_gains_ms=[0.3, 0.31, 0.32, 0.33],
                      mtf_gain_pan=0.12, mtf_taps=31))
    runner = build_model(cfg.model_type, cfg, log, None, None, None)
    assert runner.gains_ms == [0.3, 0.31, 0.32, 0.33] and runner.gain_pan == 0.12 and runner.n_taps == 31
    assert not any('placeholder' in line for line in notes.lines)
    log.removeHandler(notes)


def test_functions_refuse_cpu_tensors_and_unknown_words():
    import torch
    from lgteun_amd import mtf_hr
    ms, pan = torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 32, 32)
    for rule in hr.RULES:
        with pytest.raises(ValueError, match='no CPU path'):
            mtf_hr.fuse(ms, pan, rule)
        with pytest.raises(ValueError, match='no CPU path'):
            getattr(mtf_hr, rule)(ms, pan)
    with pytest.raises(ValueError, match="'fs', 'hpm_r', 'hpm_h' or 'bt_h'"):
        mtf_hr.fuse(ms, pan, 'nope')
    with pytest.raises(ValueError, match="'fs', 'hpm_r', 'hpm_h' or 'bt_h'"):
        mtf_hr.fuse_scene('nope', np.zeros((4, 8, 8), np.uint16), np.zeros((1, 32, 32), np.uint16), bit_depth=11)
    with pytest.raises(ValueError, match='float32 NCHW'):
        mtf_hr.fuse(ms.double(), pan, 'fs')


def test_tool_accepts_the_new_methods(capsys):
    from lgteun_amd import mtf_hr
    spec = importlib.util.spec_from_file_location('fuse_scene_tool', os.path.join(ROOT, 'tools', 'fuse_scene.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for m in sorted(mtf_hr.SCENE_METHODS):
        a = tool.parser().parse_args(['scene', '--method', m])
        assert a.method == m and a.mtf_gains is None and a.mtf_gain_pan is None
        a = tool.parser().parse_args(['scene', '--method', m, '--mtf-gains', '0.3', '0.31', '--mtf-gain-pan', '0.12'])
        assert a.mtf_gains == [0.3, 0.31] and a.mtf_gain_pan == 0.12
    with pytest.raises(SystemExit):
        tool.parser().parse_args(['scene', '--method', 'hpm_x'])
    err = capsys.readouterr().err
    assert all(m in err for m in ('fs', 'hpm_r', 'hpm_h', 'bt_h', 'sfim', 'mtf_glp', 'awlp'))


def test_haze_scene_is_the_stated_one():
    for C, h, w, seed in ((4, 8, 8, 7000), (9, 4, 8, 7001), (16, 16, 8, 7000)):
        ms, pan = hr.make_haze_scene(C, h, w, seed)
        again = hr.make_haze_scene(C, h, w, seed)
        assert ms.dtype == np.float32 and pan.dtype == np.float32 and ms.shape == (C, h, w) and pan.shape == (4 * h, 4 * w)
        assert np.array_equal(ms, again[0]) and np.array_equal(pan, again[1])
        assert ms.min() > 0 and ms.max() < 1 and pan.min() > 0 and pan.max() < 1
        for k in range(C):                                  # one dark pixel per band, where the rule puts it, well under the rest of the band
            at = (5 * k + 1 + seed) % (h * w)
            assert int(ms[k].argmin()) == at and ms[k].flat[at] == np.float32(0.04 + 0.01 * k)
            assert np.partition(ms[k].ravel(), 1)[1] - ms[k].flat[at] > 0.05
    msb, panb = hr.make_haze_batch(2, 4, 8, 8)
    assert np.array_equal(msb[1], hr.make_haze_scene(4, 8, 8, 7001)[0]) and panb.shape == (2, 1, 32, 32)


def test_shape_lists_are_the_stated_ones():
    assert hr.SHAPES['hpm_r'] == mr.SHAPES and hr.PER_BAND_SHAPES['hpm_r'] == mr.PER_BAND_SHAPES
    assert hr.SHAPES['hpm_h'] == hr.HAZE_SHAPES + [(15, 12, 12, 1)] and len(hr.HAZE_SHAPES) == 13
    assert hr.PER_BAND_SHAPES['hpm_h'] == hr.HAZE_PER_BAND_SHAPES + [(15, 12, 12, 1)] and len(hr.HAZE_PER_BAND_SHAPES) == 3
    # a replaced case stands where the listed one stood; nothing else moved
    assert [a for a, b in zip(hr.SHAPES['fs'], mr.SHAPES) if a != b] == [(4, 7, 9, 2)]
    assert [a for a, b in zip(hr.SHAPES['bt_h'], hr.HAZE_SHAPES) if a != b] == [(2, 8, 12, 2), (4, 7, 9, 2)] and hr.SHAPES['bt_h'][-1] == (12, 16, 8, 1)
    for rule in hr.RULES:
        assert (4, 136, 256, 1) in hr.SHAPES[rule]         # 1088 tiles against 768 workgroups: a walker of the moments pass takes a second tile
        assert len(set(hr.SHAPES[rule])) == len(hr.SHAPES[rule]) and set(hr.PER_BAND_SHAPES[rule]) <= set(hr.SHAPES[rule])
    for rule in hr.HAZE_RULES:
        assert {s[0] for s in hr.SHAPES[rule]} >= {2, 3, 5, 9, 16}
    assert hr.PROPERTY_SHAPES == [(4, 4, 4, 1), (4, 5, 7, 2), (8, 12, 8, 3)]


def test_band_counts_at_which_the_dynamic_lds_passes_64_kib_are_in_the_lists():
    """recomputed from the *_lds_doubles functions of the k_hr_* kernels as they stand in k_classical.hip (CL_SCRATCH 2141, CL_PX 512, HR_CHUNK 256 doubles)"""
    src = open(os.path.join(ROOT, 'lgteun_amd', 'csrc', 'k_classical.hip')).read()
    for text in ('hr_gram_ns(int C, int F) { return (C + 1) * (C + 2) / 2 + F * (C + 1); }',
                 'hr_moments_lds_doubles(int C) { return CL_SCRATCH + 4 * CL_PX + HR_SUMS * C; }',
                 'hr_gram_lds_doubles(int C, int F) { return (1 + C + F) * HR_CHUNK + hr_gram_ns(C, F) + 4 * C; }',
                 'hr_apply_lds_doubles(int C, int rule) { return rule == LG_MTFHR_BT_H ? CL_SCRATCH + C * CL_PX : MG_LDS; }',
                 'constexpr int HR_SUMS = 7;', 'constexpr int HR_CHUNK = CL_NT;'):
        assert text in src, text

    def first(doubles):
        return next((C for C in range(2, 17) if 8 * doubles(C) > 65536), None)
    assert first(lambda C: 2141 + 4 * 512 + 7 * C) is None                                           # k_hr_moments: 34 408 bytes at C = 16
    assert first(lambda C: (2 + C) * 256 + (C + 1) * (C + 2) // 2 + (C + 1) + 4 * C) is None         # k_hr_gram, one plane
    assert first(lambda C: (1 + 2 * C) * 256 + (C + 1) * (C + 2) // 2 + C * (C + 1) + 4 * C) == 15   # k_hr_gram, a plane per band: 66 976 bytes
    assert first(lambda C: 2141 + 512 * C) == 12                                                     # k_hr_apply<bt_h>: 66 280 bytes
    assert any(s[0] == 15 for s in hr.PER_BAND_SHAPES['hpm_h']) and (16, 16, 8, 1) in hr.PER_BAND_SHAPES['hpm_h'] and any(s[0] == 12 for s in hr.SHAPES['bt_h'])


def test_closed_forms_equal_the_direct_forms():
    worst = 0.0
    for C, h, w in ((4, 8, 8), (8, 12, 8), (16, 16, 8), (8, 32, 32)):
        ms, pan = hr.make_haze_scene(C, h, w, 7000)
        D = mr.lowpass(pan.astype(np.float64), mr.taps(hr.EQUAL_GAIN))[2::4, 2::4]
        direct = hr.regress(ms, D)
        closed, cond = hr.regress_closed(ms, D)
        rel = float(np.abs(closed - direct).max() / np.abs(direct).max())
        worst = max(worst, rel)
        print(f'regression C={C} h={h} w={w}: closed against lstsq {rel:.3e} relative, condition {cond:.3e}')
        assert rel <= 1e-12
        H = ms.reshape(C, -1).min(axis=1).astype(np.float64)
        m64 = ms.astype(np.float64).reshape(C, -1).mean(axis=1)
        hp_direct, hp_closed = direct[C] + direct[:C] @ H, D.mean() + closed[:C] @ (H - m64)
        assert abs(hp_direct - hp_closed) <= 1e-12
    for C, h, w in ((4, 8, 8), (8, 12, 8), (4, 5, 7)):
        ms, pan = cr.make_scene(C, h, w, seed=C * 100 + h)
        for gains in ([hr.EQUAL_GAIN] * C, mr.per_band_gains(C)):
            for rule in ('fs', 'hpm_r'):
                st = hr.mtf_hr(ms, pan, rule, gains, return_stats=True)[1]
                g, b = hr.gains_closed(ms, pan, rule, gains)
                rel = max(float(np.abs(g / st[:C] - 1).max()), float(np.abs(b - st[C:2 * C]).max()))
                worst = max(worst, rel)
                print(f'{rule} C={C} h={h} w={w}: closed against direct gains {rel:.3e}')
                assert rel <= 1e-12
    print(f'worst {worst:.3e}')


def test_explicit_sums_of_the_regression_match_lstsq():
    """the normal equations written out pixel by pixel: what k_hr_gram accumulates"""
    ms, pan = hr.make_haze_scene(3, 4, 8, 7000)
    D = mr.lowpass_decimated_explicit(pan, mr.taps(hr.GAIN_PAN))
    assert np.abs(D - mr.lowpass(pan.astype(np.float64), mr.taps(hr.GAIN_PAN))[2::4, 2::4]).max() <= 1e-15
    n, C = 32, 3
    x = ms.astype(np.float64).reshape(C, -1)
    G, r, sx, sd = np.zeros((C, C)), np.zeros(C), np.zeros(C), 0.0
    for i in range(n):
        xi = x[:, i] - x[:, 0]
        G += np.outer(xi, xi)
        r += xi * D.flat[i]
        sx += xi
        sd += D.flat[i]
    slopes = np.linalg.solve(G - np.outer(sx, sx) / n, r - sx * sd / n)
    assert np.abs(slopes - hr.regress(ms, D)[:C]).max() <= 1e-12


def test_degenerate_cases():
    ms, _ = cr.make_batch(1, 4, 8, 8, seed=408)
    flat = np.full((32, 32), 0.3, np.float32)
    u = np.clip(cr.interp23(ms[0]), 0, 1)
    u32 = np.clip(cr.interp23(ms[0], np.float32), 0, 1)
    bar = max(8.0 * float(np.abs(u32.astype(np.float64) - u).max()), 2.0 ** -23)
    for rule in ('fs', 'hpm_r'):                            # g = 0 (hpm_r: b = m, r = m / m): clip(u) bit for bit
        out, st = hr.mtf_hr(ms[0], flat, rule, return_stats=True)
        assert np.array_equal(out, u) and not st[:4].any(), rule
        if rule == 'hpm_r':
            assert np.array_equal(st[4:8], cr.interp23(ms[0]).mean(axis=(1, 2)))
    for rule in hr.HAZE_RULES:                              # pan - H = L - H up to the interpolator's DC error, or a non-positive denominator: r = 1
        out = hr.mtf_hr(ms[0], flat, rule)
        err = float(np.abs(out - u).max())
        print(f'{rule}, constant PAN: distance to clip(u) {err:.3e}, bar {bar:.3e}')
        assert err <= bar, rule
    # r = 1 where the denominator is not > 0 or the ratio is not finite; g = 0 where the denominator is not > 0
    r = hr._ratio(np.array([1.0, 1.0, 1.0, np.inf]), np.array([0.0, -1.0, 2.0, 1.0]), np.float64)
    assert list(r) == [1.0, 1.0, 0.5, 1.0]
    assert hr._gain(1.0, 0.0, np.float64) == 0 and hr._gain(1.0, -2.0, np.float64) == 0 and hr._gain(1.0, np.inf, np.float64) == 0
    assert hr._gain(np.nan, 1.0, np.float64) == 0 and hr._gain(1.0, 4.0, np.float64) == 0.25
    # a constant band: the Gram matrix is singular; lstsq (minimum norm) gives that band no weight and the result stays finite
    ms2, pan2 = hr.make_haze_batch(1, 4, 8, 8)
    ms2 = ms2.copy()
    ms2[0, 2] = 0.25
    for rule in hr.HAZE_RULES:
        out, st = hr.mtf_hr(ms2[0], pan2[0, 0], rule, return_stats=True)
        assert np.isfinite(out).all() and np.isfinite(st).all()


CASES = [(rule,) + s + (False,) for rule in hr.RULES for s in hr.SHAPES[rule]] + [(rule,) + s + (True,) for rule in hr.RULES for s in hr.PER_BAND_SHAPES[rule]]


@pytest.mark.parametrize('rule,C,h,w,B,per_band', CASES)
def test_preconditions_of_the_gpu_cases(rule, C, h, w, B, per_band):
    ms, pan = hr.make_inputs(rule, C, h, w, B)
    assert ms.dtype == np.float32 and pan.dtype == np.float32 and ms.min() >= 0 and ms.max() <= 1 and pan.min() >= 0 and pan.max() <= 1
    gains = mr.per_band_gains(C) if per_band else [hr.EQUAL_GAIN] * C
    res = [hr.mtf_hr(ms[b], pan[b, 0], rule, gains, clip=False, return_den=True) for b in range(B)]
    raw, den = np.stack([r[0] for r in res]), min(r[1] for r in res)
    share = float(((raw <= hr.CLIP_MARGIN) | (raw >= 1 - hr.CLIP_MARGIN)).mean())
    cond = 0.0
    if rule in hr.HAZE_RULES:
        cond = max(hr.regress_closed(ms[b], pan[b, 0, 2::4, 2::4])[1] for b in range(B))
    print(f'{rule} C={C} h={h} w={w} B={B} {"per-band" if per_band else "equal"} gains: smallest denominator {den:.4f}, condition {cond:.3e}, '
          f'clip share {share:.5f}')
    assert den >= hr.MIN_DENOMINATOR
    assert cond <= hr.MAX_CONDITION
    assert share <= 0.02


@pytest.mark.parametrize('rule', hr.RULES)
def test_clip_case_leaves_the_range_on_both_sides(rule):
    C, h, w, B = mr.CLIP_SHAPE
    ms, pan = mr.make_clip_batch(C, h, w, B, seed=mr.CLIP_SEED)
    raw = np.stack([hr.mtf_hr(ms[b], pan[b, 0], rule, clip=False) for b in range(B)])
    below, above = float((raw < -hr.CLIP_MARGIN).mean()), float((raw > 1 + hr.CLIP_MARGIN).mean())
    print(f'{rule}: {100 * below:.1f} % below 0, {100 * above:.1f} % above 1 by more than {hr.CLIP_MARGIN}')
    assert np.isfinite(raw).all() and below > 0 and above > 0
