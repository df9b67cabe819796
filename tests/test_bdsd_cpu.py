"""No GPU: the surface of the BDSD baseline -- the registry entry, the C ABI names, the argument checks of the function and of the library (lg_bdsd returns
before it touches a device), the command line -- and self-checks of the numpy restatement the GPU tests compare with (tests/bdsd_ref.py): its two solve
routes against each other, the MS-grid low-pass as explicit clamped sums against the scipy form, and the inputs of the GPU tests.

Measured: the weights of the two routes (lstsq against normal equations plus Cholesky) differ by 7.8e-12 .. 1.2e-9 of a sample's largest |gamma|; explicit
against scipy low-pass at most 2.0e-15; no element of an unclipped float64 result of the GPU cases lies outside (0, 1); the clip case leaves [0, 1] below on 10.7 %
and 36.2 % and above on 29.2 % and 3.0 % of its two samples."""
import importlib.util
import logging
import os

import numpy as np
import pytest

import bdsd_ref as br
import classical_ref as cr
import mtf_glp_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lg_bdsd_workspace_bytes', 'lg_bdsd')


def cases():
    for case in br.CASES:
        yield case + (False,)
        if case in br.PER_BAND_CASES:
            yield case + (True,)


def gains_of(C, per_band):
    return mr.per_band_gains(C) if per_band else [br.EQUAL_GAIN] * C


def test_the_cases_are_those_of_the_issue():
    assert len(br.CASES) == 12 and len(list(cases())) == 15 and all(c in br.CASES for c in br.PER_BAND_CASES)
    for C, h, w, B, block in br.CASES:
        assert block is None and h * w >= 2 * (C + 1) or block % 32 == 0 and (4 * h) % block == 0 and (4 * w) % block == 0


@pytest.mark.parametrize('C,h,w,B,block,per_band', list(cases()))
def test_inputs_of_the_gpu_tests_stay_in_range_and_the_two_routes_agree(C, h, w, B, block, per_band):
    ms, pan = br.make_batch(B, C, h, w, seed=C * 100 + h)
    assert ms.dtype == np.float32 and pan.dtype == np.float32
    assert ms.min() >= 0.02 and ms.max() <= 0.98 and pan.min() >= 0.02 and pan.max() <= 0.98           # the generator stays in [0.02, 0.98]
    gains = gains_of(C, per_band)
    outside = 0
    for b in range(B):
        raw, g = br.bdsd(ms[b], pan[b, 0], gains, block, return_stats=True, clip=False)
        g2 = br.weights(ms[b], pan[b, 0], gains, block, route='cholesky')
        assert g.shape == ((1, 1) if block is None else (4 * h // block, 4 * w // block)) + (C, C + 1) and np.abs(g).reshape(-1, C * (C + 1)).max(axis=1).min() > 0
        dist = br.gamma_distance(g2, g)
        print(f'C={C} h={h} w={w} block={block} sample {b}: lstsq against normal equations {dist:.3e} of the largest |gamma| {np.abs(g).max():.2f}')
        assert dist <= 1e-8                           # both routes are fp64; cond(G) up to 4e7 leaves about this much between them
        outside += int(((raw <= 0) | (raw >= 1)).sum())
    share = outside / (B * C * 16 * h * w)
    print(f'C={C} h={h} w={w} B={B} block={block} gains {gains[0]:.2f} .. {gains[-1]:.2f}: share outside (0, 1) {share:.4f}')
    assert share <= 0.02


def test_explicit_ms_lowpass_equals_the_scipy_form():
    band = np.random.default_rng(3).uniform(0, 1, (9, 14))
    for gain, n in ((0.3, 41), (0.22, 41), (0.3, 63), (0.15, 5), (0.3, 1)):
        t = mr.taps(gain, n)
        err = float(np.abs(br.lowpass_ms_explicit(band, t) - br.lowpass_ms(band, t)).max())
        print(f'gain {gain}, {n} taps: explicit against scipy {err:.3e}')
        assert err <= 1e-14


def test_degenerate_blocks_give_zero_weights_on_both_routes():
    """constant bands and constant PAN over the 41 taps' reach of the first two blocks: rank 1, so gamma = 0 there and the output is clip(u)"""
    ms, pan = br.make_batch(1, 4, 8, 64, seed=2)
    ms, pan = ms[0].copy(), pan[0, 0].copy()
    ms[:, :, :40], pan[:, :160] = 0.25, 0.5
    for route in ('lstsq', 'cholesky'):
        g = br.weights(ms, pan, [br.EQUAL_GAIN] * 4, 32, route=route)
        # (blocks 2 and 3 see the varying part through the taps' tails only: borderline, and not asked about)
        assert g.shape == (1, 8, 4, 5) and not g[0, :2].any() and all(g[0, J].any() for J in range(4, 8)), route
    out = br.bdsd(ms, pan, [br.EQUAL_GAIN] * 4, 32)
    assert np.array_equal(out[:, :, :64], np.clip(cr.interp23(ms), 0, 1)[:, :, :64])
    flat = np.full((4, 8, 8), 0.25, np.float32), np.full((32, 32), 0.5, np.float32)
    for route in ('lstsq', 'cholesky'):
        assert not br.weights(*flat, [br.EQUAL_GAIN] * 4, None, route=route).any(), route


def test_clip_case_leaves_the_range_on_both_sides():
    C, h, w, B, block = br.CLIP_CASE
    ms, pan = br.make_clip_batch(C, h, w, B, seed=br.CLIP_SEED)
    assert ms.dtype == np.float32 and pan.dtype == np.float32 and ms.min() >= 0 and ms.max() <= 1 and pan.min() >= 0 and pan.max() <= 1
    for b in range(B):
        raw = br.bdsd(ms[b], pan[b, 0], [br.EQUAL_GAIN] * C, block, clip=False)
        below, above = float((raw < -br.CLIP_MARGIN).mean()), float((raw > 1 + br.CLIP_MARGIN).mean())
        print(f'sample {b}: {100 * below:.1f} % below 0, {100 * above:.1f} % above 1 by more than {br.CLIP_MARGIN}')
        assert below >= 0.02 and above >= 0.02


def test_names_are_declared_bound_and_exported():
    import lgteun_amd
    from lgteun_amd import _lib, bdsd
    header = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + '(' in header
        assert hasattr(L, name)
    assert _lib.LG_ABI_VERSION == 2 and L.lg_abi_version() == 2 and '#define LG_ABI_VERSION 2' in header
    assert lgteun_amd.bdsd is bdsd and callable(bdsd.bdsd) and callable(bdsd.fuse_scene) and lgteun_amd.BDSD is bdsd.BDSD


def test_size_function():
    from lgteun_amd import _lib
    L = _lib.lib()
    glob, b32, b64 = (L.lg_bdsd_workspace_bytes(2, 4, 32, 32, block) for block in (0, 32, 64))
    assert all(n > 0 and n % 8 == 0 for n in (glob, b32, b64))
    assert min(glob, b32, b64) >= 2 * 5 * 32 * 32 * 8                   # D and the C planes of A, fp64 [h, w] per sample
    assert b32 - b64 >= 2 * (16 - 4) * (4 * 5 + 35) * 8 - 2 * 256       # 12 more blocks per sample: their weights and Gram entries (two regions, 256-byte aligned)
    assert L.lg_bdsd_workspace_bytes(2, 4, 32, 32, 128) > 0 and L.lg_bdsd_workspace_bytes(1, 8, 4, 8, 0) > 0
    for bad in ((0, 4, 8, 8, 0), (65536, 4, 8, 8, 0), (2, 1, 8, 8, 0), (2, 17, 8, 8, 0), (2, 4, 3, 8, 0), (2, 4, 8, 4097, 0), (2, 4, 8, 8, -32), (2, 4, 8, 8, 16),
                (2, 4, 8, 8, 48), (2, 4, 8, 8, 64), (2, 4, 24, 16, 96), (2, 4, 16, 24, 96), (1, 8, 4, 4, 0), (1, 16, 4, 8, 0)):
        assert L.lg_bdsd_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_named_before_any_device_call():
    """the pointers are made-up addresses: a call that got past its checks would fault here"""
    from lgteun_amd import _lib
    L = _lib.lib()
    ms, pan, out, tm, tpan, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x48000, 0x50000
    need = L.lg_bdsd_workspace_bytes(2, 4, 8, 8, 0)

    def call(ms=ms, pan=pan, out=out, stats=None, tm=tm, F=1, tpan=tpan, n=41, block=0, B=2, C=4, h=8, w=8, ws=ws, nbytes=need):
        return L.lg_bdsd(ms, pan, out, stats, tm, F, tpan, n, block, B, C, h, w, ws, nbytes, None)
    cases = [(dict(ms=None), 'ms is NULL'), (dict(pan=None), 'pan is NULL'), (dict(out=None), 'out is NULL'), (dict(tm=None), 'taps_ms is NULL'),
             (dict(tpan=None), 'taps_pan is NULL'), (dict(ws=None), 'workspace is NULL'), (dict(ms=ms + 4), 'ms must be 16-byte aligned'),
             (dict(pan=pan + 8), 'pan must be 16-byte aligned'), (dict(out=out + 4), 'out must be 16-byte aligned'),
             (dict(tm=tm + 4), 'taps_ms must be 8-byte aligned'), (dict(tpan=tpan + 4), 'taps_pan must be 8-byte aligned'),
             (dict(stats=0x60004), 'stats must be 8-byte aligned'), (dict(ws=ws + 4), 'workspace must be 8-byte aligned'),
             (dict(C=1), 'C must be'), (dict(C=17), 'C must be'), (dict(h=3), 'h must be'), (dict(w=4097), 'w must be'), (dict(B=0), 'B must be'),
             (dict(B=65536), 'B must be'), (dict(F=0), 'n_filters must be'), (dict(F=2), 'n_filters must be'), (dict(F=5), 'n_filters must be'),
             (dict(n=40), 'n_taps must be'), (dict(n=65), 'n_taps must be'), (dict(n=0), 'n_taps must be'), (dict(block=48), 'block must be 0 (global) or a multiple of 32'),
             (dict(block=16), 'block must be 0'), (dict(block=-32), 'block must be 0'), (dict(block=64), 'block must divide'),
             (dict(h=24, w=16, block=96), 'block must divide'), (dict(C=8, h=4, w=4), 'the global form needs'),
             (dict(nbytes=need - 8), 'workspace_bytes too small'), (dict(block=32, nbytes=8), 'workspace_bytes too small')]
    for kw, text in cases:
        assert call(**kw) < 0, text
        assert text in L.lg_last_error().decode() and 'bdsd' in L.lg_last_error().decode(), (text, L.lg_last_error())
    with pytest.raises(_lib.LgteunHipError, match='out is NULL'):
        _lib.check(call(out=None), 'lg_bdsd')


def test_registry_builds_the_runner(tmp_path, caplog):
    from lgteun_amd import MODELS, bdsd, build_model
    from lgteun_amd.base_model import Base_model
    from lgteun_amd.compat import Config
    assert MODELS.get('BDSD') is bdsd.BDSD
    cfg = Config(dict(work_dir=str(tmp_path / 'a'), datas='synthetic', bit_depth=11, model_type='BDSD', max_iter=0))
    with caplog.at_level(logging.INFO, logger='t'):
        runner = build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)
    assert sum('placeholder' in r.getMessage() for r in caplog.records) == 1          # no gains in the config: said once
    assert isinstance(runner, Base_model) and runner.module_dict == {}
    assert runner.block is None and runner.gains_ms is None and runner.gain_pan is None and runner.n_taps == 41
    assert runner.print_total_params() == 0
    runner.train()                                         # nothing to train: returns
    assert runner.save(iter_id=1) is None and not os.path.exists(runner.train_out)
    with pytest.raises(RuntimeError, match='nothing to train'):
        runner.train_iter(1, {})
    caplog.clear()
    cfg = Config(dict(work_dir=str(tmp_path / 'b'), datas='synthetic', bit_depth=11, model_type='BDSD', max_iter=0, bdsd_block=128,
                      mtf_gains_ms=[0.3, 0.28, 0.26, 0.24], mtf_gain_pan=0.11, mtf_taps=31))
    with caplog.at_level(logging.INFO, logger='t'):
        runner = build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)
    assert runner.block == 128 and list(runner.gains_ms) == [0.3, 0.28, 0.26, 0.24] and runner.gain_pan == 0.11 and runner.n_taps == 31
    assert not any('placeholder' in r.getMessage() for r in caplog.records)


def test_function_refuses_cpu_tensors_bad_blocks_and_bad_tap_counts():
    import torch
    from lgteun_amd import bdsd
    ms, pan = torch.zeros(1, 4, 8, 16), torch.zeros(1, 1, 32, 64)
    for block in (None, 32):
        with pytest.raises(ValueError, match='no CPU path'):
            bdsd.bdsd(ms, pan, block)
    for block in (48, 16, 0, -32, 32.5, True, '32'):
        with pytest.raises((ValueError, TypeError), match='multiple of 32'):
            bdsd.bdsd(ms, pan, block)
    for block in (64, 96):
        with pytest.raises(ValueError, match='does not divide'):
            bdsd.bdsd(ms, pan, block)
    with pytest.raises(ValueError, match='global form needs'):
        bdsd.bdsd(torch.zeros(1, 8, 4, 4), torch.zeros(1, 1, 16, 16))
    for n in (40, 0, 65, -1, 41.5):
        with pytest.raises(ValueError, match='n_taps must be odd'):
            bdsd.bdsd(ms, pan, n_taps=n)
    with pytest.raises(ValueError, match='float32 NCHW'):
        bdsd.bdsd(ms.double(), pan)
    with pytest.raises(ValueError, match='float32 NCHW'):
        bdsd.bdsd(ms[0], pan)
    with pytest.raises(ValueError, match='float32 NCHW'):
        bdsd.bdsd(ms.numpy(), pan)


def test_tool_accepts_the_method(capsys):
    spec = importlib.util.spec_from_file_location('fuse_scene_tool', os.path.join(ROOT, 'tools', 'fuse_scene.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parser().parse_args(['scene', '--method', 'bdsd'])
    assert a.method == 'bdsd' and a.bdsd_block is None and a.mtf_gains is None and a.mtf_gain_pan is None
    a = tool.parser().parse_args(['scene', '--method', 'bdsd', '--bdsd-block', '128', '--mtf-gains', '0.3', '0.28', '0.26', '0.24', '--mtf-gain-pan', '0.11'])
    assert a.bdsd_block == 128 and a.mtf_gains == [0.3, 0.28, 0.26, 0.24] and a.mtf_gain_pan == 0.11
    with pytest.raises(SystemExit):
        tool.parser().parse_args(['scene', '--method', 'nope'])
    assert 'bdsd' in capsys.readouterr().err
