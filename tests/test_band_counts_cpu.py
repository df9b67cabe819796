"""No GPU: the band-count cases of tests/test_gpu_band_counts.py (C = 2 .. 16 of the training-free baselines and of the evaluation indices) and what
must hold of them before a device sees them.

The lists below are the cases; the GPU file imports them from here.
  1. every new baseline case on the restatements (classical_ref, wavelet_ref, mtf_glp_ref, bdsd_ref, cs_ref), inputs by the modules' own make_batch with the
     seed 100 C + h of the existing GPU files: the float32 run's distance e32 to the float64 run is at most 4 x the largest e32 among that method's EXISTING
     cases (computed here from the existing shape lists, never typed in), and at most 2 % of the float64 output sits on a clip boundary (the cap of
     tests/test_gpu_reference_parity.py);
  2. every block of every new BDSD case has all Cholesky pivots above PIVOT_TOL in the float64 restatement: no degenerate block;
  3. the workspace sizers answer for every C = 2 .. 16 at one fixed (B, h, w) with a positive size that never decreases with C; the Q2n sizer answers
     C = 9 with 0 and a reason;
  4. C = 1, C = 17 (and C = 9 for the Q2n entries) are refused with a reason before any HIP call, with limits_helpers' never-dereferenced pointers -- only the
     rows tests/test_abi_limits_cpu.py does not hold already.

Measured (float64 / float32 numpy on the host): e32 of the new cases interp23 3.7e-8 - 4.7e-8, sfim 8.5e-8 - 1.0e-7, gsa 6.4e-8 - 1.2e-7, wavelet 1.8e-7 - 2.2e-7,
glp 7.9e-8 - 1.1e-7, hpm 8.4e-8 - 1.3e-7, cbd 1.5e-7 - 1.9e-6, bdsd 2.7e-7 - 1.4e-6, ihs 4.6e-8 - 5.2e-8, brovey 8.2e-8 - 9.1e-8, gs 7.2e-8 - 7.5e-8,
pca 5.2e-8 - 6.4e-8: each below the largest e32 of its method's existing cases (0.02 - 0.74 of it) except cbd, which reaches 2.27 x the existing 8.3e-7 at
(16, 6, 9, 2); clip share 0 everywhere except cbd at C = 2 and 3 (at most 0.0033); the smallest BDSD pivot over its G_jj is 5.2e-6 (PIVOT_TOL is 1e-12);
PCA's eigen gap on the two new cases is 0.86 - 0.90."""
import ctypes
import functools

import numpy as np
import pytest

import bdsd_ref as br
import classical_ref as cr
import cs_ref as cs
import mtf_glp_ref as mr
import wavelet_ref as wr
from limits_helpers import FAKE
from lgteun_amd import _lib

# ---- the cases: (C, h, w, B) in MS pixels ---------------------------------------------------------------------------------------------------------------
SMALL = [(C, 5, 7, 2) for C in (2, 3, 5)]                 # the minimum and the odd counts: planes and the second sample off 16-byte boundaries
PAST_64K = [(C, 5, 7, 2) for C in (9, 11, 12, 15)]        # the first counts whose dynamic LDS passes 64 KiB: k_cl_moments, k_cl_apply, k_bd_apply, k_bd_gram
MAXIMUM = [(16, 6, 9, 2), (16, 9, 17, 1)]                 # one ragged tile row and two tiles in x; 3 x 3 tiles, ragged on both sides
BAND_SHAPES = SMALL + PAST_64K + MAXIMUM                  # interp23, SFIM, GSA, Wavelet, MTF-GLP
MTF_CASES = [s + (False,) for s in BAND_SHAPES] + [(3, 5, 7, 2, True), (16, 6, 9, 2, True)]          # ..., per-band gains
# C, h, w, B, block (None: global), per-band gains
BDSD_CASES = [(16, 16, 16, 1, None, False), (11, 16, 16, 1, None, False), (5, 5, 7, 2, None, False), (16, 16, 32, 1, 64, False), (3, 8, 16, 2, 32, False),
              (16, 16, 16, 1, None, True)]
CS_SHAPES = [(3, 5, 7, 2), (16, 6, 9, 2)]
INDEX_BANDS = (2, 3, 5, 16)
REF_SIZES = [(16, 16), (44, 52)]                          # lg_iqa_ref: H, W of the images
NO_REF_SIZES = [(32, 32), (64, 96)]                       # lg_iqa_no_ref: H, W of the fused image
Q2N_BANDS = (6, 7)                                        # the <8> instance with one and two zero planes
Q2N_SIZES = [(32, 32), (48, 80)]
# D_lambda_K and HQNR: Q2n of the MS image against the degraded fused image, so 2 <= C <= 8 and MS sides >= 32 (include/lgteun_hip.h): the smallest images
# the entry takes, and one with a mirrored extension; C = 16 and the sizes of NO_REF_SIZES are refused (test_the_extended_no_reference_set_...)
EXT_NO_REF_BANDS = (2, 3, 5)
EXT_NO_REF_SIZES = [(128, 128), (128, 160)]

CLIP_CAP = 0.02
E32_FACTOR = 4.0
CLASSICAL_METHODS = ('interp23', 'sfim', 'gsa')
CLASSICAL_REF = {'interp23': lambda ms, pan, dt: cr.interp23(ms, dt), 'sfim': cr.sfim, 'gsa': cr.gsa}


def seed_of(C, h):
    return C * 100 + h


def mtf_gains(C, per_band):
    return mr.per_band_gains(C) if per_band else [mr.EQUAL_GAIN] * C


def bdsd_gains(C, per_band):
    return mr.per_band_gains(C) if per_band else [br.EQUAL_GAIN] * C


# ---- 1. restatement noise and clip share ----------------------------------------------------------------------------------------------------------------
def _figures(run, B):
    """run(b, dtype) -> one sample's output: (e32, clip share) over the batch"""
    r64 = np.stack([run(b, np.float64) for b in range(B)])
    r32 = np.stack([run(b, np.float32) for b in range(B)])
    assert r64.dtype == np.float64 and r32.dtype == np.float32
    return float(np.abs(r32.astype(np.float64) - r64).max()), float(((r64 <= 0) | (r64 >= 1)).mean())


@functools.lru_cache(maxsize=None)
def classical_figures(C, h, w, B):
    ms, pan = cr.make_batch(B, C, h, w, seed=seed_of(C, h))
    res = {m: _figures(lambda b, dt, m=m: CLASSICAL_REF[m](ms[b], pan[b, 0], dt), B) for m in CLASSICAL_METHODS}
    ms, pan = wr.make_batch(C, h, w, B)
    res['wavelet'] = _figures(lambda b, dt: wr.wavelet(ms[b], pan[b, 0], dt), B)
    return res


@functools.lru_cache(maxsize=None)
def mtf_figures(C, h, w, B, per_band):
    ms, pan = cr.make_batch(B, C, h, w, seed=seed_of(C, h))
    gains = mtf_gains(C, per_band)
    return {mode: _figures(lambda b, dt, mode=mode: mr.mtf_glp(ms[b], pan[b, 0], mode, gains, dtype=dt), B) for mode in mr.MODES}


@functools.lru_cache(maxsize=None)
def bdsd_figures(C, h, w, B, block, per_band):
    """the share is that of tests/test_gpu_bdsd.py: of the UNCLIPPED float64 output outside (0, 1)"""
    ms, pan = br.make_batch(B, C, h, w, seed=seed_of(C, h))
    gains = bdsd_gains(C, per_band)
    e32, _ = _figures(lambda b, dt: br.bdsd(ms[b], pan[b, 0], gains, block, dtype=dt), B)
    raw = np.stack([br.bdsd(ms[b], pan[b, 0], gains, block, clip=False) for b in range(B)])
    return {'bdsd': (e32, float(((raw <= 0) | (raw >= 1)).mean()))}


@functools.lru_cache(maxsize=None)
def cs_figures(C, h, w, B):
    ms, pan = cs.make_batch(B, C, h, w, seed=seed_of(C, h))
    u = {np.float64: [cr.interp23(ms[b]) for b in range(B)], np.float32: [cr.interp23(ms[b], np.float32) for b in range(B)]}
    return {mode: _figures(lambda b, dt, mode=mode: cs.fuse(ms[b], pan[b, 0], mode, dtype=dt, u=u[dt][b]), B) for mode in cs.MODES}


def existing_cases():
    """family -> (figures function, the cases the GPU files run today)"""
    bd =[c + (False,) for c in br.CASES] + [c + (True,) for c in br.PER_BAND_CASES]
    mt = [s + (False,) for s in mr.SHAPES] + [s + (True,) for s in mr.PER_BAND_SHAPES]
    assert wr.SHAPES == mr.SHAPES                     # tests/test_gpu_classical.py's seven; the Wavelet file adds one of its own
    return {'classical': (classical_figures, wr.SHAPES + [(4, 9, 72, 1)]), 'mtf': (mtf_figures, mt), 'bdsd': (bdsd_figures, bd),
            'cs': (cs_figures, cs.SHAPES)}


NEW_CASES = {'classical': BAND_SHAPES, 'mtf': MTF_CASES, 'bdsd': BDSD_CASES, 'cs': CS_SHAPES}


@functools.lru_cache(maxsize=None)
def largest_existing_e32(family):
    """method -> the largest e32 among the family's existing cases"""
    fn, cases = existing_cases()[family]
    top = {}
    for case in cases:
        for method, (e32, _) in fn(*case).items():
            top[method] = max(top.get(method, 0.0), e32)
    return top


@pytest.mark.parametrize('family,case', [(f, c) for f, cases in NEW_CASES.items() for c in cases], ids=lambda v: v if isinstance(v, str) else '-'.join(map(str, v)))
def test_restatement_noise_and_clip_share_of_the_new_cases(family, case):
    top = largest_existing_e32(family)
    for method, (e32, share) in existing_cases()[family][0](*case).items():
        print(f'{method} {case}: float32 restatement {e32:.3e} (largest of the existing cases {top[method]:.3e}, x {e32 / top[method]:.2f}), clip share {share:.4f}')
        assert e32 <= E32_FACTOR * top[method], (method, case, e32, top[method])
        assert share <= CLIP_CAP, (method, case, share)


@pytest.mark.parametrize('C,h,w,B', CS_SHAPES)
def test_pca_axis_of_the_new_cs_cases_is_well_separated(C, h, w, B):
    """what tests/test_cs_cpu.py asks of cs_ref.SHAPES: an eigen gap of at least 0.5 and no degenerate sample, or the float64 restatement's own axis is loose"""
    ms, pan = cs.make_batch(B, C, h, w, seed=seed_of(C, h))
    for b in range(B):
        st = cs.fuse(ms[b], pan[b, 0], 'pca', return_stats=True)[2]
        gap = float((st['lam'][-1] - st['lam'][-2]) / st['lam'][-1])
        print(f'pca C={C} h={h} w={w} sample {b}: eigen gap {gap:.3f}')
        assert gap >= 0.5 and not st['degenerate'], (b, gap)


def test_the_cases_are_those_of_the_issue():
    assert sorted({c[0] for c in BAND_SHAPES}) == [2, 3, 5, 9, 11, 12, 15, 16]
    assert all(h * w % 2 == 1 and B == 2 for C, h, w, B in SMALL + PAST_64K)          # odd planes: sample 1 of an odd C starts off a 16-byte boundary
    assert all(4 * h * 4 * w <= 136 * 68 for C, h, w, B in BAND_SHAPES + CS_SHAPES) and all(16 * c[1] * c[2] <= 136 * 68 for c in BDSD_CASES)
    for C, h, w, B, block, _ in BDSD_CASES:
        assert h * w >= 2 * (C + 1) if block is None else block % 32 == 0 and (4 * h) % block == 0 and (4 * w) % block == 0
        assert (h * w if block is None else (block // 4) ** 2) >= 4 * (C + 1)             # more low-resolution pixels than regressors, with room
    assert not set(NEW_CASES['classical']) & set(wr.SHAPES) and not set(CS_SHAPES) & set(cs.SHAPES) and not {c[:5] for c in BDSD_CASES} & set(br.CASES)


# ---- 2. BDSD: no degenerate block -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,h,w,B,block,per_band', BDSD_CASES)
def test_every_bdsd_block_is_regular(C, h, w, B, block, per_band):
    ms, pan = br.make_batch(B, C, h, w, seed=seed_of(C, h))
    sy, sx = (h, w) if block is None else (block // 4, block // 4)
    smallest = np.inf
    for b in range(B):
        x, _ = br.regressors(ms[b], pan[b, 0], bdsd_gains(C, per_band))
        gamma = br.weights(ms[b], pan[b, 0], bdsd_gains(C, per_band), block, route='cholesky')
        for I in range(h // sy):
            for J in range(w // sx):
                X = x[:, I * sy:(I + 1) * sy, J * sx:(J + 1) * sx].reshape(C + 1, -1).T
                G = X.T @ X
                d = np.diag(np.linalg.cholesky(G)) ** 2
                smallest = min(smallest, float((d / np.diag(G)).min()))
                assert np.all(np.isfinite(d)) and np.all(d > br.PIVOT_TOL * np.diag(G)), (b, I, J, d / np.diag(G))
                assert np.abs(gamma[I, J]).max() > 0, (b, I, J)
    print(f'C={C} h={h} w={w} B={B} block={block}: smallest pivot over its G_jj {smallest:.3e} (PIVOT_TOL {br.PIVOT_TOL:.0e})')


# ---- 3. the sizers --------------------------------------------------------------------------------------------------------------------------------------
def sizers():
    L = _lib.lib()
    B, h, w = 2, 16, 16
    return {
        'lg_classical_workspace_bytes/sfim': lambda C: L.lg_classical_workspace_bytes(B, C, h, w, _lib.LG_CLASSICAL_SFIM),
        'lg_classical_workspace_bytes/gsa': lambda C: L.lg_classical_workspace_bytes(B, C, h, w, _lib.LG_CLASSICAL_GSA),
        'lg_mtfglp_workspace_bytes/glp': lambda C: L.lg_mtfglp_workspace_bytes(B, C, h, w, 1, _lib.LG_MTFGLP_GLP),
        'lg_mtfglp_workspace_bytes/cbd per band': lambda C: L.lg_mtfglp_workspace_bytes(B, C, h, w, C, _lib.LG_MTFGLP_CBD),
        'lg_bdsd_workspace_bytes/global': lambda C: L.lg_bdsd_workspace_bytes(B, C, h, w, 0),
        'lg_bdsd_workspace_bytes/32': lambda C: L.lg_bdsd_workspace_bytes(B, C, h, w, 32),
        'lg_cs_workspace_bytes': lambda C: L.lg_cs_workspace_bytes(B, C, h, w),
        'lg_iqa_workspace_bytes/ref': lambda C: L.lg_iqa_workspace_bytes(B, C, 4 * h, 4 * w, 0),
        'lg_iqa_workspace_bytes/no_ref': lambda C: L.lg_iqa_workspace_bytes(B, C, 4 * h, 4 * w, 1),
    }


SIZER_NAMES = ('lg_classical_workspace_bytes/sfim', 'lg_classical_workspace_bytes/gsa', 'lg_mtfglp_workspace_bytes/glp', 'lg_mtfglp_workspace_bytes/cbd per band',
               'lg_bdsd_workspace_bytes/global', 'lg_bdsd_workspace_bytes/32', 'lg_cs_workspace_bytes', 'lg_iqa_workspace_bytes/ref', 'lg_iqa_workspace_bytes/no_ref')


@pytest.mark.parametrize('name', SIZER_NAMES)
def test_sizers_answer_for_every_band_count(name):
    assert set(sizers()) == set(SIZER_NAMES)
    f = sizers()[name]
    sizes = [int(f(C)) for C in range(2, 17)]
    print(f'{name}, C = 2 .. 16 at B = 2, MS 16 x 16: {sizes}')
    assert all(s > 0 and s % 8 == 0 for s in sizes), (name, sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), (name, sizes)
    assert sizes[-1] > sizes[0], (name, sizes)
    assert f(1) == 0 and f(17) == 0, name


def test_the_q2n_sizer_stops_at_eight_bands_and_says_so():
    L = _lib.lib()
    sizes = [int(L.lg_iqa_ext_workspace_bytes(2, C, 64, 64)) for C in range(2, 9)]
    assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    L.lg_cs_workspace_bytes(2, 4, 3, 8)                                      # leaves another entry's message
    assert L.lg_iqa_ext_workspace_bytes(2, 9, 64, 64) == 0
    msg = L.lg_last_error().decode()
    assert msg.startswith('lg_iqa_ext_workspace_bytes:') and 'C must be 2..8' in msg and '9' in msg, msg


# ---- 4. rejections before any HIP call ------------------------------------------------------------------------------------------------------------------
P, PW, WS = FAKE, FAKE + (1 << 24), 1 << 40
# entry -> (prefix of its messages, call(C)); tests/test_abi_limits_cpu.py holds C = 1 and C = 17 of the six classical entries and of lg_iqa_ref, C = 17 of
# lg_iqa_no_ref, C = 1 and C = 9 of lg_iqa_ref_ext and C = 9 of lg_iqa_q2n; tests/test_cs_cpu.py holds lg_cs with pointers of its own.  What is left:
MISSING = [('lg_cs', 1), ('lg_cs', 17), ('lg_iqa_no_ref', 1), ('lg_iqa_ref_ext', 17), ('lg_iqa_q2n', 1), ('lg_iqa_q2n', 16), ('lg_iqa_q2n', 17)]


def call_with_bands(entry, C):
    L = _lib.lib()
    if entry == 'lg_cs':
        return 'cs', L.lg_cs(P, P, P, P, None, _lib.LG_CS_GS, 2, C, 8, 8, PW, WS, None)
    if entry == 'lg_iqa_no_ref':
        return 'iqa', L.lg_iqa_no_ref(P, P, P, P, 2, C, 32, 32, 1.0, PW, WS, None)
    return entry, getattr(L, entry)(P, P, P, 2, C, 32, 32, 1.0, PW, WS, None)


@pytest.mark.parametrize('entry,C', MISSING)
def test_band_counts_outside_the_range_are_refused_by_name(entry, C):
    L = _lib.lib()
    L.lg_batch_assemble(None, None, None, None, 0, None, 0, None, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 1.0, 0, 1.0, None)      # another entry's message
    prefix, rc = call_with_bands(entry, C)
    msg = L.lg_last_error().decode()
    assert rc < 0, (entry, C, rc, msg)
    assert msg.startswith(prefix + ':') and 'C must be' in msg and f'got {C}' in msg, (entry, C, msg)
    assert not any(word in msg.lower() for word in ('hip', 'invalid device', 'illegal', 'launch fail', 'out of memory')), msg


def test_the_extended_no_reference_set_is_bounded_by_q2n():
    """D_lambda_K is 1 - Q2n of [B, C, H / 4, W / 4] images: lg_iqa_q2n refuses C = 16 and the MS sides of NO_REF_SIZES, which is why the GPU file runs that set
    at EXT_NO_REF_BANDS and EXT_NO_REF_SIZES"""
    L = _lib.lib()
    for H, W in NO_REF_SIZES:
        assert L.lg_iqa_q2n(P, P, P, 2, 5, H // 4, W // 4, 1.0, PW, WS, None) < 0
        assert 'H and W must be >= 32' in L.lg_last_error().decode()
    assert max(EXT_NO_REF_BANDS) <= 8 < max(INDEX_BANDS)
    for H, W in EXT_NO_REF_SIZES:
        assert min(H, W) // 4 == 32 and all(L.lg_iqa_ext_workspace_bytes(2, C, H // 4, W // 4) > 0 for C in EXT_NO_REF_BANDS)
    assert ctypes.sizeof(ctypes.c_void_p) == 8 and P % 4096 == 0
