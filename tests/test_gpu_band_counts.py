"""-m gpu: the band-count range of the training-free baselines and of the evaluation indices, C = 2 .. 16 (include/lgteun_hip.h: 2 <= C <= LG_IQA_MAX_BANDS;
2 .. 8 for Q2n).  The other GPU files run C = 4 and 8 and a few others at B = 1; the cases here are tests/test_band_counts_cpu.py's, which also holds their
preconditions (restatement noise, clip share, regular BDSD blocks, sizers, rejections).  Every case goes through the helpers and gates of its entry's own file
(raw_call, case / _reference / restate, assert_close): nothing is restated and no tolerance is new.

Which band count covers which edge (MS shapes (C, h, w, B); 16 x 32 output tiles):
  2, 3, 5 at (C, 5, 7, 2)      the minimum and the odd counts; h w = 35 is odd, so every second plane, and for C = 3 and 5 the second SAMPLE of ms, starts off a
                               16-byte boundary; sides off every grid; one upper-triangle pair at C = 2 in k_iqa_win
  9, 11, 12, 15 at (C, 5, 7, 2) the first counts whose dynamic LDS passes 64 KiB, so that the opt-in of cl_lds_attr / bd_lds_attr (lds_attr_set) decides the launch.
                               Recomputed from the *_lds_doubles functions of k_classical.hip as they stand (CL_SCRATCH 2141, CL_PX 512, CL_LPX 32, CL_MAX_SUMS 342,
                               BD_CHUNK 256 doubles):
                                 cl_moment_lds_doubles(C) = 2483 + 544 (C + 2)         C = 8: 63 384 bytes, C = 9: 67 736, C = 16: 98 200
                                 cl_apply_lds_doubles(C)  = 2861 + 512 C               C = 10: 63 848, C = 11: 67 944
                                 bd_apply_lds_doubles(C)  = 2141 + 512 C + C (C + 1)   C = 11: 63 240, C = 12: 67 528
                                 bd_gram_lds_doubles(C)   = 256 (2 C + 1) + (C + 1)(C + 2) / 2 + C (C + 1)   C = 14: 62 032, C = 15: 66 496, C = 16: 70 984
                               none has moved: the thresholds are 9, 11, 12 and 15
  16 at (16, 6, 9, 2)          the maximum: 342 pairs in k_cl_moments against CL_MAX_SUMS, vector numbers up to 17 in cl_pair, GSA's 16 x 16 and BDSD's 17 x 17 Cholesky
                               (Lm[CL_MAX_C * CL_MAX_C], BD_MAX_N), MTF-GLP's 4 * CL_MAX_C sums; one ragged tile row, two tiles in x
  16 at (16, 9, 17, 1)         3 x 3 tiles, ragged on both sides, at the workgroup budget of one per CU (`resident` in launch)
  BDSD                         global (16, 16, 16, 1), (11, 16, 16, 1), (5, 5, 7, 2); block-wise (16, 16, 32, 1, block 64), (3, 8, 16, 2, block 32); per-band gains at
                               (16, 16, 16, 1): more low-resolution pixels than regressors, or the float64 restatement itself is ill-conditioned
  MTF-GLP                      all three modes; per-band gains (one filtered plane per band) at (3, 5, 7, 2) and (16, 6, 9, 2)
  IHS / Brovey / GS / PCA      (3, 5, 7, 2) and (16, 6, 9, 2): B = 2 at the two counts tests/test_gpu_cs.py runs at B = 1
  lg_iqa_ref                   C in {2, 3, 5, 16} at 16 x 16 and 44 x 52, B = 2
  lg_iqa_no_ref                C in {2, 3, 5, 16} at 32 x 32 and 64 x 96, B = 2: 1, 3, 10 and 120 band pairs through k_iqa_win's decoder, C (C + 1) / 2 in k_iqa_fin_noref
  Q2n, SCC, CC                 C in {6, 7} at 32 x 32 and 48 x 80: k_iqa_q2n<8> with two and one zero planes
  D_lambda_K, HQNR             C in {2, 3, 5} at 128 x 128 and 128 x 160: they are Q2n of the MS image, so C <= 8 and MS sides >= 32 -- the smallest images the entry takes
                               (tests/test_band_counts_cpu.py holds the refusal of C = 16 and of smaller images); C = 5 is k_iqa_q2n<8> with three zero planes

Measured on an MI355X, over the cases above (error: the largest absolute difference to the float64 restatement; e32: the float32 restatement's own; the bar is
max(8 e32, 2^-23)).  Every launch past 64 KiB went through; nothing failed:
  interp23   error 1.5e-8 - 2.1e-8   e32 3.7e-8 - 4.7e-8   error / bar 0.040 - 0.072
  sfim       error 1.5e-8 - 3.0e-8   e32 8.5e-8 - 1.0e-7   error / bar 0.019 - 0.041
  gsa        error 1.5e-8 - 3.0e-8   e32 6.4e-8 - 1.2e-7   error / bar 0.023 - 0.057; alpha and g 1.8e-14 - 8.2e-11 relative
  wavelet    error 1.5e-8 - 2.9e-8   e32 1.8e-7 - 2.2e-7   error / bar 0.009 - 0.020
  glp        error 1.5e-8 - 3.0e-8   e32 7.9e-8 - 1.1e-7   error / bar 0.021 - 0.043; a 2.0e-15 - 2.5e-13 relative
  hpm        error 1.5e-8 - 3.0e-8   e32 8.4e-8 - 1.3e-7   error / bar 0.016 - 0.044; a 2.0e-15 - 2.5e-13
  cbd        error 2.6e-8 - 3.0e-8   e32 1.5e-7 - 1.9e-6   error / bar 0.002 - 0.025; a and g 2.2e-15 - 2.0e-12
  bdsd       error 3.0e-8            e32 2.7e-7 - 1.4e-6   error / bar 0.003 - 0.014; gamma 5.0e-12 - 4.3e-11 from lstsq (the two host routes 1.2e-11 - 1.6e-10),
                                                           distance / gate 0.005 - 0.042
  ihs, brovey, gs, pca   error 1.5e-8 - 2.7e-8   e32 4.6e-8 - 9.1e-8   error / bar 0.020 - 0.047; stats 6.9e-16 - 3.1e-15
  indices, the largest |device - host| / max(1, |host|) per column: PSNR 0, SSIM 6.7e-16, Q 2.2e-16, SAM 6.9e-18 (absolute), ERGAS 2.2e-16; D_lambda 6.6e-15,
  D_s 1.2e-14, QNR 1.3e-14; Q2n 1.1e-16, SCC 1.1e-16, CC 4.4e-16; D_lambda_K 0, HQNR 6.3e-15.
The whole file takes 4 s; its slowest case 0.4 s (the first call of the process).

What it sees, checked once with a throw-away build loaded through LGTEUN_HIP_LIB (an in-bounds, arithmetic-only edit; nothing of it is kept): with k_iqa_win's
pair decoder returning (l, r - 1) for l >= 8 -- still a band of the same sample -- test_no_reference_indices[16-32-32] and [16-64-96] fail (D_lambda off by
1.3e-3 and 1.1e-3 against the gate 1e-9) and every other index case here, C <= 8 all of them, passes, as do the no-reference parity tests of
tests/test_gpu_metrics.py and tests/test_gpu_metrics_ext.py (C = 4 and 8): no test before this file reached those pairs."""
import numpy as np
import pytest
import torch

import bdsd_ref as br
import test_band_counts_cpu as bc
import test_gpu_bdsd as tbd
import test_gpu_classical as tcl
import test_gpu_cs as tcs
import test_gpu_metrics as tme
import test_gpu_metrics_ext as tmx
import test_gpu_mtf_glp as tmg
import test_gpu_wavelet as twv
from lgteun_amd import _lib, bdsd, classical, mtf_glp
from lgteun_amd import cs as cs_pkg
from lgteun_amd import device_metrics as dmt
from lgteun_amd import metrics as mtc
from lgteun_amd.engine import _ptr, _stream_ptr
from oracle import detweights as dw

pytestmark = pytest.mark.gpu
T = torch.from_numpy
PEAK = tme.PEAK


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the cached arrays are read-only


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Untouched:
    """with Untouched(ms, pan): ... -- the inputs keep their bits"""

    def __init__(self, *tensors):
        self.tensors, self.before = tensors, [t.clone() for t in tensors]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            assert all(same_bits(t, b) for t, b in zip(self.tensors, self.before)), 'an input was written'
        return False


def last_sample_alone(ms, pan, run):
    """sample B - 1 run alone has the bits of its slice of the batch.  The slice is passed as a copy: a slice of an odd-sized batch is not 16-byte aligned, and
    the contract asks the caller for alignment.  A batch of one sample gets a variant of itself in front.  run(ms, pan) -> a tuple of tensors, batch first"""
    if ms.shape[0] == 1:
        ms, pan = torch.cat([ms.roll(1, dims=3), ms]), torch.cat([pan.flip(2), pan])
    whole = run(ms, pan)
    alone = run(ms[-1:].clone(), pan[-1:].clone())
    for k, (a, w) in enumerate(zip(alone, whole)):
        assert same_bits(a[0], w[-1]), f'tensor {k} of the last sample differs inside the batch'
    return whole


def report(what, err, e32, bar, extra=''):
    print(f'{what}: error {err:.3e}, float32 restatement {e32:.3e}, error / bar {err / bar:.3f}{extra}')


def clip_share(ref):
    share = float(((ref <= 0) | (ref >= 1)).mean())
    assert share <= bc.CLIP_CAP, f'{share:.4f} of the restatement sits on a clip boundary: saturation could hide a wrong value'
    return share


# ---------------------------------------------------------------------------------------------------------------------------------
# the baselines
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', tcl.METHODS)
@pytest.mark.parametrize('C,h,w,B', bc.BAND_SHAPES)
def test_interp23_sfim_gsa(C, h, w, B, method):
    cs = tcl.case(C, h, w, B)
    ref, bar = cs[method]['ref'], cs[method]['bar']
    share = clip_share(ref)
    ms, pan = dev(cs['ms']), dev(cs['pan'])
    with Untouched(ms, pan):
        out, stats = tcl.raw_call(method, ms, pan)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    report(f'{method} C={C} h={h} w={w} B={B}', err, cs[method]['e32'], bar, f', clip share {share:.4f}')
    assert err <= bar, (err, bar)
    if method == 'gsa':
        rel = float(np.abs(stats.cpu().numpy() / cs['stats'] - 1.0).max())
        print(f'gsa C={C} h={h} w={w} B={B}: alpha and g, largest relative difference {rel:.3e}')
        assert rel <= 1e-9, rel
    run = {'interp23': lambda m, p: (classical.interp23(m),), 'sfim': lambda m, p: (classical.sfim(m, p),),
           'gsa': lambda m, p: classical.gsa(m, p, return_stats=True)}[method]
    last_sample_alone(ms, pan, run)
    res = run(ms, pan)                                          # the Python entry is the C ABI's output, bit for bit
    assert same_bits(res[0], out) and (stats is None or same_bits(res[1], stats))


@pytest.mark.parametrize('C,h,w,B', bc.BAND_SHAPES)
def test_wavelet(C, h, w, B):
    cs = twv.case(C, h, w, B)
    ref, bar = cs['ref'], cs['bar']
    share = clip_share(ref)
    ms, pan = dev(cs['ms']), dev(cs['pan'])
    out = twv.raw_call(ms, pan)                                 # (holds the inputs' bits itself)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    report(f'wavelet C={C} h={h} w={w} B={B}', err, cs['e32'], bar, f', clip share {share:.4f}')
    assert err <= bar, (err, bar)
    last_sample_alone(ms, pan, lambda m, p: (classical.wavelet(m, p),))
    assert same_bits(classical.wavelet(ms, pan), out)


@pytest.mark.parametrize('mode', bc.mr.MODES)
@pytest.mark.parametrize('C,h,w,B,per_band', bc.MTF_CASES)
def test_mtf_glp(C, h, w, B, per_band, mode):
    cs = tmg.case(C, h, w, B, per_band, mode)
    ms, pan = (dev(a) for a in tmg.inputs(C, h, w, B))
    gains = tmg.gains_of(C, per_band)
    assert gains == bc.mtf_gains(C, per_band)
    ref, bar = cs['ref'], cs['bar']
    share = clip_share(ref)
    with Untouched(ms, pan):
        out, stats = tmg.raw_call(mode, ms, pan, gains)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    rel = float(np.abs(stats.cpu().numpy() / cs['stats'] - 1.0).max())
    report(f'{mode} C={C} h={h} w={w} B={B} {"per-band" if per_band else "equal"} gains', err, cs['e32'], bar,
           f', clip share {share:.4f}; a and g, largest relative difference {rel:.3e}')
    assert err <= bar, (err, bar)
    assert rel <= 1e-9, rel
    if mode != 'cbd':
        assert bool((stats[:, C:] == 1).all())
    run = lambda m, p: mtf_glp.mtf_glp(m, p, mode, gains, return_stats=True)      # noqa: E731
    last_sample_alone(ms, pan, run)
    o, s = run(ms, pan)
    assert same_bits(o, out) and same_bits(s, stats)


@pytest.mark.parametrize('C,h,w,B,block,per_band', bc.BDSD_CASES)
def test_bdsd(C, h, w, B, block, per_band):
    cs = tbd.case(C, h, w, B, block, per_band)
    ms, pan = (dev(a) for a in tbd.inputs(C, h, w, B))
    gains = tbd.gains_of(C, per_band)
    assert gains == bc.bdsd_gains(C, per_band)
    ref, raw, bar = cs['ref'], cs['raw'], cs['bar']
    outside = float(((raw <= 0) | (raw >= 1)).mean())
    assert outside <= bc.CLIP_CAP, f'{outside:.4f} of the unclipped restatement lies outside (0, 1): saturation could hide a wrong value'
    assert bool((np.abs(cs['gamma']).reshape(B, -1, C * (C + 1)).max(axis=2) > 0).all()), 'a block of the restatement is degenerate'
    with Untouched(ms, pan):
        out, gamma = tbd.raw_call(ms, pan, gains, block)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    dist = max(br.gamma_distance(gamma[b].cpu().numpy(), cs['gamma'][b]) for b in range(B))
    report(f'bdsd C={C} h={h} w={w} B={B} block={block} {"per-band" if per_band else "equal"} gains', err, cs['e32'], bar,
           f', share outside (0, 1) {outside:.4f}; gamma: distance to lstsq {dist:.3e}, the two routes {cs["routes"]:.3e}, gate {cs["gate"]:.3e}, '
           f'distance / gate {dist / cs["gate"]:.3f}')
    assert err <= bar, (err, bar)
    assert dist <= cs['gate'], (dist, cs['gate'])
    run = lambda m, p: bdsd.bdsd(m, p, block, gains, br.GAIN_PAN, return_stats=True)      # noqa: E731
    last_sample_alone(ms, pan, run)
    o, g = run(ms, pan)
    assert same_bits(o, out) and same_bits(g, gamma)


@pytest.mark.parametrize('mode', bc.cs.MODES)
@pytest.mark.parametrize('C,h,w,B', bc.CS_SHAPES)
def test_component_substitution(C, h, w, B, mode):
    cse = tcs.case(C, h, w, B)[mode]
    ms, pan = (dev(a) for a in tcs.inputs(C, h, w, B))
    ref, bar = cse['ref'], cse['bar']
    share = clip_share(ref)
    with Untouched(ms, pan):
        out, stats = tcs.raw_call(mode, ms, pan)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    sd = tcs.stats_distance(stats, cse['stats'])
    report(f'{mode} C={C} h={h} w={w} B={B}', err, cse['e32'], bar, f', clip share {share:.4f}; stats {sd:.3e}')
    assert err <= bar, (err, bar)
    assert sd <= 1e-9, sd
    if mode in ('ihs', 'brovey'):
        assert bool((stats[:, C:2 * C] == 1).all()) and bool((stats[:, :C] == 1.0 / C).all())
    run = lambda m, p: cs_pkg.fuse(m, p, mode, return_stats=True)      # noqa: E731
    last_sample_alone(ms, pan, run)
    o, s = run(ms, pan)
    assert same_bits(o, out) and same_bits(s, stats)


# ---------------------------------------------------------------------------------------------------------------------------------
# the indices
# ---------------------------------------------------------------------------------------------------------------------------------
def index_inputs(C, H, W, B=2):
    """-> pred (the target plus noise: no index is degenerate), pan, ms, gt on the device, normalised"""
    ms, pan, gt = dw.make_inputs(B, C, H // 4, W // 4, seed=H + W + C, kind='smooth')
    return T(tme.fused_like(gt, H + C)).cuda(), T(pan).cuda(), T(ms).cuda(), T(gt).cuda()


def relative(got, want):
    return [abs(g - w) / max(1.0, abs(w)) for g, w in zip(got, want)]


def show(what, names, rows, want):
    worst = np.max([relative(r, w) for r, w in zip(rows, want)], axis=0)
    print(f'{what}: largest |device - host| / max(1, |host|) per column ' + ', '.join(f'{n} {v:.2e}' for n, v in zip(names, worst)))


def guarded_rows(B, k):
    buf = torch.full((B * k + 2 * tmx.GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    return buf, buf[tmx.GUARD:tmx.GUARD + B * k]


def assert_row_guards(buf, what):
    assert bool(torch.isnan(buf[:tmx.GUARD]).all()) and bool(torch.isnan(buf[-tmx.GUARD:]).all()), (what, 'written outside the output')


@pytest.mark.parametrize('H,W', bc.REF_SIZES)
@pytest.mark.parametrize('C', bc.INDEX_BANDS)
def test_reference_based_indices(C, H, W):
    B = 2
    pred, _, _, gt = index_inputs(C, H, W)
    p, g = tme.host_np(pred, PEAK), tme.host_np(gt, PEAK)
    want = [mtc.ref_evaluate(p[i], g[i]) for i in range(B)]
    assert np.all(np.isfinite(want)) and all(0.0 < r[1] < 1.0 and 0.0 < r[2] < 1.0 and r[3] > 0.0 for r in want), want
    got = dmt.ref_evaluate_batch(pred, gt, PEAK)
    assert got.dtype == torch.float64 and got.shape == (B, 5)
    rows = got.cpu().numpy()
    show(f'lg_iqa_ref C={C} {H} x {W}', dmt.REF_NAMES, rows, want)
    for i in range(B):
        tme.assert_close(rows[i], want[i], f'image {i}', sam_col=3)
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 1] < 1.0) and np.all(rows[:, 3] > 0.0)
    for i in range(B):
        assert same_bits(got[i:i + 1], dmt.ref_evaluate_batch(pred[i:i + 1].contiguous(), gt[i:i + 1].contiguous(), PEAK)), i
    L = _lib.lib()
    need = int(L.lg_iqa_workspace_bytes(B, C, H, W, 0))
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device='cuda')
    buf, out = guarded_rows(B, 5)
    _lib.check(L.lg_iqa_ref(_ptr(pred), _ptr(gt), _ptr(out), B, C, H, W, PEAK, _ptr(ws), need, _stream_ptr()), 'lg_iqa_ref')
    assert_row_guards(buf, 'lg_iqa_ref')
    assert same_bits(out.view(B, 5), got)


@pytest.mark.parametrize('H,W', bc.NO_REF_SIZES)
@pytest.mark.parametrize('C', bc.INDEX_BANDS)
def test_no_reference_indices(C, H, W):
    B = 2
    pred, pan, ms, _ = index_inputs(C, H, W)
    p, pn, m = tme.host_np(pred, PEAK), tme.host_np(pan, PEAK), tme.host_np(ms, PEAK)
    want = [mtc.no_ref_evaluate(p[i], pn[i], m[i]) for i in range(B)]
    assert np.all(np.isfinite(want)) and all(0.0 < v < 1.0 for r in want for v in r), want
    got = dmt.no_ref_evaluate_batch(pred, pan, ms, PEAK)
    assert got.dtype == torch.float64 and got.shape == (B, 3)
    rows = got.cpu().numpy()
    show(f'lg_iqa_no_ref C={C} {H} x {W}', dmt.NO_REF_NAMES, rows, want)
    for i in range(B):
        tme.assert_close(rows[i], want[i], f'image {i}')        # D_s and QNR at 1e-9 too, as tests/test_gpu_metrics.py holds them
    for i in range(B):
        alone = dmt.no_ref_evaluate_batch(pred[i:i + 1].contiguous(), pan[i:i + 1].contiguous(), ms[i:i + 1].contiguous(), PEAK)
        assert same_bits(got[i:i + 1], alone), i
    L = _lib.lib()
    need = int(L.lg_iqa_workspace_bytes(B, C, H, W, 1))
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device='cuda')
    buf, out = guarded_rows(B, 3)
    _lib.check(L.lg_iqa_no_ref(_ptr(pred), _ptr(pan), _ptr(ms), _ptr(out), B, C, H, W, PEAK, _ptr(ws), need, _stream_ptr()), 'lg_iqa_no_ref')
    assert_row_guards(buf, 'lg_iqa_no_ref')
    assert same_bits(out.view(B, 3), got)


@pytest.mark.parametrize('H,W', bc.Q2N_SIZES)
@pytest.mark.parametrize('C', bc.Q2N_BANDS)
def test_q2n_scc_cc_with_padded_bands(C, H, W):
    B = 2
    pred, _, _, gt = index_inputs(C, H, W)
    want = tmx.host_ext(pred, gt, PEAK)
    assert np.all(np.isfinite(want)) and all(0.0 < v < 1.0 for r in want for v in r), want
    got = dmt.ref_evaluate_ext_batch(pred, gt, PEAK)
    assert got.dtype == torch.float64 and got.shape == (B, 8)
    assert same_bits(got[:, :5], dmt.ref_evaluate_batch(pred, gt, PEAK))
    rows = got.cpu().numpy()
    show(f'lg_iqa_ref_ext C={C} {H} x {W}', dmt.REF_EXT_NAMES[5:], rows[:, 5:], want)
    for i in range(B):
        tmx.assert_close(rows[i, 5:], want[i], f'image {i}')
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 5:] < 1.0) and np.all(rows[:, 5:] > 0.0)
    for i in range(B):
        assert same_bits(got[i:i + 1], dmt.ref_evaluate_ext_batch(pred[i:i + 1].contiguous(), gt[i:i + 1].contiguous(), PEAK)), i
    need = int(_lib.lib().lg_iqa_ext_workspace_bytes(B, C, H, W))
    assert need > 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device='cuda')
    buf, out = guarded_rows(B, 3)
    assert tmx.raw_ref_ext(pred, gt, PEAK, out, ws, need) == 0
    assert_row_guards(buf, 'lg_iqa_ref_ext')
    assert same_bits(out.view(B, 3), got[:, 5:])


@pytest.mark.parametrize('H,W', bc.EXT_NO_REF_SIZES)
@pytest.mark.parametrize('C', bc.EXT_NO_REF_BANDS)
def test_d_lambda_k_and_hqnr(C, H, W):
    B = 2
    pred, pan, ms, _ = index_inputs(C, H, W)
    p, pn, m = tme.host_np(pred, PEAK), tme.host_np(pan, PEAK), tme.host_np(ms, PEAK)
    want = []
    for i in range(B):
        dk = mtc.d_lambda_k(p[i], m[i], None)
        want.append([dk, (1.0 - dk) * (1.0 - mtc.d_s(p[i], m[i], pn[i]))])
        assert 0.0 < dk < 1.0 and 0.0 < want[-1][1] < 1.0, want
    got = dmt.no_ref_evaluate_ext_batch(pred, pan, ms, PEAK)
    assert got.dtype == torch.float64 and got.shape == (B, 5)
    assert same_bits(got[:, :3], dmt.no_ref_evaluate_batch(pred, pan, ms, PEAK))
    rows = got.cpu().numpy()
    show(f'no_ref_evaluate_ext C={C} {H} x {W}', dmt.NO_REF_EXT_NAMES[3:], rows[:, 3:], want)
    for i in range(B):
        tmx.assert_close(rows[i, 3:], want[i], f'image {i}')
    for i in range(B):
        alone = dmt.no_ref_evaluate_ext_batch(pred[i:i + 1].contiguous(), pan[i:i + 1].contiguous(), ms[i:i + 1].contiguous(), PEAK)
        assert same_bits(got[i:i + 1], alone), i
