"""-m gpu: the FFT (global) mixer alone, element by element, on every path of k_fft.hip.

What a C = 4 / 8 plan routes the global mixer to -- the real-input in-LDS kernels k_fftmix_r<3..7> / k_fftmix_bwd_r (two thread-count instances at
128 x 128), the complex-row kernels k_fftmix<3..7> / k_fftmix_bwd (LG_FFT=full), the three-launch split path (256 x 256, 512 x 512), the three-launch
Bluestein path (every rectangle, every side that is no power of two, up to 1024) and fft_bwd_reduce's sum of the partial rows -- through
lg_op_block / lg_op_block_bwd with which = 0, against the fp64 oracle (torch autograd over oracle.global_mixer on LayerNorm(feat)) with the
deterministic weights.  The per-op shape files hold this op constant (their docstrings: angle()'s branch cut and the division by bin amplitudes
make the fp32 reference itself noisy on random features); the other gates on it are relative L2 at 2e-4 / 2e-3.  Both troubles are properties
of the INPUT: helpers.fft_designed_features draws the spectrum itself, tests/test_fft_design_cpu.py proves for every case here that no bin with
Re F < 0 is within 0.05 ||plane|| of the cut, no amplitude below 0.05 ||plane||, at most 1e-3 of the pixels on the kink of abs() (dy is exactly 0
there: helpers.fft_kink_mask) and that the fp32 oracle is within 2e-6 of fp64 -- so the fp32 oracle is a yardstick.  Each case:

  * PRECONDITIONS FIRST (helpers.fft_assert_preconditions), ahead of any launch; then ROUTE: `fft=k_fftmix_r` (or `fft=k_fftmix` under
    LG_FFT=full) from the net line of lg_plan_describe, and from the fwd line of the block's level the path the plan resolved for that plane
    (route.hip: resolve_fft): `fft=k_fftmix_r`, `k_fftmix`, `split` or `bluestein`, asserted against the case's family.  The path follows from the
    plane's size alone; _expected_family restates that rule on its own and is asserted against the case's family as well, with the Bluestein
    length M = next power of two >= 2n - 1 deciding 'blue' (M <= 512) / 'blue1k' (M >= 1024);
  * FORWARD in a NaN-filled buffer with 1024 floats of band on each side: no NaN left, both bands intact; relative L2 at the existing 2e-4;
    element by element, max |got - fp64| over the plane's fp64 RMS, maximised over planes, at most BAR_FWD x the same figure of the fp32 oracle.
    The edited spectrum's phases are nearly coherent (conv_pha's weights are small): the output has a peak of 6 .. 450 x RMS around pixel (0, 0),
    and 2^-24 of that peak is what this figure measures on either side (fp32 oracle 9e-7 .. 5e-5).  So a second figure beside it: each element on
    its own size, max |got - fp64| / (|fp64| + RMS), at most BAR_LOC x the fp32 oracle's (variant (a) below: red in 14 of 16 cases where the first
    is red in 2);
  * BACKWARD: dy standard normal, 0 on the kink mask; dx in the guarded buffer, relative L2 at the existing 2e-3, element by element on the RMS of
    dx64 at BAR_BWD; the gradient buffer with owned = the four global_mixer tensors (every other float a sentinel that must keep its bits); one
    line per tensor, err = max |got - g64| / max |g64| <= max(BAR_BWD x err32, G);
  * BATCH INDEPENDENCE: the last sample alone on a fresh plan, bitwise.  The 272-plane case runs k_fftmix_r<7, 512> and its last sample alone
    k_fftmix_r<7, 1024>: both are held to the bar and to each other within the bar (measured: the two instances agree bitwise);
  * SAVING FORWARD: lg_op_block_bwd runs the FFT forward with its amp / pha / sgn stores (LG_FLAG_SAVE) into workspace slots whose offsets the C ABI
    does not export (lg_workspace_deadout is the only one it does): an FFT-only bitwise comparison of the saving forward's o2 with the plain one
    needs a new entry point and is NOT here.  What the saving forward stores is what dx and the four gradients above are computed from;
    test_gpu_forward_shapes.py compares lg_op_lgt with LG_FLAG_SAVE bitwise at (3,80,48).

Measured on an MI355X (ratio = the figure over the fp32 oracle's; every test prints its rows and one line per gradient tensor):
  family                                        cases  direction  rel-L2               element-wise         fp32 oracle          ratio          bar
  in-LDS k_fftmix_r<3..7>, both 128^2 instances    11  forward    1.5e-07 .. 2.2e-07   8.3e-07 .. 4.3e-05   9.3e-07 .. 1.8e-05   0.81 ..  2.53    8
                                                       own size                        4.8e-07 .. 6.3e-06   4.2e-07 .. 7.0e-06   0.59 ..  2.54    8
                                                       dx         1.6e-07 .. 2.6e-07   6.2e-07 .. 1.6e-06   5.3e-07 .. 1.3e-06   0.84 ..  1.35    4
  LG_FFT=full k_fftmix<3|5|7>                       3  forward    1.5e-07 .. 2.0e-07   8.3e-07 .. 4.3e-05   1.0e-06 .. 1.7e-05   0.81 ..  2.53    8
                                                       own size                        5.3e-07 .. 2.7e-06   4.2e-07 .. 3.5e-06   0.48 ..  1.27    4
                                                       dx         1.6e-07 .. 2.5e-07   5.9e-07 .. 1.4e-06   7.3e-07 .. 1.3e-06   0.80 ..  1.13    4
  split 256^2 / 512^2                               3  forward    2.1e-07 .. 2.2e-07   4.9e-05 .. 7.2e-05   1.5e-05 .. 5.2e-05   1.38 ..  4.32   16
                                                       own size                        5.7e-06 .. 1.0e-05   4.1e-06 .. 2.1e-05   0.50 ..  2.23    8
                                                       dx         2.6e-07 .. 2.7e-07   1.4e-06 .. 1.6e-06   1.4e-06 .. 1.4e-06   1.01 ..  1.12    4
  Bluestein, M <= 512                              10  forward    3.7e-07 .. 5.2e-07   3.0e-06 .. 1.2e-04   8.4e-07 .. 1.8e-05   1.69 ..  6.25   16
                                                       own size                        8.4e-07 .. 5.2e-06   4.4e-07 .. 4.8e-06   1.05 ..  2.68    8
                                                       dx         3.9e-07 .. 6.1e-07   1.7e-06 .. 3.0e-06   7.1e-07 .. 1.3e-06   2.08 ..  2.66    8
  Bluestein, M >= 1024                              6  forward    4.3e-07 .. 5.2e-07   2.1e-05 .. 2.1e-04   5.9e-06 .. 4.6e-05   2.92 .. 11.35   32
                                                       own size                        4.6e-06 .. 2.0e-05   1.6e-06 .. 8.7e-06   1.07 ..  2.95    8
                                                       dx         4.7e-07 .. 6.3e-07   2.3e-06 .. 3.2e-06   9.2e-07 .. 1.4e-06   2.18 ..  2.69    8
  Each bar: twice the family's largest ratio, rounded up to a power of two, at least 4, never above 64.  No family measures above 32.  The largest,
  11.35, is the forward of (1,1024,32) on the peak: a length-1024 column goes through three radix-2 transforms of length 2048 and four chirp products
  where pocketfft runs five radix-4 passes of length 1024, and at the peak every one of those roundings is on the scale of 160 x RMS; each element
  on its own size the same case is at 2.9.
  parameter gradients (132 lines), worst err = max |got - g64| / max |g64| per family | largest multiple of the fp32 oracle's:
    in-LDS 6.3e-07 | 3.5 x   full 4.5e-07 | 1.9 x   split 5.2e-07 | 1.9 x   Bluestein M <= 512 1.2e-06 | 7.6 x   Bluestein M >= 1024 8.2e-07 | 5.2 x
  G = 4 x the worst of the file (1.21e-06: conv_amp.0.weight at C=4 blk=0 (1,208,176)) = 4.9e-6, against 4.2e-4 in test_gpu_backward_shapes.py
  (whose random features have amplitude floors of 7e-4 .. 1e-2 where these have 0.08 .. 0.36).
  The file: 33 tests in 7.9 s on the MI355X machine, the slowest 1.2 s (the first, which loads the library) and 0.7 s ((16,128,128) and (17,128,128)
  at C = 8: fp64 + fp32 autograd over 256 / 272 planes).

What it sees, checked once with three variant builds loaded through LGTEUN_HIP_LIB (arithmetic-only edits inside the buffers; nothing of them is kept):
  (a) gdft_setup: entry k = 3 of the chirp table wch turned by 1e-5 rad.  RED: all 16 Bluestein cases -- dx element-wise at 26 .. 68 x the fp32
      oracle's (bar 8) in every one, 34 of the 64 gradient lines (up to 1.5e-5; G 4.9e-6; 60 of them above 8 x the fp32 oracle's); forward, each element on
      its own size, at 10 .. 80 x (bar 8) in 14 of them ((1,208,176) blk 0 at 5.2 and (1,400,400) at 3.1 stay under it), forward on the RMS at
      22 / 54 x (bar 16) in the two 8 x 24 / 24 x 8 cases only (4.2 .. 21 elsewhere, under the bars of 16 / 32).  The relative-L2 gates notice NOTHING: forward 1.5e-6 .. 7.4e-6
      (gate 2e-4), dx 2.0e-6 .. 9.7e-6 (gate 2e-3).  GREEN: the 17 in-LDS, full and split cases.
  (b) k_fft_cols: a column group that holds one column is not stored back (kx = n/2 keeps the row transform's unedited value).  RED: (1,256,256),
      (2,256,256) and (1,512,512) (129 = 4 x 32 + 1 and 257 = 16 x 16 + 1 columns): forward 0.87 .. 0.89 of the plane's RMS (ratio 1.7e4 .. 5.8e4),
      rel-L2 3.7e-2 .. 5.3e-2; dx 4.8 .. 5.4 x RMS, rel-L2 0.24 .. 0.29.  GREEN: the other 30 (in-LDS, full, Bluestein).
  (c) fft_bwd_reduce with nslices one short.  RED: all 33 cases, on the gradient lines only (err 5.3e-3 .. 1.35; a case of B = 1 with one column
      group sums no slice at all: err 1.0).  dx GREEN in all 33, bit for bit the product build's rows; forward untouched.
"""
import pytest
import torch

from helpers import FFT_CASES, FFT_FULL_CASES, fft_assert_preconditions, fft_grad_err, fft_local_err, fft_mixer_refs, fft_plane, fft_plane_err, rel_l2
from oracle import lgteun_oracle as orc

pytestmark = pytest.mark.gpu

# element by element: at most this many times the fp32 oracle's own error (per family and direction: docstring)
BAR_FWD = {'lds': 8.0, 'full': 8.0, 'split': 16.0, 'blue': 16.0, 'blue1k': 32.0}
BAR_LOC = {'lds': 8.0, 'full': 4.0, 'split': 8.0, 'blue': 8.0, 'blue1k': 8.0}     # forward, each element on its own size
BAR_BWD = {'lds': 4.0, 'full': 4.0, 'split': 4.0, 'blue': 8.0, 'blue1k': 8.0}
G = 4.9e-6                  # the four parameter gradients: err <= max(BAR_BWD x the fp32 oracle's err, G)
L2_FWD, L2_BWD = 2e-4, 2e-3     # the existing relative-L2 gates of test_gpu_anysize.py / test_gpu_backward.py
NUM_CUS = 256               # k_fft.hip lg_num_cus(): more 128 x 128 planes than this run k_fftmix_r<7, 512>


@pytest.fixture(autouse=True)
def canonical_real_bins(monkeypatch):
    """as in the shape files: pin the +0 convention of the four purely-real bins (oracle/lgteun_oracle.py)"""
    monkeypatch.setattr(orc, 'CANONICAL_REAL_BINS', True)


def _bluestein_m(n):
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def _expected_family(h, w):
    """the size rule of the plan's FFT route (route.hip: resolve_fft), restated on its own: lg_plan_describe's per-level fft= token is held against it"""
    if h == w and h & (h - 1) == 0 and 8 <= h <= 512:
        return 'split' if h > 128 else 'lds'
    return 'blue1k' if max(_bluestein_m(h), _bluestein_m(w)) >= 1024 else 'blue'


FFT_TOKEN = {'lds': 'k_fftmix_r', 'full': 'k_fftmix', 'split': 'split', 'blue': 'bluestein', 'blue1k': 'bluestein'}


def _assert_route(ops, family, blk, H, W):
    """route first: the switch on the net line of lg_plan_describe, the path on the fwd line of the block's level, and the size rule restated"""
    lines = ops.eng.describe(H, W).splitlines()
    want = 'fft=k_fftmix' if family == 'full' else 'fft=k_fftmix_r'
    assert want in lines[0].split(': ')[1].split(), (want, lines[0])
    h, w = fft_plane(blk, H, W)
    fwd = [ln for ln in lines if ln.startswith(f'L{1 if blk == 2 else 0} ') and ' fwd: ' in ln]   # (block 2 is the bottleneck: level 1)
    assert len(fwd) == 1 and fwd[0].split(' | ')[-1] == 'fft=' + FFT_TOKEN[family], (family, blk, H, W, fwd)
    assert _expected_family(h, w) == ('lds' if family == 'full' else family), (family, blk, H, W)


def _elementwise(tag, what, got, ref64, ref32, gate, bar, bad):
    """no NaN left, relative L2, the element-wise bar; prints the measured row"""
    n_nan = int(torch.isnan(got).sum())
    assert n_nan == 0, (tag, what, 'elements never written', n_nan)
    rel, e_got, e_32 = rel_l2(got, ref64), fft_plane_err(got, ref64), fft_plane_err(ref32, ref64)
    print(f'{tag}: {what} rel-L2 {rel:.2e}  element-wise {e_got:.2e}  fp32 oracle {e_32:.2e}  ratio {e_got / e_32:.2f}  (bar {bar:g})')
    if not rel < gate:
        bad.append((what, 'rel-L2', rel, gate))
    if not e_got <= bar * e_32:
        d = (got.double() - ref64).abs()
        worst = [tuple(int(v) for v in torch.unravel_index(i, d.shape)) for i in torch.topk(d.flatten(), 4).indices]
        bad.append((what, 'element-wise', e_got, e_32, e_got / e_32, 'worst elements', worst))


def _check(family, C, blk, B, H, W, monkeypatch):
    from gpu_helpers import make_ops
    tag = f'fft mixer {family} C={C} blk={blk} ({B},{H},{W})'
    ref = fft_mixer_refs(C, blk, B, H, W)
    fft_assert_preconditions(tag, ref['pre'])            # ahead of any launch
    if family == 'full':
        monkeypatch.setenv('LG_FFT', 'full')             # read once per plan: a fresh module builds a fresh plan
    else:
        monkeypatch.delenv('LG_FFT', raising=False)
    ops = make_ops(C, H, W)
    _assert_route(ops, family, blk, H, W)
    feat, dy, names = ref['feat'].cuda(), ref['dy'].cuda(), ref['names']
    bad = []
    # forward: a view into the NaN buffer (gpu_helpers asserts both bands)
    y = ops.block(0, blk, 0, feat, guard=True).cpu()
    _elementwise(tag, 'forward', y, ref['y64'], ref['y32'], L2_FWD, BAR_FWD[family], bad)
    l_got, l_32 = fft_local_err(y, ref['y64']), fft_local_err(ref['y32'], ref['y64'])
    print(f'{tag}: forward, each element on its own size: {l_got:.2e}  fp32 oracle {l_32:.2e}  ratio {l_got / l_32:.2f}  (bar {BAR_LOC[family]:g})')
    if not l_got <= BAR_LOC[family] * l_32:
        bad.append(('forward', 'each element on its own size', l_got, l_32, l_got / l_32))
    # backward: dx in the NaN buffer, the gradient buffer with every float that is not one of the four tensors' a sentinel
    assert float(ref['dy'][ref['mask']].abs().sum()) == 0.0
    dx, flat = ops.block_bwd(0, blk, 0, feat, dy, guard=True, owned=names)
    _elementwise(tag, 'dx', dx.cpu(), ref['dx64'], ref['dx32'], L2_BWD, BAR_BWD[family], bad)
    for n in names:
        err, err32 = fft_grad_err(ops.grad_of(flat, n).cpu(), ref['g64'][n]), fft_grad_err(ref['g32'][n], ref['g64'][n])
        print(f'    {tag} | {n.split("global_mixer.")[1]}: err {err:.2e}  fp32 oracle {err32:.2e}  G {G:.1e}')
        if not err <= max(BAR_BWD[family] * err32, G):
            bad.append((n, err, err32, G))
    # batch independence: the last sample alone, on a fresh plan
    if B > 1:
        y1 = make_ops(C, H, W).block(0, blk, 0, feat[-1:].contiguous(), guard=True).cpu()
        h, w = fft_plane(blk, H, W)
        if h == 128 and B * y.shape[1] > NUM_CUS >= y.shape[1]:
            # the batch ran k_fftmix_r<7, 512>, the sample alone runs k_fftmix_r<7, 1024>: two evaluations, each held to the bar, and to each other
            e32 = fft_plane_err(ref['y32'][-1:], ref['y64'][-1:])
            e1, e12 = fft_plane_err(y1, ref['y64'][-1:]), fft_plane_err(y1, y[-1:].double())
            print(f'{tag}: alone (1024 threads) element-wise {e1:.2e}  against the batch (512 threads) {e12:.2e}  fp32 oracle {e32:.2e}')
            if not (e1 <= BAR_FWD[family] * e32 and e12 <= BAR_FWD[family] * e32):
                bad.append(('alone / against the batch', e1, e12, e32))
        elif not torch.equal(y1.view(torch.int32), y[-1:].view(torch.int32)):
            bad.append(('the last sample alone differs from the same sample in the batch', fft_plane_err(y1, y[-1:].double())))
    assert not bad, (tag, bad)


@pytest.mark.parametrize('family,C,blk,B,H,W', FFT_CASES)
def test_fft_mixer_element_by_element(family, C, blk, B, H, W, monkeypatch):
    """k_fftmix_r<3..7> and both thread-count instances at 128 x 128, the split path, the Bluestein path: forward, dx and the four gradients against
    the fp64 oracle on the fp32 oracle's yardstick; the last sample alone bitwise"""
    _check(family, C, blk, B, H, W, monkeypatch)


@pytest.mark.parametrize('C,blk,B,H,W', FFT_FULL_CASES)
def test_complex_row_kernels_element_by_element(C, blk, B, H, W, monkeypatch):
    """LG_FFT=full: k_fftmix<3|5|7> / k_fftmix_bwd<3|5|7> against the oracle themselves (test_gpu_ops_bwd.py holds them against k_fftmix_r only)"""
    _check('full', C, blk, B, H, W, monkeypatch)
