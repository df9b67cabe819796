"""-m gpu: the inference forward kernels one op at a time, at the shapes where their launch geometry changes, element by element.

What lg_op_block / lg_op_lgt / lg_op_data_step / lg_op_resample launch with nothing saved -- k_ffn_xr<0,2>, k_ffn_x32<0,2>, k_ffn1_x64 +
k_ffn2_x64, k_attn_m<.,2>, the data step's tile kernels and its one-launch form, k_embed / k_down / k_upfuse / k_tail, k_resample -- against
the fp64 oracle with the deterministic weights.  The backward tests launch the SAVING template instances and never read the forward's
output; the whole-net tests gate a global relative L2 of 1e-3, under which a wrong border row, a ragged last strip, one wrong window in a
few thousand or a pixel that was never written all disappear.  Here:

  * every output is a view into a NaN-filled buffer with 1024 floats of band on each side (gpu_helpers guard=True): no NaN left in the
    output = every pixel written; both bands still NaN = nothing written next to it;
  * relative L2 at the project's per-op gates (FFN 5e-6, mixer 1e-4, data step / resample 2e-6, LGT 1e-4);
  * ELEMENT BY ELEMENT: max |got - fp64| over max |fp64 - x| (half-blocks: the residual branch's largest entry) or max |fp64| (data step,
    resample) is at most 8 x the same figure of the oracle's own fp32 run on the same inputs.  The split arithmetic is built to be as accurate
    per dot product as an fp32 chain (1.3 - 1.5 x in L2, test_matrix_pipe_mixer_is_as_close_to_fp64_as_the_fp32_kernel); a maximum over up to
    1e7 elements fluctuates more than a norm, hence 8.  One wrong tap of the depthwise conv, one stale pixel or one wrong window is >= 1e-2 of
    the residual: four orders of magnitude above the fp32 yardstick of 3e-7 .. 6e-7;
  * the mixer half-block takes angle()'s branch cut out as test_matrix_pipe_mixer... does: the fp64 restatement is
    x + proj(cat(local_mixer(LN(x)[..., :e/2]), o2)) with o2 THIS build's global-mixer output (which = 0) on the same x; the 1e-4 gate
    against the whole fp64 mixer stays beside it;
  * batch independence, bitwise: the last sample run alone (B = 1, a fresh plan) equals its slice of the batch output;
  * precondition of every case: the oracle's fp32 run is within 1e-6 of its fp64 run (otherwise the INPUT drew a branch-cut flip in the
    reference's own arithmetic: change the seed, never the gate).

Shapes (PAN sizes; level 1 is half of it) are the smallest that reach each edge of the launchers: one strip only; level-1 planes 8 x 8,
8 x 24, 40 x 24 and 24 x 104 (half-empty 16-wide tiles, strips that end inside an 8-row step); 576 strips on a grid of 512 / 256 (workgroups
walk two or three strips); strip height 24 over 80 rows (24, 24, 24, 8) with 516 strips on 512 slots; one window in a quad, ragged last
quads (9 and 45 windows), 576 quads in two rounds, 528 quads at level 1; data-step tiles on planes that are no multiple of 32, the 4 x 4 MS
plane, the one-launch form at an odd batch; a bicubic support wider than the plane.

Measured on an MI355X (ratio = element-wise error over the fp32 oracle's; the test prints every row):
  op                                                       cases   rel-L2                 element-wise           fp32 oracle            ratio
  FFN half-block e = 16 (k_ffn_xr: C=4 blk 0)                  6   3.6e-08 .. 3.8e-08   5.2e-07 .. 8.3e-07   3.8e-07 .. 6.7e-07   1.00 .. 1.39
  FFN half-block e = 32 (k_ffn_x32: C=4 blk 2, C=8 blk 0)     10   3.7e-08 .. 4.4e-08   4.4e-07 .. 7.7e-07   3.5e-07 .. 5.8e-07   0.96 .. 1.42
  FFN half-block e = 64 (k_ffn1_x64 + k_ffn2_x64: C=8 blk 2)   5   4.8e-08 .. 5.2e-08   6.6e-07 .. 9.7e-07   5.1e-07 .. 5.7e-07   1.18 .. 1.70
  FFN half-block, blocks 1 / 3 / 4 at (3,48,32)                6   3.3e-08 .. 4.6e-08   5.8e-07 .. 7.6e-07   4.3e-07 .. 6.4e-07   1.00 .. 1.36
  mixer half-block, level 0 (blk 0)                            8   4.2e-08 .. 5.1e-08   1.0e-07 .. 3.1e-07   9.3e-08 .. 2.7e-07   0.70 .. 2.14
  mixer half-block, level 1 (blk 2)                           10   4.3e-08 .. 6.1e-08   1.6e-07 .. 5.7e-07   1.1e-07 .. 3.0e-07   1.08 .. 2.61
  mixer half-block, blocks 1 / 3 / 4 at (3,48,32)              6   3.9e-08 .. 4.9e-08   1.4e-07 .. 3.0e-07   6.5e-08 .. 1.7e-07   1.12 .. 3.11
  data step                                                    6   3.0e-08 .. 3.4e-08   5.6e-08 .. 8.3e-08   6.0e-08 .. 1.1e-07   0.79 .. 0.96
  resample x0.5 / x2 / x4                                     12   4.5e-08 .. 7.0e-08   6.4e-08 .. 2.0e-07   8.0e-08 .. 1.7e-07   0.41 .. 1.28
  LG_FFN_IMPL=strip (fp32 MFMAs)                               8   3.0e-08 .. 3.6e-08   3.7e-07 .. 6.1e-07   3.5e-07 .. 5.6e-07   0.82 .. 1.24
  LG_FFN_FWD=xs                                                2   3.6e-08 .. 3.7e-08   5.6e-07 .. 6.1e-07   3.8e-07 .. 5.6e-07   1.08 .. 1.50
  LG_ATTN_FWD=valu (fp32 FMAs; one: stage 1 of K = 2, blk 4)    9   3.3e-08 .. 4.3e-08   6.2e-08 .. 2.0e-07   9.3e-08 .. 2.0e-07   0.67 .. 1.00
  largest ratio of all 88 rows: 3.11 (mixer C=8 blk=1 (3,48,32)); the bar is 8
  one LGT (6 cases): rel-L2 1.0e-07 .. 1.3e-07, max-norm 1.8e-07 .. 5.6e-07 of max |fp64| (gates 1e-4); saving forward bitwise the plain one, 4 cases
  precision='bf16' (12 cases): rel-L2 1.8e-04 .. 5.7e-04 of the fp64 output (gate 5e-3); the e = 64 FFN runs the default kernels in this mode: 6.6e-8

What it sees, checked once with variant builds of k_ffn_xr loaded through LGTEUN_HIP_LIB (nothing of them is kept): with the halo row below
every strip left out of the depthwise conv, the e = 16 FFN cases with more than one strip per plane -- (3,80,48), (2,48,208), (9,128,128),
(43,80,48) -- go to 0.21 .. 0.27 of the residual (ratio 3.4e5 .. 4.3e5, rel-L2 4.6e-3 .. 5.6e-3) while (1,16,16) and (3,16,48), one strip per
plane, stay green; with ONE pixel of that row left out under the first strip only, the same four cases are at 6e-2 .. 7.6e-2 (ratio 1e5,
rel-L2 5.7e-5 .. 1.9e-4).  The whole-net test at 80 x 48 (gate 1e-3) notices both as well, at 3.9e-3 and 1.5e-3: the global mixers behind
the FFN spread one wrong pixel over the plane -- it is less blind than a global gate suggests, but it does not say where, and no
whole-net test runs the batches at which workgroups walk several strips or quads.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import DSTEP_CASES, LGT_CASES, block_features as _features, block_prefix as _pre, det_params, ffn_half_block as _ffn, lgt_input as _lgt_input
from helpers import mixer_half_block as _mixer, mixer_restated as _mixer_restated, rel_l2
from oracle import lgteun_oracle as orc

pytestmark = pytest.mark.gpu

T = torch.from_numpy
BAR = 8.0                   # element-wise error: at most this many times the fp32 oracle's own


@pytest.fixture(autouse=True)
def canonical_real_bins(monkeypatch):
    """non-power-of-two sizes: the sign of the zero imaginary part torch's FFT leaves in the four purely-real bins -- hence
    angle() = +pi or -pi where they are negative -- depends on the host CPU (oracle/lgteun_oracle.py); pin the +0 convention"""
    monkeypatch.setattr(orc, 'CANONICAL_REAL_BINS', True)


@functools.lru_cache(maxsize=None)
def _params(C, K, dtype, stage=0):
    """stage > 0: the weights of that stage's LGT under stage 0's names, which is where the helpers' block prefixes look"""
    P = det_params(C, K, dtype=dtype)
    if stage == 0:
        return P
    src = f'prior_module.{stage}.'
    return {k.replace(src, 'prior_module.0.'): v for k, v in P.items() if k.startswith(src)}


def _local(P, blk, x):
    p = _pre(blk)
    y = orc.layer_norm(x, P[p + '0.fn.norm.weight'], P[p + '0.fn.norm.bias'])
    return orc.local_mixer(P, p + '0.fn.fn.local_mixer.', y[..., :x.shape[-1] // 2])


@functools.lru_cache(maxsize=None)
def _ffn_refs(C, blk, B, H, W):
    """(x, fp64 oracle, fp32 oracle) of the FFN half-block: computed once, shared by the tests of that case, never written to"""
    x = _features(C, blk, B, H, W)
    with torch.no_grad():
        return x, _ffn(_params(C, 1, torch.float64), blk, x.double()), _ffn(_params(C, 1, torch.float32), blk, x).double()


@functools.lru_cache(maxsize=None)
def _mixer_refs(C, blk, B, H, W, K=1, stage=0):
    """(x, whole fp64 mixer, whole fp32 mixer, fp64 local mixer, fp32 local mixer)"""
    x = _features(C, blk, B, H, W)
    with torch.no_grad():
        P64, P32 = _params(C, K, torch.float64, stage), _params(C, K, torch.float32, stage)
        return x, _mixer(P64, blk, x.double()), _mixer(P32, blk, x).double(), _local(P64, blk, x.double()), _local(P32, blk, x)


def _ops(C, H, W, K=1, precision=None):
    from gpu_helpers import make_ops
    return make_ops(C, H, W, K, precision)


def _max_err(a, b, den):
    return float((a - b).abs().max()) / den


def _elementwise(tag, got, want64, want32, den, l2_gate):
    """precondition, relative L2 and the element-wise bar of one case; prints the measured row"""
    assert not torch.isnan(got).any(), (tag, 'pixels never written', int(torch.isnan(got).sum()))
    pre = rel_l2(want32, want64)
    rel = rel_l2(got, want64)
    e_got, e_32 = _max_err(got, want64, den), _max_err(want32, want64, den)
    print(f'{tag}: rel-L2 {rel:.2e}  element-wise {e_got:.2e}  fp32 oracle {e_32:.2e} (rel-L2 {pre:.1e})  ratio {e_got / e_32:.2f}')
    assert pre < 1e-6, (tag, 'the fp32 oracle is not clean on this input: change the seed', pre)
    assert rel < l2_gate, (tag, rel)
    if e_got > BAR * e_32:
        d = (got - want64).abs()
        worst = [tuple(int(v) for v in np.unravel_index(int(i), tuple(d.shape))) for i in torch.topk(d.flatten(), 8).indices]
        assert False, (tag, e_got, e_32, e_got / e_32, 'worst elements', worst)


def _check_ffn(tag, ops_of, C, blk, B, H, W, l2_gate=5e-6):
    x, want64, want32 = _ffn_refs(C, blk, B, H, W)
    got = ops_of(H, W).block(0, blk, 2, x.cuda(), guard=True).cpu()
    _elementwise(tag, got.double(), want64, want32, float((want64 - x.double()).abs().max()), l2_gate)
    if B > 1:
        alone = ops_of(H, W).block(0, blk, 2, x[-1:].cuda(), guard=True).cpu()
        assert torch.equal(alone, got[-1:]), (tag, 'batch independence', float((alone - got[-1:]).abs().max()))


def _check_mixer(tag, ops_of, C, blk, B, H, W, K=1, stage=0):
    """ops_of builds the Ops of a K-stage net; the block is `blk` of its stage `stage`"""
    x, want64, want32, x1_64, x1_32 = _mixer_refs(C, blk, B, H, W, K, stage)
    ops = ops_of(H, W)
    got = ops.block(stage, blk, 1, x.cuda(), guard=True).cpu()
    o2 = ops.block(stage, blk, 0, x.cuda(), guard=True).cpu()
    assert not torch.isnan(got).any() and not torch.isnan(o2).any(), tag
    pre, whole = rel_l2(want32, want64), rel_l2(got, want64)
    assert pre < 1e-6, (tag, 'the fp32 oracle of the whole mixer is not clean on this input: change the seed', pre)
    assert whole < 1e-4, (tag, whole)
    with torch.no_grad():
        r64 = _mixer_restated(_params(C, K, torch.float64, stage), blk, x.double(), x1_64, o2.double())
        r32 = _mixer_restated(_params(C, K, torch.float32, stage), blk, x, x1_32, o2).double()
    _elementwise(f'{tag} (whole fp64 mixer {whole:.1e})', got.double(), r64, r32, float((r64 - x.double()).abs().max()), 1e-4)
    if B > 1:
        alone = ops_of(H, W).block(stage, blk, 1, x[-1:].cuda(), guard=True).cpu()
        assert torch.equal(alone, got[-1:]), (tag, 'batch independence', float((alone - got[-1:]).abs().max()))


def _default(C, K=1):
    return lambda H, W: _ops(C, H, W, K)


# ---- 1. FFN half-block: k_ffn_xr<0,2> (e = 16), k_ffn_x32<0,2> (e = 32), k_ffn1_x64 + k_ffn2_x64 (e = 64)
FFN_SHAPES = [(1, 16, 16), (3, 16, 48), (3, 80, 48), (2, 48, 208), (9, 128, 128)]
FFN_CASES = [(C, blk) + s for C in (4, 8) for blk in (0, 2) for s in FFN_SHAPES] + [(4, 0, 43, 80, 48)]


@pytest.mark.parametrize('C,blk,B,H,W', FFN_CASES)
def test_ffn_half_block_at_awkward_shapes(C, blk, B, H, W):
    """one strip only; level-1 planes 8 x 8 / 8 x 24 / 40 x 24 / 24 x 104; 576 strips on 512 / 256 workgroups; (43,80,48): strips of 24, 24, 24 and
    8 rows, 516 of them on 512 slots"""
    _check_ffn(f'ffn C={C} blk={blk} ({B},{H},{W})', _default(C), C, blk, B, H, W)


# ---- 2. mixer half-block: k_attn_m<8|16|32, 2> behind the FFT mixer
MIXER_SHAPES = [(1, 16, 16), (3, 16, 48), (3, 80, 48), (9, 128, 128)]
MIXER_CASES = [(C, blk) + s for C in (4, 8) for blk in (0, 2) for s in MIXER_SHAPES] + [(C, 2, 33, 128, 128) for C in (4, 8)]


@pytest.mark.parametrize('C,blk,B,H,W', MIXER_CASES)
def test_mixer_half_block_at_awkward_shapes(C, blk, B, H, W):
    """a quad that holds one window (level 1 of 16 x 16); ragged last quads (9 and 45 windows); rectangular window grids; 2304 windows = 576
    quads in two rounds at level 0; 2112 windows = 528 quads at level 1"""
    _check_mixer(f'mixer C={C} blk={blk} ({B},{H},{W})', _default(C), C, blk, B, H, W)


# ---- 3. the blocks no per-op test calls: their own weight offsets, scale jobs and pos_emb tables
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('blk', [1, 3, 4])
@pytest.mark.parametrize('which', [1, 2])
def test_second_encoder_and_decoder_blocks(C, blk, which):
    check = _check_mixer if which == 1 else _check_ffn
    check(f'{"mixer" if which == 1 else "ffn"} C={C} blk={blk} (3,48,32)', _default(C), C, blk, 3, 48, 32)


# ---- 5. one LGT: k_embed / k_down / k_upfuse / k_tail around the blocks, at rectangles and half-tiles
@pytest.mark.parametrize('C,B,H,W', LGT_CASES)
def test_one_lgt_at_awkward_shapes(C, B, H, W):
    z = _lgt_input(C, B, H, W)
    with torch.no_grad():
        want64 = orc.lgt(_params(C, 1, torch.float64), 'prior_module.0.', z.double())
        want32 = orc.lgt(_params(C, 1, torch.float32), 'prior_module.0.', z).double()
    got = _ops(C, H, W).lgt(0, z.cuda(), guard=True).cpu().double()
    assert not torch.isnan(got).any()
    den = float(want64.abs().max())
    pre, rel, mx = rel_l2(want32, want64), rel_l2(got, want64), _max_err(got, want64, den)
    print(f'lgt C={C} ({B},{H},{W}): rel-L2 {rel:.2e}  max-norm {mx:.2e}  fp32 oracle rel-L2 {pre:.1e} max-norm {_max_err(want32, want64, den):.2e}')
    assert pre < 1e-6, ('the fp32 oracle is not clean on this input: change the seed', pre)
    assert rel < 1e-4 and mx < 1e-4, (rel, mx)


# ---- 4. the saving instances against the plain ones
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('B,H,W', [(3, 80, 48), (2, 16, 48)])
def test_saving_forward_is_bitwise_the_plain_forward(C, B, H, W):
    """lg_op_lgt with LG_FLAG_SAVE launches k_ffn_xr<3,.> / k_ffn_x32 / k_ffn_x64 / k_attn_m with their save arguments set and k_down / k_upfuse
    with their save pointers: the same templates, whose stores of h2, h3, the softmax statistics and the resampled planes are side effects of
    values the plain instances compute too (k_ffn_xr: `if (SAVE && ..) XR_ST2(..)` beside the ring store of the same registers) -- the
    output is bit for bit the plain forward's"""
    from lgteun_amd import _lib
    z = _lgt_input(C, B, H, W).cuda()
    ops = _ops(C, H, W)
    plain = ops.lgt(0, z, guard=True)
    saving = ops.lgt(0, z, flags=_lib.LG_FLAG_SAVE, guard=True)
    assert not torch.isnan(plain).any() and not torch.isnan(saving).any()
    assert torch.equal(plain, saving), float((plain - saving).abs().max())


# ---- 6. data step forward: stage 1 of K = 2
@pytest.mark.parametrize('B,C,H,W', DSTEP_CASES)
def test_data_step_at_awkward_shapes(B, C, H, W):
    """the 32 x 32 tile kernels on planes that are no multiple of 32, an MS plane of 4 x 4, the one-launch form (64 x 64) at an odd batch"""
    rng = np.random.default_rng(C * 1000 + H)
    z = T(rng.uniform(0, 1, (B, C, H, W)).astype(np.float32))
    ms = T(rng.uniform(0, 1, (B, C, H // 4, W // 4)).astype(np.float32))
    pan = T(rng.uniform(0, 1, (B, 1, H, W)).astype(np.float32))
    P64, P32 = _params(C, 2, torch.float64), _params(C, 2, torch.float32)
    with torch.no_grad():
        want64 = orc.data_step(P64, z.double(), ms.double(), pan.double(), P64['eta.1'])
        want32 = orc.data_step(P32, z, ms, pan, P32['eta.1']).double()
    got = _ops(C, H, W, K=2).data_step(1, z.cuda(), ms.cuda(), pan.cuda(), guard=True).cpu()
    _elementwise(f'data step C={C} ({B},{H},{W})', got.double(), want64, want32, float(want64.abs().max()), 2e-6)
    if B > 1:
        alone = _ops(C, H, W, K=2).data_step(1, z[-1:].cuda(), ms[-1:].cuda(), pan[-1:].cuda(), guard=True).cpu()
        assert torch.equal(alone, got[-1:]), float((alone - got[-1:]).abs().max())


# ---- 7. plain bicubic resample
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('planes,hi,wi', [(3, 4, 4), (5, 4, 12), (7, 20, 12), (1, 52, 44)])
def test_resample_at_awkward_shapes(mode, planes, hi, wi):
    """a 4-tap support that is clamped from both sides at once (x0.5 of a 4-wide plane reads taps -1 .. 4 of 4), odd plane counts"""
    x = T(np.random.default_rng(100 * mode + hi + wi).standard_normal((1, planes, hi, wi)).astype(np.float32))
    scale = {0: 0.5, 1: 2, 2: 4}[mode]
    want64, want32 = orc.resample(x.double(), scale), orc.resample(x, scale).double()
    got = _ops(4, 32, 32).resample(x.cuda(), mode, guard=True).cpu()
    assert got.shape == want64.shape
    _elementwise(f'resample mode={mode} [{planes},{hi},{wi}]', got.double(), want64, want32, float(want64.abs().max()), 2e-6)


# ---- 8. precision = 'bf16': the <., 1> instances
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('which', [1, 2])
@pytest.mark.parametrize('blk,B,H,W', [(0, 3, 80, 48), (2, 3, 80, 48), (0, 9, 128, 128)])
def test_bf16_instances_at_awkward_shapes(C, which, blk, B, H, W):
    """one round-to-nearest bf16 piece per operand: the project's bf16 forward gate (5e-3 of the fp64 result), every pixel written, nothing
    beside the output, batch independence bitwise.  No element-wise bar: nothing independent of the code under test yields one."""
    x, want64 = (_mixer_refs if which == 1 else _ffn_refs)(C, blk, B, H, W)[:2]
    got = _ops(C, H, W, precision='bf16').block(0, blk, which, x.cuda(), guard=True).cpu()
    assert not torch.isnan(got).any()
    rel = rel_l2(got, want64)
    res = float((got.double() - want64).norm() / (want64 - x.double()).norm())
    print(f'bf16 {"mixer" if which == 1 else "ffn"} C={C} blk={blk} ({B},{H},{W}): rel-L2 {rel:.2e} ({res:.2e} of the residual branch)')
    assert rel < 5e-3, rel
    alone = _ops(C, H, W, precision='bf16').block(0, blk, which, x[-1:].cuda(), guard=True).cpu()
    assert torch.equal(alone, got[-1:]), float((alone - got[-1:]).abs().max())


# ---- 9. the shipped A/B forward kernels other tests use as yardsticks
@pytest.mark.parametrize('B,H,W', [(3, 80, 48), (1, 16, 16)])
@pytest.mark.parametrize('var,val,which,cases', [
    ('LG_FFN_IMPL', 'strip', 2, [(4, 0), (4, 2), (8, 0), (8, 2)]),     # e = 16 k_ffn_strip, e = 32 k_ffn_fused, e = 64 k_ffn1 + k_ffn2: fp32 MFMAs
    ('LG_FFN_FWD', 'xs', 2, [(4, 0)]),                                 # e = 16 only: the channel-split k_ffn_xs
    ('LG_ATTN_FWD', 'valu', 1, [(4, 0), (4, 2), (8, 0), (8, 2)])])     # k_attn: fp32 FMAs on the vector pipe
def test_ab_forward_kernels_at_awkward_shapes(var, val, which, cases, B, H, W, monkeypatch):
    monkeypatch.setenv(var, val)                                       # read once per plan: a fresh module builds a fresh plan
    try:
        for C, blk in cases:
            check = _check_mixer if which == 1 else _check_ffn
            check(f'{var}={val} C={C} blk={blk} ({B},{H},{W})', _default(C), C, blk, B, H, W)
        if which == 1 and (B, H, W) == (1, 16, 16):
            # the last block of the last stage of K = 2: its own row of the transposed pos_emb tables, the one furthest from row 0 (only k_attn reads them)
            _check_mixer(f'{var}={val} C=4 stage 1 of K=2 blk=4 ({B},{H},{W})', _default(4, 2), 4, 4, B, H, W, K=2, stage=1)
    finally:
        monkeypatch.delenv(var, raising=False)
