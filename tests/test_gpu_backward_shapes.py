"""-m gpu: the backward kernels one op at a time, at the shapes where their launch geometry changes, tensor by tensor.

What lg_op_block_bwd / lg_op_lgt_bwd / lg_op_data_step_bwd launch -- k_ffn_dw_bwd_xs + k_ffn1_bwd_xs (e = 16, and e = 32 on whole strips), the level-1
fallback k_ffn_dw_bwd + k_ffn1_bwd_xs + k_wgrad(W3) (e = 32 on planes that are no whole number of 16-column strips: no square power of two reaches
it), k_ffn_dw_bwd + k_ffn1_bwd + three k_wgrad launches (e = 64), k_attn_bwd_f (e = 16), k_attn_bwd_core<16|32, 4> + k_attn_bwd_epi (e = 32, 64),
the data step's tile kernels and its one-launch form, k_tail_bwd / k_upfuse_bwd_a/b / k_down_bwd_a/b / k_embed_bwd -- against torch autograd over
the fp64 oracle with the deterministic weights.  The other backward tests gate norms of dx and pooled or per-tensor norms of the parameter
gradients at 32 x 32 and 16 x 16 planes of B = 2, blocks 0 and 2 only; the whole-net tests gate a global relative L2 of 1e-3 / 5e-3.  Here, mirroring
test_gpu_forward_shapes.py:

  * ROUTE FIRST: every case asserts, from the `L0` / `L1` `bwd:` line of lg_plan_describe, the kernels it believes it runs -- a route change that
    moves a case onto another kernel fails the case;
  * dx / dz is a view into a NaN-filled buffer with 1024 floats of band on each side (gpu_helpers guard=True): no NaN left = every element
    written; both bands still NaN = nothing written beside it;
  * the flat gradient buffer is such a view too (gpu_helpers owned=[names]): the owned tensors start at zero, every other float -- the other
    blocks' tensors, the other stage, the 16-byte padding -- starts as 2^-100 x (1 + index mod 251) and must be that bit pattern afterwards: a
    half-block's backward leaves every gradient tensor that is not its own untouched (a stray store or a stray `+=` both change the bits);
  * dx in relative L2 at the project's per-op gates (FFN 2e-5, k_attn_bwd_f mixer 1e-4, e >= 32 mixer 2e-4, data step 2e-6, LGT 2e-4);
  * dx ELEMENT BY ELEMENT: max |got - fp64| over the branch's largest entry (half-blocks: max |dx64 - dy|, data step: max |dz64|) is at most BAR x
    the same figure of the fp32 oracle's autograd on the same inputs.  A wrong tap or a stale pixel is >= 1e4 on this scale;
  * the mixer half-block takes the FFT mixer out of the element-wise figure (its backward divides by bin amplitudes: its fp32 noise depends on the
    algorithm, the existing gates on it are 2e-3): the reference is the autograd, fp64 and again fp32, of the restated scalar
    <x + proj(cat(local_mixer(LN(x)[..., :e/2]), o2)), dy> + <LN(x)[..., e/2:], dg> with o2 THIS build's which = 0 forward output on x and dg THIS
    build's which = 0 backward output for do2 = (proj^T dy)'s global half (computed in fp64, cast to fp32), both held constant.  That gives dx and
    the seven local tensors (pos_emb, to_qkv w/b, proj w/b, the LayerNorm pair); the whole fp64 mixer stays beside it at the L2 gates, and the four
    global_mixer gradients against it at 2e-3;
  * PARAMETER GRADIENTS: one line per tensor, never a pooled norm.  err = max |got - g64| / max |g64| <= max(8 x err32, G), err32 the fp32
    oracle's figure on that tensor, G per family (below); the data step's tensors at 2e-5 relative L2 as in test_gpu_ops_bwd.py;
  * preconditions of every case, asserted ahead of the launch under test: the fp32 oracle's output within 1e-6 of its fp64 output, and its dx within PRE_BWD of its fp64 dx (otherwise
    the INPUT drew a branch-cut flip in the reference's own fp32 arithmetic: change the seed, never the gate).  Measured on the CPU before any GPU
    run, relative L2: FFN 4.3e-8 .. 4.9e-8, restated mixer 4.5e-8 .. 4.9e-8, data step 3.5e-8 .. 3.7e-8, whole mixer 6.0e-8 .. 2.6e-7 (median
    1.0e-7), one LGT 8.4e-7 .. 7.3e-6 (median 2.1e-6); PRE_BWD is 4 x the largest of each family.  Five first draws stood out by more than 4 x
    above their family's median and got another seed (RESEED): mixer C=4 blk=0 (5,128,128) at 8.9e-4, C=8 blk=2 (3,16,48) at 1.1e-6, C=4 blk=3
    (3,48,32) at 6.4e-7, LGT C=4 (1,16,16) at 2.0e-5 and (2,16,48) at 1.2e-5;
  * NO bitwise batch independence, unlike the forward: k_ffn1_bwd_xs scales its f16 pairs by max |dh2| over the WHOLE batch (ffn_scales word 6,
    written by k_ffn_dw_bwd_xs), so a sample's dx legitimately depends on its neighbours in the last bits.

Shapes (PAN sizes (B, H, W); level 1 is half of it) are the smallest that reach each edge of the launchers: one strip only; the level-1 planes 8 x 8,
8 x 24, 40 x 24 and 24 x 104 on the fallback and 40 x 32 on the strip route (strip heights 16 / 16 / 8); 576 strips on a grid of 512 (e = 16) and 288 on
256 (e = 32), 516 strips of 24 / 24 / 24 / 8 rows on 512 slots, 272 level-1 strips on 256: workgroups of k_ffn_dw_bwd_xs that walk a second strip;
one window in a group of four, a last group that holds one window (45 windows); 1280 level-0 windows = 320 groups of four on 256 workgroups, for k_attn_bwd_f
(F_NS = 4 window slots per workgroup, ATTN_BWD_F_WGS = 256) and for k_attn_bwd_core<16,4> (NW = 4, grid capped at 256) alike; 1088 level-1 windows = 272 groups on 256;
blocks 1, 3, 4 at (3,48,32); one LGT at rectangles and half-tiles with stage 0 of K = 2 as the sentinel; data-step tiles on planes that are no
multiple of 32, the 4 x 4 MS plane, the one-launch form at odd batches.

Measured on an MI355X (ratio = element-wise error of dx over the fp32 oracle's; the test prints every row, and one line per gradient tensor):
  op                                                              cases   rel-L2                 element-wise           fp32 oracle            ratio
  FFN e = 16 (k_ffn_dw_bwd_xs + k_ffn1_bwd_xs: C=4 blk 0)              7   2.7e-08 .. 2.8e-08   6.3e-07 .. 8.9e-07   1.4e-06 .. 2.1e-06   0.40 .. 0.51
  FFN e = 32 (strips and the fallback: C=4 blk 2, C=8 blk 0)          13   2.8e-08 .. 2.8e-08   7.5e-07 .. 1.3e-06   1.5e-06 .. 2.6e-06   0.34 .. 0.65
  FFN e = 64 (k_ffn_dw_bwd + k_ffn1_bwd + 3 k_wgrad: C=8 blk 2)        6   3.0e-08 .. 3.1e-08   9.2e-07 .. 1.4e-06   1.8e-06 .. 2.7e-06   0.42 .. 0.65
  FFN, blocks 1 / 3 / 4 at (3,48,32)                                   6   2.7e-08 .. 2.8e-08   5.5e-07 .. 1.1e-06   1.0e-06 .. 2.5e-06   0.30 .. 0.68
  mixer e = 16, restated (k_attn_bwd_f: C=4 blk 0)                     4   4.8e-08 .. 6.1e-08   2.3e-07 .. 3.4e-07   2.0e-07 .. 2.8e-07   0.83 .. 1.57
  mixer e = 32, restated (k_attn_bwd_core<16,4>: C=4 blk 2, C=8 blk 0) 9   4.4e-08 .. 6.6e-08   1.4e-07 .. 3.8e-07   1.8e-07 .. 2.7e-07   0.69 .. 1.56
  mixer e = 64, restated (k_attn_bwd_core<32,4>: C=8 blk 2)            5   5.0e-08 .. 6.4e-08   2.3e-07 .. 3.3e-07   1.8e-07 .. 2.6e-07   1.21 .. 1.68
  mixer, blocks 1 / 3 / 4 at (3,48,32), restated                       6   6.0e-08 .. 7.8e-08   2.9e-07 .. 3.9e-07   1.8e-07 .. 2.5e-07   1.45 .. 1.81
  data step                                                            7   3.5e-08 .. 3.7e-08   5.2e-08 .. 8.9e-08   5.4e-08 .. 8.9e-08   0.96 .. 1.03
  largest ratio of all 63 rows: 1.81 (mixer C=4 blk=1 (3,48,32)); twice that, rounded up to a power of two: the bar is 4
  the whole fp64 mixer beside the restated one (24 cases): dx rel-L2 5.4e-08 .. 4.8e-07 (the fp32 oracle's own: 6.0e-08 .. 2.7e-07; gates 1e-4 / 2e-4)
  one LGT (6 cases): dz rel-L2 9.0e-07 .. 6.6e-06, max-norm 1.6e-06 .. 1.3e-05 of max |dz64| (the fp32 oracle's: 1.0e-06 .. 1.9e-05; gates 2e-4)
  precision='bf16' (8 cases): dx rel-L2 up to 1.7e-04 (gate 2e-2), worst parameter gradient up to 6.2e-03 of its tensor's largest entry (gate 5e-2);
    the e = 64 FFN runs the default kernels in this mode: 3.1e-08
  parameter gradients, worst err = max |got - g64| / max |g64| per family, per-op cases | inside one LGT  ->  G = 4 x the worst where that is below the
  existing gate (the results are deterministic; the margin is for a compiler change):
    FFN (10 tensors)                  7.7e-06 | 2.4e-05   existing 2e-4  ->  1.0e-4
    k_attn_bwd_f local tensors (7)    9.9e-07 | 6.9e-05   existing 1e-4  ->  1e-4 stays (4 x 6.9e-05 is above it)
    e >= 32 local tensors (7)         7.2e-07 | 2.5e-05   existing 2e-3  ->  1.1e-4
    global_mixer (4)                  1.2e-06 | 1.0e-04   existing 2e-3  ->  4.2e-4
    LGT-level tensors (14)                    | 3.8e-05   existing 2e-3  ->  1.5e-4
    data step (13), relative L2       8.5e-06 (eta.1)     existing 2e-5  ->  2e-5 stays
  1389 gradient lines in all; 19 of them are above 8 x the fp32 oracle's figure (worst 19 x: the FFN's LayerNorm bias at (9,128,128), 7.7e-06 against
  4.5e-07 -- a sum over 1.5e5 pixels of split-arithmetic products) and pass on G; every other line passes on the fp32 yardstick alone.
  The file: 77 tests in 27 s on the MI355X machine, the slowest case 4.6 s (FFN C=8 blk=0 (9,128,128): fp64 + fp32 autograd over 1.5e5 pixels x 128 channels).
  The per-op entries at other stage indices (stages 0 and 2 of K = 3, at the smallest LGT and data-step shape of each C; every other stage's slots the
  sentinel; the fp32 oracle clean on the first draw of all eight, no RESEED entry): one LGT, dz rel-L2 3.7e-07 .. 3.6e-06 (the fp32 oracle's: 3.9e-07 ..
  1.0e-05), the worst of the 4 x 119 gradient lines at 0.26 of its bar (C=8 stage 2, block 1's point_conv.weight: 2.6e-05, fp32 oracle 9.8e-06, G 1e-4);
  the data step, dz ratio 1.00 on all four, the worst of the 4 x 13 gradient lines 2.2e-06 (R.bias, C=8 stage 2) against 2e-5.  85 tests with them.

What it sees, checked once with three variant builds loaded through LGTEUN_HIP_LIB (arithmetic-only edits inside the buffers; nothing of them is kept):
  (a) k_ffn_dw_bwd_xs with the ring row below each strip left out of the depthwise transpose.  RED: every FFN case on the strip route whose planes
      hold more than one strip -- C=4 blk 0 and C=8 blk 0 at (3,80,48), (3,80,64), (2,48,208), (9,128,128), and C=4 blk 0 at (43,80,48); C=4 blk 2 at (3,80,64),
      (9,128,128), (17,128,128); all six FFN cases of blocks 1 / 3 / 4 -- at 0.24 .. 0.70 of the branch's largest entry (ratio 1.7e5 .. 3.7e5, rel-L2
      3.5e-3 .. 5.3e-3 against the gate of 2e-5); one LGT at (4,3,80,48), (8,1,48,208), (8,2,48,48), (8,3,80,48): dz rel-L2 2.6e-3 .. 3.2e-3 (gate 2e-4);
      bf16 FFN blk 0, C = 4 and 8: worst parameter gradient 0.19 / 0.27 (gate 5e-2; dx 4.9e-3 / 5.0e-3 stays under its 2e-2).  GREEN: (1,16,16) and
      (3,16,48), one strip per plane; C=4 blk 2 at (3,80,48) and (2,48,208), the fallback's tile kernel; every C=8 blk 2 case (e = 64); the LGT at
      (4,1,16,16) and (4,2,16,48); the mixer cases.
  (b) k_attn_bwd_core: where the window count is no multiple of four, the LAST window (the last one of the ragged group) reads the FIRST window's
      x.  (Read as "the first window of its own group" the edit would be invisible in this file and in the issue's shapes: their ragged groups
      hold one window.)  RED: mixer blk 2 at (3,16,48) and (3,80,48), 9 and 45 level-1 windows, C = 4 and 8: dx against the whole fp64 mixer at
      4.4e-3 .. 1.2e-2 (gate 2e-4); the LGT at (4,2,16,48), (4,3,80,48), (8,1,48,208), (8,2,48,48), (8,3,80,48) -- 6, 45, 39, 18 and 45 level-1
      windows -- on dz (up to 3.4e-4) or, where dz stays under 2e-4, on the bottleneck mixer's own gradient lines; bf16 mixer blk 2: pos_emb at
      0.37 / 0.38 (gate 5e-2).  GREEN: blk 2 at (1,16,16) (one window: the last is the first), (5,128,128) and (17,128,128) (whole groups), every
      blk 0 case (C = 4: k_attn_bwd_f; C = 8: 4, 36, 180 and 1280 windows), blocks 1 / 3 / 4 (72 windows), the LGT at (4,1,16,16).
  (c) block 3's db3 reduce pointed at block 4's slot.  RED: the block-3 FFN cases, C = 4 and 8, on the sentinel -- 16 / 32 floats of block 4's
      net.4.bias written -- ahead of any gradient line; all six LGT cases: block 3's net.4.bias at err 1.0 and block 4's at 1.03 .. 1.30.  GREEN: the
      FFN cases of blocks 1 and 4 and every mixer case of blocks 1 / 3 / 4.
"""
import functools
import re

import numpy as np
import pytest
import torch

from helpers import BLOCKS, DSTEP_CASES as FWD_DSTEP_CASES, LGT_CASES, block_features, block_prefix, det_params, ffn_half_block, lgt_input
from helpers import mixer_half_block, mixer_restated, rel_l2
from oracle import lgteun_oracle as orc

pytestmark = pytest.mark.gpu

T = torch.from_numpy
BAR = 4.0                   # dx element by element: at most this many times the fp32 oracle's own error
PRE_FWD = 1e-6              # the fp32 oracle's output against its fp64 output
# the fp32 oracle's dx against its fp64 dx, relative L2: 4 x the largest over the cases of this file (change the seed, never the gate)
PRE_BWD = {'ffn': 2.0e-7, 'mixer': 1.1e-6, 'restated': 2.0e-7, 'dstep': 1.5e-7, 'lgt': 3.0e-5}
# parameter gradients, per tensor: err <= max(8 x the fp32 oracle's err, G)
G = {'ffn': 1.0e-4, 'mixer16': 1e-4, 'mixer32': 1.1e-4, 'global': 4.2e-4, 'lgt': 1.5e-4}     # (tightened from 2e-4, 1e-4, 2e-3, 2e-3, 2e-3: docstring)
L2 = {'ffn': 2e-5, 'mixer16': 1e-4, 'mixer32': 2e-4, 'dstep': 2e-6, 'lgt': 2e-4}


@pytest.fixture(autouse=True)
def canonical_real_bins(monkeypatch):
    """as in the forward file: pin the +0 convention of the four purely-real bins (oracle/lgteun_oracle.py)"""
    monkeypatch.setattr(orc, 'CANONICAL_REAL_BINS', True)


@functools.lru_cache(maxsize=None)
def _params(C, K, dtype):
    return det_params(C, K, dtype=dtype, requires_grad=True)


def _ops(C, H, W, K=1, precision=None):
    from gpu_helpers import make_ops
    return make_ops(C, H, W, K, precision)


def _level(blk):
    return 1 if blk == 2 else 0


def _width(C, blk):
    return 8 * C if blk == 2 else 4 * C


# ---- route first: what the plan says it launches
def _ffn_route(C, blk, H, W, bf16=False):
    e = _width(C, blk)
    if e == 64:
        return 'ffn=k_ffn_dw_bwd+k_ffn1_bwd+k_wgrad(W2)+k_wgrad(W1)+k_wgrad(W3) arith=f32'
    h, w = (H // 2, W // 2) if blk == 2 else (H, W)
    if (h & 7) or (w & 15):        # resolve_ffn: no whole 8-row steps of 16-column strips -> the strip walk is off (here: level-1 planes only)
        return 'ffn=k_ffn_dw_bwd+k_ffn1_bwd_xs+k_wgrad(W3) arith=' + ('bf16' if bf16 else 'bf16x3')
    return 'ffn=k_ffn_dw_bwd_xs+k_ffn1_bwd_xs arith=' + ('bf16' if bf16 else 'f16x2')


def _mixer_route(C, blk, bf16=False):
    kernels = 'k_attn_bwd_f' if _width(C, blk) == 16 else 'k_attn_bwd_core+k_attn_bwd_epi'
    return f'mixer={kernels} stats=' + ('recomputed' if bf16 else 'saved')


def _assert_route(ops, H, W, level, ffn=None, mixer=None):
    lines = [ln for ln in ops.eng.describe(H, W).splitlines() if ln.startswith(f'L{level} ') and ' bwd: ' in ln]
    assert len(lines) == 1, lines
    got_ffn, got_mixer = lines[0].split(' bwd: ')[1].split(' | ')
    if ffn is not None:
        assert got_ffn.startswith(ffn + ' reads='), (got_ffn, ffn)
    if mixer is not None:
        assert got_mixer == mixer, (got_mixer, mixer)


# ---- references: torch autograd over the oracle, fp64 and fp32
def _block_names(P, blk, which, stage=0):
    pre = f'prior_module.{stage}.' + BLOCKS[blk] + ('0.fn.' if which == 1 else '1.fn.')
    return [n for n in P if n.startswith(pre)]


# cases whose first draw stood out by more than 4 x above its family's median in the fp32 oracle's own dx error (a branch-cut flip of angle() in
# the reference's fp32 arithmetic): another seed, never another gate.  Key: (which, C, blk, B, H, W), 'lgt' for a whole LGT
RESEED = {(1, 4, 0, 5, 128, 128): 1, (1, 8, 2, 3, 16, 48): 1, (1, 4, 3, 3, 48, 32): 1, ('lgt', 4, None, 1, 16, 16): 1, ('lgt', 4, None, 2, 16, 48): 1}


def _features(C, blk, B, H, W, seed=0):
    """helpers.block_features: standard-normal NHWC features, the last sample's global half shifted by -0.7; seed > 0: another draw of the same"""
    x = block_features(C, blk, B, H, W)
    if seed:
        x = T(np.random.default_rng(1000 + H + W + 7 * blk + C + 100000 * seed).standard_normal(tuple(x.shape)).astype(np.float32))
        x[-1, ..., x.shape[-1] // 2:] -= 0.7
    return x


def _dy(shape, *key):
    return T(np.random.default_rng([5000, *key]).standard_normal(tuple(shape)).astype(np.float32))


def _autograd(fn, P, names, x, dy):
    """(y, dx, {name: grad}) of <fn(P, x), dy> in P's precision; fn returns y or (y, an extra scalar)"""
    dtype = P[names[0]].dtype
    xx = x.to(dtype).requires_grad_(True)
    y = fn(P, xx)
    y, extra = y if isinstance(y, tuple) else (y, 0.0)
    g = torch.autograd.grad((y * dy.to(dtype)).sum() + extra, [xx] + [P[n] for n in names])
    return y.detach().double(), g[0].double(), {n: v.double() for n, v in zip(names, g[1:])}


_REFS = {}


def _block_refs(C, blk, which, B, H, W):
    """x, dy and the whole half-block's (y, dx, grads) in fp64 and fp32: computed once per case, shared, never written to"""
    key = (C, blk, which, B, H, W)
    if key not in _REFS:
        seed = RESEED.get((which, C, blk, B, H, W), 0)
        x = _features(C, blk, B, H, W, seed)
        dy = _dy(x.shape, C, blk, H, W, seed)
        fn = (lambda P, v: mixer_half_block(P, blk, v)) if which == 1 else (lambda P, v: ffn_half_block(P, blk, v))
        P64, P32 = _params(C, 1, torch.float64), _params(C, 1, torch.float32)
        names = _block_names(P64, blk, which)
        assert len(names) == (11 if which == 1 else 10), names
        y64, dx64, g64 = _autograd(fn, P64, names, x, dy)
        y32, dx32, g32 = _autograd(fn, P32, names, x, dy)
        ref = (x, dy, names, rel_l2(y32, y64), dx64, dx32, g64, g32)
        if B * H * W > 3 * 80 * 48:            # (the large cases are used once; the small ones again by the bf16 tests)
            return ref
        _REFS[key] = ref
    return _REFS[key]


def _max_err(a, b, den):
    return float((a - b).abs().max()) / den


def _precondition(tag, family, pre_fwd, dx64, dx32):
    """before the launch under test: the fp32 oracle is clean on this input, forward and backward (on the CPU; the restated mixer's needs this
    build's which = 0 outputs and is checked behind those two launches, ahead of the which = 1 launch)"""
    pre = rel_l2(dx32, dx64)
    assert pre_fwd < PRE_FWD, (tag, 'the fp32 oracle is not clean on this input: change the seed, never the gate', pre_fwd)
    assert pre < PRE_BWD[family], (tag, "the fp32 oracle's dx is not clean on this input: change the seed, never the gate", pre)


def _dx_checks(tag, got, dx64, dx32, den, l2_gate, pre_fwd, bar=True):
    """no NaN left, relative L2, the element-wise bar; prints the measured row"""
    assert not torch.isnan(got).any(), (tag, 'elements of dx never written', int(torch.isnan(got).sum()))
    got = got.double()
    pre, rel = rel_l2(dx32, dx64), rel_l2(got, dx64)
    e_got, e_32 = _max_err(got, dx64, den), _max_err(dx32, dx64, den)
    print(f'{tag}: rel-L2 {rel:.2e}  element-wise {e_got:.2e}  fp32 oracle {e_32:.2e} (rel-L2 {pre:.1e}, forward {pre_fwd:.1e})  ratio {e_got / e_32:.2f}')
    assert rel < l2_gate, (tag, rel)
    if bar and e_got > BAR * e_32:
        d = (got - dx64).abs()
        worst = [tuple(int(v) for v in np.unravel_index(int(i), tuple(d.shape))) for i in torch.topk(d.flatten(), 8).indices]
        assert False, (tag, e_got, e_32, e_got / e_32, 'worst elements', worst)


def _grad_checks(tag, ops, flat, names, g64, g32, family_of):
    """item 6: one line per tensor, err = max |got - g64| / max |g64| <= max(8 x the fp32 oracle's, G of its family)"""
    bad = []
    for n in names:
        got, den = ops.grad_of(flat, n).cpu().double(), float(g64[n].abs().max())
        err, err32, fam = _max_err(got, g64[n], den), _max_err(g32[n], g64[n], den), family_of(n)
        print(f'    {tag} | {fam} | {n}: err {err:.2e}  fp32 oracle {err32:.2e}  G {G[fam]:.1e}')
        if not err <= max(8 * err32, G[fam]):
            bad.append((n, err, err32, G[fam]))
    assert not bad, (tag, bad)


def _mixer_family(C, blk):
    return 'mixer16' if _width(C, blk) == 16 else 'mixer32'


def _do2(C, blk, dy):
    """(proj^T dy)'s global half, planar [B, e/2, h, w]: computed in fp64, cast to fp32"""
    half = dy.shape[-1] // 2
    with torch.no_grad():
        w = _params(C, 1, torch.float64)[block_prefix(blk) + '0.fn.fn.proj.weight'][:, half:, 0, 0]
        return torch.einsum('bhwo,oc->bchw', dy.double(), w).float().contiguous()


def _restated_refs(C, blk, x, dy, o2, dg):
    """autograd, fp64 and fp32, of <x + proj(cat(local_mixer(LN(x)[..., :e/2]), o2)), dy> + <LN(x)[..., e/2:], dg>: o2 and dg planar [B, e/2, h, w]
    and held constant.  Returns the seven local tensors' names and (y, dx, grads) twice"""
    p = block_prefix(blk) + '0.fn.'
    half = x.shape[-1] // 2
    dgn = dg.permute(0, 2, 3, 1)

    def restated(P, v):
        ln = orc.layer_norm(v, P[p + 'norm.weight'], P[p + 'norm.bias'])
        x1 = orc.local_mixer(P, p + 'fn.local_mixer.', ln[..., :half])
        return mixer_restated(P, blk, v, x1, o2.to(v.dtype)), (ln[..., half:] * dgn.to(v.dtype)).sum()
    P64, P32 = _params(C, 1, torch.float64), _params(C, 1, torch.float32)
    local = [n for n in _block_names(P64, blk, 1) if 'global_mixer' not in n]
    assert len(local) == 7, local
    return local, _autograd(restated, P64, local, x, dy), _autograd(restated, P32, local, x, dy)


def _check_ffn_bwd(C, blk, B, H, W):
    tag = f'ffn bwd C={C} blk={blk} ({B},{H},{W})'
    ops = _ops(C, H, W)
    _assert_route(ops, H, W, _level(blk), ffn=_ffn_route(C, blk, H, W))
    x, dy, names, pre_fwd, dx64, dx32, g64, g32 = _block_refs(C, blk, 2, B, H, W)
    _precondition(tag, 'ffn', pre_fwd, dx64, dx32)
    dx, flat = ops.block_bwd(0, blk, 2, x.cuda(), dy.cuda(), guard=True, owned=names)
    _dx_checks(tag, dx.cpu(), dx64, dx32, float((dx64 - dy.double()).abs().max()), L2['ffn'], pre_fwd)
    _grad_checks(tag, ops, flat, names, g64, g32, lambda n: 'ffn')


def _check_mixer_bwd(C, blk, B, H, W):
    tag = f'mixer bwd C={C} blk={blk} ({B},{H},{W})'
    fam = _mixer_family(C, blk)
    ops = _ops(C, H, W)
    _assert_route(ops, H, W, _level(blk), mixer=_mixer_route(C, blk))
    x, dy, names, pre_fwd, dx64, dx32, g64, g32 = _block_refs(C, blk, 1, B, H, W)
    _precondition(tag, 'mixer', pre_fwd, dx64, dx32)
    # the restated scalar: o2 and dg are this build's own global mixer (which = 0), forward and backward
    xd = x.cuda()
    o2 = ops.block(0, blk, 0, xd).cpu()
    dg = ops.block_bwd(0, blk, 0, xd, _do2(C, blk, dy).cuda())[0].cpu()
    assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(dg).all()), tag
    local, (y64, r64, gr64), (y32, r32, gr32) = _restated_refs(C, blk, x, dy, o2, dg)
    pre_fwd_r = max(pre_fwd, rel_l2(y32, y64))
    _precondition(tag + ' restated', 'restated', pre_fwd_r, r64, r32)
    dx, flat = ops.block_bwd(0, blk, 1, xd, dy.cuda(), guard=True, owned=names)
    dx = dx.cpu()
    # the whole fp64 mixer: dx in relative L2, the four global_mixer gradients
    assert not torch.isnan(dx).any(), (tag, 'elements of dx never written', int(torch.isnan(dx).sum()))
    pre, whole = rel_l2(dx32, dx64), rel_l2(dx, dx64)
    print(f'{tag}: whole fp64 mixer rel-L2 {whole:.2e}  fp32 oracle rel-L2 {pre:.1e}')
    assert whole < L2[fam], (tag, whole)
    glob = [n for n in names if 'global_mixer' in n]
    assert len(glob) == 4
    _grad_checks(tag, ops, flat, glob, g64, g32, lambda n: 'global')
    _dx_checks(tag + ' restated', dx, r64, r32, float((r64 - dy.double()).abs().max()), L2[fam], pre_fwd_r)
    _grad_checks(tag, ops, flat, local, gr64, gr32, lambda n: fam)


# ---- 1. FFN half-block backward: k_ffn_dw_bwd_xs + k_ffn1_bwd_xs (e = 16, e = 32 on strips), k_ffn_dw_bwd + k_ffn1_bwd_xs + k_wgrad(W3) (e = 32, the
# level-1 fallback), k_ffn_dw_bwd + k_ffn1_bwd + three k_wgrad launches (e = 64)
FFN_SHAPES = [(1, 16, 16), (3, 16, 48), (3, 80, 48), (3, 80, 64), (2, 48, 208), (9, 128, 128)]
# (9,128,128): 576 strips on a grid of 512 at e = 16, 288 on 256 at e = 32.  (43,80,48): 516 strips on 512.  (17,128,128): 272 level-1 strips on 256
FFN_CASES = [(C, blk) + s for C in (4, 8) for blk in (0, 2) for s in FFN_SHAPES] + [(4, 0, 43, 80, 48), (4, 2, 17, 128, 128)]


@pytest.mark.parametrize('C,blk,B,H,W', FFN_CASES)
def test_ffn_half_block_backward_at_awkward_shapes(C, blk, B, H, W):
    """one strip only; the level-1 fallback planes 8 x 8 / 8 x 24 / 40 x 24 / 24 x 104 (half-empty 16-wide tiles, strips ending inside a tile row) and
    the strip route at 40 x 32 (strip heights 16 / 16 / 8); workgroups of k_ffn_dw_bwd_xs that walk a second strip; 2304 pixel tiles on 512 / 256
    workgroups"""
    _check_ffn_bwd(C, blk, B, H, W)


# ---- 2. mixer half-block backward: k_attn_bwd_f (e = 16), k_attn_bwd_core<16|32, 4> + k_attn_bwd_epi (e = 32, 64) behind the FFT mixer's backward
MIXER_SHAPES = [(1, 16, 16), (3, 16, 48), (3, 80, 48), (5, 128, 128)]
# (5,128,128): 1280 level-0 windows = 320 groups of four (k_attn_bwd_f: F_NS = 4; k_attn_bwd_core: NW = 4) on a grid of 256.  (17,128,128): 1088 level-1 windows = 272 groups on 256
MIXER_CASES = [(C, blk) + s for C in (4, 8) for blk in (0, 2) for s in MIXER_SHAPES] + [(C, 2, 17, 128, 128) for C in (4, 8)]


@pytest.mark.parametrize('C,blk,B,H,W', MIXER_CASES)
def test_mixer_half_block_backward_at_awkward_shapes(C, blk, B, H, W):
    """a group of four that holds one window (level 1 of 16 x 16); ragged last groups (45 windows: 12 groups, the last holds one); rectangular window
    grids; more groups than the grid of 256 at both levels"""
    _check_mixer_bwd(C, blk, B, H, W)


# ---- 3. the blocks no per-op backward test calls: their own weight offsets, reduce jobs, scale words and pos_emb tables
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('blk', [1, 3, 4])
@pytest.mark.parametrize('which', [1, 2])
def test_second_encoder_and_decoder_blocks_backward(C, blk, which):
    """the gradients land in that block's own tensors and nowhere else, and are right against that block's own weights"""
    (_check_mixer_bwd if which == 1 else _check_ffn_bwd)(C, blk, 3, 48, 32)


# ---- 4. one LGT backward: k_tail_bwd, k_upfuse_bwd_a/b, k_down_bwd_a/b, k_embed_bwd and the k_wgrad launches between them, around the five blocks
def _lgt_family(C):
    def family(n):
        m = re.search(r'blocks\.\d\.([01])\.fn\.', n)
        if m is None:
            return 'lgt'
        if 'global_mixer' in n:
            return 'global'
        if m.group(1) == '1':
            return 'ffn'
        return 'mixer32' if (C == 8 or 'bottleneck' in n) else 'mixer16'
    return family


def _lgt_inputs(C, B, H, W, stage=1, K=2):
    seed = RESEED.get(('lgt', C, None if (stage, K) == (1, 2) else (stage, K), B, H, W), 0)
    z = lgt_input(C, B, H, W)
    if seed:
        z = T(np.random.default_rng(H + W + 100000 * seed).uniform(0, 1, tuple(z.shape)).astype(np.float32))
    return z, _dy(z.shape, 7, C, H, W, seed)


def _stage_cases(cases, c_of):
    """the cases at stage 1 of K = 2 under the ids they have always had, then stages 0 and 2 of K = 3 at the smallest shape of each C: the per-op
    backward entries at the first stage and at a last stage that is not stage 1, each against its own stage's weights
    (tests/test_gpu_composition.py strings the entries into networks)"""
    out = [pytest.param(*c, 1, 2, id='-'.join(str(v) for v in c)) for c in cases]
    for C in (4, 8):
        small = min((c for c in cases if c_of(c) == C), key=lambda c: int(np.prod(c)) // C)
        out += [pytest.param(*small, st, 3, id='-'.join(str(v) for v in small) + f'-stage{st}of3') for st in (0, 2)]
    return out


@pytest.mark.parametrize('C,B,H,W,stage,K', _stage_cases(LGT_CASES, lambda c: c[0]))
def test_one_lgt_backward_at_awkward_shapes(C, B, H, W, stage, K):
    """stage 1 of K = 2, and stages 0 and 2 of K = 3: the other stages' slots and the data-step tensors of the gradient buffer stay the sentinel; every
    one of the 119 tensors on its own line.  dz: relative L2 and max-norm, no element-wise bar (the FFT mixers are inside)"""
    tag = f'lgt bwd C={C} ({B},{H},{W})' + ('' if (stage, K) == (1, 2) else f' stage {stage} of {K}')
    ops = _ops(C, H, W, K=K)
    for level, blk in ((0, 0), (1, 2)):
        _assert_route(ops, H, W, level, ffn=_ffn_route(C, blk, H, W), mixer=_mixer_route(C, blk))
    z, dy = _lgt_inputs(C, B, H, W, stage, K)
    pre = f'prior_module.{stage}.'
    P64, P32 = _params(C, K, torch.float64), _params(C, K, torch.float32)
    names = [n for n in P64 if n.startswith(pre)]
    assert len(names) == 119
    y64, dz64, g64 = _autograd(lambda P, v: orc.lgt(P, pre, v), P64, names, z, dy)
    y32, dz32, g32 = _autograd(lambda P, v: orc.lgt(P, pre, v), P32, names, z, dy)
    pre_fwd = rel_l2(y32, y64)
    _precondition(tag, 'lgt', pre_fwd, dz64, dz32)
    dz, flat = ops.lgt_bwd(stage, z.cuda(), dy.cuda(), guard=True, owned=names)
    den = float(dz64.abs().max())
    _dx_checks(tag, dz.cpu(), dz64, dz32, den, L2['lgt'], pre_fwd, bar=False)
    mx = _max_err(dz.cpu().double(), dz64, den)
    assert mx < L2['lgt'], (tag, 'max-norm', mx)
    _grad_checks(tag, ops, flat, names, g64, g32, _lgt_family(C))


# ---- 5. data-step backward: stage 1 of K = 2; stages 0 and 2 of K = 3
DSTEP_CASES = FWD_DSTEP_CASES + [(3, 4, 128, 128)]


@pytest.mark.parametrize('B,C,H,W,stage,K', _stage_cases(DSTEP_CASES, lambda c: c[1]))
def test_data_step_backward_at_awkward_shapes(B, C, H, W, stage, K):
    """the tile kernels on planes that are no multiple of 32 and on a 4 x 4 MS plane; the one-launch form (64 x 64, 128 x 128) at an odd batch; stage 1 of
    K = 2, and stages 0 and 2 of K = 3 (their own eta, every other stage's eta and every LGT tensor the sentinel)"""
    tag = f'data step bwd C={C} ({B},{H},{W})' + ('' if (stage, K) == (1, 2) else f' stage {stage} of {K}')
    ops = _ops(C, H, W, K=K)
    net_line = ops.eng.describe(H, W).splitlines()[0]
    assert ('dstep=fused' if (H, W) in ((64, 64), (128, 128)) else 'dstep=tiles') in net_line.split(': ')[1].split(), net_line
    rng = np.random.default_rng(C * 1000 + H)
    z = T(rng.uniform(0, 1, (B, C, H, W)).astype(np.float32))
    ms = T(rng.uniform(0, 1, (B, C, H // 4, W // 4)).astype(np.float32))
    pan = T(rng.uniform(0, 1, (B, 1, H, W)).astype(np.float32))
    dy = T(rng.standard_normal((B, C, H, W)).astype(np.float32))
    P64, P32 = _params(C, K, torch.float64), _params(C, K, torch.float32)
    eta = f'eta.{stage}'
    names = [n for n in P64 if n.split('.')[0] in ('D', 'DT', 'R', 'RT')] + [eta]
    assert len(names) == 13
    y64, dz64, g64 = _autograd(lambda P, v: orc.data_step(P, v, ms.to(v.dtype), pan.to(v.dtype), P[eta]), P64, names, z, dy)
    y32, dz32, g32 = _autograd(lambda P, v: orc.data_step(P, v, ms.to(v.dtype), pan.to(v.dtype), P[eta]), P32, names, z, dy)
    pre_fwd = rel_l2(y32, y64)
    _precondition(tag, 'dstep', pre_fwd, dz64, dz32)
    dz, flat = ops.data_step_bwd(stage, z.cuda(), ms.cuda(), pan.cuda(), dy.cuda(), guard=True, owned=names)
    _dx_checks(tag, dz.cpu(), dz64, dz32, float(dz64.abs().max()), L2['dstep'], pre_fwd)
    bad = []
    for n in names:
        err, err32 = rel_l2(ops.grad_of(flat, n).cpu(), g64[n]), rel_l2(g32[n], g64[n])
        print(f'    {tag} | dstep | {n}: rel-L2 {err:.2e}  fp32 oracle {err32:.2e}')
        if not err < 2e-5:
            bad.append((n, err))
    assert not bad, (tag, bad)


# ---- 6. precision = 'bf16': the fallback route included, with bf16 storage of the saved tensors
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('blk', [0, 2])
@pytest.mark.parametrize('which', [1, 2])
def test_bf16_backward_at_awkward_shapes(C, blk, which):
    """the project's bf16 gates (dx 2e-2 relative, parameter gradients 5e-2 of the tensor's largest entry), every element of dx written, nothing beside
    it, no foreign gradient float touched.  No element-wise bar: nothing independent of the code under test yields one."""
    B, H, W = 3, 80, 48
    tag = f'bf16 {"mixer" if which == 1 else "ffn"} bwd C={C} blk={blk} ({B},{H},{W})'
    ops = _ops(C, H, W, precision='bf16')
    if which == 2:
        _assert_route(ops, H, W, _level(blk), ffn=_ffn_route(C, blk, H, W, bf16=True))
    else:
        _assert_route(ops, H, W, _level(blk), mixer=_mixer_route(C, blk, bf16=True))
    x, dy, names, _, dx64, _, g64, _ = _block_refs(C, blk, which, B, H, W)
    dx, flat = ops.block_bwd(0, blk, which, x.cuda(), dy.cuda(), guard=True, owned=names)
    dx = dx.cpu()
    assert not torch.isnan(dx).any(), (tag, 'elements of dx never written', int(torch.isnan(dx).sum()))
    rel = rel_l2(dx, dx64)
    worst = sorted(((_max_err(ops.grad_of(flat, n).cpu().double(), g64[n], float(g64[n].abs().max())), n) for n in names), reverse=True)
    print(f'{tag}: dx rel-L2 {rel:.2e}  worst parameter gradient {worst[0][0]:.2e} ({worst[0][1]})')
    assert rel < 2e-2, (tag, rel)
    assert worst[0][0] < 5e-2, (tag, worst[:5])
