"""-m gpu: TRAIN MODE (LG_FLAG_DROPOUT, what every training run and bench.py's headline execute) against the fp64 oracle.  The
LGMixer dropout is a counter hash of (seed, stage, block, element), and the library exports it (lg_dropout_mask): every test here
draws the masks of an explicit seed from that export, hands them to oracle.lgt / oracle.forward (`drop_masks`) and compares the
kernels' outputs and gradients with the oracle's autograd in fp64.  A mask fault -- a wrong stage or block in one of the places that
form mix_seed(seed, stage, blk), an element index that transposes h and w or forgets the batch offset, a forward and a backward
that disagree -- moves the results by 1e-1 or more (the negative control of test (a) measures it in every case); the gates are the
ones the dropout-off tests of the same entries hold, three orders of magnitude below that.

Power-of-two sides only (rectangles included: their FFT mixer runs Bluestein lines): on other sides the fp32 oracle itself sits
~1e-2 from the fp64 one with dropout on (pocketfft's mixed radix against the branch cut of angle()), so such a case could not
tell a fault from noise at these gates."""
import numpy as np
import pytest
import torch

from helpers import det_params, rel_l2
from oracle import detweights as dw
from oracle import lgteun_oracle as orc

pytestmark = pytest.mark.gpu
T = torch.from_numpy
M64 = (1 << 64) - 1

BLOCKS = ('encoder_layers.0.0.blocks.0.', 'encoder_layers.0.0.blocks.1.', 'bottleneck.blocks.0.', 'decoder_layers.0.2.blocks.0.',
          'decoder_layers.0.2.blocks.1.')
# right behind the mask (proj.bias), right in front of it (proj.weight) and the LayerNorm in front of the mixer, of every block ...
AROUND_THE_MASK = tuple(b + n for b in BLOCKS for n in ('0.fn.fn.proj.weight', '0.fn.fn.proj.bias', '0.fn.norm.weight'))
# ... and the pieces test_lgt_backward_vs_oracle lists
OUTSIDE_THE_BLOCKS = ('patch_embed.proj.0.weight', 'patch_embed.proj.1.weight', 'patch_embed.norm.weight', 'encoder_layers.0.1.1.weight',
                      'decoder_layers.0.0.1.weight', 'decoder_layers.0.1.weight', 'decoder_layers.0.1.bias', 'tail.1.weight', 'tail.1.bias')


def _oracle_lgt(C, K, stage, z, dy, masks):
    """fp64 oracle of one LGT and its autograd: (out, dz, {name: gradient})"""
    P = det_params(C, K, dtype=torch.float64, requires_grad=True)
    zz = z.double().requires_grad_(True)
    out = orc.lgt(P, f'prior_module.{stage}.', zz, drop_masks=masks, stage=stage)
    (out * dy.double()).sum().backward()
    return out.detach(), zz.grad, {n: v.grad for n, v in P.items() if v.grad is not None}


# (a) + (b) ----------------------------------------------------------------------------------------------------------------------
LGT_CASES = [(4, 16, 16, 5, 1234), (4, 16, 16, 5, 2 ** 63 + 77), (8, 16, 16, 1, 4321), (4, 32, 32, 2, 77), (8, 32, 32, 2, 78),
             (4, 32, 64, 3, 79), (8, 64, 32, 2, 80), (4, 64, 64, 2, 81)]     # (C, H, W, B, seed)


@pytest.mark.parametrize('C,H,W,B,seed', LGT_CASES)
def test_lgt_train_mode_vs_oracle_with_the_exported_masks(C, H, W, B, seed):
    """lg_op_lgt / lg_op_lgt_bwd with LG_FLAG_DROPOUT, stage 1 of a K = 2 module (a non-zero stage enters mix_seed), against the fp64
    oracle fed the masks lg_dropout_mask exports for the same seed.  Gates of the dropout-off test of the same entry
    (test_lgt_backward_vs_oracle): output 1e-4, dz 2e-4, the 119 parameter gradients 5e-4 globally, 2e-3 per tensor for the tensors
    around the mask in each of the five blocks and for the pieces outside the blocks; nothing outside stage 1's slots is written.
    Negative control: the oracle with the masks of seed + 1 must be MORE than 1e-2 away in output and dz (both sides fed from one
    wrong source would otherwise agree for ever).
    Measured on an MI355X over the eight cases: output 1.3 ... 1.9e-7 (dropout off: the same), dz 5.5e-7 ... 4.4e-6, parameter gradients
    4.8e-7 ... 3.4e-6, worst single tensor 1.1e-5; negative control: output 0.226 ... 0.235, dz 0.110 ... 0.152."""
    from gpu_helpers import Ops, make_module
    from lgteun_amd._lib import LG_FLAG_DROPOUT
    K, stage = 2, 1
    pre = f'prior_module.{stage}.'
    net = make_module(C, K)
    ops = Ops(net, H, W)
    rng = np.random.default_rng(C * 100 + H + 3 * W + B)
    z = T(rng.uniform(0, 1, (B, C, H, W)).astype(np.float32))
    dy = T(rng.standard_normal((B, C, H, W)).astype(np.float32))
    y = ops.lgt(stage, z.cuda(), LG_FLAG_DROPOUT, seed).cpu()
    dz, grads = ops.lgt_bwd(stage, z.cuda(), dy.cuda(), LG_FLAG_DROPOUT, seed)
    y_off = ops.lgt(stage, z.cuda()).cpu()
    dz, grads = dz.cpu(), grads.cpu()

    out, want_dz, g = _oracle_lgt(C, K, stage, z, dy, ops.dropout_masks(seed))
    names = [n for n in g if n.startswith(pre)]
    assert len(names) == 119 and len(g) == 119
    with torch.no_grad():
        P64 = det_params(C, K, dtype=torch.float64)
        e_off = rel_l2(y_off, orc.lgt(P64, pre, z.double()))
    e_out, e_dz = rel_l2(y, out), rel_l2(dz, want_dz)
    num = sum(float(((ops.grad_of(grads, n).double() - g[n]) ** 2).sum()) for n in names)
    den = sum(float((g[n] ** 2).sum()) for n in names)
    e_g = (num / den) ** 0.5
    per = {n: rel_l2(ops.grad_of(grads, pre + n), g[pre + n]) for n in AROUND_THE_MASK + OUTSIDE_THE_BLOCKS}
    worst = max(per, key=per.get)
    # (b) the masks of another seed
    out_n, dz_n, _ = _oracle_lgt(C, K, stage, z, dy, ops.dropout_masks((seed + 1) & M64))
    n_out, n_dz = rel_l2(y, out_n), rel_l2(dz, dz_n)
    print(f'lgt train mode C={C} {H}x{W} B={B} seed={seed}: out {e_out:.2e} (gate 1e-4; dropout off {e_off:.2e})  dz {e_dz:.2e} (2e-4)  '
          f'grads {e_g:.2e} (5e-4)  worst tensor {worst} {per[worst]:.2e} (2e-3)  |  masks of seed + 1: out {n_out:.2e} dz {n_dz:.2e} (> 1e-2)')
    assert not torch.equal(y, y_off)
    assert e_out < 1e-4, e_out
    assert e_dz < 2e-4, e_dz
    assert e_g < 5e-4, e_g
    for n, e in per.items():
        assert e < 2e-3, (n, e)
    touched = torch.zeros_like(grads, dtype=torch.bool)
    for n in names:
        i = ops.eng.names.index(n)
        touched[ops.eng.offsets[i]:ops.eng.offsets[i] + ops.eng.params[i].numel()] = True
    assert float(grads[~touched].abs().max()) == 0.0           # nothing outside stage 1's slots is written
    assert n_out > 1e-2 and n_dz > 1e-2, (n_out, n_dz)


# (c) + (e) ----------------------------------------------------------------------------------------------------------------------
def _recorded_train_step(net, ms, pan, gt):
    """one Engine.train_step (dropout on, lr = 0) through the production route; returns (loss, seed the engine drew, its output)"""
    from lgteun_amd import FusedAdam
    from lgteun_amd._lib import LG_FLAG_DROPOUT
    opt = FusedAdam(net.parameters(), lr=0.0)
    opt.dropout = True
    eng = net.engine()
    rec = {'seeds': []}
    real_seed, real_fwd = eng.next_seed, eng.forward_raw

    def next_seed():
        rec['seeds'].append(real_seed())
        return rec['seeds'][-1]

    def forward_raw(ms_, pan_, flags, seed=0, lease=False):
        out, saved = real_fwd(ms_, pan_, flags, seed, lease)
        rec['out'], rec['flags'], rec['fwd_seed'] = out.clone(), flags, seed
        return out, saved
    eng.next_seed, eng.forward_raw = next_seed, forward_raw
    try:
        loss = float(eng.train_step(ms.cuda(), pan.cuda(), gt.cuda(), opt).item())
    finally:
        del eng.next_seed, eng.forward_raw
    assert len(rec['seeds']) == 1 and rec['fwd_seed'] == rec['seeds'][0] and rec['flags'] & LG_FLAG_DROPOUT
    return loss, rec['seeds'][0], rec['out'].cpu()


def _train_step_vs_oracle(C, K, H, B, mode, precision='fp32'):
    """(e_out, e_cpu32, loss, loss_ref, e_grad) of one recorded train step against orc.forward(drop_masks) + l1_loss in fp64"""
    from gpu_helpers import device_drop_masks, make_module
    ms, pan, gt = (T(a) for a in dw.make_inputs(B, C, H // 4, H // 4, seed=500 + H + B + K, kind='smooth'))
    net = make_module(C, K)
    net.mode = mode
    net.precision = precision
    loss, seed, y = _recorded_train_step(net, ms, pan, gt)
    eng = net.engine()
    P = det_params(C, K, dtype=torch.float64, requires_grad=True)
    want = orc.forward(P, ms.double(), pan.double(), K, mode=mode, drop_masks=device_drop_masks(seed))
    with torch.no_grad():
        # dead stages' masks never reach the output (tests/test_dropout_oracle_cpu.py): 'live' is 'faithful' here
        got32 = orc.forward(det_params(C, K), ms, pan, K, mode='live' if mode == 'faithful' else mode,
                            drop_masks=device_drop_masks(seed, torch.float32))
        e_cpu32 = rel_l2(got32, want.detach())
    loss_ref = orc.l1_loss(want, gt.double())
    loss_ref.backward()
    live = [eng.names[i] for i in eng.live_idx]
    assert sorted(live) == sorted(n for n, v in P.items() if v.grad is not None)
    assert len(live) == (len(eng.names) if mode == 'chained' else 12 + K + 119)
    num = den = 0.0
    for i in eng.live_idx:
        n, o, p = eng.names[i], eng.offsets[i], eng.params[i]
        got = eng.gflat[o:o + p.numel()].view(p.shape).cpu().double()
        num += float(((got - P[n].grad) ** 2).sum())
        den += float((P[n].grad ** 2).sum())
    if mode == 'faithful':
        a, b = eng.live_ranges[0][1], eng.live_ranges[1][0]
        assert b > a and float(eng.gflat[a:b].abs().max()) == 0.0        # dead-stage slots: never written
    else:
        g0 = [eng.gflat[o:o + p.numel()] for n, o, p in zip(eng.names, eng.offsets, eng.params) if n.startswith('prior_module.0.')]
        assert float(torch.cat(g0).abs().max()) > 0.0
    return rel_l2(y, want.detach()), e_cpu32, loss, float(loss_ref.detach()), (num / den) ** 0.5


STEP_CASES = [('faithful', 4, 2, 32, 3), ('faithful', 8, 2, 32, 2), ('faithful', 4, 3, 64, 2),
              ('chained', 4, 2, 32, 3), ('chained', 8, 2, 64, 2), ('chained', 4, 3, 64, 2)]     # (mode, C, K, PAN, B)


@pytest.mark.parametrize('mode,C,K,H,B', STEP_CASES)
def test_train_step_with_dropout_vs_oracle(mode, C, K, H, B):
    """Engine.train_step with opt.dropout = True and lr = 0, the seed it drew recorded from eng.next_seed: loss and every live gradient
    against orc.forward(drop_masks = the export of that seed) + l1_loss in fp64.  In 'faithful' mode only the last stage's masks reach
    the output; in 'chained' mode every stage's do, so a wrong stage index in any mix_seed shows there.  Gates of these routes
    (test_gpu_chained.py): output max(1e-3, 2 x e_cpu32), e_cpu32 = the fp32 oracle's distance from the fp64 one on the same inputs
    and masks; loss 1e-4; gradient 5e-3 globally; dead-stage slots exactly zero in faithful mode.
    Measured on an MI355X, in the order of STEP_CASES: output 1.6e-7, 2.1e-7, 1.3e-7, 2.0e-7, 1.2e-5, 1.5e-7 with e_cpu32 (the oracle on that box's host
    CPU) 1.5e-7, 1.9e-7, 1.3e-7, 2.0e-7, 6.8e-6, 4.3e-4 (the last one a branch-cut flip of the fp32 oracle's own); loss equal to 1e-6; gradient
    1.3e-7, 2.4e-7, 1.8e-7, 1.7e-7, 7.6e-6, 1.9e-7.  No case needed the 2 x e_cpu32 arm of the gate."""
    e_out, e_cpu32, loss, loss_ref, e_g = _train_step_vs_oracle(C, K, H, B, mode)
    print(f'train step {mode} C={C} K={K} {H}x{H} B={B}: out {e_out:.2e} (gate max(1e-3, 2 x e_cpu32 = {2 * e_cpu32:.2e}))  '
          f'loss {loss:.6f} / {loss_ref:.6f} (1e-4)  grads {e_g:.2e} (5e-3)')
    assert e_out < max(1e-3, 2 * e_cpu32), (e_out, e_cpu32)
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref)), (loss, loss_ref)
    assert e_g < 5e-3, e_g


def test_live_mode_gives_bitwise_the_faithful_gradients_with_dropout_on():
    from gpu_helpers import make_module
    C, K, H, B = 4, 2, 32, 3
    ms, pan, gt = (T(a) for a in dw.make_inputs(B, C, H // 4, H // 4, seed=500 + H + B + K, kind='smooth'))
    res = {}
    for mode in ('faithful', 'live'):
        net = make_module(C, K)
        net.mode = mode
        loss, seed, y = _recorded_train_step(net, ms, pan, gt)      # a fresh engine each: the same step counter, so the same seed
        res[mode] = (loss, seed, y, net.engine().gflat.clone())
    assert res['faithful'][1] == res['live'][1]
    assert torch.equal(res['faithful'][2], res['live'][2]) and torch.equal(res['faithful'][3], res['live'][3])
    assert float(res['live'][3].abs().max()) > 0
    assert abs(res['faithful'][0] - res['live'][0]) <= 1e-6 * abs(res['live'][0])    # the logged scalar is summed with float atomics


def test_bf16_train_step_with_dropout_vs_oracle():
    """precision = 'bf16' with dropout on: case (4, 2, 32, 3) of the faithful train step, at the gates of
    test_bf16_mode_at_the_measured_sizes against the fp64 oracle with the exported masks: output 1e-2, loss 2e-3, gradient 2e-2.
    Measured on an MI355X: output 2.3e-3, loss 1.05e-3 (0.407879 against 0.408309), gradient 2.5e-3."""
    e_out, e_cpu32, loss, loss_ref, e_g = _train_step_vs_oracle(4, 2, 32, 3, 'faithful', precision='bf16')
    print(f'bf16 train step with dropout: out {e_out:.2e} (gate 1e-2)  loss {loss:.6f} / {loss_ref:.6f} (2e-3)  grads {e_g:.2e} (2e-2)')
    assert e_out < 1e-2, e_out
    assert abs(loss - loss_ref) < 2e-3 * abs(loss_ref), (loss, loss_ref)
    assert e_g < 2e-2, e_g


# (d) ----------------------------------------------------------------------------------------------------------------------------
def test_lgt_train_mode_at_the_measured_shape():
    """One LGT in train mode at the shape bench.py measures: C = 4, 128 x 128, 32 pairs -- the only shape at which the e = 16 kernels
    take their uneven workgroup partitions.  The per-op entries run the same lgt_fwd / lgt_bwd and the same launchers as
    lgteun_forward / lgteun_backward, and every launcher decides from the shape alone, so lg_op_lgt / lg_op_lgt_bwd take them here:
      k_ffn_xr       (launch_ffn_xr: 512 strips of 64 rows, dS = 16): strip_geo gives rows 0 .. 79 of EVERY sample to a workgroup of the
                     first half of the grid and rows 80 .. 127 to one of the second half (10 : 6 steps);
      k_attn_m       (512 workgroups, 2048 window quads, uneven = 5): first-half workgroups walk quads 0 .. 1279 = samples 0 .. 19, second-half
                     ones quads 1280 .. 2047 = samples 20 .. 31 (5 : 3);
      k_ffn1_bwd_xs  (512 workgroups, 8192 tiles of 64 pixels, uneven = 9): first-half workgroups walk tiles 0 .. 4607 = samples 0 .. 17,
                     second-half ones tiles 4608 .. 8191 = samples 18 .. 31 (9 : 7).
    Out and dz are per-sample results: samples 0 (first half of both), 17 (the last one of k_ffn1_bwd_xs' first half), 20 (the first one of
    k_attn_m's second half; second half of both) and 31 (the last one) of the 32-pair call against the fp64 oracle run on those four
    alone, each with its own slice of the batch's masks.  Four is what the oracle's CPU time allows (about 1 s per sample); parameter
    gradients at this shape stay with the linearity and half-batch tests.  Gates: output 1e-4, dz 2e-4.
    Measured on an MI355X: output 1.3e-7 for each of the four; dz 8.1e-7, 6.1e-7, 9.7e-7, 3.9e-7."""
    from gpu_helpers import Ops, make_module
    from lgteun_amd._lib import LG_FLAG_DROPOUT
    C, K, stage, H, B, seed = 4, 2, 1, 128, 32, 2024
    pick = [0, 17, 20, 31]
    ops = Ops(make_module(C, K), H, H)
    rng = np.random.default_rng(128 + B)
    z = T(rng.uniform(0, 1, (B, C, H, H)).astype(np.float32))
    dy = T(rng.standard_normal((B, C, H, H)).astype(np.float32))
    y = ops.lgt(stage, z.cuda(), LG_FLAG_DROPOUT, seed).cpu()
    dz, _ = ops.lgt_bwd(stage, z.cuda(), dy.cuda(), LG_FLAG_DROPOUT, seed)
    dz = dz.cpu()
    whole = ops.dropout_masks(seed, torch.float32)

    def masks(st, blk, B_, h, w, e):
        assert B_ == len(pick)
        return whole(st, blk, B, h, w, e)[pick].double()
    out, want_dz, _ = _oracle_lgt(C, K, stage, z[pick], dy[pick], masks)
    errs = [(b, rel_l2(y[b], out[i]), rel_l2(dz[b], want_dz[i])) for i, b in enumerate(pick)]
    print('lgt train mode 128x128 B=32, per sample (out, gate 1e-4; dz, gate 2e-4): ' + '  '.join(f'{b}: {eo:.2e} {ed:.2e}' for b, eo, ed in errs))
    for b, eo, ed in errs:
        assert eo < 1e-4 and ed < 2e-4, (b, eo, ed)
