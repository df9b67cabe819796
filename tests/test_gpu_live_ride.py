"""-m gpu: the live stage riding in the dead pass's plane and pixel launches (include/lgteun_hip.h: LG_FLAG_LIVE_APART; k_fwd.hip: lgt_fwd, live_out).

A faithful forward on a plan that batches its dead stages launches k_embed, k_fftmix_r, k_down, k_upfuse and k_tail ONCE over K B samples -- stages
0 .. K-2 dead, stage K-1 live and the only one that saves -- and the persistent k_attn_m / k_ffn_xr / k_ffn_x32 twice, as before.  LG_FLAG_LIVE_APART keeps
the dead pass and the live pass apart: the reference of every comparison here, which is BITWISE (same kernels, same arithmetic, same order of every sum:
the parameter-gradient reductions of the backward are deterministic).  Every run uses a guarded workspace of exactly lg_workspace_bytes, filled with NaN
bytes before the run, and dropout on.

Shapes (C = 4, faithful), the smallest that reach each risk:
  K = 3, B = 1, 16 x 16    two dead stages + live, one window row per level, level-1 planes of 8 x 8.  (A 16 x 16 plan has one level-1 window per sample,
                           no whole window quad per stage: lg_plan_stage_batch declines it, so this case pins that the flag changes nothing on a plan that
                           keeps one slot.)
  K = 3, B = 2, 32 x 32    the smallest plan that DOES batch: the ride-along itself at k_fftmix_r<5,.> / <4,.>
  K = 4, B = 3, 64 x 64    odd B: stage boundaries inside the persistent kernels' runs, k_fftmix_r<6,.> and <5,.>, the save bound (sample 9) at no multiple of
                           anything
  K = 4, B = 9, 128 x 128  288 planes per stage > 256 CUs: k_fftmix_r<7,512> with the saving planes in its last round; level-1 <6,512>
"""
import ctypes

import pytest
import torch

from test_gpu_workspace_contract import BWD_DATA, BWD_LGT, DEFER_DEAD, DROPOUT, FAITHFUL, SAVE, STAGEWISE, Net, _bits, _same

pytestmark = pytest.mark.gpu

LIVE_APART = 256
SEED = 0x11FE57A6
CASES = [(3, 1, 16), (3, 2, 32), (4, 3, 64), (4, 9, 128)]


def test_the_flag_is_the_header_s():
    from lgteun_amd import _lib
    assert _lib.LG_FLAG_LIVE_APART == LIVE_APART


def _deadout_region(net):
    off, stride = ctypes.c_size_t(), ctypes.c_size_t()
    assert net.lib.lg_workspace_deadout(net.plan, net.B, net.train, ctypes.byref(off), ctypes.byref(stride)) == 0
    n = (net.K - 1 if stride.value else 1) * net.B * net.C * net.H * net.W * 4
    assert off.value + n <= net.need
    return off.value, n


def _loss_dout(out, gt):
    """what an l1 loss hands the backward: depends on the forward's own output"""
    return (torch.sign(out - gt) / out.numel()).contiguous()


def _step(net, inp, gt, extra, second=False):
    """NaN-filled workspace, saving forward, backward on the fixed dout, then ANOTHER backward on the same forward with the loss-side dout"""
    ms, pan, dout = inp
    flags = FAITHFUL | DROPOUT | SAVE | extra
    net.fill('nan')
    rc, out = net.forward(ms, pan, flags, SEED)
    assert rc == 0, net.lib.lg_last_error()
    off, n = _deadout_region(net)
    got = {'out': out.clone(), 'deadout': net.ws[off:off + n].clone()}
    assert net.backward(ms, pan, dout, flags, SEED) == 0, net.lib.lg_last_error()
    got['grads'] = net.grads.clone()
    assert net.backward(ms, pan, _loss_dout(out, gt), flags, SEED) == 0, net.lib.lg_last_error()
    got['grads_loss'] = net.grads.clone()
    if second:      # and the first one again: a backward leaves the saved forward as it found it
        assert net.backward(ms, pan, dout, flags, SEED) == 0, net.lib.lg_last_error()
        got['grads_again'] = net.grads.clone()
    net.guards('step')
    return got


def _assert_same(tag, ref, got):
    for k in ref:
        v = got[k].view(torch.float32) if k == 'deadout' else got[k]
        assert bool(torch.isfinite(v).all()), (tag, k, 'not finite')
        nd = int((_bits(ref[k]) != _bits(got[k])).sum()) if ref[k].shape == got[k].shape else -1
        assert _same(ref[k], got[k]), (tag, k, nd, 'of', ref[k].numel(), 'words differ')


def _case(K, B, n):
    net = Net(4, K, n, n, B, 1)
    inp = net.inputs(5)
    gt = net.inputs(7)[2]
    return net, inp, gt


@pytest.mark.parametrize('K,B,n', CASES)
def test_ride_along_gives_the_bits_of_the_passes_kept_apart(K, B, n):
    net, inp, gt = _case(K, B, n)
    apart = _step(net, inp, gt, LIVE_APART)
    ride = _step(net, inp, gt, 0, second=True)
    assert float(ride['grads'].norm()) > 0 and float(ride['grads_loss'].norm()) > 0
    _assert_same(f'K={K} B={B} {n}x{n} ride-along vs apart', apart, {k: ride[k] for k in apart})
    assert _same(ride['grads'], ride['grads_again']), 'a second backward on one forward moved the gradients'
    stagewise = _step(net, inp, gt, STAGEWISE)      # the live stage alone in slot K-1, the dead ones one by one in slot 0
    _assert_same(f'K={K} B={B} {n}x{n} stage-wise vs apart', apart, stagewise)


def test_eval_forward_rides_along_too():
    """train = 0, no dropout, nothing saved: the faithful inference forward of (4, 3, 64) = the stage-wise call, output and last dead output bitwise"""
    K, B, n = 4, 3, 64
    net = Net(4, K, n, n, B, 0)
    ms, pan, _ = net.inputs(5)
    got = {}
    for name, extra in (('ride', 0), ('apart', LIVE_APART), ('stagewise', STAGEWISE)):
        net.fill('nan')
        rc, out = net.forward(ms, pan, FAITHFUL | extra, 0)
        assert rc == 0, net.lib.lg_last_error()
        got[name] = out.clone()
        assert bool(torch.isfinite(out).all()), name
    assert _same(got['ride'], got['stagewise']) and _same(got['ride'], got['apart'])


def test_deferred_dead_stages_give_the_ride_along_s_bits():
    """(4, 3, 64): forward with LG_FLAG_DEFER_DEAD (the live stage alone, in slot K-1), backward LG_FLAG_BWD_LGT, lgteun_dead_forward (slots 0 .. K-2: it no
    longer runs over the live stage's buffers), backward LG_FLAG_BWD_DATA = the one-call ride-along: out, dead outputs, gradients"""
    K, B, n = 4, 3, 64
    net, inp, gt = _case(K, B, n)
    ms, pan, dout = inp
    ride = _step(net, inp, gt, 0)
    flags = FAITHFUL | DROPOUT | SAVE | DEFER_DEAD
    net.fill('nan')
    rc, out = net.forward(ms, pan, flags, SEED)
    assert rc == 0, net.lib.lg_last_error()
    assert net.backward(ms, pan, dout, flags | BWD_LGT, SEED) == 0, net.lib.lg_last_error()
    assert net.dead_forward(flags, SEED) == 0, net.lib.lg_last_error()
    assert net.backward(ms, pan, dout, flags | BWD_DATA, SEED, zero=False) == 0, net.lib.lg_last_error()
    off, nb = _deadout_region(net)
    split = {'out': out.clone(), 'deadout': net.ws[off:off + nb].clone(), 'grads': net.grads.clone()}
    _assert_same('deferred dead stages vs ride-along', {k: ride[k] for k in split}, split)
