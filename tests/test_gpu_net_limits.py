"""-m gpu: the ACCEPTED side of the network entries' argument contract (include/lgteun_hip.h; tests/test_net_abi_cpu.py holds the rejected side on the
host): the batch bound B_max = min(floor(65535 / C), floor((2^31 - 1) / (S 16 C H W))) run on the device, the plan extremes, and inputs that are not
16-byte aligned through the Python layer.  Nothing here calls a launcher with a rejected argument, and nothing launches above the bound.

The smallest plan, PAN 16 x 16, is where the bound is cheapest to reach: 16383 samples of C = 4 and 8191 of C = 8 put 65532 / 65528 planes into the
z dimension of the data step's tile launches, one workgroup each.  Inputs are uniform random numbers drawn on the device, so every sample is
distinct; every case asserts that its probe samples (first, middle, last) differ from the samples 65536 / C, 65536 / e (e = 4 C, 8 C) and 2^16
positions away in every tensor of the call -- a plane or sample index that wrapped at 16 bits would land on one of those and cannot go unseen.  Every
case runs inside limits_helpers.Measured (prints seconds and peak memory, asserts the 16 GiB limit) and frees what it allocated.

  (a) lgteun_forward at the bound: C = 4 K = 1 (B = 16383), C = 8 K = 1 (B = 8191), C = 4 K = 3 faithful (B = 16383).  Every sample of `out` bit for
      bit the same sample run in a batch of 32; samples first / middle / last against the fp64 oracle at 1e-4 relative L2 (the whole-net gate of
      tests/test_gpu_forward.py: test_edge_shapes_vs_oracle).  A 16 x 16 plan does not run its dead stages as one pass (one window quad per sample is
      not whole: api.hip lg_plan_stage_batch; lg_workspace_deadout reports stage stride 0, asserted), and the smallest plan that does, 32 x 32, needs
      36 GiB at its bound of 10922.  So the one-pass case is 32 x 32, K = 3, B = 4096 (13.5 GiB): (K - 1) B = 8192 dead and B live samples ride in
      one launch of the plane and pixel kernels, 98304 planes in the FFT mixer's grid; lg_workspace_deadout's stage stride (B C H W floats) is the
      assertion that the plan batches -- lg_plan_describe does not print it.
  (b) lg_op_data_step_bwd and lg_op_lgt_bwd at B = 6016, the largest multiple of 32 whose train workspace (13.3 GiB) leaves room under 16 GiB (the
      bound's 36 GiB does not fit).  dz_in of the data step bit for bit batches of 32.  dz of the LGT is NOT bitwise batch independent, by design:
      k_ffn1_bwd_xs scales its f16 pairs by max |dh2| over the whole batch (tests/test_gpu_backward_shapes.py says so and claims none); it is held, per
      sample, to that file's LGT gate, 2e-4 relative L2, against the batch-of-32 result, and samples first / middle / last to the same gate against
      autograd over the fp64 oracle.  Parameter gradients: against the float64 sum of the 188 chunk gradients, tensor by tensor, err = max |got - sum64|
      / max |sum64| at that file's per-family bars G (FFN 1e-4, local mixer 1e-4 / 1.1e-4 at level 1, global mixer 4.2e-4, LGT level 1.5e-4; data step 2e-5
      relative L2).  Where the fp32 batch reduction's own rounding passes a bar, the yardstick is the distance of a SEQUENTIAL fp32 sum of the chunk
      gradients from their fp64 sum, and twice that is allowed; the test prints both figures for every tensor that needs it.
  (c) one whole train step, lgteun_forward(LG_FLAG_SAVE | LG_FLAG_FAITHFUL) + lgteun_backward, C = 4, K = 2, B = 6016: out bit for bit batches of 32, the
      flat gradient buffer by the rule of (b), the dead stage's slots exactly zero.
  (d) plan extremes: K = 16 (LG_MAX_K) at 16 x 16, B = 2, both widths, and PAN 16 x 1024 / 1024 x 16 at K = 1: forward, loss and gradients against the
      fp64 oracle by tests/test_gpu_anysize.py's whole-net check, unchanged (1e-3 / 1e-4 / 5e-3).  No existing test runs K > 8 or a side of 1024.
  (e) ms, pan, gt and dout as contiguous views that start 4 bytes into a larger storage: Engine.forward_raw, Engine.backward_raw and
      Engine.train_step (l1) give the bits of the aligned tensors, and the caller's storage keeps its bits.

Measured on an MI355X (the file: 11 tests in 7.8 s, the slowest 1.2 s; nothing was wrong at the bound):
  (a) bitwise equal to the batches of 32 in all four cases; fp64 oracle on samples first / middle / last, gate 1e-4:
        C=4 K=1 B=16383  1.29e-07   0.36 s   5.43 GiB peak        C=8 K=1 B=8191            3.56e-07   0.12 s    5.42 GiB
        C=4 K=3 B=16383  1.39e-07   0.39 s   5.63 GiB             C=4 K=3 32 x 32 B=4096    1.22e-07   0.15 s   13.69 GiB
  (b) B = 6016, 1.17 s, 13.97 GiB peak.  Data step: dz_in bitwise; 13 gradient tensors, worst 1.53e-06 relative L2 (R.bias) = 0.08 of 2e-5; the
      sequential fp32 sum of the 188 chunk gradients lies 2.84e-07 from their fp64 sum.  LGT: dz against the batches of 32 at most 6.41e-08 per sample
      (gate 2e-4: the batch-wide max |dh2| scale of k_ffn1_bwd_xs moves last bits only), against fp64 autograd 1.15e-06 (gate 2e-4); 119 gradient tensors,
      worst 2.73e-06 = 0.03 of its bar 1e-4 (decoder block 0 FFN net.4.weight; sequential fp32 sum 3.11e-07).  No tensor needed the yardstick.
  (c) B = 6016, 0.28 s, 13.95 GiB peak: out bitwise; 133 live gradient tensors, worst 5.84e-06 = 0.06 of its bar 1e-4 (stage 1 decoder block 1 FFN
      net.0.weight; sequential fp32 sum 4.06e-07); the 119 dead-stage tensors exactly zero.
  (d) K = 16: 1.16 s (C = 4), 0.63 s (C = 8); 16 x 1024: 0.28 s; 1024 x 16: 0.24 s -- most of it the fp64 oracle's autograd on the host.
  (e) 0.13 s."""
import pytest
import torch

from helpers import det_params, rel_l2
from limits_helpers import F_FAITHFUL, F_SAVE, GIB, Measured, memory_gate, net_max_batch, same_bits
from oracle import lgteun_oracle as orc

pytestmark = pytest.mark.gpu

CHUNK = 32
B_TRAIN = 6016           # 188 x 32: lg_workspace_bytes(16 x 16, C = 4, train = 1) is 13.3 GiB there


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: -m gpu tests must run on the MI355X box')
    return torch.device('cuda')


def device_inputs(B, C, H, W, seed):
    """ms [B,C,H/4,W/4], pan [B,1,H,W], dout [B,C,H,W]: uniform on the device, every sample distinct"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    ms = torch.rand(B, C, H // 4, W // 4, device='cuda', generator=g)
    pan = torch.rand(B, 1, H, W, device='cuda', generator=g)
    dout = torch.rand(B, C, H, W, device='cuda', generator=g) - 0.5
    return ms, pan, dout


def assert_probes_distinct(C, tensors, what):
    """samples first / middle / last differ from the samples 65536 / C, 65536 / e and 2^16 positions away, in every tensor given"""
    for name, t in tensors.items():
        B = t.shape[0]
        for s in (0, B // 2, B - 1):
            for d in (65536 // C, 65536 // (4 * C), 65536 // (8 * C), 65536):
                for o in (s - d, s + d):
                    if 0 <= o < B:
                        assert not torch.equal(t[s], t[o]), (what, name, s, o)


def chunks(B):
    return [(a, min(a + CHUNK, B)) for a in range(0, B, CHUNK)]


def oracle_forward(C, K, ms, pan, idx, mode):
    P = det_params(C, K, dtype=torch.float64)
    with torch.no_grad():
        return orc.forward(P, ms[idx].cpu().double(), pan[idx].cpu().double(), K, mode=mode)


# ------------------------------------------------------------------------------------------------------------------------
# (a) inference at the bound
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,K,N,B,one_pass', [(4, 1, 16, None, False), (8, 1, 16, None, False), (4, 3, 16, None, False), (4, 3, 32, 4096, True)],
                         ids=['C4-K1-bound', 'C8-K1-bound', 'C4-K3-faithful-bound', 'C4-K3-faithful-one-pass'])
def test_forward_at_the_bound_is_bitwise_batches_of_32(gpu, C, K, N, B, one_pass):
    import ctypes
    from gpu_helpers import make_module
    bound = net_max_batch(C, K, N, N, 0)
    B = bound if B is None else B
    assert B <= bound
    eng = make_module(C, K).engine()
    plan = eng.plan(N, N)
    need = int(eng.lib.lg_workspace_bytes(plan, B, 0))
    assert need > 0 and int(eng.lib.lg_workspace_bytes(plan, bound, 0)) > 0 and int(eng.lib.lg_workspace_bytes(plan, bound + 1, 0)) == 0
    memory_gate(need + GIB)
    off, stride = ctypes.c_size_t(), ctypes.c_size_t()
    assert eng.lib.lg_workspace_deadout(plan, B, 0, ctypes.byref(off), ctypes.byref(stride)) == 0
    assert (stride.value == B * C * N * N * 4) == one_pass and (stride.value == 0) != one_pass, (stride.value, one_pass)
    flags = F_FAITHFUL if K > 1 else 0
    with Measured(f'forward C={C} K={K} {N}x{N} B={B} ({need / GIB:.2f} GiB workspace)'):
        ms, pan, _ = device_inputs(B, C, N, N, seed=100 * C + K)
        out, _ = eng.forward_raw(ms, pan, flags)
        assert_probes_distinct(C, dict(ms=ms, pan=pan, out=out), 'forward')
        assert bool(torch.isfinite(out).all())
        bad = []
        for a, b in chunks(B):
            part, _ = eng.forward_raw(ms[a:b], pan[a:b], flags)
            if not torch.equal(part, out[a:b]):
                bad.append(a + int((part != out[a:b]).flatten(1).any(1).nonzero()[0]))
        assert not bad, ('samples whose bits differ from their batch of 32', len(bad), bad[:8])
        idx = [0, B // 2, B - 1]
        want = oracle_forward(C, K, ms, pan, idx, 'faithful' if K > 1 else 'live')
        err = rel_l2(out[idx].cpu(), want)
        print(f'[net limits] forward C={C} K={K} {N}x{N} B={B}: bitwise batches of 32, samples {idx} vs fp64 oracle {err:.2e} (gate 1e-4)')
        assert err < 1e-4, err
        del out, ms, pan, part
        eng._ws.clear()


# ------------------------------------------------------------------------------------------------------------------------
# (b), (c): gradients of a large batch against the float64 sum of its chunks
# ------------------------------------------------------------------------------------------------------------------------
def family_bar(name):
    """tests/test_gpu_backward_shapes.py's per-family G; None: a data-step tensor (2e-5 relative L2)"""
    if not name.startswith('prior_module.'):
        return None
    if 'blocks.' not in name:
        return 1.5e-4                                  # LGT level: patch embedding, down, up, fusion, tail
    if 'global_mixer' in name:
        return 4.2e-4
    if 'bottleneck' in name and '.0.fn.' in name:
        return 1.1e-4                                  # e >= 32 local tensors
    return 1e-4                                        # FFN, k_attn_bwd_f's local tensors


def assert_grads_match_chunk_sum(eng, got, sum64, seq32, idxs, what):
    """tensor by tensor at the bars of family_bar; the sequential-fp32-sum yardstick (twice it) where the reduction's own rounding passes a bar"""
    worst = (0.0, None)
    for i in idxs:
        n, o, p = eng.names[i], eng.offsets[i], eng.params[i]
        g, s, q = got[o:o + p.numel()].double(), sum64[o:o + p.numel()], seq32[o:o + p.numel()].double()
        bar = family_bar(n)
        if bar is None:
            err, yard, bar = float((g - s).norm() / s.norm()), float((q - s).norm() / s.norm()), 2e-5
        else:
            err, yard = float((g - s).abs().max() / s.abs().max()), float((q - s).abs().max() / s.abs().max())
        if err > bar:
            print(f'[net limits] {what} {n}: err {err:.2e} over its bar {bar:.1e}; sequential fp32 sum of the chunks {yard:.2e}, allowed {2 * yard:.2e}')
        assert err <= max(bar, 2 * yard), (what, n, err, bar, yard)
        if err / bar > worst[0]:
            worst = (err / bar, n, err, bar, yard)
    print(f'[net limits] {what}: {len(idxs)} gradient tensors, worst {worst[2]:.2e} = {worst[0]:.2f} of its bar {worst[3]:.1e} ({worst[1]}; sequential fp32 sum {worst[4]:.2e})')


def test_backward_ops_at_a_large_batch_match_batches_of_32(gpu):
    from gpu_helpers import Ops, make_module
    C, K, N, B = 4, 1, 16, B_TRAIN
    assert B <= net_max_batch(C, K, N, N, 1)
    net = make_module(C, K)
    ops = Ops(net, N, N)
    eng = ops.eng
    need = int(eng.lib.lg_workspace_bytes(ops.plan, B, 1))
    memory_gate(need + GIB)
    names = eng.names
    with Measured(f'backward ops C={C} K={K} {N}x{N} B={B} ({need / GIB:.2f} GiB workspace)'):
        ms, pan, dy = device_inputs(B, C, N, N, seed=7)
        z = torch.rand(B, C, N, N, device='cuda', generator=torch.Generator(device='cuda').manual_seed(8))
        assert_probes_distinct(C, dict(ms=ms, pan=pan, dy=dy, z=z), 'backward ops')
        dstep = [i for i, n in enumerate(names) if not n.startswith('prior_module.')]
        lgt = [i for i, n in enumerate(names) if n.startswith('prior_module.0.')]
        for op, idxs in (('data_step_bwd', dstep), ('lgt_bwd', lgt)):
            run = (lambda a, b: ops.data_step_bwd(0, z[a:b], ms[a:b], pan[a:b], dy[a:b])) if op == 'data_step_bwd' else (lambda a, b: ops.lgt_bwd(0, z[a:b], dy[a:b]))
            dz, g = run(0, B)
            assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(g).all())
            sum64, seq32, worst = torch.zeros_like(g, dtype=torch.float64), torch.zeros_like(g), 0.0
            for a, b in chunks(B):
                dzc, gc = run(a, b)
                sum64 += gc.double()
                seq32 += gc
                if op == 'data_step_bwd':
                    assert torch.equal(dzc, dz[a:b]), (op, 'dz_in differs from its batch of 32', a)
                else:                                  # k_ffn1_bwd_xs: batch-wide max |dh2| scale -> the LGT gate per sample, not bits
                    e = ((dz[a:b] - dzc).double().flatten(1).norm(dim=1) / dzc.double().flatten(1).norm(dim=1)).max()
                    worst = max(worst, float(e))
            if op == 'lgt_bwd':
                print(f'[net limits] lgt_bwd dz at B={B} vs batches of 32: worst sample {worst:.2e} relative L2 (gate 2e-4; k_ffn1_bwd_xs scales by the batch-wide max |dh2|)')
                assert worst < 2e-4, worst
                idx = [0, B // 2, B - 1]
                P = det_params(C, K, dtype=torch.float64)
                zz = z[idx].cpu().double().requires_grad_(True)
                orc.lgt(P, 'prior_module.0.', zz).backward(dy[idx].cpu().double())
                err = rel_l2(dz[idx].cpu(), zz.grad)
                print(f'[net limits] lgt_bwd dz samples {idx} vs fp64 autograd: {err:.2e} (gate 2e-4)')
                assert err < 2e-4, err
            assert_grads_match_chunk_sum(eng, g, sum64, seq32, idxs, f'{op} B={B}')
            del dz, g, sum64, seq32
        eng._ws.clear()


def test_train_step_at_a_large_batch_matches_batches_of_32(gpu):
    from gpu_helpers import make_module
    C, K, N, B = 4, 2, 16, B_TRAIN
    assert B <= net_max_batch(C, K, N, N, 1)
    eng = make_module(C, K).engine()
    plan = eng.plan(N, N)
    need = int(eng.lib.lg_workspace_bytes(plan, B, 1))
    memory_gate(need + GIB)
    flags = F_FAITHFUL | F_SAVE
    with Measured(f'train step C={C} K={K} {N}x{N} B={B} ({need / GIB:.2f} GiB workspace)'):
        ms, pan, dout = device_inputs(B, C, N, N, seed=11)
        g = torch.zeros_like(eng.flat)
        out, saved = eng.forward_raw(ms, pan, flags)
        eng.backward_raw(saved, dout, g, flags)
        assert_probes_distinct(C, dict(ms=ms, pan=pan, dout=dout, out=out), 'train step')
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
        sum64, seq32, gc = torch.zeros_like(g, dtype=torch.float64), torch.zeros_like(g), torch.zeros_like(g)
        for a, b in chunks(B):
            part, sv = eng.forward_raw(ms[a:b], pan[a:b], flags)
            assert torch.equal(part, out[a:b]), ('out differs from its batch of 32', a)
            gc.zero_()
            eng.backward_raw(sv, dout[a:b], gc, flags)
            sum64 += gc.double()
            seq32 += gc
        live = set(eng.live_idx)
        assert_grads_match_chunk_sum(eng, g, sum64, seq32, sorted(live), f'train step B={B}')
        for i, (n, o, p) in enumerate(zip(eng.names, eng.offsets, eng.params)):
            if i not in live:
                assert not bool(g[o:o + p.numel()].any()), ('a dead-stage slot was written', n)
        del out, saved, g, sum64, seq32, gc, sv, part
        eng._ws.clear()


# ------------------------------------------------------------------------------------------------------------------------
# (d) plan extremes
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,K,H,W,B', [(4, 16, 16, 16, 2), (8, 16, 16, 16, 2), (4, 1, 16, 1024, 1), (4, 1, 1024, 16, 1)])
def test_plan_extremes_vs_oracle(gpu, monkeypatch, C, K, H, W, B):
    """LG_MAX_K stages, and the longest FFT lines on the narrowest planes: tests/test_gpu_anysize.py's whole-net check (forward 1e-3, l1 loss 1e-4,
    pooled gradients 5e-3 against autograd over the oracle), unchanged"""
    from test_gpu_anysize import test_whole_net_any_size_vs_oracle
    monkeypatch.setattr(orc, 'CANONICAL_REAL_BINS', True)
    with Measured(f'plan extreme C={C} K={K} {H}x{W} B={B}'):
        test_whole_net_any_size_vs_oracle(C, K, H, W, B)


# ------------------------------------------------------------------------------------------------------------------------
# (e) misaligned inputs through the Python layer
# ------------------------------------------------------------------------------------------------------------------------
def off_by_four(t):
    """(storage, view): a contiguous view of t's shape and values that starts 4 bytes into a larger storage"""
    store = torch.full((t.numel() + 8,), -7.0, device=t.device)
    view = store[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return store, view


def test_misaligned_inputs_give_the_bits_of_aligned_ones_and_stay_untouched(gpu):
    from gpu_helpers import make_module
    from lgteun_amd import FusedAdam
    C, K, N, B = 4, 2, 16, 3
    flags = F_FAITHFUL | F_SAVE
    ms, pan, dout = device_inputs(B, C, N, N, seed=21)
    gt = torch.rand(B, C, N, N, device='cuda', generator=torch.Generator(device='cuda').manual_seed(22))
    stores = {k: off_by_four(v) for k, v in dict(ms=ms, pan=pan, dout=dout, gt=gt).items()}
    before = {k: s.clone() for k, (s, _) in stores.items()}

    def step(ms, pan, dout):
        eng = make_module(C, K).engine()
        g = torch.zeros_like(eng.flat)
        out, saved = eng.forward_raw(ms, pan, flags)
        eng.backward_raw(saved, dout, g, flags)
        return out, g

    def train(ms, pan, gt):
        net = make_module(C, K)
        opt = FusedAdam(net.parameters(), lr=1e-3)
        opt.dropout = False
        loss = net.engine().train_step(ms, pan, gt, opt).clone()
        return loss, net.engine().flat.clone(), net.engine().gflat.clone()

    with Measured('misaligned inputs'):
        want, got = step(ms, pan, dout), step(stores['ms'][1], stores['pan'][1], stores['dout'][1])
        assert same_bits(want[0], got[0]) and same_bits(want[1], got[1])
        want, got = train(ms, pan, gt), train(stores['ms'][1], stores['pan'][1], stores['gt'][1])
        assert all(same_bits(a, b) for a, b in zip(want, got))
        assert bool(want[1].ne(make_module(C, K).engine().flat).any())          # the step moved the parameters
        for k, (s, _) in stores.items():
            assert same_bits(s, before[k]), (k, "the caller's storage was written")
