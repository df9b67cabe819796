"""-m gpu: HIP backward / optimizer path vs gradients produced by the reference itself (tests/golden/grad_*.npz,
train3_*.npz) and vs the oracle's autograd.  Dropout off (module.eval()) -> exact-gradient parity."""
import numpy as np
import pytest
import torch

from conftest import load_gold
from helpers import det_params, rel_l2
from oracle import detweights as dw
from oracle import lgteun_oracle as orc

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _grad_report(named_grads, gold):
    """per-tensor max-abs error relative to the tensor's max (floored), plus a global relative-L2 gate.
    Per-kernel backward parity is pinned tightly in test_half_block_backward_vs_oracle; here, through the whole net, a few
    cancellation-dominated sums (FFT-mixer amp/pha biases, pos_emb) carry fp32 noise of ~1e-2 of their (tiny) magnitude --
    the reference's own fp32 gradients are up to 6e-3 off its fp64 ones on the same tensors (tools/debug_grads.py)."""
    num = sum(float(((g - gold[k.replace('.', '/')]) ** 2).sum()) for k, g in named_grads.items())
    den = sum(float((gold[k.replace('.', '/')] ** 2).sum()) for k in named_grads)
    assert (num / den) ** 0.5 < 1e-3, (num / den) ** 0.5
    worst, rows = 0.0, []
    for k, g in named_grads.items():
        ref = gold[k.replace('.', '/')]
        # floor: gradients that are numerically zero (pos_emb rows sum to ~0: |g|max ~ 5e-7 under the 1/N L1 scale,
        # where the reference's own fp32 is 6e-3 off its fp64) are compared on an absolute scale
        scale = max(float(np.abs(ref).max()), 2e-5)
        err = float(np.abs(g - ref).max() / scale)
        rows.append((err, k))
        worst = max(worst, err)
    rows.sort(reverse=True)
    return worst, rows[:8]


@pytest.mark.parametrize('name', ['grad_c4_k2_p32', 'grad_c8_k2_p32'])
def test_autograd_path_vs_reference_gradients(manifest, name):
    from gpu_helpers import make_module
    m = manifest[name]
    g = load_gold(name)
    ms, pan, gt = dw.make_inputs(m['B'], m['C'], m['h'], m['h'], seed=m['seed'], kind=m['kind'])
    net = make_module(m['C'], m['K'])          # eval(): dropout off
    out = net(T(ms).cuda(), T(pan).cuda())
    loss = torch.nn.functional.l1_loss(out, T(gt).cuda())
    loss.backward()
    assert abs(loss.item() - float(g['loss'])) < 2e-5
    none = sorted(k for k, p in net.named_parameters() if p.grad is None)
    assert none == sorted(m['none_grad'])       # dead stages keep grad None like the reference (D3)
    grads = {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters() if p.grad is not None}
    worst, top = _grad_report(grads, g)
    assert worst < 3e-2, top


def test_fused_train_step_gradients_match_autograd_path(manifest):
    """Engine.train_step's flat gradient buffer == autograd-path gradients (same kernels, fused L1)."""
    from gpu_helpers import make_module
    from lgteun_amd import FusedAdam
    m = manifest['grad_c4_k2_p32']
    g = load_gold('grad_c4_k2_p32')
    ms, pan, gt = dw.make_inputs(m['B'], m['C'], m['h'], m['h'], seed=m['seed'], kind=m['kind'])
    net = make_module(m['C'], m['K'])
    opt = FusedAdam(net.parameters(), lr=0.0)   # lr 0: parameters unchanged, gradients observable
    opt.dropout = False
    eng = net.engine()
    loss = eng.train_step(T(ms).cuda(), T(pan).cuda(), T(gt).cuda(), opt)
    assert abs(float(loss.item()) - float(g['loss'])) < 2e-5
    grads = {}
    for i in eng.live_idx:
        n, o, p = eng.names[i], eng.offsets[i], eng.params[i]
        grads[n] = eng.gflat[o:o + p.numel()].view(p.shape).cpu().numpy()
    worst, top = _grad_report(grads, g)
    assert worst < 3e-2, top
    # dead-stage slots of the flat gradient buffer are never written
    a, b = eng.live_ranges[0][1], eng.live_ranges[1][0]
    assert float(eng.gflat[a:b].abs().max()) == 0.0


def test_three_train_iterations_vs_reference_runner(manifest, tmp_path):
    """UnlgFormer.train_iter x3 with fused Adam + StepLR-per-iteration vs the reference runner's losses / weights."""
    import logging
    import lgteun_amd
    from lgteun_amd.compat import Config
    from helpers import state_shapes
    m = manifest['train3_c4_k2_p32']
    g = load_gold('train3_c4_k2_p32')
    cfg = Config(dict(ms_chans=4, work_dir=str(tmp_path), datas='GF-2', cuda=True, max_iter=3, bit_depth=11,
                      loss_cfg={'rec_loss': dict(type='l1', w=1.)},
                      optim_cfg={'core_module': dict(type='Adam', betas=(0.9, 0.999), lr=m['lr'])},
                      sched_cfg=dict(step_size=m['step_size'], gamma=m['gamma']),
                      model_cfg={'core_module': dict(stage=m['K'])}))
    runner = lgteun_amd.build_model('UnlgFormer', cfg, logging.getLogger('t'), None, None, None)
    core = runner.module_dict['core_module']
    sd = dw.fill_state_dict(state_shapes(4, m['K']), salt=0)
    core.load_state_dict({k: T(v) for k, v in sd.items()})
    runner.set_cuda()
    core = runner.module_dict['core_module']
    core.eval()
    runner.set_optim()
    runner.optim_dict['core_module'].dropout = False
    runner.set_sched()
    ms, pan, gt = dw.make_inputs(m['B'], 4, m['h'], m['h'], seed=m['seed'], kind=m['kind'])
    batch = dict(input_lr=T(ms).cuda(), input_pan=T(pan).cuda(), target=T(gt).cuda(), image_id=['a', 'b'])
    losses, lrs = [], []
    runner.print_train_log = lambda it, res, freq=10: losses.append(res['full_loss'])
    for it in range(1, 4):
        lrs.append(runner.optim_dict['core_module'].param_groups[0]['lr'])
        runner.train_iter(it, batch, log_freq=1)
        runner.sched_dict['core_module'].step()
    assert np.allclose(lrs, g['lrs'], rtol=1e-12)
    assert np.allclose(losses, g['losses'], rtol=5e-4), (losses, g['losses'])
    sd_out = core.state_dict()
    for k, v in sd_out.items():
        if k.startswith('prior_module.0.'):
            assert torch.equal(v.cpu(), T(sd[k]))          # dead stage untouched by Adam
        else:
            assert rel_l2(v.cpu(), g[k.replace('.', '/')]) < 1e-2, k


def _oracle_block(P, C, blk, which, x, dy):
    """oracle autograd of one half-block: returns (dx, {param_name: grad})"""
    E = 4 * C
    pre = 'prior_module.0.' + {0: 'encoder_layers.0.0.blocks.0.', 1: 'encoder_layers.0.0.blocks.1.', 2: 'bottleneck.blocks.0.',
                               3: 'decoder_layers.0.2.blocks.0.', 4: 'decoder_layers.0.2.blocks.1.'}[blk]
    x = x.clone().requires_grad_(True)
    if which == 0:
        y = orc.layer_norm(x, P[pre + '0.fn.norm.weight'].detach(), P[pre + '0.fn.norm.bias'].detach())
        hc = x.shape[-1] // 2
        g = y[..., hc:].detach().clone().requires_grad_(True)
        out = orc.global_mixer(P, pre + '0.fn.fn.global_mixer.', g).permute(0, 3, 1, 2)
        (out * dy).sum().backward()
        dx = g.grad.permute(0, 3, 1, 2)
    elif which == 1:
        y = orc.layer_norm(x, P[pre + '0.fn.norm.weight'], P[pre + '0.fn.norm.bias'])
        out = x + orc.lg_mixer(P, pre + '0.fn.fn.', y)
        (out * dy).sum().backward()
        dx = x.grad
    else:
        y = orc.layer_norm(x, P[pre + '1.fn.norm.weight'], P[pre + '1.fn.norm.bias'])
        out = x + orc.feed_forward(P, pre + '1.fn.fn.', y)
        (out * dy).sum().backward()
        dx = x.grad
    return dx, {k: v.grad for k, v in P.items() if v.grad is not None}


@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('blk,which', [(0, 0), (0, 1), (0, 2), (2, 0), (2, 1), (2, 2)])
def test_half_block_backward_vs_oracle(C, blk, which):
    """per-kernel backward parity in isolation (FFT mixer / window attention+proj / feed_forward), fp64 oracle"""
    from gpu_helpers import Ops, make_module
    net = make_module(C, 1)
    ops = Ops(net, 32, 32)
    E = 4 * C
    e, hw = (2 * E, 16) if blk == 2 else (E, 32)
    rng = np.random.default_rng(100 * blk + which + C)
    x = T(rng.standard_normal((2, hw, hw, e)).astype(np.float32))
    x[1, :, :, e // 2:] -= 0.7
    dy_shape = (2, e // 2, hw, hw) if which == 0 else (2, hw, hw, e)
    dy = T(rng.standard_normal(dy_shape).astype(np.float32))
    P64 = det_params(C, 1, dtype=torch.float64, requires_grad=True)
    want_dx, want_g = _oracle_block(P64, C, blk, which, x.double(), dy.double())
    got_dx, flat = ops.block_bwd(0, blk, which, x.cuda(), dy.cuda())
    assert rel_l2(got_dx.cpu(), want_dx) < 2e-4, rel_l2(got_dx.cpu(), want_dx)
    worst = []
    for k, g in want_g.items():
        got = ops.grad_of(flat, k).cpu().numpy()
        ref = g.numpy()
        worst.append((float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)), k))
    worst.sort(reverse=True)
    assert worst[0][0] < 2e-3, worst[:5]


@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('blk,which', [(0, 1), (0, 2), (2, 1), (2, 2)])
def test_half_block_backward_vs_oracle_bf16_mode(C, blk, which):
    """precision='bf16' at kernel level, both band counts (the NP = 1 instances k_attn_m<.,1>, k_ffn_xs / k_ffn_x32<.,1>,
    k_ffn_dw_bwd_xs<.,1>, k_ffn1_bwd_xs<.,1> and the tanh-GELU forward / backward pair were exercised by one 32 x 32 whole-net test only):
    the mixer and feed_forward half-blocks of both levels against torch autograd over the fp64 oracle, gated at what one round-to-nearest
    bf16 piece per operand and bf16 storage of the saved tensors allow -- dx 2e-2 relative, parameter gradients 5e-2 of the tensor's
    largest entry (measured 3e-3 ... 2e-2)"""
    from gpu_helpers import Ops, make_module
    net = make_module(C, 1)
    net.precision = 'bf16'
    ops = Ops(net, 32, 32)
    E = 4 * C
    e, hw = (2 * E, 16) if blk == 2 else (E, 32)
    rng = np.random.default_rng(100 * blk + which + C)
    x = T(rng.standard_normal((2, hw, hw, e)).astype(np.float32))
    x[1, :, :, e // 2:] -= 0.7
    dy = T(rng.standard_normal((2, hw, hw, e)).astype(np.float32))
    P64 = det_params(C, 1, dtype=torch.float64, requires_grad=True)
    want_dx, want_g = _oracle_block(P64, C, blk, which, x.double(), dy.double())
    got_dx, flat = ops.block_bwd(0, blk, which, x.cuda(), dy.cuda())
    err_dx = rel_l2(got_dx.cpu(), want_dx)
    worst = []
    for k, g in want_g.items():
        got = ops.grad_of(flat, k).cpu().numpy()
        ref = g.numpy()
        worst.append((float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)), k))
    worst.sort(reverse=True)
    print(f'bf16 mode C={C} blk={blk} which={which}: dx {err_dx:.2e}  worst parameter gradient {worst[0][0]:.2e} ({worst[0][1]})')
    assert err_dx < 2e-2, err_dx
    assert worst[0][0] < 5e-2, worst[:5]


@pytest.mark.parametrize('which', [0, 1])
def test_half_block_backward_256_split_fft(which):
    """level-0 mixer half-block at 256x256 (plane too large for LDS: three-kernel FFT path), fp64 oracle"""
    from gpu_helpers import Ops, make_module
    C = 4
    net = make_module(C, 1)
    ops = Ops(net, 256, 256)
    e, hw = 16, 256
    rng = np.random.default_rng(77 + which)
    x = T(rng.standard_normal((1, hw, hw, e)).astype(np.float32))
    dy_shape = (1, e // 2, hw, hw) if which == 0 else (1, hw, hw, e)
    dy = T(rng.standard_normal(dy_shape).astype(np.float32))
    P64 = det_params(C, 1, dtype=torch.float64, requires_grad=True)
    want_dx, want_g = _oracle_block(P64, C, 0, which, x.double(), dy.double())
    got_dx, flat = ops.block_bwd(0, 0, which, x.cuda(), dy.cuda())
    assert rel_l2(got_dx.cpu(), want_dx) < 5e-4, rel_l2(got_dx.cpu(), want_dx)
    for k, g in want_g.items():
        got = ops.grad_of(flat, k).cpu().numpy()
        ref = g.numpy()
        assert float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)) < 5e-3, k


def test_bf16_saved_activations_mode(manifest):
    """precision='bf16' (throughput mode, opt-in): the FFN's three 1x1-conv GEMMs AND (round 5) the local mixer's four products
    (to_qkv, Q K^T, P V, proj: k_attn_m with one round-to-nearest piece per operand) take 16-bit operands on the matrix cores
    (fp32 accumulate) and the 4e-wide tensors saved for the backward are stored as bf16; everything else is fp32.
    Gates: forward within 5e-3 relative L2 and >= 50 dB PSNR of the fp32 mode, loss within 2e-3 relative of the
    reference's (1e-3 while only the FFN ran in bf16: measured 1.2e-3 with the mixer in), gradients within 2e-2 global relative
    L2 of the reference's fp32 gradients."""
    from gpu_helpers import make_module
    from lgteun_amd import FusedAdam
    m = manifest['grad_c4_k2_p32']
    g = load_gold('grad_c4_k2_p32')
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(m['B'], m['C'], m['h'], m['h'], seed=m['seed'], kind=m['kind']))
    net = make_module(m['C'], m['K'])
    with torch.no_grad():
        y32 = net(ms, pan)
    net.precision = 'bf16'
    with torch.no_grad():
        y16 = net(ms, pan)
    fwd_rel = rel_l2(y16.cpu(), y32.cpu())
    mse = float(((y16 - y32) ** 2).mean())
    psnr = 10 * np.log10(1.0 / max(mse, 1e-30))
    print(f'bf16 mode: forward rel_l2 {fwd_rel:.3e}  PSNR vs fp32 mode {psnr:.1f} dB')
    assert fwd_rel < 5e-3 and psnr >= 50.0, (fwd_rel, psnr)
    opt = FusedAdam(net.parameters(), lr=0.0)
    opt.dropout = False
    eng = net.engine()
    loss = float(eng.train_step(ms, pan, gt, opt).item())
    assert abs(loss - float(g['loss'])) < 2e-3 * abs(float(g['loss'])), (loss, float(g['loss']))
    num = den = 0.0
    for i in eng.live_idx:
        n, o, p = eng.names[i], eng.offsets[i], eng.params[i]
        got = eng.gflat[o:o + p.numel()].view(p.shape).cpu().numpy()
        ref = g[n.replace('.', '/')]
        num += float(((got - ref) ** 2).sum())
        den += float((ref ** 2).sum())
    print(f'bf16 mode: grad rel_l2 {(num / den) ** 0.5:.3e}')
    assert (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5


def test_runner_train_eval_save_load_roundtrip(tmp_path):
    """the reference-style runner loop on the GPU path: Base_model.train (StepLR per iteration, base_model.py:164-204),
    test() with PSNR/SAM/ERGAS (267-352), save() of whole modules + load_checkpoint() (354-369,102-108)"""
    import logging
    import lgteun_amd
    from lgteun_amd.compat import Config
    rng = np.random.default_rng(0)

    def batch(i):
        ms, pan, gt = dw.make_inputs(2, 4, 8, 8, seed=100 + i, kind='smooth')
        return dict(input_lr=T(ms) * 2047.5, input_pan=T(pan) * 2047.5, target=T(gt) * 2047.5, image_id=[f'a{i}', f'b{i}'])
    loader = [batch(i) for i in range(3)]
    cfg = Config(dict(ms_chans=4, work_dir=str(tmp_path), datas='GF-2', cuda=True, max_iter=6, bit_depth=11, norm_input=True,
                      save_freq=3, eval_freq=-1, test_freq=-1,
                      loss_cfg={'rec_loss': dict(type='l1', w=1.)},
                      optim_cfg={'core_module': dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3)},
                      sched_cfg=dict(step_size=2, gamma=0.85), model_cfg={'core_module': dict(stage=2)}))
    torch.manual_seed(1)
    runner = lgteun_amd.build_model('UnlgFormer', cfg, logging.getLogger('runner'), loader, None, loader)
    runner.set_cuda()
    runner.set_optim()
    runner.set_sched()
    before = runner.test(iter_id=0, ref=True)
    runner.train()
    after = runner.test(iter_id=6, ref=True)
    assert after['PSNR'][0] > before['PSNR'][0]                       # six Adam steps on three batches help
    assert abs(runner.optim_dict['core_module'].param_groups[0]['lr'] - 1.5e-3 * 0.85 ** 3) < 1e-12
    ckpt = tmp_path / 'GF-2' / 'train_out' / 'model_iter_3.pth'      # the reference's location (base_model.py:44,360)
    assert ckpt.exists()                                              # save_freq = 3
    path = runner.save(iter_id=6)
    runner2 = lgteun_amd.build_model('UnlgFormer', cfg, logging.getLogger('runner2'), loader, None, loader)
    runner2.load_checkpoint(path)
    assert runner2.last_iter == 6
    runner2.set_cuda()
    again = runner2.test(iter_id=6, ref=True)
    assert abs(again['PSNR'][0] - after['PSNR'][0]) < 1e-9 and abs(again['SAM'][0] - after['SAM'][0]) < 1e-12
    # resume: the optimizer state saved with the checkpoint (absent in the reference) continues the Adam moments and step count
    runner2.set_optim()
    o1, o2 = runner.optim_dict['core_module'], runner2.optim_dict['core_module']
    assert o2._step == o1._step == 6
    assert torch.equal(o2._state['exp_avg'].cpu(), o1._state['exp_avg'].cpu()) and torch.equal(o2._state['exp_avg_sq'].cpu(), o1._state['exp_avg_sq'].cpu())
    # ... and the restored moments (loaded to the host) move to the device with the first fused step
    runner2.set_sched()
    runner2.train_iter(iter_id=7, input_batch=lgteun_amd.base_model.data_normalize({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in loader[0].items()}, 11))
    assert o2._step == 7 and o2._state['exp_avg'].is_cuda
    # the full-resolution pass runs the model, writes the fused images when asked and reports the no-reference indices
    runner2.test_data_loader0 = loader[:1]
    nr = runner2.test(iter_id=6, save=True, ref=False)
    assert set(nr) == {'D_lambda', 'D_s', 'QNR'} and 0.0 <= nr['QNR'][0] <= 1.0
    assert runner2.eval_results['QNR_mean'][-1] == round(nr['QNR'][0], 4)
    assert (tmp_path / 'GF-2' / 'test_out0' / 'iter_6' / 'a0_mul_hat.tif').exists()


@pytest.mark.parametrize('C,H', [(4, 32), (4, 256)])
def test_gradients_are_bitwise_reproducible(C, H):
    """every parameter-gradient sum is a per-workgroup partial row + a fixed-order reduction (no float atomics, in-LDS and
    split FFT paths included): two backward passes from the same state give bit-identical flat gradient buffers"""
    from gpu_helpers import make_module
    from lgteun_amd import FusedAdam
    B = 3 if H == 32 else 1
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(B, C, H // 4, H // 4, seed=77, kind='smooth'))
    net = make_module(C, 2)
    opt = FusedAdam(net.parameters(), lr=0.0)
    opt.dropout = False
    eng = net.engine()
    eng.train_step(ms, pan, gt, opt)
    g1 = eng.gflat.clone()
    eng.train_step(ms, pan, gt, opt)
    assert torch.equal(g1, eng.gflat)
    assert float(g1.abs().max()) > 0


@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('B,h,w', [(1, 16, 16), (3, 80, 48), (2, 48, 208), (1, 128, 128)])
def test_ffn_backward_kernels_at_awkward_shapes(C, B, h, w):
    """the e = 16 FFN backward pair (k_ffn_dw_bwd_xs<16>: strip walk with an LDS ring of dh3; k_ffn1_bwd_xs: h1 re-computed, dx and all
    weight gradients on the bf16 pipe in split arithmetic) and, with 8 bands, the e = 32 path (round 4: k_ffn_dw_bwd_xs<32>, the same walk
    with eight waves, + k_ffn1_bwd_x32) in isolation against the fp64 oracle at sizes that exercise their edges: one strip step only,
    strips that end inside a step, rectangular planes, an odd batch, a multi-step strip walk"""
    from gpu_helpers import Ops, make_module
    net = make_module(C, 1)
    ops = Ops(net, h, w)
    e = 4 * C
    rng = np.random.default_rng(1000 + h + w)
    x = T(rng.standard_normal((B, h, w, e)).astype(np.float32))
    dy = T(rng.standard_normal((B, h, w, e)).astype(np.float32))
    P64 = det_params(C, 1, dtype=torch.float64, requires_grad=True)
    want_dx, want_g = _oracle_block(P64, C, 0, 2, x.double(), dy.double())
    got_dx, flat = ops.block_bwd(0, 0, 2, x.cuda(), dy.cuda())
    assert rel_l2(got_dx.cpu(), want_dx) < 2e-5, rel_l2(got_dx.cpu(), want_dx)
    assert len(want_g) == 10                                       # W1 b1 W2 b2 dww dwb W3 b3 + the LayerNorm pair
    for k, g in want_g.items():
        got = ops.grad_of(flat, k).cpu().numpy()
        ref = g.numpy()
        assert float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)) < 2e-4, (k, float(np.abs(got - ref).max() / np.abs(ref).max()))


@pytest.mark.parametrize('env', [{'LG_FFN_DWBWD': 'tile'}, {'LG_FFN_SAVE': '3'}, {'LG_FFN_BWD32': 'pair'}, {'LG_FFN_BWD_SPLIT': 'bf16x3'}, {'LG_FFN_H3': 'recompute'}])
def test_ffn_backward_ab_paths_agree_with_the_default(env, monkeypatch):
    """the A/B switches of the FFN backward (LG_FFN_H3=recompute: round 6's k_ffn_dw_bwd_h, which re-computes h3 from an LDS ring of h2 -- the forward then saves h2 only -- against the default k_ffn_dw_bwd_xs on a saved h3; round 2's tile kernel + weight-gradient launch; the three-tensor save mode; round 2's
    k_ffn1_bwd_x32 + weight-gradient launches at e = 32 instead of k_ffn1_bwd_xs<32>; bf16 triples instead of f16 pairs in k_ffn1_bwd_xs) give the default path's gradients to rounding on a whole train step (C = 4: e = 16 at level 0, e = 32 at
    level 1)"""
    from gpu_helpers import make_module
    from lgteun_amd import FusedAdam
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(2, 4, 16, 16, seed=11, kind='smooth'))

    def grads():
        net = make_module(4, 2)
        opt = FusedAdam(net.parameters(), lr=0.0)
        opt.dropout = False
        eng = net.engine()
        eng.train_step(ms, pan, gt, opt)
        return eng.gflat.clone(), eng
    for k in env:
        monkeypatch.delenv(k, raising=False)
    # LG_FFN_SAVE=3 runs the channel-split forward k_ffn_xs (the register chain k_ffn_xr saves h2 / h3 or nothing): its baseline is the default
    # backward behind the SAME forward kernel -- the two forwards differ by rounding, which the cancelling-sum gradient kinds (pos_emb, 1e-8) amplify
    base = {'LG_FFN_FWD': 'xs'} if 'LG_FFN_SAVE' in env else {}
    for k, v in base.items():
        monkeypatch.setenv(k, v)
    g0, eng = grads()
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                   # read once per plan: a fresh module builds a fresh plan
    g1, _ = grads()
    for i in eng.live_idx:
        o, n = eng.offsets[i], eng.params[i].numel()
        a, b = g0[o:o + n].double(), g1[o:o + n].double()
        assert float((a - b).norm()) <= 5e-6 * float(a.norm()) + 1e-12, (env, eng.names[i], float((a - b).norm()), float(a.norm()))
    for k in base:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize('drop', [False, True])
def test_fused_attention_backward_agrees_with_the_round3_path(drop, monkeypatch):
    """k_attn_bwd_f (round 4: the local-mixer half-block backward in one kernel, dropout through one keep-bit word per pixel written by
    k_proj_o2_bwd_k) against round 3's k_attn_bwd_core + k_attn_bwd_epi + k_wgrad_t on a whole train step, with and without dropout
    (same counter seed: the two paths must apply the same mask): every live gradient tensor to rounding"""
    from gpu_helpers import make_module
    from lgteun_amd.engine import LG_FLAG_DROPOUT, LG_FLAG_SAVE, LG_FLAG_FAITHFUL
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(3, 4, 16, 24, seed=12, kind='smooth'))
    flags = (LG_FLAG_DROPOUT if drop else 0) | LG_FLAG_SAVE | LG_FLAG_FAITHFUL
    gen = torch.Generator(device='cpu').manual_seed(6)

    def grads():
        net = make_module(4, 2)
        eng = net.engine()
        y, saved = eng.forward_raw(ms, pan, flags, seed=4321)
        r = torch.randn(y.shape, generator=torch.Generator(device='cpu').manual_seed(6)).cuda()
        g = torch.zeros_like(eng.flat)
        eng.backward_raw(saved, r, g, flags, seed=4321)
        return g, eng
    monkeypatch.delenv('LG_ATTN_BWD', raising=False)
    g1, eng = grads()
    monkeypatch.setenv('LG_ATTN_BWD', 'r3')                       # read once per plan: a fresh module builds a fresh plan
    g0, _ = grads()
    assert float(g0.abs().max()) > 0
    for i in eng.live_idx:
        o, n = eng.offsets[i], eng.params[i].numel()
        a, b = g0[o:o + n].double(), g1[o:o + n].double()
        tol = 2e-4 if eng.names[i].endswith(('pos_emb', 'conv_amp.0.bias', 'conv_pha.0.bias')) else 2e-5   # the cancelling sums
        assert float((a - b).norm()) <= tol * float(a.norm()) + 1e-10, (drop, eng.names[i], float((a - b).norm()), float(a.norm()))


@pytest.mark.parametrize('drop,C', [(False, 4), (True, 4), (False, 8), (True, 8)])
def test_attention_backward_on_the_forwards_row_statistics_agrees_with_its_own_reduction_pass(drop, C, monkeypatch):
    """round 6: k_attn_bwd_f<STATS> (e = 16) and k_attn_bwd_core<.., STATS> (e = 32, 64: C = 4 has a 32-wide bottleneck, C = 8 is 32 / 64 wide) read the log-sum-exp of every score row and the attention output that k_attn_m's saving launch left (one loop over
    the keys in pass 1) -- against the same kernel re-deriving both with its reduction pass (LG_ATTN_BWD_STATS=recompute, rounds 4 - 5) on a whole train
    step, with and without dropout: every live gradient tensor to rounding (the forward's statistics come out of split 16-bit products, the backward's
    own out of fp32 multiply-adds: the two differ by ~1e-6 of a score)"""
    from gpu_helpers import make_module
    from lgteun_amd.engine import LG_FLAG_DROPOUT, LG_FLAG_SAVE, LG_FLAG_FAITHFUL
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(3, C, 16, 24, seed=12, kind='smooth'))
    flags = (LG_FLAG_DROPOUT if drop else 0) | LG_FLAG_SAVE | LG_FLAG_FAITHFUL

    def grads():
        net = make_module(C, 2)
        eng = net.engine()
        y, saved = eng.forward_raw(ms, pan, flags, seed=4321)
        r = torch.randn(y.shape, generator=torch.Generator(device='cpu').manual_seed(6)).cuda()
        g = torch.zeros_like(eng.flat)
        eng.backward_raw(saved, r, g, flags, seed=4321)
        return y.clone(), g, eng
    monkeypatch.delenv('LG_ATTN_BWD_STATS', raising=False)
    y1, g1, eng = grads()
    monkeypatch.setenv('LG_ATTN_BWD_STATS', 'recompute')          # read once per plan: a fresh module builds a fresh plan
    y0, g0, _ = grads()
    assert torch.equal(y0, y1)                                    # the forward's output does not depend on what it saves
    assert float(g0.abs().max()) > 0 and bool(torch.isfinite(g1).all())
    for i in eng.live_idx:
        o, n = eng.offsets[i], eng.params[i].numel()
        a, b = g0[o:o + n].double(), g1[o:o + n].double()
        tol = 2e-4 if eng.names[i].endswith(('pos_emb', 'conv_amp.0.bias', 'conv_pha.0.bias')) else 2e-5   # the cancelling sums
        assert float((a - b).norm()) <= tol * float(a.norm()) + 1e-10, (drop, C, eng.names[i], float((a - b).norm()), float(a.norm()))


@pytest.mark.parametrize('C', [4, 8])
def test_one_launch_data_step_agrees_with_the_tile_kernels_on_a_train_step(C, monkeypatch):
    """k_dstep.hip (round 4: the data step of a 128 x 128 plane as one pixelwise + one plane-in-LDS launch per direction) against the four + nine
    tile launches it replaces (LG_DSTEP=tiles), whole train step, K = 3 so that the shared D / DT / R / RT gradients are sums over stages:
    the output bitwise (the forward is the same arithmetic in the same order), every live gradient tensor to rounding"""
    from gpu_helpers import make_module
    from lgteun_amd.engine import LG_FLAG_SAVE, LG_FLAG_FAITHFUL
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(2, C, 32, 32, seed=21, kind='smooth'))
    flags = LG_FLAG_SAVE | LG_FLAG_FAITHFUL

    def run():
        eng = make_module(C, 3).engine()
        y, saved = eng.forward_raw(ms, pan, flags, seed=1)
        r = torch.randn(y.shape, generator=torch.Generator(device='cpu').manual_seed(8)).cuda()
        g = torch.zeros_like(eng.flat)
        eng.backward_raw(saved, r, g, flags, seed=1)
        return y.clone(), g, eng
    monkeypatch.delenv('LG_DSTEP', raising=False)
    y1, g1, eng = run()
    monkeypatch.setenv('LG_DSTEP', 'tiles')                        # read once per plan: a fresh module builds a fresh plan
    y0, g0, _ = run()
    assert torch.equal(y0, y1)
    assert float(g0.abs().max()) > 0
    for i in eng.live_idx:
        o, n = eng.offsets[i], eng.params[i].numel()
        a, b = g0[o:o + n].double(), g1[o:o + n].double()
        assert float((a - b).norm()) <= 2e-5 * float(a.norm()) + 1e-10, (eng.names[i], float((a - b).norm()), float(a.norm()))


@pytest.mark.parametrize('B,h,w', [(1, 16, 16), (1, 16, 32), (3, 16, 48), (5, 32, 32), (5, 128, 128)])
def test_mixer_backward_kernel_at_awkward_shapes(B, h, w):
    """the fused local-mixer backward in isolation against the fp64 oracle at sizes that exercise its edges: one window group (a single workgroup), two,
    rectangular planes with an odd batch, and more window groups (320) than resident workgroups (256: some walk two groups)"""
    from gpu_helpers import Ops, make_module
    C = 4
    net = make_module(C, 1)
    ops = Ops(net, h, w)
    e = 4 * C
    rng = np.random.default_rng(2000 + h + w)
    x = T(rng.standard_normal((B, h, w, e)).astype(np.float32))
    dy = T(rng.standard_normal((B, h, w, e)).astype(np.float32))
    P64 = det_params(C, 1, dtype=torch.float64, requires_grad=True)
    want_dx, want_g = _oracle_block(P64, C, 0, 1, x.double(), dy.double())
    got_dx, flat = ops.block_bwd(0, 0, 1, x.cuda(), dy.cuda())
    assert rel_l2(got_dx.cpu(), want_dx) < 1e-4, rel_l2(got_dx.cpu(), want_dx)
    assert len(want_g) == 11, sorted(want_g)     # pos_emb, to_qkv w/b, conv_amp w/b, conv_pha w/b, proj w/b, LayerNorm pair
    for k, g in want_g.items():
        got = ops.grad_of(flat, k).cpu().numpy()
        ref = g.numpy()
        err = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))
        assert err < (2e-3 if 'global_mixer' in k else 1e-4), (k, err)


@pytest.mark.parametrize('C', [4, 8])
def test_matrix_pipe_attention_backward_core_agrees_with_the_vector_pipe_core(C, monkeypatch):
    """k_attn_bwd_core_m (round 5, LG_ATTN_BWD_CORE=m: the e = 32 local-mixer backward core on the matrix pipe -- LayerNorm / to_qkv / proj^T,
    S^T / dP^T and S / dP as f16-pair MFMAs in two orientations, P and dS from the accumulator registers into the O, dQ, dV, dK products,
    the pos_emb gradient in 64 accumulator registers; an A/B variant: correct, not faster than the vector-pipe core yet)
    against the default k_attn_bwd_core on a whole train step: C = 4 has its e = 32 block at level 1
    (8 x 8 planes of a 16 x 16 PAN: one window per sample), C = 8 at level 0 -- every live gradient tensor to rounding (2e-5 of its norm:
    two fp32-equivalent evaluations; pos_emb sums over all windows)"""
    from gpu_helpers import make_module
    from lgteun_amd import FusedAdam
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(3, C, 32, 48, seed=21, kind='smooth'))

    def grads():
        net = make_module(C, 2)
        opt = FusedAdam(net.parameters(), lr=0.0)
        opt.dropout = False
        eng = net.engine()
        eng.train_step(ms, pan, gt, opt)
        return eng.gflat.clone(), eng
    monkeypatch.setenv('LG_ATTN_BWD_STATS', 'recompute')             # both cores re-derive the softmax row statistics (the matrix-pipe core always does): what differs is the core alone
    monkeypatch.delenv('LG_ATTN_BWD_CORE', raising=False)
    g0, eng = grads()
    monkeypatch.setenv('LG_ATTN_BWD_CORE', 'm')                      # read once per plan: a fresh module builds a fresh plan
    g1, _ = grads()
    monkeypatch.delenv('LG_ATTN_BWD_CORE', raising=False)
    assert float(g0.abs().max()) > 0
    for i in eng.live_idx:
        o, n = eng.offsets[i], eng.params[i].numel()
        a, b = g0[o:o + n].double(), g1[o:o + n].double()
        assert torch.isfinite(b).all(), eng.names[i]
        assert float((a - b).norm()) <= 2e-5 * float(a.norm()) + 1e-12, (eng.names[i], float((a - b).norm()), float(a.norm()))

