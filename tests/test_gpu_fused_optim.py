"""-m gpu: the fused train step beyond l1 + Adam -- `lg_l2_loss`, `lg_optim_step` (Adam / AdamW / SGD / RMSprop with their options)
and the routes through Engine.train_step / UnlgFormer.train_iter, against torch.optim and nn.MSELoss (what the reference executes),
against the `fused=False` route and against a fixture the reference runner itself produced."""
import json
import logging

import numpy as np
import pytest
import torch

from conftest import load_gold
from helpers import rel_l2, state_shapes
from optim_helpers import flat_engine
from oracle import detweights as dw

pytestmark = pytest.mark.gpu
T = torch.from_numpy


# ------------------------------------------------------------------------------------------------------------------------
# 1. optimizer arithmetic against torch.optim
# ------------------------------------------------------------------------------------------------------------------------
N_FLAT = 100003
RANGES = [(3, 30001), (40002, 70007), (70011, 99998)]      # gaps in front, between and behind; no start on a 16-byte boundary
GRAD_AMP = [1.0, 0.3, 2.0, 0.1, 1.0]                        # per step: the amsgrad maximum and the centred variance see rises and falls

OPTION_SETS = [
    ('Adam', dict()),
    ('Adam', dict(weight_decay=1e-2)),
    ('Adam', dict(amsgrad=True)),
    ('Adam', dict(amsgrad=True, weight_decay=1e-2)),
    ('AdamW', dict(weight_decay=1e-2)),
    ('AdamW', dict(weight_decay=0.0)),
    ('AdamW', dict(amsgrad=True, weight_decay=1e-2)),
    ('SGD', dict()),
    ('SGD', dict(weight_decay=1e-2)),
    ('SGD', dict(momentum=0.9)),
    ('SGD', dict(momentum=0.9, weight_decay=1e-2)),
    ('SGD', dict(momentum=0.9, dampening=0.1)),
    ('SGD', dict(momentum=0.9, nesterov=True)),
    ('SGD', dict(momentum=0.9, nesterov=True, weight_decay=1e-2)),
    ('RMSprop', dict()),
    ('RMSprop', dict(weight_decay=1e-2)),
    ('RMSprop', dict(momentum=0.9)),
    ('RMSprop', dict(momentum=0.9, weight_decay=1e-2)),
    ('RMSprop', dict(centered=True)),
    ('RMSprop', dict(centered=True, weight_decay=1e-2)),
    ('RMSprop', dict(centered=True, momentum=0.9)),
    ('RMSprop', dict(alpha=0.9, eps=1e-6, weight_decay=1e-2, centered=True, momentum=0.5)),
]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _synthetic():
    """the parameters, the per-step (lr, gradient) pairs -- lr lowered between steps as StepLR would -- and the mask of the ranges"""
    gen = torch.Generator().manual_seed(1234)
    p0 = torch.randn(N_FLAT, generator=gen)
    steps = [(1e-2 * 0.85 ** i, torch.randn(N_FLAT, generator=gen) * GRAD_AMP[i]) for i in range(5)]
    inside = torch.zeros(N_FLAT, dtype=torch.bool)
    for a, b in RANGES:
        inside[a:b] = True
    return p0, steps, inside, gen


def _torch_runs(name, kwargs, p0, steps):
    """{dtype: (one parameter per range, the torch.optim instance)} after the steps, in fp64 (a) and fp32 (b) on the host"""
    refs = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(p0[a:b].to(dt).clone()) for a, b in RANGES]
        ref = getattr(torch.optim, name)(ps, lr=1e-2, **kwargs)
        for lr, g in steps:
            ref.param_groups[0]['lr'] = lr
            for p, (a, b) in zip(ps, RANGES):
                p.grad = g[a:b].to(dt).clone()
            ref.step()
        refs[dt] = (ps, ref)
    return refs


def _torch_spread(refs):
    """max|(b) - (a)| over the parameters, and the largest parameter magnitude"""
    err_32 = pmax = 0.0
    for p64, p32 in zip(refs[torch.float64][0], refs[torch.float32][0]):
        err_32 = max(err_32, float((p32.detach().double() - p64.detach()).abs().max()))
        pmax = max(pmax, float(p64.detach().abs().max()))
    return err_32, pmax


@pytest.mark.parametrize('name,kwargs', OPTION_SETS, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in kw.items()) or 'plain'}" for n, kw in OPTION_SETS])
def test_optimizer_step_vs_torch(name, kwargs):
    """five steps (fresh gradient each, lr lowered between steps as StepLR would) of the fused class against the torch.optim class
    in fp64 (a) and in fp32 (b) on the host, one tensor per range:  max|fused - a| <= 2 max|b - a| + one fp32 ulp of the largest
    parameter.  Floats outside the ranges keep their bits, in the parameters and in every state buffer."""
    import lgteun_amd
    p0, steps, inside, gen = _synthetic()
    flat = p0.clone().cuda()
    gflat = torch.zeros(N_FLAT, device='cuda')
    eng = flat_engine(flat, gflat, RANGES)
    opt = getattr(lgteun_amd, 'Fused' + name)([torch.nn.Parameter(torch.zeros(1))], lr=1e-2, **kwargs)
    # state buffers: torch's initial zeros inside the ranges, a pattern outside them that must survive
    names = [n for n in opt.state_names() if n is not None]
    marks = {n: torch.where(inside, torch.zeros(N_FLAT), torch.randn(N_FLAT, generator=gen)) for n in names}
    opt._state = {n: v.clone().cuda() for n, v in marks.items()}
    for lr, g in steps:
        gflat.copy_(g)
        opt.param_groups[0]['lr'] = lr
        opt.step_flat(eng)
    torch.cuda.synchronize()
    refs = _torch_runs(name, kwargs, p0, steps)
    got = flat.cpu()
    err_32, pmax = _torch_spread(refs)
    err_fused = max(float((got[a:b].double() - refs[torch.float64][0][i].detach()).abs().max()) for i, (a, b) in enumerate(RANGES))
    floor = float(np.spacing(np.float32(pmax)))
    print(f'{name} {kwargs}: max|fused - fp64| {err_fused:.3e}  max|torch fp32 - fp64| {err_32:.3e}  ratio {err_fused / max(err_32, 1e-300):.2f}  '
          f'floor {floor:.3e}')
    assert np.isfinite(err_fused) and err_fused <= 2 * err_32 + floor, (err_fused, err_32, floor)
    # the state agrees with what the torch class keeps under the same name (same band, per buffer).  The plain Adam set is served by
    # lg_adam_step, which this test leaves as it found it: that kernel takes 1 - beta from the fp32 beta (and its bias corrections
    # from the same value, so its PARAMETERS meet the gate above), torch from the fp64 one -- its moments may differ from torch's by the
    # rounding of beta, half an fp32 ulp of beta relative to 1 - beta, which is the extra term of that one set
    beta_term = dict(exp_avg=2.0 ** -24 * 0.9 / 0.1, exp_avg_sq=2.0 ** -24 * 0.999 / 0.001) if (name == 'Adam' and not kwargs) else {}
    for n in names:
        e_f = e_32 = smax = 0.0
        for i, (a, b) in enumerate(RANGES):
            s64 = refs[torch.float64][1].state[refs[torch.float64][0][i]][n]
            s32 = refs[torch.float32][1].state[refs[torch.float32][0][i]][n]
            e_f = max(e_f, float((opt._state[n][a:b].cpu().double() - s64).abs().max()))
            e_32 = max(e_32, float((s32.double() - s64).abs().max()))
            smax = max(smax, float(s64.abs().max()))
        print(f'    state {n}: fused {e_f:.3e}  torch fp32 {e_32:.3e}')
        assert e_f <= 2 * e_32 + float(np.spacing(np.float32(smax))) + beta_term.get(n, 0.0) * smax, (n, e_f, e_32)
    # outside the ranges: bit-identical
    out = ~inside
    assert torch.equal(_bits(got)[out], _bits(p0)[out])
    for n in names:
        assert torch.equal(_bits(opt._state[n])[out], _bits(marks[n])[out]), n
    assert opt._step == 5


# ------------------------------------------------------------------------------------------------------------------------
# 2. lg_l2_loss against nn.MSELoss
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1003, 100003, 2097155])
def test_l2_loss_vs_mseloss(n):
    """n not a multiple of 4, n_global = 2 n_local, scale = 0.5.  The loss (this rank's share of the global mean) against fp64
    nn.MSELoss within 2 x the error of fp32 nn.MSELoss + one fp32 ulp; every dout element within one fp32 ulp of
    2 (out - gt) scale / n_global evaluated in fp32, and the whole of it against the fp64 autograd gradient."""
    from lgteun_amd import _lib
    from lgteun_amd.engine import _ptr, _stream_ptr
    assert n % 4
    gen = torch.Generator().manual_seed(n)
    out, gt = torch.rand(n, generator=gen), torch.rand(n, generator=gen)
    n_global, scale = 2 * n, 0.5
    d_out, d_gt = out.cuda(), gt.cuda()
    dout = torch.full((n + 8,), 7.0, device='cuda')       # 8 floats behind the end: must stay as they are
    accum = torch.zeros(1, device='cuda')
    lib = _lib.lib()
    for call in range(2):                                 # the scalar is ACCUMULATED: two calls, twice the loss
        _lib.check(lib.lg_l2_loss(_ptr(d_out), _ptr(d_gt), _ptr(dout), _ptr(accum), n, n_global, scale, _stream_ptr()), 'lg_l2_loss')
        if call == 0:
            got = float(accum.item())
    twice = float(accum.item())
    # (a) fp64 and (b) fp32 nn.MSELoss on the host; the share of a rank that holds half of the global batch is exactly half of its local mean
    o64 = out.double().requires_grad_(True)
    l64 = torch.nn.MSELoss()(o64, gt.double()) * n / n_global
    (l64 * scale).backward()
    a = float(l64)
    b = float(torch.nn.MSELoss()(out, gt)) * n / n_global
    ulp = float(np.spacing(np.float32(a)))
    print(f'n {n}: |fused - fp64| {abs(got - a):.3e}  |torch fp32 - fp64| {abs(b - a):.3e}  ulp {ulp:.3e}')
    assert abs(got - a) <= 2 * abs(b - a) + ulp, (got, a, b)
    # each call adds one float rounded from the fp64 sum (half an ulp) and the second add rounds at the magnitude of the total
    assert abs(twice - 2 * a) <= 2 * ulp + 2 * float(np.spacing(np.float32(2 * a)))
    want = (2 * (out - gt) * scale) / n_global            # fp32 on the host
    g = dout[:n].cpu()
    assert bool((g - want).abs().le(T(np.spacing(want.abs().numpy()))).all()), float((g - want).abs().max())
    assert rel_l2(g, o64.grad) < 1e-6
    assert bool((dout[n:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------------
# runner plumbing shared by 3, 4 and 6
# ------------------------------------------------------------------------------------------------------------------------
def _runner(tmp_path, loss, optim_entry, K=2, step_size=1, gamma=0.85, tag='r'):
    """the runner of test_three_train_iterations_vs_reference_runner (tests/test_gpu_backward.py): C = 4, name-hashed weights,
    core.eval() and optim.dropout = False -> no dropout on either route"""
    import lgteun_amd
    from lgteun_amd.compat import Config
    cfg = Config(dict(ms_chans=4, work_dir=str(tmp_path / tag), datas='GF-2', cuda=True, max_iter=3, bit_depth=11,
                      loss_cfg={'rec_loss': dict(type=loss, w=1.)}, optim_cfg={'core_module': dict(optim_entry)},
                      sched_cfg=dict(step_size=step_size, gamma=gamma), model_cfg={'core_module': dict(stage=K)}))
    runner = lgteun_amd.build_model('UnlgFormer', cfg, logging.getLogger('t'), None, None, None)
    sd = dw.fill_state_dict(state_shapes(4, K), salt=0)
    runner.module_dict['core_module'].load_state_dict({k: T(v) for k, v in sd.items()})
    return runner, sd


def _start(runner):
    runner.set_cuda()
    runner.module_dict['core_module'].eval()
    runner.set_optim()
    runner.optim_dict['core_module'].dropout = False
    runner.set_sched()


def _batch(B=2, h=8, seed=11, kind='smooth'):
    ms, pan, gt = dw.make_inputs(B, 4, h, h, seed=seed, kind=kind)
    return dict(input_lr=T(ms).cuda(), input_pan=T(pan).cuda(), target=T(gt).cuda(), image_id=['a', 'b'])


def _iterate(runner, batch, its):
    losses, lrs = [], []
    runner.print_train_log = lambda it, res, freq=10: losses.append(res['full_loss'])
    for it in its:
        lrs.append(runner.optim_dict['core_module'].param_groups[0]['lr'])
        runner.train_iter(it, batch, log_freq=1)
        runner.sched_dict['core_module'].step()
    return losses, lrs


# ------------------------------------------------------------------------------------------------------------------------
# 3. route equivalence, end to end
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss,entry', [
    ('l2', dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3)),
    ('l2', dict(type='AdamW', lr=1.5e-3, weight_decay=1e-2)),
    ('l1', dict(type='SGD', lr=1e-2, momentum=0.9)),
    ('l1', dict(type='RMSprop', lr=1.5e-3)),
], ids=['l2-Adam', 'l2-AdamW', 'l1-SGD', 'l1-RMSprop'])
def test_fused_route_agrees_with_the_torch_route(tmp_path, loss, entry):
    """three train_iter calls (StepLR every iteration) with the fused class and with `fused=False`: both routes run the same gradient
    kernels, so only the loss and the optimizer arithmetic differ.  Losses to rtol 1e-5, live weights to rel_l2 < 1e-5, and the dead
    stage keeps its initial bits on BOTH routes (no gradient: no weight decay, no state).  Where a live tensor is looser than 1e-5 the
    measured value and the tensor are reported and the weights are gated at 2 x the fp32-vs-fp64 spread of torch.optim that
    test_optimizer_step_vs_torch measures for that optimizer (+ its one-ulp floor), as max|fused route - torch route|.

    Why the gate needs the kernels to round like torch's: softmax does not see a key bias, so the gradient of the key third of every
    to_qkv bias is the rounding noise of a sum that cancels (~1e-10), and it changes completely with the last bit of the weights.
    Adam, AdamW and RMSprop divide by the root of that noise's own running square: such an element moves by the order of lr whatever
    the size of its gradient, with the sign of the noise.  Two routes that differ in one rounding after the first iteration are
    therefore 1e-4 apart on those tensors after the third (measured with an earlier form of k_optim: AdamW 4.3e-5, RMSprop 1.4e-4).
    lg_optim_step and lg_l2_loss round every step the way torch's device kernels do, so the routes stay on the same bits.
    Measured on the MI355X, worst live tensor: l2 + AdamW, l1 + SGD, l1 + RMSprop rel_l2 0 (bit-identical weights); l2 + Adam 9.8e-6
    (local_mixer.to_qkv.bias of decoder block 1: the plain Adam set is lg_adam_step, whose arithmetic is not torch's to the bit)."""
    batch = _batch()
    res = {}
    for fused in (True, False):
        runner, sd = _runner(tmp_path, loss, dict(entry, fused=fused), tag=f'f{int(fused)}')
        _start(runner)
        assert bool(getattr(runner.optim_dict['core_module'], 'is_fused_lgteun', False)) == fused
        losses, _ = _iterate(runner, batch, range(1, 4))
        res[fused] = (losses, {k: v.detach().cpu() for k, v in runner.module_dict['core_module'].state_dict().items()})
        for k, v in res[fused][1].items():
            if k.startswith('prior_module.0.'):
                assert torch.equal(v, T(sd[k])), (fused, k)
    worst = max((rel_l2(res[True][1][k], v), k) for k, v in res[False][1].items() if not k.startswith('prior_module.0.'))
    print(f'{loss} + {entry["type"]}: losses fused {res[True][0]} torch {res[False][0]}; worst live weight rel_l2 {worst[0]:.3e} ({worst[1]})')
    assert len(res[True][0]) == 3 and np.allclose(res[True][0], res[False][0], rtol=1e-5, atol=0), (res[True][0], res[False][0])
    if worst[0] >= 1e-5:
        kw = {k: v for k, v in entry.items() if k not in ('type', 'lr')}
        spread, pmax = _torch_spread(_torch_runs(entry['type'], kw, *_synthetic()[:2]))
        gate = 2 * spread + float(np.spacing(np.float32(pmax)))
        diff = max((float((res[True][1][k] - v).abs().max()), k) for k, v in res[False][1].items() if not k.startswith('prior_module.0.'))
        print(f'    looser than 1e-5: {worst}; max|fused route - torch route| {diff[0]:.3e} ({diff[1]}) against 2 x {spread:.3e} + floor = {gate:.3e}')
        assert diff[0] <= gate, (worst, diff, gate)


# ------------------------------------------------------------------------------------------------------------------------
# 4. the reference runner's own three iterations with l2 + AdamW
# ------------------------------------------------------------------------------------------------------------------------
def test_three_l2_adamw_iterations_vs_reference_runner(tmp_path):
    """UnlgFormer.train_iter x3 with loss type l2, fused AdamW and StepLR-per-iteration against the reference runner's losses / weights
    (tests/golden/train3_l2_adamw_c4_k2_p32.npz; its parameters sit in the file).  The gates of
    test_three_train_iterations_vs_reference_runner: the network and the sizes are the same, only the loss and the update rule differ."""
    g = load_gold('train3_l2_adamw_c4_k2_p32')
    m = json.loads(str(g['meta']))
    runner, sd = _runner(tmp_path, m['loss'], dict(type=m['optim'], betas=tuple(m['betas']), lr=m['lr'], weight_decay=m['weight_decay']),
                         K=m['K'], step_size=m['step_size'], gamma=m['gamma'])
    _start(runner)
    assert type(runner.optim_dict['core_module']).__name__ == 'FusedAdamW'
    losses, lrs = _iterate(runner, _batch(m['B'], m['h'], m['seed'], m['kind']), range(1, 4))
    assert np.allclose(lrs, g['lrs'], rtol=1e-12)
    assert np.allclose(losses, g['losses'], rtol=5e-4), (losses, g['losses'])
    for k, v in runner.module_dict['core_module'].state_dict().items():
        if k.startswith('prior_module.0.'):
            assert torch.equal(v.cpu(), T(sd[k]))          # dead stage: no gradient, so no decay either
        else:
            assert rel_l2(v.cpu(), g[k.replace('.', '/')]) < 1e-2, k


# ------------------------------------------------------------------------------------------------------------------------
# 5. 'chained' mode and the data-parallel path
# ------------------------------------------------------------------------------------------------------------------------
def _l2_adamw_steps(net, steps, eng=None):
    from lgteun_amd import FusedAdamW
    batch = _batch()
    opt = FusedAdamW(net.parameters(), lr=1.5e-3, weight_decay=1e-2)
    opt.dropout = False
    eng = eng or net.engine()
    for _ in range(steps):
        eng.train_step(batch['input_lr'], batch['input_pan'], batch['target'], opt, loss_type='l2')
    torch.cuda.synchronize()
    return eng


def test_chained_mode_l2_adamw_moves_every_stage():
    from gpu_helpers import make_module
    net = make_module(4, 2)
    net.mode = 'chained'
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    eng = _l2_adamw_steps(net, 1)
    assert eng.live_ranges == [(0, eng.total)]              # no dead range
    same = [k for k, v in net.state_dict().items() if torch.equal(v.cpu(), before[k])]
    assert not same, same
    # more than the decay alone (p * (1 - lr * wd) moves a weight by 1.5e-5 of itself): the Adam update of the first step is ~lr per element
    for k in ('prior_module.0.tail.1.weight', 'prior_module.1.tail.1.weight', 'D.1.weight'):
        assert float((net.state_dict()[k].cpu() - before[k]).abs().max()) > 1e-3, k


def test_one_rank_process_group_l2_adamw_is_bitwise_the_unattached_run(tmp_path):
    """the bucket all-reduce and the n_global path of train_step with the new loss and optimizer, in a gloo group of ONE rank joined
    by this process (attach_ddp(force=True)): a sum over one rank is the identity, so three steps give the bits of the unattached
    run.  (Two ranks on hardware with the new optimizers: not run here -- a process that has initialised the GPU starts no programs;
    nothing between the loss kernel and step_flat differs from what the two-rank Adam tests cover.)"""
    import torch.distributed as dist
    from gpu_helpers import make_module
    net0 = make_module(4, 2)
    _l2_adamw_steps(net0, 3)
    want = net0.engine().flat.cpu().numpy().copy()
    first = make_module(4, 2).engine().flat.cpu().numpy().copy()
    assert not dist.is_initialized()
    dist.init_process_group('gloo', store=dist.FileStore(str(tmp_path / 'store'), 1), rank=0, world_size=1)
    try:
        net1 = make_module(4, 2)
        eng = net1.attach_ddp(force=True)
        assert eng.force_collectives and eng.buckets is not None and eng.world == 1
        _l2_adamw_steps(net1, 3, eng)
        got = eng.flat.cpu().numpy().copy()
        a, b = eng.live_ranges[0][1], eng.live_ranges[1][0]
    finally:
        dist.destroy_process_group()
    assert not dist.is_initialized()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert b > a and np.array_equal(got[a:b].view(np.int32), first[a:b].view(np.int32))      # the dead range: its initial bits
    assert not np.array_equal(got[:a], first[:a])


# ------------------------------------------------------------------------------------------------------------------------
# 6. checkpoint resume
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry,buffers', [
    (dict(type='SGD', lr=1e-2, momentum=0.9), ['momentum_buffer']),
    (dict(type='RMSprop', lr=1.5e-3, centered=True), ['square_avg', 'grad_avg']),
], ids=['SGD-momentum', 'RMSprop-centered'])
def test_checkpoint_resume_is_bitwise(tmp_path, entry, buffers):
    """two fused steps, Base_model.save, load_checkpoint into a fresh runner (the resume order of main.py: load, set_cuda, set_optim,
    set_sched), one more step == three uninterrupted steps, bit for bit (step count and every state buffer travel in sd['lgteun'])"""
    batch = _batch()
    a, _ = _runner(tmp_path, 'l1', entry, step_size=100, tag='a')
    _start(a)
    _iterate(a, batch, range(1, 4))
    want = {k: v.detach().cpu() for k, v in a.module_dict['core_module'].state_dict().items()}
    b, _ = _runner(tmp_path, 'l1', entry, step_size=100, tag='b')
    _start(b)
    _iterate(b, batch, range(1, 3))
    path = b.save(iter_id=2)
    c, _ = _runner(tmp_path, 'l1', entry, step_size=100, tag='c')
    c.load_checkpoint(path)
    assert c.last_iter == 2
    _start(c)
    oc = c.optim_dict['core_module']
    assert oc.is_fused_lgteun and oc._step == 2 and sorted(oc._state) == sorted(buffers) and not any(v.is_cuda for v in oc._state.values())
    _iterate(c, batch, [3])
    assert oc._step == 3 and all(v.is_cuda for v in oc._state.values())      # the restored buffers moved to the device with the step
    for k, v in c.module_dict['core_module'].state_dict().items():
        assert torch.equal(v.cpu(), want[k]), k
