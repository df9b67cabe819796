"""CPU (no GPU) checks of the fused optimizers' host side: which class `set_optim` picks, the options in `param_groups[0]`, torch's
argument validation, the checkpoint round trip of step count and state buffers -- and that the reference-generated l2 + AdamW fixture
is reproduced by the oracle with torch.optim.AdamW, i.e. that the gates of its GPU test can be met by the reference arithmetic."""
import json
import logging

import numpy as np
import pytest
import torch

from conftest import load_gold
from helpers import det_params, rel_l2
from oracle import detweights as dw
from oracle import lgteun_oracle as orc

T = torch.from_numpy

ENTRIES = [
    ('FusedAdam', dict(type='Adam', lr=1e-3, weight_decay=1e-4)),
    ('FusedAdam', dict(type='Adam', lr=1e-3, amsgrad=True)),
    ('FusedAdamW', dict(type='AdamW', lr=1e-3, weight_decay=1e-2)),
    ('FusedSGD', dict(type='SGD', lr=1e-2, momentum=0.9, nesterov=True)),
    ('FusedRMSprop', dict(type='RMSprop', lr=1e-3, centered=True, momentum=0.9)),
]


def _runner(tmp_path, optim_entry, loss='l1'):
    """a runner built like test_runner_from_config_file (tests/test_boundary_cpu.py), with the optimizer entry under test"""
    import lgteun_amd
    from lgteun_amd.compat import Config
    cfg_file = tmp_path / 'unlg_former.py'
    cfg_file.write_text(
        "name = 'LGTEUN'\nms_chans = 4\nmodel_type = 'UnlgFormer'\ndatas = 'GF-2'\n"
        f"work_dir = r'{tmp_path}/out'\ncuda = True\nbit_depth = 11\nmax_iter = 10\nseed = 19971118\n"
        f"optim_cfg = {{'core_module': dict({', '.join(f'{k}={v!r}' for k, v in optim_entry.items())})}}\n"
        f"sched_cfg = dict(step_size=1, gamma=0.85)\nloss_cfg = {{'rec_loss': dict(type={loss!r}, w=1.)}}\n"
        "model_cfg = {'core_module': dict(stage=2)}\n")
    cfg = Config.fromfile(str(cfg_file))
    return lgteun_amd.build_model(cfg.model_type, cfg, logging.getLogger('t'), None, None, None)


@pytest.mark.parametrize('cls,entry', ENTRIES)
def test_set_optim_picks_the_fused_class(tmp_path, cls, entry):
    import lgteun_amd
    runner = _runner(tmp_path, entry)
    runner.set_optim()
    runner.set_sched()
    opt = runner.optim_dict['core_module']
    assert getattr(opt, 'is_fused_lgteun', False) and type(opt) is getattr(lgteun_amd, cls)
    assert isinstance(opt, torch.optim.Optimizer) and opt.dropout is True and callable(opt.step_flat)
    # the options sit in param_groups[0] under torch's names, with torch's defaults for the ones the entry leaves out
    g = opt.param_groups[0]
    want = getattr(torch.optim, entry['type'])([torch.nn.Parameter(torch.zeros(1))], **{k: v for k, v in entry.items() if k != 'type'})
    for k in set(g) - {'params', 'initial_lr'}:          # initial_lr: StepLR's own entry
        assert g[k] == want.param_groups[0][k], k
    # StepLR drives lr
    lrs = []
    for _ in range(3):
        lrs.append(opt.param_groups[0]['lr'])
        runner.sched_dict['core_module'].step()
    assert np.allclose(lrs, [entry['lr'] * 0.85 ** i for i in range(3)], rtol=1e-12)


@pytest.mark.parametrize('cls,entry', ENTRIES + [('FusedAdam', dict(type='Adam', lr=1e-3))])
def test_fused_false_opts_out(tmp_path, cls, entry):
    runner = _runner(tmp_path, dict(entry, fused=False))
    runner.set_optim()
    opt = runner.optim_dict['core_module']
    assert type(opt) is getattr(torch.optim, entry['type']) and not getattr(opt, 'is_fused_lgteun', False)
    assert all(opt.param_groups[0][k] == v for k, v in entry.items() if k != 'type')


def _p():
    return [torch.nn.Parameter(torch.zeros(3))]


@pytest.mark.parametrize('name,kwargs', [
    ('Adam', dict(lr=-1e-3)), ('Adam', dict(eps=-1e-8)), ('Adam', dict(weight_decay=-1e-4)), ('Adam', dict(betas=(1.0, 0.999))),
    ('Adam', dict(betas=(0.9, -0.1))),
    ('AdamW', dict(lr=-1e-3)), ('AdamW', dict(eps=-1.0)), ('AdamW', dict(weight_decay=-1e-2)), ('AdamW', dict(betas=(0.9, 1.0))),
    ('SGD', dict(lr=-1e-2)), ('SGD', dict(momentum=-0.5)), ('SGD', dict(weight_decay=-1e-4)),
    ('SGD', dict(nesterov=True)), ('SGD', dict(nesterov=True, momentum=0.9, dampening=0.1)),
    ('RMSprop', dict(lr=-1e-2)), ('RMSprop', dict(eps=-1e-8)), ('RMSprop', dict(momentum=-0.1)), ('RMSprop', dict(weight_decay=-1.0)),
    ('RMSprop', dict(alpha=-0.5)),
])
def test_invalid_arguments_raise_what_torch_raises(name, kwargs):
    import lgteun_amd
    with pytest.raises(ValueError):
        getattr(torch.optim, name)(_p(), **kwargs)
    with pytest.raises(ValueError):
        getattr(lgteun_amd, 'Fused' + name)(_p(), **kwargs)


@pytest.mark.parametrize('name', ['Adam', 'AdamW', 'SGD', 'RMSprop'])
@pytest.mark.parametrize('kw', ['maximize', 'foreach', 'capturable', 'differentiable', 'no_such_option'])
def test_options_outside_the_fused_set_name_the_way_out(name, kw):
    import lgteun_amd
    with pytest.raises(TypeError, match='fused=False'):
        getattr(lgteun_amd, 'Fused' + name)(_p(), **{kw: False})


def test_defaults_are_torchs():
    import lgteun_amd
    for name in ('Adam', 'AdamW', 'SGD', 'RMSprop'):
        got = getattr(lgteun_amd, 'Fused' + name)(_p()).param_groups[0]
        want = getattr(torch.optim, name)(_p()).param_groups[0]
        for k in set(got) - {'params'}:
            assert got[k] == want[k], (name, k)


@pytest.mark.parametrize('name,kwargs,buffers', [
    ('Adam', dict(), ['exp_avg', 'exp_avg_sq']),
    ('Adam', dict(amsgrad=True, weight_decay=1e-4), ['exp_avg', 'exp_avg_sq', 'max_exp_avg_sq']),
    ('AdamW', dict(amsgrad=True), ['exp_avg', 'exp_avg_sq', 'max_exp_avg_sq']),
    ('SGD', dict(), []),
    ('SGD', dict(momentum=0.9), ['momentum_buffer']),
    ('RMSprop', dict(), ['square_avg']),
    ('RMSprop', dict(momentum=0.5, centered=True), ['square_avg', 'momentum_buffer', 'grad_avg']),
])
def test_state_round_trip(tmp_path, name, kwargs, buffers):
    """state_dict() -> torch.save -> weights_only load -> load_state_dict() on a fresh instance: the step count, lr and every buffer"""
    import lgteun_amd
    cls = getattr(lgteun_amd, 'Fused' + name)
    a = cls(_p(), lr=3e-3, **kwargs)
    assert [n for n in a.state_names() if n is not None] == buffers
    a._step = 5
    a._state = {n: torch.arange(7, dtype=torch.float32) + i for i, n in enumerate(buffers)}
    a.param_groups[0]['lr'] = 1e-3                      # what a scheduler left behind
    sd = a.state_dict()
    assert sd['lgteun']['step'] == 5
    torch.save(sd, tmp_path / 'o.pth')
    sd = torch.load(tmp_path / 'o.pth', map_location='cpu', weights_only=True)     # what Base_model._read_checkpoint does
    b = cls(_p(), lr=3e-3, **kwargs)
    b.load_state_dict(sd)
    assert 'lgteun' in sd                               # the caller's dict stays as it was
    assert b._step == 5 and b.param_groups[0]['lr'] == 1e-3
    assert sorted(b._state) == sorted(buffers)
    for n in buffers:
        assert torch.equal(b._state[n], a._state[n])


def test_l2_adamw_fixture_is_reproduced_by_the_oracle_with_torch_adamw():
    """the fixture tests/golden/train3_l2_adamw_c4_k2_p32.npz (three iterations of the reference runner with loss type l2 and AdamW)
    against the oracle's forward + autograd, nn.MSELoss and torch.optim.AdamW over the live tensors, at the gates of the GPU test
    (losses rtol 5e-4, live weights rel_l2 < 1e-2): the reference arithmetic alone satisfies them."""
    g = load_gold('train3_l2_adamw_c4_k2_p32')
    m = json.loads(str(g['meta']))
    assert m['loss'] == 'l2' and m['optim'] == 'AdamW'
    ms, pan, gt = dw.make_inputs(m['B'], m['C'], m['h'], m['h'], seed=m['seed'], kind=m['kind'])
    P = det_params(m['C'], m['K'], requires_grad=True)
    first = {k: v.detach().clone() for k, v in P.items()}
    opt = torch.optim.AdamW(list(P.values()), lr=m['lr'], betas=tuple(m['betas']), weight_decay=m['weight_decay'])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=m['step_size'], gamma=m['gamma'])
    losses, lrs = [], []
    for _ in range(3):
        lrs.append(opt.param_groups[0]['lr'])
        opt.zero_grad()
        loss = torch.nn.MSELoss()(orc.forward(P, T(ms), T(pan), m['K']), T(gt))
        loss.backward()
        losses.append(loss.item())
        opt.step()
        sched.step()
    assert np.allclose(lrs, g['lrs'], rtol=1e-12)
    assert np.allclose(losses, g['losses'], rtol=5e-4), (losses, g['losses'])
    for k, v in P.items():
        if k.startswith('prior_module.0.'):
            assert torch.equal(v.detach(), first[k]), k          # no gradient: no decay either
        else:
            assert rel_l2(v.detach(), g[k.replace('.', '/')]) < 1e-2, k


def test_checkpoint_written_before_the_options_existed_loads():
    """a FusedAdam state_dict whose param_groups hold lr / betas / eps only (what this class wrote before it had weight_decay and
    amsgrad) loads, and the missing options take their defaults"""
    import lgteun_amd
    a = lgteun_amd.FusedAdam(_p(), lr=2e-3)
    sd = a.state_dict()
    for g in sd['param_groups']:
        del g['weight_decay'], g['amsgrad']
    sd['lgteun'] = dict(step=4, state=dict(exp_avg=torch.ones(5), exp_avg_sq=torch.ones(5)))
    b = lgteun_amd.FusedAdam(_p(), lr=1e-3)
    b.load_state_dict(sd)
    g = b.param_groups[0]
    assert g['lr'] == 2e-3 and g['weight_decay'] == 0 and g['amsgrad'] is False and b._step == 4
    assert b.state_names() == ['exp_avg', 'exp_avg_sq', None]
