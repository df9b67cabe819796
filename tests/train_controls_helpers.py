"""Shared by tests/test_gpu_train_controls.py and tests/ddp_train_controls_worker.py: the small runner (C = 4, K = 2, PAN 32 x 32, B = 2,
name-hashed weights, no dropout on either route) with an optional `train_cfg`, fixed micro-batches, and bit-level comparisons."""
import logging

import torch

from helpers import state_shapes
from oracle import detweights as dw

T = torch.from_numpy
C, K = 4, 2


def make_runner(tmp_path, loss, optim_entry, train_cfg=None, step_size=1, gamma=0.85, tag='r', mode=None, loaders=(None, None, None)):
    import lgteun_amd
    from lgteun_amd.compat import Config
    cfg = dict(ms_chans=C, work_dir=str(tmp_path / tag), datas='GF-2', cuda=True, max_iter=8, bit_depth=11,
               loss_cfg={'rec_loss': dict(type=loss, w=1.)}, optim_cfg={'core_module': dict(optim_entry)},
               sched_cfg=dict(step_size=step_size, gamma=gamma), model_cfg={'core_module': dict(stage=K)})
    if train_cfg is not None:
        cfg['train_cfg'] = dict(train_cfg)
    runner = lgteun_amd.build_model('UnlgFormer', Config(cfg), logging.getLogger('t'), *loaders)
    sd = dw.fill_state_dict(state_shapes(C, K), salt=0)
    runner.module_dict['core_module'].load_state_dict({k: T(v) for k, v in sd.items()})
    if mode is not None:
        runner.module_dict['core_module'].mode = mode
    return runner, sd


def start(runner):
    """the order of main.py: set_cuda, set_optim, set_sched; eval mode and optim.dropout = False switch dropout off on both routes"""
    runner.set_cuda()
    runner.module_dict['core_module'].eval()
    runner.set_optim()
    runner.optim_dict['core_module'].dropout = False
    runner.set_sched()
    return runner


def make_batch(B=2, h=8, seed=11, kind='smooth'):
    ms, pan, gt = dw.make_inputs(B, C, h, h, seed=seed, kind=kind)
    return dict(input_lr=T(ms).cuda(), input_pan=T(pan).cuda(), target=T(gt).cuda(), image_id=[f'i{i}' for i in range(B)])


def iterate(runner, batches, its):
    """train_iter + one StepLR tick per call, as Base_model.train does; batches: one batch for every call, or a list taken in turn"""
    losses = []
    runner.print_train_log = lambda it, res, freq=10: losses.append(res['full_loss'])
    for n, it in enumerate(its):
        batch = batches[(it - 1) % len(batches)] if isinstance(batches, (list, tuple)) else batches
        runner.train_iter(it, batch, log_freq=1)
        runner.sched_dict['core_module'].step()
    return losses


def engine_of(runner):
    return runner.module_dict['core_module'].engine()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def weights_of(runner):
    return {k: v.detach().cpu().clone() for k, v in runner.module_dict['core_module'].state_dict().items()}
