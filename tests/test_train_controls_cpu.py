"""CPU (no GPU, library built) checks of the train-step controls' host side: `TrainControls` validation, which calls end an accumulation
window, the checkpoint round trip of the averaged weights and the window position, how `set_optim` reads `cfg.train_cfg`, and the
argument checks of `lg_grad_norm` / `lg_optim_step_ex`."""
import ctypes
import logging

import pytest
import torch


def _p():
    return [torch.nn.Parameter(torch.zeros(3))]


def _runner(tmp_path, optim_entry, train_cfg=None):
    """a runner built like the one of tests/test_fused_optim_cpu.py, with an optional train_cfg"""
    import lgteun_amd
    from lgteun_amd.compat import Config
    cfg = dict(name='LGTEUN', ms_chans=4, model_type='UnlgFormer', datas='GF-2', work_dir=str(tmp_path / 'out'), cuda=True, bit_depth=11,
               max_iter=10, optim_cfg={'core_module': dict(optim_entry)}, sched_cfg=dict(step_size=1, gamma=0.85),
               loss_cfg={'rec_loss': dict(type='l1', w=1.)}, model_cfg={'core_module': dict(stage=2)})
    if train_cfg is not None:
        cfg['train_cfg'] = dict(train_cfg)
    return lgteun_amd.build_model('UnlgFormer', Config(cfg), logging.getLogger('t'), None, None, None)


# ------------------------------------------------------------------------------------------------------------------------
# TrainControls
# ------------------------------------------------------------------------------------------------------------------------
def test_defaults_switch_everything_off():
    from lgteun_amd import TrainControls
    c = TrainControls()
    assert c.as_dict() == dict(accumulate=1, max_grad_norm=None, ema_decay=None, eval_ema=True)
    c = TrainControls(accumulate=4, max_grad_norm=1, ema_decay=0.999, eval_ema=False)
    assert c.as_dict() == dict(accumulate=4, max_grad_norm=1.0, ema_decay=0.999, eval_ema=False)


@pytest.mark.parametrize('kwargs,match', [
    (dict(accumulate=0), 'accumulate must be an integer >= 1'),
    (dict(accumulate=-2), 'accumulate must be an integer >= 1'),
    (dict(accumulate=2.0), 'accumulate must be an integer >= 1'),
    (dict(accumulate=True), 'accumulate must be an integer >= 1'),
    (dict(accumulate=None), 'accumulate must be an integer >= 1'),
    (dict(max_grad_norm=0), 'max_grad_norm must be None .* or a finite number > 0'),
    (dict(max_grad_norm=-1.0), 'max_grad_norm must be None .* or a finite number > 0'),
    (dict(max_grad_norm=float('inf')), 'max_grad_norm must be None .* or a finite number > 0'),
    (dict(max_grad_norm=float('nan')), 'max_grad_norm must be None .* or a finite number > 0'),
    (dict(max_grad_norm='1'), 'max_grad_norm must be None .* or a finite number > 0'),
    (dict(ema_decay=0.5), 'ema_decay must be None .* or lie in 0.5 < decay < 1'),
    (dict(ema_decay=1.0), 'ema_decay must be None .* or lie in 0.5 < decay < 1'),
    (dict(ema_decay=0.1), 'ema_decay must be None .* or lie in 0.5 < decay < 1'),
    (dict(ema_decay=float('nan')), 'ema_decay must be None .* or lie in 0.5 < decay < 1'),
    (dict(ema_decay='0.9'), 'ema_decay must be None .* or lie in 0.5 < decay < 1'),
])
def test_bad_values_say_what_to_change(kwargs, match):
    from lgteun_amd import TrainControls
    with pytest.raises(ValueError, match=match):
        TrainControls(**kwargs)


@pytest.mark.parametrize('A,ends', [(1, [True] * 6), (2, [False, True] * 3), (3, [False, False, True] * 2)])
def test_which_calls_end_a_window(A, ends):
    from lgteun_amd import TrainControls
    c = TrainControls(accumulate=A)
    assert [c.is_window_end(i) for i in range(6)] == ends


def test_controls_are_attached_not_constructed():
    """the options do not go through the constructors: an unknown keyword keeps raising the TypeError that names the way out"""
    import lgteun_amd
    for kw in ('accumulate', 'max_grad_norm', 'ema_decay'):
        with pytest.raises(TypeError, match='fused=False'):
            lgteun_amd.FusedAdam(_p(), **{kw: 2})
    opt = lgteun_amd.FusedSGD(_p(), lr=1e-2)
    assert opt.controls is None
    c = lgteun_amd.TrainControls(accumulate=2)
    assert opt.set_controls(c) is opt and opt.controls is c
    with pytest.raises(ValueError, match='TrainControls'):
        opt.set_controls(dict(accumulate=2))
    opt.set_controls(None)
    assert opt.controls is None


# ------------------------------------------------------------------------------------------------------------------------
# checkpoints
# ------------------------------------------------------------------------------------------------------------------------
def _save_load(tmp_path, sd):
    torch.save(sd, tmp_path / 'o.pth')
    return torch.load(tmp_path / 'o.pth', map_location='cpu', weights_only=True)     # what Base_model._read_checkpoint does


def test_state_round_trip_with_controls(tmp_path):
    """the 'ema' tensor, the position inside the window and the gradients its earlier calls accumulated survive
    state_dict -> torch.save -> weights_only load -> load_state_dict"""
    import lgteun_amd
    ctl = lgteun_amd.TrainControls(accumulate=3, max_grad_norm=2.0, ema_decay=0.99)
    a = lgteun_amd.FusedAdamW(_p(), lr=3e-3).set_controls(ctl)
    a._step = 5
    a._state = dict(exp_avg=torch.arange(7.), exp_avg_sq=torch.arange(7.) + 1, ema=torch.arange(7.) + 2)
    a._window_pos, a._window_gbuf = 2, torch.arange(11.)
    sd = a.state_dict()
    assert set(sd['lgteun']) == {'step', 'state', 'window'} and sd['lgteun']['window']['pos'] == 2
    sd = _save_load(tmp_path, sd)
    b = lgteun_amd.FusedAdamW(_p(), lr=3e-3).set_controls(lgteun_amd.TrainControls(accumulate=3, max_grad_norm=2.0, ema_decay=0.99))
    b.load_state_dict(sd)
    assert b._step == 5 and b._window_pos == 2 and torch.equal(b._window_gbuf, torch.arange(11.))
    assert sorted(b._state) == ['ema', 'exp_avg', 'exp_avg_sq'] and torch.equal(b._state['ema'], torch.arange(7.) + 2)
    # at a window boundary no gradients travel
    a._window_pos = 0
    assert a.state_dict()['lgteun']['window'] == dict(pos=0, accumulate=3, gbuf=None)


def test_checkpoints_cross_between_runs_with_and_without_controls(tmp_path):
    import lgteun_amd
    plain = lgteun_amd.FusedSGD(_p(), lr=1e-2, momentum=0.9)
    plain._step, plain._state = 4, dict(momentum_buffer=torch.ones(5))
    sd_plain = _save_load(tmp_path, plain.state_dict())
    assert set(sd_plain['lgteun']) == {'step', 'state'}
    # (a) written without controls, loaded with them: the state is kept, the window starts at its first call
    b = lgteun_amd.FusedSGD(_p(), lr=1e-2, momentum=0.9).set_controls(lgteun_amd.TrainControls(accumulate=2, ema_decay=0.9))
    b.load_state_dict(sd_plain)
    assert b._step == 4 and b._window_pos == 0 and b._window_gbuf is None and torch.equal(b._state['momentum_buffer'], torch.ones(5))
    # (b) written with controls at a window boundary, loaded without: the step count and the buffers load
    b._state = dict(b._state, ema=torch.zeros(5))
    sd_ctl = _save_load(tmp_path, b.state_dict())
    c = lgteun_amd.FusedSGD(_p(), lr=1e-2, momentum=0.9)
    c.load_state_dict(sd_ctl)
    assert c._step == 4 and c._window_pos == 0 and torch.equal(c._state['momentum_buffer'], torch.ones(5))
    # (c) written INSIDE a window: only a run with the same window can continue it, and the error says so
    b._window_pos, b._window_gbuf = 1, torch.zeros(9)
    sd_mid = _save_load(tmp_path, b.state_dict())
    with pytest.raises(ValueError, match='accumulate=2'):
        lgteun_amd.FusedSGD(_p(), lr=1e-2, momentum=0.9).load_state_dict(sd_mid)
    with pytest.raises(ValueError, match='accumulate=2'):
        lgteun_amd.FusedSGD(_p(), lr=1e-2, momentum=0.9).set_controls(lgteun_amd.TrainControls(accumulate=3)).load_state_dict(sd_mid)


# ------------------------------------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------------------------------------
def test_set_optim_attaches_train_cfg_on_the_fused_route(tmp_path):
    import lgteun_amd
    runner = _runner(tmp_path, dict(type='AdamW', lr=1e-3), dict(accumulate=2, max_grad_norm=0.5, ema_decay=0.999, eval_ema=False))
    runner.set_optim()
    opt = runner.optim_dict['core_module']
    assert type(opt) is lgteun_amd.FusedAdamW and isinstance(opt.controls, lgteun_amd.TrainControls)
    assert opt.controls.as_dict() == dict(accumulate=2, max_grad_norm=0.5, ema_decay=0.999, eval_ema=False)
    assert set(opt.state_dict()['lgteun']) == {'step', 'state', 'window'}


def test_train_cfg_on_the_torch_route(tmp_path):
    runner = _runner(tmp_path, dict(type='SGD', lr=1e-2, momentum=0.9, fused=False), dict(accumulate=2, max_grad_norm=0.5))
    runner.set_optim()
    opt = runner.optim_dict['core_module']
    assert type(opt) is torch.optim.SGD and opt.lgteun_controls.accumulate == 2 and opt.lgteun_window_pos == 0
    runner = _runner(tmp_path, dict(type='SGD', lr=1e-2, fused=False), dict(ema_decay=0.99))
    with pytest.raises(ValueError, match='ema_decay needs the fused optimizer'):
        runner.set_optim()


def test_train_cfg_is_validated(tmp_path):
    with pytest.raises(ValueError, match='unknown key'):
        _runner(tmp_path, dict(type='Adam', lr=1e-3), dict(clip=1.0)).set_optim()
    with pytest.raises(ValueError, match='accumulate must be an integer'):
        _runner(tmp_path, dict(type='Adam', lr=1e-3), dict(accumulate=0)).set_optim()


@pytest.mark.parametrize('entry', [dict(type='Adam', lr=1e-3), dict(type='SGD', lr=1e-2, momentum=0.9), dict(type='RMSprop', lr=1e-3)])
def test_without_train_cfg_the_optimizer_state_has_todays_keys(tmp_path, entry):
    runner = _runner(tmp_path, entry)
    runner.set_optim()
    opt = runner.optim_dict['core_module']
    assert opt.controls is None
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups', 'lgteun'} and set(sd['lgteun']) == {'step', 'state'}
    assert sd['lgteun'] == dict(step=0, state=None)


# ------------------------------------------------------------------------------------------------------------------------
# the library's argument checks (they run before any HIP call)
# ------------------------------------------------------------------------------------------------------------------------
def _err(lib):
    return lib.lg_last_error().decode()


def test_grad_norm_rejects_bad_arguments():
    from lgteun_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()              # host memory: never dereferenced, every call below is rejected first
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.lg_grad_norm_workspace_bytes(2, 1000)
    assert need == 2 * 4 * 8                    # one fp64 partial per workgroup: 2 ranges x ceil(1000 / 256)
    assert lib.lg_grad_norm_workspace_bytes(1, 512 * 256 + 5) == 512 * 8      # the grid is capped at 512 workgroups per range
    assert lib.lg_grad_norm_workspace_bytes(0, 1000) == 0 and lib.lg_grad_norm_workspace_bytes(2, 0) == 0
    ok = dict(grads=p, ranges=p, n_ranges=2, max_range=1000, max_norm=1.0, out=p, ws=p, ws_bytes=need)
    for change, text in [(dict(grads=None), 'null pointer'), (dict(ranges=None), 'null pointer'), (dict(out=None), 'null pointer'),
                         (dict(ws=None), 'null pointer'), (dict(n_ranges=0), 'n_ranges'), (dict(max_range=0), 'max_range'),
                         (dict(max_norm=0.0), 'max_norm'), (dict(max_norm=float('nan')), 'max_norm'), (dict(max_norm=-1.0), 'max_norm'),
                         (dict(ws_bytes=need - 8), 'workspace too small'),
                         (dict(ws=ctypes.c_void_p(p.value + 4)), '8-byte aligned')]:
        a = dict(ok, **change)
        rc = lib.lg_grad_norm(a['grads'], a['ranges'], a['n_ranges'], a['max_range'], a['max_norm'], a['out'], a['ws'], a['ws_bytes'], None)
        assert rc == -1 and text in _err(lib), (change, rc, _err(lib))


def test_optim_step_ex_rejects_bad_arguments():
    from lgteun_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(params=p, grads=p, s0=p, s1=p, s2=None, ranges=p, n_ranges=1, step=1, algo=_lib.LG_OPT_ADAM, flags=0, wd=0.0, clip=None,
             ema=None, decay=0.0, plain=0):
        return lib.lg_optim_step_ex(params, grads, s0, s1, s2, ranges, n_ranges, 16, step, algo, flags, 1e-3, 0.9, 0.999, 1e-8, wd, 1.0,
                                    clip, ema, decay, plain, None)
    for kwargs, text in [(dict(params=None), 'invalid argument'), (dict(grads=None), 'invalid argument'), (dict(ranges=None), 'invalid argument'),
                         (dict(step=0), 'invalid argument'), (dict(algo=7), 'invalid argument'), (dict(n_ranges=0), 'invalid argument'),
                         (dict(s1=None), 'state buffer'),
                         (dict(ema=p, decay=0.0), 'ema_decay'), (dict(ema=p, decay=1.0), 'ema_decay'), (dict(ema=p, decay=0.3), 'ema_decay'),
                         (dict(plain=2), 'plain_adam must be 0 or 1'),
                         (dict(plain=1, algo=_lib.LG_OPT_ADAMW), 'plain_adam is algo LG_OPT_ADAM'),
                         (dict(plain=1, wd=1e-2), 'plain_adam is algo LG_OPT_ADAM'),
                         (dict(plain=1, flags=_lib.LG_OPT_AMSGRAD), 'plain_adam is algo LG_OPT_ADAM'),
                         (dict(plain=1, s0=None), 'invalid argument'), (dict(plain=1, params=None), 'invalid argument'),
                         (dict(clip=ctypes.c_void_p(p.value + 2)), '4-byte aligned')]:
        rc = call(**kwargs)
        assert rc == -1 and text in _err(lib), (kwargs, rc, _err(lib))


def test_profiler_ids_are_untouched():
    """the new kernels run without a profiler id, like the Wald kernels"""
    from lgteun_amd import _lib
    assert len(_lib.KERNEL_IDS) == 18 and _lib.lib().lg_kernel_name(len(_lib.KERNEL_IDS)) == b'?'
