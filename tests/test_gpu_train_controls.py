"""-m gpu: the controls around the fused train step -- `lg_grad_norm`, `lg_optim_step_ex` (device clip coefficient, weight EMA in the
optimizer launch), the accumulation window of `Engine.train_step`, `cfg.train_cfg` through the runner, its checkpoints, 'chained' mode
and the data-parallel path.  At C = 4, K = 2, PAN 32 x 32, B = 2 with dropout off (tests/train_controls_helpers.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import rel_l2
from train_controls_helpers import T, engine_of, iterate, make_batch, make_runner, same_bits, start, weights_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from lgteun_amd import _lib
    return _lib, _lib.lib()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------------
# 1. lg_grad_norm
# ------------------------------------------------------------------------------------------------------------------------
NORM_N = 300000
NORM_LENS = [1, 63, 64, 65, 255, 256, 257, 512 * 256 + 5]      # the last one: longer than one pass of a 512-workgroup grid


def _norm_ranges():
    ranges, at = [], 3
    for n in NORM_LENS:
        assert at % 4                                          # no range starts on a 16-byte boundary
        ranges.append((at, at + n))
        at += n + 20001
        at += (at % 4 == 0)
    assert ranges[-1][1] < NORM_N
    return ranges


def _norm_call(buf, ranges, max_norm, out=None):
    _, lib = _lib()
    rd = torch.tensor([v for r in ranges for v in r], dtype=torch.int64, device='cuda')
    mr = max(b - a for a, b in ranges)
    need = lib.lg_grad_norm_workspace_bytes(len(ranges), mr)
    ws = torch.full((need // 8 + 2,), float('nan'), dtype=torch.float64, device='cuda')
    out = torch.full((4,), 7.0, device='cuda') if out is None else out
    rc = lib.lg_grad_norm(_ptr(buf), _ptr(rd), len(ranges), mr, float(max_norm), _ptr(out), _ptr(ws), need, _stream())
    assert rc == 0, lib.lg_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[need // 8:]).all()) and bool((out[2:] == 7.0).all())     # nothing written behind the workspace or the pair
    return out[:2].cpu().numpy().copy()


def _norm_buffer(fill=None):
    """(host buffer with NaN in every gap, the ranges, the elements inside them as fp64)"""
    ranges = _norm_ranges()
    host = np.full(NORM_N, np.nan, dtype=np.float32)
    rng = np.random.default_rng(7)
    for a, b in ranges:
        host[a:b] = rng.standard_normal(b - a).astype(np.float32) if fill is None else fill
    return host, ranges


def _coef(norm32, max_norm):
    """clip_grad_norm_'s coefficient in numpy float32 from the RETURNED norm"""
    with np.errstate(all='ignore'):
        return np.minimum(np.float32(1.0), np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6)))


def _f64_norm(host, ranges):
    inside = np.concatenate([host[a:b] for a, b in ranges]).astype(np.float64)
    return float(np.sqrt(np.sum(inside * inside))), inside.size


def test_grad_norm_against_numpy_fp64():
    """Gate: one fp32 ulp of the fp64 value.  Every square of an fp32 value is exact in fp64 (24 x 24 = 48 bits of significand), the
    sum of n = 132 038 non-negative terms loses at most n * 2^-53 = 1.5e-11 relative in any order, the fp64 square root half an fp64 ulp:
    all far below the 2^-24 of the final rounding to fp32, which is therefore the only error -- at most one fp32 ulp away from numpy's own
    fp64 result (half an ulp of rounding, and the 1.5e-11 may move the value across a rounding boundary).  The gaps between the ranges
    hold NaN: one read outside a range would make the norm NaN."""
    host, ranges = _norm_buffer()
    want, n = _f64_norm(host, ranges)
    assert n == sum(NORM_LENS)
    buf = T(host).cuda()
    got = _norm_call(buf, ranges, max_norm=want / 2)
    ulp = float(np.spacing(np.float32(want)))
    print(f'norm {got[0]!r} against fp64 {want!r}: |diff| {abs(float(got[0]) - want):.3e}, one fp32 ulp {ulp:.3e}; coefficient {got[1]!r}')
    assert abs(float(got[0]) - want) <= ulp
    assert got[1].tobytes() == _coef(got[0], want / 2).tobytes() and 0.49 < got[1] < 0.51
    again = _norm_call(buf, ranges, max_norm=want / 2)
    assert again.tobytes() == got.tobytes()                    # no atomics: the same call, the same bits
    # every range on its own (lengths 1 .. one grid pass and more), and a norm below max_norm: coefficient exactly 1
    for a, b in ranges:
        w1, _ = _f64_norm(host, [(a, b)])
        g1 = _norm_call(buf, [(a, b)], max_norm=1e30)
        assert abs(float(g1[0]) - w1) <= float(np.spacing(np.float32(w1))), (a, b)
        assert g1[1] == np.float32(1.0)
    # ranges of ONE element: as many partials as ranges, so these counts sit on the edges of the finishing pass's 8 x 256 unrolled loop
    # (fewer terms than above: the same gate holds)
    one = np.full(2 * 4100 + 1, np.nan, dtype=np.float32)
    one[1::2] = np.random.default_rng(11).standard_normal(4100).astype(np.float32)
    buf1 = T(one).cuda()
    for n in (1, 255, 256, 257, 2047, 2048, 2049, 4100):
        r1 = [(2 * k + 1, 2 * k + 2) for k in range(n)]
        w1, _ = _f64_norm(one, r1)
        g1 = _norm_call(buf1, r1, max_norm=1e30)
        print(f'{n} partials: norm {g1[0]!r} against fp64 {w1!r}')
        assert abs(float(g1[0]) - w1) <= float(np.spacing(np.float32(w1))), n
        assert _norm_call(buf1, r1, max_norm=1e30).tobytes() == g1.tobytes(), n


def test_grad_norm_carries_fp64():
    """1e20 everywhere: every square overflows fp32, the norm 1e20 sqrt(n) does not"""
    host, ranges = _norm_buffer(fill=np.float32(1e20))
    want, n = _f64_norm(host, ranges)
    got = _norm_call(T(host).cuda(), ranges, max_norm=1.0)
    assert np.isfinite(got[0]) and abs(float(got[0]) - want) <= float(np.spacing(np.float32(want)))
    assert abs(want / (1e20 * np.sqrt(n)) - 1) < 1e-6           # float32(1e20) is 1e20 to 3e-8
    assert got[1].tobytes() == _coef(got[0], 1.0).tobytes() and 0 < got[1] < 1e-20


@pytest.mark.parametrize('case', ['zeros', 'inf', 'nan'])
def test_grad_norm_edge_values(case):
    """all zeros: norm 0 and coefficient exactly 1; one +inf: coefficient 0; one NaN: coefficient NaN -- what
    torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False) gives"""
    host, ranges = _norm_buffer(fill=np.float32(0.0) if case == 'zeros' else None)
    if case != 'zeros':
        host[ranges[4][0] + 17] = np.inf if case == 'inf' else np.nan
    got = _norm_call(T(host).cuda(), ranges, max_norm=0.5)
    g = torch.nn.Parameter(torch.zeros(sum(NORM_LENS)))
    g.grad = T(np.concatenate([host[a:b] for a, b in ranges]))
    tn = torch.nn.utils.clip_grad_norm_([g], 0.5)
    tc = torch.clamp(0.5 / (tn + 1e-6), max=1.0).numpy()
    if case != 'nan':                                           # (a NaN has many bit patterns)
        assert got[1].tobytes() == _coef(got[0], 0.5).tobytes()
    if case == 'zeros':
        assert got[0] == 0.0 and got[1] == np.float32(1.0) and tc == 1.0
    elif case == 'inf':
        assert np.isposinf(got[0]) and got[1] == 0.0 and tc == 0.0
    else:
        assert np.isnan(got[0]) and np.isnan(got[1]) and np.isnan(tc)


# ------------------------------------------------------------------------------------------------------------------------
# 2. / 3. lg_optim_step_ex
# ------------------------------------------------------------------------------------------------------------------------
N_FLAT = 100003
RANGES = [(3, 30001), (40002, 70007), (70011, 99998)]          # gaps in front, between and behind; no start on a 16-byte boundary
MAX_RANGE = max(b - a for a, b in RANGES)
# (name, algo, flags, (lr, h0, h1, eps, weight_decay), state slots used, plain_adam): one row per instance of the switch in optim_step
# (k_optim.hip; the OPT_FIRST instances are step 1 of the momentum rows) + the plain-Adam route.  tests/test_gpu_optim_bits.py ties every
# instance without controls to torch's device bits; the clipped and the averaging launches are tied to those here.
_ADAM_HP, _RMS_HP = (1e-2, 0.9, 0.999, 1e-8), (1e-2, 0.99, 0.0, 1e-8)
EX_SETS = [
    ('Adam', 0, 0, _ADAM_HP + (0.0,), (1, 1, 0), 0),
    ('Adam-wd', 0, 0, _ADAM_HP + (1e-2,), (1, 1, 0), 0),
    ('Adam-amsgrad', 0, 1, _ADAM_HP + (0.0,), (1, 1, 1), 0),
    ('Adam-amsgrad-wd', 0, 1, _ADAM_HP + (1e-2,), (1, 1, 1), 0),
    ('AdamW', 1, 0, _ADAM_HP + (1e-2,), (1, 1, 0), 0),
    ('AdamW-amsgrad', 1, 1, _ADAM_HP + (1e-2,), (1, 1, 1), 0),
    ('SGD', 2, 0, (1e-2, 0.0, 0.0, 0.0, 0.0), (0, 0, 0), 0),
    ('SGD-wd', 2, 0, (1e-2, 0.0, 0.0, 0.0, 1e-2), (0, 0, 0), 0),
    ('SGD-momentum', 2, 0, (1e-2, 0.9, 0.0, 0.0, 0.0), (1, 0, 0), 0),
    ('SGD-momentum-wd', 2, 0, (1e-2, 0.9, 0.0, 0.0, 1e-2), (1, 0, 0), 0),
    ('SGD-nesterov', 2, 2, (1e-2, 0.9, 0.0, 0.0, 0.0), (1, 0, 0), 0),
    ('SGD-nesterov-wd', 2, 2, (1e-2, 0.9, 0.0, 0.0, 1e-2), (1, 0, 0), 0),
    ('RMSprop', 3, 0, _RMS_HP + (0.0,), (1, 0, 0), 0),
    ('RMSprop-wd', 3, 0, _RMS_HP + (1e-2,), (1, 0, 0), 0),
    ('RMSprop-centered', 3, 4, _RMS_HP + (0.0,), (1, 0, 1), 0),
    ('RMSprop-centered-wd', 3, 4, _RMS_HP + (1e-2,), (1, 0, 1), 0),
    ('RMSprop-momentum', 3, 0, (1e-2, 0.99, 0.9, 1e-8, 0.0), (1, 1, 0), 0),
    ('RMSprop-momentum-wd', 3, 0, (1e-2, 0.99, 0.9, 1e-8, 1e-2), (1, 1, 0), 0),
    ('RMSprop-centered-momentum', 3, 4, (1e-2, 0.99, 0.9, 1e-8, 0.0), (1, 1, 1), 0),
    ('RMSprop-centered-momentum-wd', 3, 4, (1e-2, 0.99, 0.9, 1e-8, 1e-2), (1, 1, 1), 0),
    ('Adam-plain', 0, 0, _ADAM_HP + (0.0,), (1, 1, 0), 1),
]
EMA_SETS = [s for s in EX_SETS if s[0] in ('AdamW-amsgrad', 'SGD-momentum', 'Adam-plain')]


class _Flat:
    """parameters, gradients per step and state buffers over synthetic flat storage"""

    def __init__(self, slots):
        gen = torch.Generator().manual_seed(4321)
        self.p = torch.randn(N_FLAT, generator=gen).cuda()
        self.grads = [(torch.randn(N_FLAT, generator=gen) * a).cuda() for a in (1.0, 0.3, 2.0)]
        self.s = [torch.zeros(N_FLAT, device='cuda') if u else None for u in slots]
        self.rd = torch.tensor([v for r in RANGES for v in r], dtype=torch.int64, device='cuda')

    def tensors(self):
        return [self.p] + [s for s in self.s if s is not None]


def _existing(f, g, step, algo, flags, hp, plain):
    """the entry points every earlier build has"""
    _, lib = _lib()
    lr, h0, h1, eps, wd = hp
    if plain:
        rc = lib.lg_adam_step(_ptr(f.p), _ptr(g), _ptr(f.s[0]), _ptr(f.s[1]), _ptr(f.rd), len(RANGES), MAX_RANGE, step, lr, h0, h1, eps, 1.0,
                              _stream())
    else:
        rc = lib.lg_optim_step(_ptr(f.p), _ptr(g), _ptr(f.s[0]), _ptr(f.s[1]), _ptr(f.s[2]), _ptr(f.rd), len(RANGES), MAX_RANGE, step, algo,
                               flags, lr, h0, h1, eps, wd, 1.0, _stream())
    assert rc == 0, lib.lg_last_error()


def _ex(f, g, step, algo, flags, hp, plain, clip=None, ema=None, decay=0.0):
    _, lib = _lib()
    lr, h0, h1, eps, wd = hp
    rc = lib.lg_optim_step_ex(_ptr(f.p), _ptr(g), _ptr(f.s[0]), _ptr(f.s[1]), _ptr(f.s[2]), _ptr(f.rd), len(RANGES), MAX_RANGE, step, algo,
                              flags, lr, h0, h1, eps, wd, 1.0, _ptr(clip), _ptr(ema), decay, plain, _stream())
    assert rc == 0, lib.lg_last_error()


@pytest.mark.parametrize('name,algo,flags,hp,slots,plain', EX_SETS, ids=[s[0] for s in EX_SETS])
def test_clipped_step_is_bitwise_the_step_on_premultiplied_gradients(name, algo, flags, hp, slots, plain):
    """two steps.  lg_optim_step_ex with a DEVICE coefficient c = 0.37 against the existing entry point fed a gradient buffer torch
    multiplied by c on the device (what clip_grad_norm_'s g.mul_(c) leaves): parameters and every state buffer, bit for bit.  And with
    clip_coef = NULL, ema = NULL it is the existing entry point."""
    coef = torch.tensor([9.0, 0.37], device='cuda')[1:]         # not 16-byte aligned, like out + 1 of lg_grad_norm
    a, b, c, d = _Flat(slots), _Flat(slots), _Flat(slots), _Flat(slots)
    for step in (1, 2):
        g = a.grads[step - 1]
        _ex(a, g, step, algo, flags, hp, plain, clip=coef)
        _existing(b, g * coef, step, algo, flags, hp, plain)
        _ex(c, g, step, algo, flags, hp, plain)
        _existing(d, g, step, algo, flags, hp, plain)
        torch.cuda.synchronize()
        for x, y, z, w in zip(a.tensors(), b.tensors(), c.tensors(), d.tensors()):
            assert same_bits(x, y), (name, step, 'clipped')
            assert same_bits(z, w), (name, step, 'no controls')
        assert not same_bits(a.p, c.p)                          # the coefficient did something


@pytest.mark.parametrize('decay', [0.999, 0.9])
@pytest.mark.parametrize('name,algo,flags,hp,slots,plain', EMA_SETS, ids=[s[0] for s in EMA_SETS])
def test_ema_in_the_optimizer_launch_is_torchs_lerp(name, algo, flags, hp, slots, plain, decay):
    """after each of three lg_optim_step_ex calls with `ema`: ema == torch._foreach_lerp_(previous average, new parameters, 1 - decay) on
    the device, inside the ranges; outside them the average keeps its initial bits; the parameters are those of the same calls without it"""
    a, b = _Flat(slots), _Flat(slots)
    inside = torch.zeros(N_FLAT, dtype=torch.bool, device='cuda')
    for lo, hi in RANGES:
        inside[lo:hi] = True
    ema = torch.randn(N_FLAT, generator=torch.Generator().manual_seed(99)).cuda()
    first = ema.clone()
    for step in (1, 2, 3):
        g = a.grads[step - 1]
        want = ema.clone()
        _ex(a, g, step, algo, flags, hp, plain, ema=ema, decay=decay)
        _ex(b, g, step, algo, flags, hp, plain)
        torch._foreach_lerp_([want], [a.p], 1 - decay)
        torch.cuda.synchronize()
        assert same_bits(ema[inside], want[inside]), (name, step)
        assert same_bits(ema[~inside], first[~inside]), (name, step)
        assert not same_bits(ema[inside], first[inside])
        for x, y in zip(a.tensors(), b.tensors()):
            assert same_bits(x, y), (name, step)


# ------------------------------------------------------------------------------------------------------------------------
# 4. the accumulation window of Engine.train_step
# ------------------------------------------------------------------------------------------------------------------------
def _adamw(net, controls=None):
    import lgteun_amd
    opt = lgteun_amd.FusedAdamW(net.parameters(), lr=1.5e-3, weight_decay=1e-2)
    opt.dropout = False
    return opt.set_controls(controls)


def _args(batch):
    return batch['input_lr'], batch['input_pan'], batch['target']


@pytest.mark.parametrize('mode', ['faithful', 'chained'])
def test_window_of_two_is_the_hand_sequence(mode):
    """Engine.train_step with accumulate = 2 over micro-batches a, b == forward_raw / lg_l2_loss with scale 1/2 / backward_raw for a then
    b into ONE zeroed gradient buffer, then one optimizer step: weights, optimizer state and loss scalar bit for bit; `_step` advances
    once per window; global_loss() is the mean over the micro-batches seen so far.

    Semantics: the window's gradient buffer against the gradient of ONE step over the concatenated batch of 4 (no scale: its mean is
    over twice the elements) within the project's global gradient gate, 1e-3 relative L2.  Measured on the MI355X: faithful 7.2e-8,
    chained 7.3e-8 (fp32 summation order only)."""
    from gpu_helpers import make_module
    import lgteun_amd
    from lgteun_amd._lib import LG_FLAG_DROPOUT, LG_FLAG_SAVE, check
    ba, bb = make_batch(seed=11), make_batch(seed=12)
    net = make_module(4, 2)
    net.mode = mode
    eng = net.engine()
    opt = _adamw(net, lgteun_amd.TrainControls(accumulate=2))
    eng.train_step(*_args(ba), opt, loss_type='l2')
    loss_a = eng.global_loss()
    assert opt._step == 0 and opt._window_pos == 1
    eng.train_step(*_args(bb), opt, loss_type='l2')
    assert opt._step == 1 and opt._window_pos == 0
    # by hand, on a second module with the same weights
    net2 = make_module(4, 2)
    net2.mode = mode
    e2 = net2.engine()
    opt2 = _adamw(net2)
    e2._gbuf.zero_()
    flags = (e2.base_flags(True) | LG_FLAG_SAVE) & ~LG_FLAG_DROPOUT
    hand_losses = []
    for batch in (ba, bb):
        ms, pan, gt = _args(batch)
        out, saved = e2.forward_raw(ms, pan, flags, 0)
        dout = torch.empty_like(out)
        check(e2.lib.lg_l2_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(e2._loss), out.numel(), out.numel(), 0.5, _stream()), 'lg_l2_loss')
        e2.backward_raw(saved, dout, e2.gflat, flags, 0)
        hand_losses.append(float(e2._loss.item()))
    opt2.step_flat(e2)
    torch.cuda.synchronize()
    assert same_bits(eng.gflat, e2.gflat) and same_bits(eng._loss, e2._loss)
    assert same_bits(eng.flat, e2.flat)
    assert sorted(opt._state) == sorted(opt2._state) == ['exp_avg', 'exp_avg_sq']
    for n in opt._state:
        assert same_bits(opt._state[n], opt2._state[n]), n
    assert loss_a == hand_losses[0] and eng.global_loss() == float((e2._loss / 2).item())
    if mode == 'chained':
        assert eng.live_ranges == [(0, eng.total)]
    # one step over the concatenated batch
    net3 = make_module(4, 2)
    net3.mode = mode
    e3 = net3.engine()
    cat = [torch.cat([x, y]) for x, y in zip(_args(ba), _args(bb))]
    e3.train_step(*cat, _adamw(net3), loss_type='l2')
    torch.cuda.synchronize()
    rel = rel_l2(eng.gflat.cpu(), e3.gflat.cpu())
    print(f'{mode}: window gradient against the gradient of the concatenated batch: rel_l2 {rel:.3e}')
    assert rel < 1e-3


def test_window_cut_by_a_checkpoint_resumes_to_the_same_bits(tmp_path):
    """accumulate = 2 with clipping and the average on; save after the FIRST call of the second window, load into a fresh runner (the
    order of main.py), one more call == four uninterrupted calls: weights, average and optimizer state bit for bit.  The checkpoint keeps
    the reference's top-level keys, and the raw weights under core_module."""
    entry = dict(type='SGD', lr=1e-2, momentum=0.9)
    tc = dict(accumulate=2, max_grad_norm=0.05, ema_decay=0.9)
    batches = [make_batch(seed=11), make_batch(seed=12)]
    a, _ = make_runner(tmp_path, 'l1', entry, tc, step_size=100, tag='a')
    iterate(start(a), batches, range(1, 5))
    oa = a.optim_dict['core_module']
    assert oa._step == 2 and oa._window_pos == 0
    b, _ = make_runner(tmp_path, 'l1', entry, tc, step_size=100, tag='b')
    iterate(start(b), batches, range(1, 4))
    assert b.optim_dict['core_module']._step == 1 and b.optim_dict['core_module']._window_pos == 1
    path = b.save(iter_id=3)
    ck = torch.load(path, map_location='cpu', weights_only=True)
    assert set(ck) == {'iter_num', 'core_module', 'optim'}
    assert all(torch.equal(v, weights_of(b)[k]) for k, v in ck['core_module'].items())          # the RAW weights
    c, _ = make_runner(tmp_path, 'l1', entry, tc, step_size=100, tag='c')
    c.load_checkpoint(path)
    start(c)
    oc = c.optim_dict['core_module']
    assert oc._step == 1 and oc._window_pos == 1 and oc._window_gbuf is not None and sorted(oc._state) == ['ema', 'momentum_buffer']
    iterate(c, batches, [4])
    assert oc._step == 2 and oc._window_pos == 0
    wa, wc = weights_of(a), weights_of(c)
    for k in wa:
        assert same_bits(wa[k], wc[k]), k
    for n in ('ema', 'momentum_buffer'):
        assert same_bits(oa._state[n], oc._state[n]), n
    assert engine_of(a).last_grad_norm() == engine_of(c).last_grad_norm()


# ------------------------------------------------------------------------------------------------------------------------
# 5. controls change nothing they should not
# ------------------------------------------------------------------------------------------------------------------------
# every case with the l2 loss: its scalar is ONE float add per launch.  lg_l1_loss adds one float per workgroup to the scalar with atomics, in
# the order the workgroups arrive, so two runs of the SAME configuration may differ in the last bit of an l1 loss (tests/test_gpu_resident.py)
ENTRIES = [('l2', dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3)), ('l2', dict(type='AdamW', lr=1.5e-3, weight_decay=1e-2)),
           ('l2', dict(type='SGD', lr=1e-2, momentum=0.9)), ('l2', dict(type='RMSprop', lr=1.5e-3))]


def _three(tmp_path, loss, entry, train_cfg, tag, mode=None):
    runner, sd = make_runner(tmp_path, loss, entry, train_cfg, tag=tag, mode=mode)
    losses = iterate(start(runner), make_batch(), range(1, 4))
    assert len(losses) == 3
    return runner, losses, weights_of(runner), sd


@pytest.mark.parametrize('loss,entry,mode', [(lo, e, None) for lo, e in ENTRIES] + [ENTRIES[1] + ('chained',)],
                         ids=[e['type'] for _, e in ENTRIES] + ['AdamW-chained'])
def test_controls_leave_the_trajectory_alone(tmp_path, loss, entry, mode):
    """three train_iter calls.  With ema_decay alone the raw weights and the losses are, bit for bit, those of a run without train_cfg;
    with max_grad_norm = 1e30 the coefficient is exactly 1 and they are again.  Adam (plain) stays on lg_adam_step's arithmetic."""
    _, l0, w0, sd = _three(tmp_path, loss, entry, None, 'plain', mode)
    r1, l1, w1, _ = _three(tmp_path, loss, entry, dict(ema_decay=0.99), 'ema', mode)
    r2, l2, w2, _ = _three(tmp_path, loss, entry, dict(max_grad_norm=1e30), 'clip', mode)
    assert l1 == l0 and l2 == l0
    moved = 0
    for k in w0:
        assert same_bits(w1[k], w0[k]), ('ema', k)
        assert same_bits(w2[k], w0[k]), ('clip', k)
        moved += not torch.equal(w0[k], T(sd[k]))
    assert moved > 100
    assert 'ema' in r1.optim_dict['core_module']._state and 'ema' not in r2.optim_dict['core_module']._state
    pair = engine_of(r2)._clip.cpu().numpy()
    assert pair[1] == np.float32(1.0) and 0 < pair[0] < 1e30 and engine_of(r2).last_grad_norm() == float(pair[0])


# ------------------------------------------------------------------------------------------------------------------------
# 6. the fused route against the torch route with clipping engaged
# ------------------------------------------------------------------------------------------------------------------------
def test_clipped_fused_route_agrees_with_the_torch_route(tmp_path):
    """SGD with momentum, three iterations at max_grad_norm = n0 / 2 (n0: the first-step norm of an unclipped run), fused and
    `fused=False` (torch.nn.utils.clip_grad_norm_ + torch.optim.SGD on the same gradient kernels): losses to rtol 1e-5, live weights to
    rel_l2 < 1e-5 (the gates of test_fused_route_agrees_with_the_torch_route), the norm of the last step to rtol 1e-6, the dead stage on
    its initial bits.  Measured on the MI355X: losses equal to 1e-7 relative, worst live weight rel_l2 4.0e-8, the two norms equal.

    Why SGD only: the two routes' norms differ in the last bit (fp64 sum against torch's fp32 reduction), so their coefficients do.
    That bit rescales the gradients of the key third of every to_qkv bias, which are the rounding noise of a sum that cancels; Adam, AdamW
    and RMSprop normalise such an element to the order of lr whatever its size, with the sign of the noise (see the route test of
    tests/test_gpu_fused_optim.py), so an end-to-end comparison of those optimizers measures that noise and nothing of the clipping.
    Their clipped arithmetic is pinned bit for bit in test_clipped_step_is_bitwise_the_step_on_premultiplied_gradients instead."""
    entry = dict(type='SGD', lr=1e-2, momentum=0.9)
    batch = make_batch()
    probe, _ = make_runner(tmp_path, 'l1', entry, dict(max_grad_norm=1e30), tag='probe')
    iterate(start(probe), batch, [1])
    n0 = probe.last_grad_norm()
    assert n0 > 0
    res = {}
    for fused in (True, False):
        runner, sd = make_runner(tmp_path, 'l1', dict(entry, fused=fused), dict(max_grad_norm=n0 / 2), tag=f'f{int(fused)}')
        start(runner)
        assert bool(getattr(runner.optim_dict['core_module'], 'is_fused_lgteun', False)) == fused
        losses = iterate(runner, batch, range(1, 4))
        res[fused] = (losses, weights_of(runner), runner.last_grad_norm())
        for k, v in res[fused][1].items():
            if k.startswith('prior_module.0.'):
                assert torch.equal(v, T(sd[k])), (fused, k)
    worst = max((rel_l2(res[True][1][k], v), k) for k, v in res[False][1].items() if not k.startswith('prior_module.0.'))
    print(f'n0 {n0!r}; losses fused {res[True][0]} torch {res[False][0]}; norms {res[True][2]!r} {res[False][2]!r}; worst live weight {worst}')
    assert res[True][2] > n0 / 2                                # clipping is engaged
    assert np.allclose(res[True][0], res[False][0], rtol=1e-5, atol=0)
    assert worst[0] < 1e-5, worst
    assert abs(res[True][2] - res[False][2]) <= 1e-6 * res[False][2]


# ------------------------------------------------------------------------------------------------------------------------
# 7. the average, end to end
# ------------------------------------------------------------------------------------------------------------------------
def test_ema_end_to_end(tmp_path):
    """three fused AdamW iterations at decay 0.99: the 'ema' state is the torch lerp recursion over the weight snapshots, bit for bit;
    test() with eval_ema gives the output of a module loaded from ema_state_dict(); the raw weights are back afterwards, and after an
    exception inside engine.ema_weights(); save -> load into a fresh runner -> one more iteration is the uninterrupted run."""
    import lgteun_amd
    from lgteun_amd.base_model import NormalizedBatch
    from lgteun_amd.compat import Config
    entry = dict(type='AdamW', lr=1.5e-3, weight_decay=1e-2)
    tc = dict(ema_decay=0.99)
    batch = make_batch()
    a, _ = make_runner(tmp_path, 'l2', entry, tc, step_size=100, tag='a', loaders=(None, None, [NormalizedBatch(batch)]))
    start(a)
    eng, opt = engine_of(a), a.optim_dict['core_module']
    want = eng.flat.clone()
    for it in (1, 2, 3):
        iterate(a, batch, [it])
        torch._foreach_lerp_([want], [eng.flat], 1 - 0.99)
        torch.cuda.synchronize()
        assert same_bits(opt._state['ema'], want), it
    lo, hi = eng.live_ranges[0][1], eng.live_ranges[1][0]
    assert hi > lo and same_bits(want[lo:hi], eng.flat[lo:hi])       # dead stage: the average equals the weights
    raw = eng.flat.clone()
    # evaluation with the averaged weights
    seen = []
    inner = a.get_model_output
    a.get_model_output = lambda b: seen.append(inner(b).clone()) or seen[-1]
    a.test(iter_id=3, save=False, ref=True)
    assert same_bits(eng.flat, raw) and len(seen) == 1
    core = a.module_dict['core_module']
    esd = core.ema_state_dict()
    assert same_bits(eng.flat, raw) and list(esd) == list(core.state_dict())
    other = lgteun_amd.Pansharpening(Config(ms_chans=4), None, stage=2)
    other.load_state_dict(esd)
    other = other.cuda().eval()
    with torch.no_grad():
        out = other(batch['input_lr'], batch['input_pan'])
        out_raw = core(batch['input_lr'], batch['input_pan'])
    assert same_bits(out, seen[0]) and not same_bits(out_raw, seen[0])
    with pytest.raises(KeyError, match='inside'):
        with eng.ema_weights():
            assert same_bits(eng.flat, opt._state['ema'])
            raise KeyError('inside')
    assert same_bits(eng.flat, raw)
    # eval_ema = False: the raw weights are evaluated
    opt.controls.eval_ema = False
    a.test(iter_id=3, save=False, ref=True)
    assert same_bits(seen[1], out_raw)
    opt.controls.eval_ema = True
    # resume
    path = a.save(iter_id=3)
    ck = torch.load(path, map_location='cpu', weights_only=True)
    assert set(ck) == {'iter_num', 'core_module', 'optim'} and 'ema' in ck['optim']['core_module']['lgteun']['state']
    flat_ck = torch.cat([torch.nn.functional.pad(v.reshape(-1), (0, -v.numel() % 4)) for v in ck['core_module'].values()])
    assert same_bits(flat_ck, raw)
    iterate(a, batch, [4])
    c, _ = make_runner(tmp_path, 'l2', entry, tc, step_size=100, tag='c')     # (StepLR's own count is not part of a checkpoint)
    c.load_checkpoint(path)
    start(c)
    iterate(c, batch, [4])
    assert same_bits(engine_of(c).flat, eng.flat)
    assert same_bits(c.optim_dict['core_module']._state['ema'], opt._state['ema'])


# ------------------------------------------------------------------------------------------------------------------------
# 9. process groups
# ------------------------------------------------------------------------------------------------------------------------
def _window_steps(net, eng=None, calls=4):
    import lgteun_amd
    opt = _adamw(net, lgteun_amd.TrainControls(accumulate=2, max_grad_norm=0.05, ema_decay=0.9))
    eng = eng or net.engine()
    batches = [make_batch(seed=11), make_batch(seed=12)]
    for i in range(calls):
        eng.train_step(*_args(batches[i % 2]), opt, loss_type='l2')
    torch.cuda.synchronize()
    return eng, opt


def test_one_rank_process_group_with_controls_is_bitwise_the_unattached_run(tmp_path):
    """accumulate = 2, clipping and the average in a gloo group of ONE rank joined by this process (attach_ddp(force=True)): the bucket
    all-reduce runs at the window ends only -- a sum over one rank is the identity -- so four calls give the bits of the unattached run"""
    import torch.distributed as dist
    from gpu_helpers import make_module
    e0, o0 = _window_steps(make_module(4, 2))
    assert not dist.is_initialized()
    dist.init_process_group('gloo', store=dist.FileStore(str(tmp_path / 'store'), 1), rank=0, world_size=1)
    try:
        net1 = make_module(4, 2)
        eng = net1.attach_ddp(force=True)
        assert eng.force_collectives and eng.buckets is not None and eng.world == 1
        calls = []
        for bk in eng.buckets.values():
            inner = bk.all_reduce
            bk.all_reduce = lambda g, inner=inner: calls.append(1) or inner(g)
        e1, o1 = _window_steps(net1, eng)
    finally:
        dist.destroy_process_group()
    assert len(calls) == 2 and o1._step == 2                   # one collective per window, not per call
    assert same_bits(e1.flat, e0.flat) and same_bits(e1._clip, e0._clip) and float(e0._clip[1]) < 1.0
    for n in ('exp_avg', 'exp_avg_sq', 'ema'):
        assert same_bits(o1._state[n], o0._state[n]), n


def test_two_ranks_with_controls_equal_the_single_process(tmp_path):
    """two ranks of tests/ddp_train_controls_worker.py on the one MI355X (gloo), B = 1 each, accumulate = 2 with clipping engaged,
    against a single process with B = 2: the tolerances of test_two_rank_engine_train_step_equals_single_process (gradient rel 2e-5,
    live weights rel 1e-4, replicas and dead stages bit for bit), and the clip coefficient identical on both ranks."""
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs, logs = [], []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        env.pop('LG_DDP_OVERLAP', None)
        logs.append(str(tmp_path / f'rank{rank}.log'))
        procs.append(subprocess.Popen([sys.executable, '-W', 'ignore', os.path.join(ROOT, 'tests', 'ddp_train_controls_worker.py'), str(tmp_path)],
                                      stdout=open(logs[-1], 'w'), stderr=subprocess.STDOUT, env=env, cwd=ROOT))
    try:
        for p in procs:
            assert p.wait(timeout=240) == 0, ''.join(open(f).read()[-3000:] for f in logs)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r0, r1 = (np.load(tmp_path / f'rank{r}.npz') for r in (0, 1))
    assert int(r0['world']) == 2 and int(r1['world']) == 2 and int(r0['steps']) == 2 and int(r1['steps']) == 2
    assert int(r0['collectives']) == 2 and int(r1['collectives']) == 2      # one all-reduce per window, none inside it
    (a0, b0), (a1, b1) = r0['ranges']
    for k in ('clip0', 'clip1', 'gflat', 'weights', 'ema'):
        assert r0[k].tobytes() == r1[k].tobytes(), k            # one all-reduce result, one coefficient, replicas in lock-step
    assert 0 < float(r0['clip0'][1]) < 1 and 0 < float(r0['clip1'][1]) < 1        # clipping is engaged
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))      # noqa: E731
    assert rel(r0['gflat'], r0['single_gflat']) < 2e-5
    for k in ('clip0', 'clip1'):
        assert np.allclose(r0[k], r0['single_' + k], rtol=2e-5, atol=0), k
    assert abs(float(r0['loss']) + float(r1['loss']) - float(r0['single_loss'])) < 1e-4 * float(r0['single_loss'])
    for k in ('weights', 'ema'):
        w, ws = r0[k], r0['single_' + k]
        assert rel(w[a1:b1], ws[a1:b1]) < 1e-4 and rel(w[a0:b0], ws[a0:b0]) < 1e-4, k
        assert np.array_equal(w[b0:a1], ws[b0:a1]), k
    assert not np.array_equal(r0['weights'][a1:b1], r0['first'][a1:b1])
