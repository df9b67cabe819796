"""-m gpu: every instance of `k_optim<ALGO, OPT, CTL = 0>` (lgteun_amd/csrc/k_optim.hip) against torch's own DEVICE optimizer, bit for bit,
and the launch geometry of the optimizer kernels.

A.  One option set per (algo, opt) word of the switch in `optim_step` -- 24 words, asserted from the table below -- against
    `torch.optim.{Adam, AdamW, SGD, RMSprop}(foreach=True)` on device tensors in fp32, one nn.Parameter per range.  A second torch leg is
    built with no `foreach` argument (what base_model.set_optim builds for `fused=False`) and must land on the first leg's bits.  Five
    steps, lr lowered between them through `param_groups`, gradient amplitudes 1, 0.3, 2, 0.1, 1, over 100 003 floats with three unaligned
    ranges; planted in range 0: 64 gradients that are 0 at every step, 64 parameters that start at 0, gradients of 1e-12, 1e12 and
    1e-20 (its square is a denormal).  After EVERY step: the parameters and every state buffer, under torch's name, have torch's bits
    inside the ranges and their initial bits outside.  Every set but plain Adam runs through its `Fused*` class and `step_flat`, so the
    Python scalar plumbing is pinned with the kernel; plain Adam goes through the C ABI `lg_optim_step` (FusedAdam sends that set to
    `lg_adam_step`, whose documented deviation -- 1 - beta from the fp32 beta -- stays).  Every set also runs once with
    `grad_scale = 1/3` against a torch leg fed `g.mul(1/3)` on the device.

B.  A second layout of 400 003 floats: a range of one float, one of 131 072 + 777 floats from an odd offset (the grid is capped at
    512 x 256 threads: its first workgroups take a second trip of the stride loop, the last of them a partial one), two adjacent ranges
    and one that ends at the buffer's end.  Three sets against torch as in A for two steps; and for `lg_adam_step` and
    `lg_optim_step_ex(plain_adam = 1, clip, ema)` the same buffers with the long range cut into pieces of 1000: bitwise equal -- an
    element's result may not depend on how the ranges are cut.  That comparison is the library with itself, on purpose: it speaks
    about geometry only.

Measured on the MI355X (torch 2.10 + ROCm 7.0), first run, k_optim.hip as the parent commit has it: ALL 22 option sets -- so all 24
instances -- are on torch's bits after each of the five steps, parameters and every state buffer, with grad_scale = 1/3 too, and so are
the three sets of part B after both steps; the default-`foreach` leg is on the bits of foreach=True for every set.  Nothing differed, so
nothing in k_optim.hip changed and no set carries a gate of its own.  The denormal element is treated alike by torch's kernels and
ours (its bits agree at every step of every set): it is compared like every other one, EXCLUDED is empty.  The cut ranges of
part B give the same bits for both entry points.  The file: 51 tests in 5.2 s.

The tests were themselves checked once, against a scratch build of the library that is not kept: the `_foreach_lerp_` of the Adam / AdamW
branch written as a rounded product plus a rounded sum, `mi = a.c0 * (gi - mi) + mi`, where the kernel has LG_OPT_FMA.  Every Adam and
AdamW case went red (7 sets here, their 7 grad_scale cases, the AdamW set of part B: 15 tests), each at step 2 -- step 1 starts from a zero
moment, where the two forms agree -- on `exp_avg`: 17 879 of 89 985 elements (17 980 with weight decay); the report's
largest distance was 5519 ulps (23 690 with weight decay) because an average near a sign change is small against the rounding of its
terms.  Every SGD and RMSprop case and the range-cutting tests stayed green, and so did all 22 cases of test_optimizer_step_vs_torch
(tests/test_gpu_fused_optim.py), whose band is 2 x the fp32-vs-fp64 spread."""
import functools

import pytest
import torch

from optim_helpers import bits, flat_engine, parting

pytestmark = pytest.mark.gpu

ADAM, ADAMW, SGD, RMSPROP = 0, 1, 2, 3          # LG_OPT_* of include/lgteun_hip.h
WD, ALT, MOM, FIRST = 1, 2, 4, 8                # OPT_* of k_optim.hip; ALT: amsgrad / nesterov / centered

LAYOUT_A = (100003, ((3, 30001), (40002, 70007), (70011, 99998)))
LONG = 131072 + 777                              # one pass of the capped grid is 512 * 256 = 131 072 floats
LAYOUT_B = (400003, ((5, 6), (1001, 1001 + LONG), (140003, 150001), (150001, 160000), (390000, 400003)))
GRAD_AMP = [1.0, 0.3, 2.0, 0.1, 1.0]
ZERO_GRAD, ZERO_PARAM, TINY, HUGE, DENORMAL = 100, 200, 300, 301, 302      # offsets into range 0 of the planted elements
EXCLUDED = ()                                    # offsets into range 0 taken out of the comparison with torch: none

# (id, torch.optim class, its keywords, the (algo, opt) words this set is the one to launch).  The two sets that own no word launch
# a word of another set with other scalars.
SETS = [
    ('Adam-0', 'Adam', dict(), [(ADAM, 0)]),
    ('Adam-wd', 'Adam', dict(weight_decay=1e-2), [(ADAM, WD)]),
    ('Adam-alt', 'Adam', dict(amsgrad=True), [(ADAM, ALT)]),
    ('Adam-alt.wd', 'Adam', dict(amsgrad=True, weight_decay=1e-2), [(ADAM, ALT | WD)]),
    ('AdamW-0', 'AdamW', dict(weight_decay=1e-2), [(ADAMW, 0)]),
    ('AdamW-0-nodecay', 'AdamW', dict(weight_decay=0.0), []),
    ('AdamW-alt', 'AdamW', dict(amsgrad=True), [(ADAMW, ALT)]),
    ('SGD-0', 'SGD', dict(), [(SGD, 0)]),
    ('SGD-wd', 'SGD', dict(weight_decay=1e-2), [(SGD, WD)]),
    ('SGD-mom', 'SGD', dict(momentum=0.9), [(SGD, MOM | FIRST), (SGD, MOM)]),
    ('SGD-mom.wd', 'SGD', dict(momentum=0.9, weight_decay=1e-2), [(SGD, MOM | FIRST | WD), (SGD, MOM | WD)]),
    ('SGD-mom-dampening', 'SGD', dict(momentum=0.9, dampening=0.1), []),
    ('SGD-mom.alt', 'SGD', dict(momentum=0.9, nesterov=True), [(SGD, MOM | ALT | FIRST), (SGD, MOM | ALT)]),
    ('SGD-mom.alt.wd', 'SGD', dict(momentum=0.9, nesterov=True, weight_decay=1e-2), [(SGD, MOM | ALT | FIRST | WD), (SGD, MOM | ALT | WD)]),
    ('RMSprop-0', 'RMSprop', dict(), [(RMSPROP, 0)]),
    ('RMSprop-wd', 'RMSprop', dict(weight_decay=1e-2), [(RMSPROP, WD)]),
    ('RMSprop-alt', 'RMSprop', dict(centered=True), [(RMSPROP, ALT)]),
    ('RMSprop-alt.wd', 'RMSprop', dict(centered=True, weight_decay=1e-2), [(RMSPROP, ALT | WD)]),
    ('RMSprop-mom', 'RMSprop', dict(momentum=0.9), [(RMSPROP, MOM)]),
    ('RMSprop-mom.wd', 'RMSprop', dict(momentum=0.9, weight_decay=1e-2), [(RMSPROP, MOM | WD)]),
    ('RMSprop-mom.alt', 'RMSprop', dict(centered=True, momentum=0.9), [(RMSPROP, MOM | ALT)]),
    ('RMSprop-mom.alt.wd', 'RMSprop', dict(alpha=0.9, eps=1e-6, weight_decay=1e-2, centered=True, momentum=0.5), [(RMSPROP, MOM | ALT | WD)]),
]
SET_IDS = [s[0] for s in SETS]
# the cases of the switch in optim_step, written out
ALL_WORDS = ([(ADAM, o) for o in (0, WD, ALT, WD | ALT)] + [(ADAMW, 0), (ADAMW, ALT)] + [(SGD, 0), (SGD, WD)] +
             [(SGD, MOM | a | f | w) for a in (0, ALT) for f in (0, FIRST) for w in (0, WD)] +
             [(RMSPROP, m | a | w) for m in (0, MOM) for a in (0, ALT) for w in (0, WD)])
# the three sets of part B
GEOMETRY_SETS = [('AdamW-alt.wd', 'AdamW', dict(amsgrad=True, weight_decay=1e-2)),
                 ('SGD-mom.alt.wd', 'SGD', dict(momentum=0.9, nesterov=True, weight_decay=1e-2)),
                 ('RMSprop-mom.alt.wd', 'RMSprop', dict(centered=True, momentum=0.9, weight_decay=1e-2))]


def _word(step, algo, flags, h0, h1, weight_decay):
    """the instance optim_step selects for these arguments (k_optim.hip, restated)"""
    opt = (WD if weight_decay != 0.0 and algo != ADAMW else 0) | (ALT if flags else 0)
    if algo == SGD and h0 != 0.0:
        opt |= MOM | (FIRST if step == 1 else 0)
    if algo == RMSPROP and h1 > 0.0:
        opt |= MOM
    return algo, opt


def test_the_table_names_every_instance_once():
    owned = [w for s in SETS for w in s[3]]
    assert len(ALL_WORDS) == 24 and len(set(ALL_WORDS)) == 24
    assert sorted(owned) == sorted(ALL_WORDS), sorted(set(ALL_WORDS) ^ set(owned))      # all there, each once


@functools.lru_cache(maxsize=None)
def _data(layout, steps, plant):
    """on the device: the parameters, the (lr, gradient) pairs, the pattern the state buffers hold outside the ranges, the mask of the
    ranges and the mask of what is compared with torch"""
    n, ranges = layout
    assert all(0 <= a < b <= n for a, b in ranges) and all(ranges[i][1] <= ranges[i + 1][0] for i in range(len(ranges) - 1))
    gen = torch.Generator().manual_seed(1234)
    p0 = torch.randn(n, generator=gen)
    sched = [(1e-2 * 0.85 ** i, torch.randn(n, generator=gen) * GRAD_AMP[i]) for i in range(steps)]
    marks = torch.randn(n, generator=gen)
    inside = torch.zeros(n, dtype=torch.bool)
    for a, b in ranges:
        inside[a:b] = True
    compared = inside.clone()
    if plant:
        a0 = ranges[0][0]
        assert ranges[0][1] - a0 > DENORMAL
        p0[a0 + ZERO_PARAM:a0 + ZERO_PARAM + 64] = 0.0
        for _, g in sched:
            g[a0 + ZERO_GRAD:a0 + ZERO_GRAD + 64] = 0.0
            g[a0 + TINY], g[a0 + HUGE], g[a0 + DENORMAL] = 1e-12, 1e12, 1e-20
        assert float(sched[0][1][a0 + DENORMAL]) ** 2 < 2.0 ** -126
        for off in EXCLUDED:
            compared[a0 + off] = False
    return p0.cuda(), [(lr, g.cuda()) for lr, g in sched], marks.cuda(), inside.cuda(), compared.cuda()


def _fused_class(name, kwargs):
    import lgteun_amd
    if name != 'Adam' or kwargs:
        return getattr(lgteun_amd, 'Fused' + name)

    class AdamThroughOptimStep(lgteun_amd.FusedAdam):
        """the plain set through lg_optim_step: the instance (LG_OPT_ADAM, 0), which FusedAdam itself never launches"""

        def _launch(self, engine, g, state):
            self._optim_step(engine, state, self.ALGO, 0, g['lr'], g['betas'][0], g['betas'][1], g['eps'], 0.0)

    return AdamThroughOptimStep


def _torch_leg(name, kwargs, ranges, p0, **route):
    ps = [torch.nn.Parameter(p0[a:b].clone()) for a, b in ranges]
    return ps, getattr(torch.optim, name)(ps, lr=1e-2, **kwargs, **route)


def _torch_step(leg, ranges, lr, g):
    ps, opt = leg
    opt.param_groups[0]['lr'] = lr
    for p, (a, b) in zip(ps, ranges):
        p.grad = g[a:b].clone()
    opt.step()


def _pieces(leg, tensor):
    """torch's tensors of one name, one per range: the parameters or a state buffer"""
    ps, opt = leg
    return [p.detach() if tensor == 'param' else opt.state[p][tensor] for p in ps]


def _run(tag, name, kwargs, layout, steps, plant, grad_scale=None):
    """the fused leg and two torch legs, compared after every step; -> the (algo, opt) words the fused leg launched"""
    n, ranges = layout
    p0, sched, marks, inside, compared = _data(layout, steps, plant)
    flat, gflat, calls = p0.clone(), torch.zeros_like(p0), []
    eng = flat_engine(flat, gflat, ranges, grad_scale, calls)
    opt = _fused_class(name, kwargs)([torch.nn.Parameter(torch.zeros(1))], lr=1e-2, **kwargs)
    names = [s for s in opt.state_names() if s is not None]
    start = dict({s: torch.where(inside, torch.zeros_like(marks), marks) for s in names}, param=p0)
    opt._state = {s: start[s].clone() for s in names}
    first = _torch_leg(name, kwargs, ranges, p0, foreach=True)
    default = _torch_leg(name, kwargs, ranges, p0)
    for i, (lr, g) in enumerate(sched):
        gflat.copy_(g)
        opt.param_groups[0]['lr'] = lr
        opt.step_flat(eng)
        g_ref = g if grad_scale is None else g.mul(grad_scale)
        _torch_step(first, ranges, lr, g_ref)
        _torch_step(default, ranges, lr, g_ref)
        where = f'{tag} {kwargs} step {i + 1}'
        for tensor in names + ['param']:          # the states first: a rounding that parts shows there at its own size
            ref = _pieces(first, tensor)
            assert all(bool(torch.isfinite(t).all()) for t in ref), f'{where} {tensor}: the torch reference is not finite'
            for t, u in zip(ref, _pieces(default, tensor)):
                assert torch.equal(bits(t), bits(u)), (f"{where} {tensor}: torch's default route has moved -- the optimizer built with "
                                                       f'no `foreach` argument is no longer on the bits of foreach=True: {parting(u, t)}')
            got = flat if tensor == 'param' else opt._state[tensor]
            want = start[tensor].clone()
            for (a, b), t in zip(ranges, ref):
                want[a:b] = t
            msg = parting(got, want, compared)
            assert msg is None, f"{where} {tensor}: not on torch's bits: {msg}"
            msg = parting(got, start[tensor], ~inside)
            assert msg is None, f'{where} {tensor}: floats outside the ranges changed: {msg}'
    assert opt._step == steps and len(calls) == steps
    return [_word(*c) for c in calls]


@pytest.mark.parametrize('tag,name,kwargs,owns', SETS, ids=SET_IDS)
def test_every_instance_is_on_torchs_device_bits(tag, name, kwargs, owns):
    launched = _run(tag, name, kwargs, LAYOUT_A, 5, True)
    if owns:
        assert sorted(set(launched)) == sorted(owns), (launched, owns)
        assert (launched[0] in owns) and all(w == launched[1] for w in launched[1:])
    else:
        assert set(launched) <= set(ALL_WORDS)


@pytest.mark.parametrize('tag,name,kwargs,owns', SETS, ids=SET_IDS)
def test_grad_scale_is_torchs_mul_on_the_device(tag, name, kwargs, owns):
    """grad_scale = 1/3 in the launch against torch fed g.mul(1/3): one more rounding, in the same place"""
    _run(tag, name, kwargs, LAYOUT_A, 2, True, grad_scale=1.0 / 3.0)


# ------------------------------------------------------------------------------------------------------------------------
# B. launch geometry
# ------------------------------------------------------------------------------------------------------------------------
def test_layout_b_is_what_part_b_asks_for():
    n, ranges = LAYOUT_B
    lens = [b - a for a, b in ranges]
    assert 1 in lens and ranges[-1][1] == n
    assert any(ranges[i][1] == ranges[i + 1][0] for i in range(len(ranges) - 1))          # two adjacent ranges
    (a, b), = [r for r in ranges if r[1] - r[0] == LONG]
    assert a % 2 == 1 and max(lens) == LONG
    # Engine.max_range is the longest range: the grid is capped at 512 workgroups, so the first 777 elements of the long range are a second trip
    assert (LONG + 255) // 256 > 512 and 0 < LONG - 512 * 256 < 256 * 512 and (LONG - 512 * 256) % 256


@pytest.mark.parametrize('tag,name,kwargs', GEOMETRY_SETS, ids=[s[0] for s in GEOMETRY_SETS])
def test_second_trip_of_the_stride_loop_is_on_torchs_device_bits(tag, name, kwargs):
    _run(tag, name, kwargs, LAYOUT_B, 2, False)


def _cut(ranges, piece=1000):
    out = []
    for a, b in ranges:
        out += [(x, min(x + piece, b)) for x in range(a, b, piece)] if b - a == LONG else [(a, b)]
    assert sum(b - a for a, b in out) == sum(b - a for a, b in ranges) and all(x[1] <= y[0] for x, y in zip(out, out[1:]))
    return out


@pytest.mark.parametrize('entry', ['lg_adam_step', 'lg_optim_step_ex-plain_adam-clip-ema'])
def test_a_result_does_not_depend_on_how_the_ranges_are_cut(entry):
    """two steps over LAYOUT_B and over the same floats with the long range cut into pieces of 1000 (136 ranges, max_range 10 003: a
    grid of 40 x 136 against 512 x 5): parameters, both moments and the average bit for bit; the floats outside untouched"""
    import ctypes
    from lgteun_amd import _lib
    from lgteun_amd.engine import _ptr, _stream_ptr
    lib = _lib.lib()
    n, ranges = LAYOUT_B
    p0, sched, marks, inside, _ = _data(LAYOUT_B, 2, False)
    coef = torch.tensor([9.0, 0.37], device='cuda')                        # read at + 4 bytes, like out + 1 of lg_grad_norm
    legs = []
    for rs in (list(ranges), _cut(ranges)):
        assert all(0 <= a < b <= n for a, b in rs)
        rd = torch.tensor([v for r in rs for v in r], dtype=torch.int64, device='cuda')
        legs.append(dict(p=p0.clone(), m=torch.where(inside, torch.zeros_like(marks), marks), v=torch.where(inside, torch.zeros_like(marks), marks.abs()),
                         ema=marks.flip(0).clone(), rd=rd, nr=len(rs), mr=max(b - a for a, b in rs)))
    assert legs[0]['mr'] == LONG and legs[1]['mr'] == 10003 and legs[1]['nr'] == 136
    keys = ('p', 'm', 'v') if entry == 'lg_adam_step' else ('p', 'm', 'v', 'ema')
    first = {k: legs[0][k].clone() for k in keys}
    for i, (lr, g) in enumerate(sched):
        for L in legs:
            if entry == 'lg_adam_step':
                rc = lib.lg_adam_step(_ptr(L['p']), _ptr(g), _ptr(L['m']), _ptr(L['v']), _ptr(L['rd']), L['nr'], L['mr'], i + 1, lr, 0.9, 0.999,
                                      1e-8, 1.0, _stream_ptr())
            else:
                rc = lib.lg_optim_step_ex(_ptr(L['p']), _ptr(g), _ptr(L['m']), _ptr(L['v']), None, _ptr(L['rd']), L['nr'], L['mr'], i + 1, ADAM, 0,
                                          lr, 0.9, 0.999, 1e-8, 0.0, 1.0, ctypes.c_void_p(coef.data_ptr() + 4), _ptr(L['ema']), 0.99, 1,
                                          _stream_ptr())
            assert rc == 0, lib.lg_last_error()
        torch.cuda.synchronize()
        for k in keys:
            msg = parting(legs[1][k], legs[0][k])
            assert msg is None, f'{entry} step {i + 1} {k}: the cut ranges give other bits: {msg}'
            msg = parting(legs[0][k], first[k], ~inside)
            assert msg is None, f'{entry} step {i + 1} {k}: floats outside the ranges changed: {msg}'
            assert not torch.equal(bits(legs[0][k])[inside], bits(first[k])[inside]), (entry, k)
