"""No GPU needed: the argument contract of the NETWORK entries of include/lgteun_hip.h ("The network entries' argument contract") -- lgteun_forward,
lgteun_backward, lgteun_dead_forward, the lg_op_* entries, lg_l1_loss / lg_l2_loss, the optimizer steps and lg_dropout_mask -- the way
tests/test_abi_limits_cpu.py holds the entries around the network (tests/test_gpu_net_limits.py runs the accepted side on the device).

The header promises that arguments are validated before any HIP call.  So a call with ONE argument outside its range is safe with pointers that are
never dereferenced (limits_helpers.FAKE): every case below was read against the validator (csrc/net_args.h, and the entry's own lines behind it)
before it was written, returns a negative code, and leaves a message that begins with the entry's prefix, names the argument and is no HIP error
string.  No value inside the ranges ever goes to a launcher with fake pointers: the accepted values go to the sizers only.

The batch bound is computed HERE from the header's formula (limits_helpers.net_max_batch), never read back from the library.

Held elsewhere, not repeated: tests/test_fused_optim_cpu.py and tests/test_train_controls_cpu.py hold the null pointers, step, algo, the foreign option
flag, the missing state buffer, ema_decay, plain_adam and the 4-byte alignment of clip_coef of lg_optim_step / lg_optim_step_ex; tests/test_route_cpu.py
holds lg_plan_create's own rejections.

The sizer.  lg_workspace_bytes is the forward carving (workspace.h: carve) plus, for train != 0, the backward's slabs, and lg_debug_live_slot reports
the two parts.  The issue's form of the 32-bit-product check, ws(bound) / ws(2) against bound / 2, cannot hold for this sizer as it stands: the
carving has regions that do not depend on B (the per-block tables: 160 KiB of pos_emb rows per stage) and the backward's slabs are capped per
launch (516 MB at B = 2 on 16 x 16 planes, 36 GiB at B = 16383: a quotient of 75 against 8191.5), so the exact expected value is stated instead:
every B-dependent region of the carving holds a whole number of floats per sample, so at batches that are multiples of 64 every region ends on a
256-byte line and the carving is EXACTLY affine in B -- carve(b) = carve(64) + (b - 64) / 64 (carve(128) - carve(64)) for the largest multiple of 64
up to the bound, with no slack at all -- and at the bound itself it lies within one 256-byte line per region (at most 160) above that line.  A product
that wrapped anywhere between B = 128 and the bound breaks the equality.

The backward's part (k_bwd.hip: the gradient tensors dh2, dh1, dx, dqkv ..., each a whole number of floats per sample, and the arena of the
weight-gradient slabs, whose size stops growing once every launch has reached its cap of workgroups) gets its exact statement too.  With u = 64
samples (4 where the bound is below 256) and top the largest multiple of u up to the bound, bwd(top) - bwd(top - u) == bwd(top - u) - bwd(top - 2 u) =: s,
the bytes of u more samples, exactly.  The remainder r(m) = bwd(m) - s m / u -- the arena beyond its B-proportional share -- is then asserted, over the
doubling ladder m = u, 2 u, 4 u ... and the last three multiples: never growing with m (516 MB of fixed slabs at small batches fall to 85 MB once the
proportional regions have outgrown them), the same value at the last three, positive, and at most bwd(u).  A 32-bit product that wrapped anywhere
below the bound lowers bwd by a multiple of 4 GiB from there on and drives r(top), at most 0.6 GB on every plan, below zero; one that wraps inside the last 2 u
samples breaks the equality of the differences."""
import ctypes

import pytest

from limits_helpers import (FAKE, F_BWD_DATA, F_BWD_LGT, F_CHAINED, F_DEFER_DEAD, F_DEFINED, F_DROPOUT, F_FAITHFUL, F_LIVE_APART, F_SAVE, F_STAGEWISE,
                            F_UNDEFINED_BIT, NetPlan, net_max_batch)
from lgteun_amd import _lib

P, PW, Q = FAKE, FAKE + (1 << 24), FAKE + 4          # two aligned fake pointers; one that is 4 bytes off every 8-, 16- and 256-byte alignment
WS = 1 << 40                                         # workspace_bytes that no sizer exceeds: a size check never fires before the one under test
NULL = None
HIP_WORDS = ('hip', 'invalid device', 'no rocm', 'illegal', 'launch fail', 'out of memory')
PLAN_SHAPES = [(C, K, H, W) for C in (4, 8) for K in (1, 3, 16) for H, W in ((16, 16), (128, 128), (16, 1024), (1024, 1024))]
FWD_ONLY = F_DEFINED & ~(F_BWD_LGT | F_BWD_DATA)

_plans = {}


def plan(shape):
    if shape not in _plans:
        _plans[shape] = NetPlan(*shape)
    return _plans[shape]


def L():
    return _lib.lib()


# entry -> (message prefix, argument names in ABI order, arguments every check accepts ('plan' is filled per plan), the float tensors (16-byte aligned),
#           train of lg_workspace_bytes for the accepted flags, flag sets that do not apply (each a whole `flags` word))
NOT_FWD = [F_BWD_LGT, F_BWD_DATA]
NOT_OP = [F_FAITHFUL, F_BWD_LGT, F_BWD_DATA, F_CHAINED, F_DEFER_DEAD, F_STAGEWISE, F_LIVE_APART]
PLAN_ENTRIES = {
    'lgteun_forward': ('forward', 'plan params ms pan out workspace workspace_bytes B flags seed stream',
                       dict(params=P, ms=P, pan=P, out=P, workspace=PW, workspace_bytes=WS, B=2, flags=0, seed=0), 'params ms pan out', 0, NOT_FWD),
    'lgteun_backward': ('backward', 'plan params grads ms pan dout workspace workspace_bytes B flags seed stream',
                        dict(params=P, grads=P, ms=P, pan=P, dout=P, workspace=PW, workspace_bytes=WS, B=2, flags=F_SAVE, seed=0), 'params grads ms pan dout', 1,
                        [F_CHAINED | F_BWD_LGT, F_CHAINED | F_BWD_DATA]),
    'lgteun_dead_forward': ('dead_forward', 'plan params workspace workspace_bytes B flags seed stream',
                            dict(params=P, workspace=PW, workspace_bytes=WS, B=2, flags=F_FAITHFUL, seed=0), 'params', 0,
                            [0, F_FAITHFUL | F_CHAINED, F_FAITHFUL | F_BWD_LGT, F_FAITHFUL | F_BWD_DATA]),
    'lg_op_data_step': ('op_data_step', 'plan params stage z_in ms pan z_out tmp B stream',
                        dict(params=P, stage=0, z_in=P, ms=P, pan=P, z_out=P, tmp=P, B=2), 'params z_in ms pan z_out tmp', 0, []),
    'lg_op_lgt': ('op_lgt', 'plan params stage z out workspace workspace_bytes B flags seed stream',
                  dict(params=P, stage=0, z=P, out=P, workspace=PW, workspace_bytes=WS, B=2, flags=0, seed=0), 'params z out', 0, NOT_OP),
    'lg_op_lgt_stages': ('op_lgt_stages', 'plan params stage0 n z out workspace workspace_bytes B flags seed grid_cap stream',
                         dict(params=P, stage0=0, n=1, z=P, out=P, workspace=PW, workspace_bytes=WS, B=2, flags=0, seed=0, grid_cap=0), 'params z out', 0,
                         NOT_OP + [F_SAVE]),
    'lg_op_block': ('op_block', 'plan params stage blk which x y workspace workspace_bytes B stream',
                    dict(params=P, stage=0, blk=0, which=0, x=P, y=P, workspace=PW, workspace_bytes=WS, B=2), 'params x y', 0, []),
    'lg_op_block_bwd': ('op_block_bwd', 'plan params grads stage blk which x dy dx workspace workspace_bytes B stream',
                        dict(params=P, grads=P, stage=0, blk=0, which=0, x=P, dy=P, dx=P, workspace=PW, workspace_bytes=WS, B=2), 'params grads x dy dx', 1, []),
    'lg_op_data_step_bwd': ('op_data_step_bwd', 'plan params grads stage z_in ms pan dz_out dz_in workspace workspace_bytes B stream',
                            dict(params=P, grads=P, stage=0, z_in=P, ms=P, pan=P, dz_out=P, dz_in=P, workspace=PW, workspace_bytes=WS, B=2),
                            'params grads z_in ms pan dz_out dz_in', 1, []),
    'lg_op_lgt_bwd': ('op_lgt_bwd', 'plan params grads stage z dout dz workspace workspace_bytes B flags seed stream',
                      dict(params=P, grads=P, stage=0, z=P, dout=P, dz=P, workspace=PW, workspace_bytes=WS, B=2, flags=0, seed=0), 'params grads z dout dz', 1,
                      NOT_OP + [F_SAVE]),
}


def plan_cases(entry, shape):
    """every (one bad argument, what the message must name) of a plan entry on one plan"""
    _, names, good, floats, train, not_applicable = PLAN_ENTRIES[entry]
    C, K, H, W = shape
    names = names.split()
    cases = [(dict(plan=NULL), 'plan is NULL')]
    cases += [({n: NULL}, f'{n} is NULL') for n in floats.split()]
    cases += [({n: Q}, f'{n} must be 16-byte aligned') for n in floats.split()]
    if 'workspace' in names:
        cases += [(dict(workspace=NULL), 'workspace is NULL'), (dict(workspace=Q), 'workspace must be 256-byte aligned'),
                  (dict(workspace=PW + 128), 'workspace must be 256-byte aligned'),
                  (dict(workspace_bytes=plan(shape).ws(2, train) - 1), 'workspace too small (workspace_bytes')]
    cases += [(dict(B=b), 'B must be') for b in (0, -1, net_max_batch(C, K, H, W, train) + 1)]
    for st in ('stage', 'stage0'):
        if st in names:
            cases += [({st: -1}, f'{st} must be'), ({st: K}, f'{st} must be')]
    if 'n' in names:
        cases += [(dict(n=0), 'n must be'), (dict(n=K + 1), 'n must be'), (dict(grid_cap=-1), 'grid_cap must be')]
        if K >= 2 and not (C == 4 and K >= 3 and H <= 128 and W <= 128):
            cases += [(dict(n=2), 'one stage per pass')]          # (tests/test_gpu_stage_batch.py holds this text too)
        if K >= 3:
            cases += [(dict(n=K), 'n: this plan')]                            # n > K-1 where the plan batches, one stage per pass where it does not
    if 'blk' in names:
        cases += [(dict(blk=-1), 'blk must be'), (dict(blk=5), 'blk must be'), (dict(which=3), 'which must be'), (dict(which=-1), 'which must be')]
    if 'flags' in names:
        cases += [(dict(flags=good['flags'] | F_UNDEFINED_BIT), 'flags has bits'), (dict(flags=good['flags'] | (1 << 30)), 'flags has bits')]
        cases += [(dict(flags=f), 'flags') for f in not_applicable]            # ('flags 0x.. do not apply' or 'flags: ...', the entry's own rule)
    return cases


def call(entry, names, good, bad, handle):
    args = dict(good, stream=NULL)
    if 'plan' in names:
        args['plan'] = handle
    assert set(bad) <= set(names) and set(args) == set(names), (entry, bad, sorted(set(names) ^ set(args)))
    args.update(bad)
    L().lg_batch_assemble(NULL, NULL, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, 0, 0, 0, 1.0, 0, 1.0, NULL)     # leaves another entry's message
    rc = getattr(L(), entry)(*[args[n] for n in names])
    return rc, L().lg_last_error().decode()


def check_rejected(entry, prefix, bad, says, rc, msg):
    assert rc < 0, (entry, bad, rc, msg)
    assert msg.startswith(prefix + ':'), (entry, bad, msg)
    assert says in msg, (entry, bad, says, msg)
    assert not any(w in msg.lower() for w in HIP_WORDS), (entry, bad, msg)


@pytest.mark.parametrize('entry', sorted(PLAN_ENTRIES))
@pytest.mark.parametrize('shape', PLAN_SHAPES, ids=lambda s: 'C%d-K%d-%dx%d' % s)
def test_plan_entry_rejects_one_argument_outside_its_range_by_name(entry, shape):
    prefix, names, good = PLAN_ENTRIES[entry][:3]
    cases = plan_cases(entry, shape)
    assert len(cases) >= 8
    for bad, says in cases:
        rc, msg = call(entry, names.split(), good, bad, plan(shape).handle)
        check_rejected(entry, prefix, bad, says, rc, msg)


def test_return_codes_keep_their_meaning():
    """-1 null / invalid, -2 unsupported (a defined flag that does not apply), -3 workspace too small -- and the texts existing tests match"""
    shape = (4, 3, 16, 16)
    prefix, names, good = PLAN_ENTRIES['lgteun_forward'][:3]
    for bad, code, says in ((dict(ms=NULL), -1, 'ms is NULL'), (dict(B=0), -1, 'B must be in 1 .. 16383'), (dict(flags=F_UNDEFINED_BIT), -1, 'does not define'),
                            (dict(flags=F_BWD_LGT), -2, 'do not apply'), (dict(workspace_bytes=plan(shape).ws(2, 0) - 1), -3, 'workspace too small')):
        rc, msg = call('lgteun_forward', names.split(), good, bad, plan(shape).handle)
        assert rc == code and says in msg, (bad, rc, msg)
    prefix, names, good = PLAN_ENTRIES['lgteun_backward'][:3]
    rc, msg = call('lgteun_backward', names.split(), good, dict(flags=F_CHAINED | F_BWD_LGT), plan(shape).handle)
    assert rc == -2 and 'do not apply to LG_FLAG_CHAINED' in msg, (rc, msg)
    prefix, names, good = PLAN_ENTRIES['lgteun_dead_forward'][:3]
    rc, msg = call('lgteun_dead_forward', names.split(), good, dict(flags=0), plan(shape).handle)
    assert rc == -2 and 'only the faithful unfolding has dead stages' in msg, (rc, msg)
    # the size check uses the train the flags imply: a forward-only workspace is too small for LG_FLAG_SAVE, a one-set workspace for LG_FLAG_CHAINED
    prefix, names, good = PLAN_ENTRIES['lgteun_forward'][:3]
    for flags, have in ((F_SAVE, plan(shape).ws(2, 0)), (F_SAVE | F_CHAINED, plan(shape).ws(2, 1))):
        rc, msg = call('lgteun_forward', names.split(), good, dict(flags=flags, workspace_bytes=have), plan(shape).handle)
        assert rc == -3 and 'workspace too small' in msg, (flags, rc, msg)


# ------------------------------------------------------------------------------------------------------------------------
# the entries without a plan
# ------------------------------------------------------------------------------------------------------------------------
LOSS = dict(out=P, gt=P, dout=P, loss_accum=P, n_local=64, n_global=64, scale=1.0)
ADAM = dict(params=P, grads=P, exp_avg=P, exp_avg_sq=P, ranges=P, n_ranges=2, max_range=100, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0)
OPT = dict(params=P, grads=P, state0=P, state1=P, state2=NULL, ranges=P, n_ranges=2, max_range=100, step=1, algo=_lib.LG_OPT_ADAM, flags=0, lr=1e-3, h0=0.9, h1=0.999,
           eps=1e-8, weight_decay=0.0, grad_scale=1.0)
FLAT_ENTRIES = {
    'lg_op_resample': ('op_resample', 'x y planes hi wi mode stream', dict(x=P, y=P, planes=3, hi=8, wi=8, mode=2)),
    'lg_l1_loss': ('l1_loss', 'out gt dout loss_accum n_local n_global scale stream', LOSS),
    'lg_l2_loss': ('l2_loss', 'out gt dout loss_accum n_local n_global scale stream', LOSS),
    'lg_adam_step': ('adam_step', 'params grads exp_avg exp_avg_sq ranges n_ranges max_range step lr beta1 beta2 eps grad_scale stream', ADAM),
    'lg_optim_step': ('optim_step', 'params grads state0 state1 state2 ranges n_ranges max_range step algo flags lr h0 h1 eps weight_decay grad_scale stream', OPT),
    'lg_optim_step_ex': ('optim_step', 'params grads state0 state1 state2 ranges n_ranges max_range step algo flags lr h0 h1 eps weight_decay grad_scale clip_coef ema '
                         'ema_decay plain_adam stream', dict(OPT, clip_coef=NULL, ema=NULL, ema_decay=0.0, plain_adam=0)),
    'lg_optim_step_ex-plain': ('optim_step_ex', 'params grads state0 state1 state2 ranges n_ranges max_range step algo flags lr h0 h1 eps weight_decay grad_scale clip_coef '
                               'ema ema_decay plain_adam stream', dict(OPT, clip_coef=NULL, ema=NULL, ema_decay=0.0, plain_adam=1)),
    'lg_dropout_mask': ('dropout_mask', 'seed stage blk first n out stream', dict(seed=1, stage=0, blk=0, first=0, n=64, out=P)),
}
FLAT_REJECTED = [('lg_op_resample', dict([kv]), says) for kv, says in (
    (('x', NULL), 'x is NULL'), (('y', NULL), 'y is NULL'), (('x', Q), 'x must be 16-byte aligned'), (('y', Q), 'y must be 16-byte aligned'), (('planes', 0), 'planes must be'),
    (('planes', -1), 'planes must be'), (('hi', 0), 'hi must be'), (('wi', 0), 'wi must be'), (('mode', 3), 'mode must be'), (('mode', -1), 'mode must be'))]
FLAT_REJECTED += [('lg_op_resample', dict(hi=16384, wi=16384), 'hi * wi'), ('lg_op_resample', dict(mode=0, hi=7), 'hi and wi'), ('lg_op_resample', dict(mode=0, wi=7), 'hi and wi')]
for _e in ('lg_l1_loss', 'lg_l2_loss'):
    FLAT_REJECTED += [(_e, {n: NULL}, f'{n} is NULL') for n in ('out', 'gt', 'dout', 'loss_accum')]
    FLAT_REJECTED += [(_e, {n: Q}, f'{n} must be 16-byte aligned') for n in ('out', 'gt', 'dout')]
    FLAT_REJECTED += [(_e, dict(loss_accum=P + 2), 'loss_accum must be 4-byte aligned'), (_e, dict(n_local=0), 'n_local must be'), (_e, dict(n_global=0), 'n_global must be')]
FLAT_REJECTED += [('lg_adam_step', {n: NULL}, f'{n} is NULL') for n in ('params', 'grads', 'exp_avg', 'exp_avg_sq', 'ranges')]
FLAT_REJECTED += [('lg_adam_step', {n: Q}, f'{m} must be 16-byte aligned') for n, m in (('params', 'params'), ('grads', 'grads'), ('exp_avg', 'state0'), ('exp_avg_sq', 'state1'))]
FLAT_REJECTED += [('lg_adam_step', dict(ranges=Q), 'ranges must be 8-byte aligned'), ('lg_adam_step', dict(n_ranges=0), 'n_ranges must be in 1 .. 65535'),
                  ('lg_adam_step', dict(n_ranges=65536), 'n_ranges must be in 1 .. 65535'), ('lg_adam_step', dict(step=0), 'step must be')]
for _e in ('lg_optim_step', 'lg_optim_step_ex', 'lg_optim_step_ex-plain'):        # (nulls, step, algo, flags, state buffers: the two files the docstring names)
    FLAT_REJECTED += [(_e, {n: Q}, f'{n} must be 16-byte aligned') for n in ('params', 'grads', 'state0', 'state1')]
    FLAT_REJECTED += [(_e, dict(ranges=Q), 'ranges must be 8-byte aligned'), (_e, dict(n_ranges=65536), 'n_ranges must be in 1 .. 65535'), (_e, dict(n_ranges=-1), 'n_ranges must be')]
FLAT_REJECTED += [('lg_optim_step', dict(state2=Q, flags=_lib.LG_OPT_AMSGRAD), 'state2 must be 16-byte aligned'), ('lg_optim_step', dict(flags=8), 'flags'),
                  ('lg_optim_step', dict(state1=NULL), 'state1 is NULL'), ('lg_optim_step', dict(algo=4), 'algo must be')]
FLAT_REJECTED += [('lg_dropout_mask', dict([kv]), says) for kv, says in (
    (('out', NULL), 'out is NULL'), (('out', Q), 'out must be 16-byte aligned'), (('stage', -1), 'stage must be'), (('stage', 16), 'stage must be'), (('blk', -1), 'blk must be'),
    (('blk', 5), 'blk must be'), (('first', -1), 'first must be'), (('n', -1), 'n must be'))]


@pytest.mark.parametrize('entry,bad,says', FLAT_REJECTED, ids=[f'{e}-{"-".join(f"{k}={v}" for k, v in b.items())}' for e, b, _ in FLAT_REJECTED])
def test_flat_entry_rejects_one_argument_outside_its_range_by_name(entry, bad, says):
    prefix, names, good = FLAT_ENTRIES[entry]
    rc, msg = call(entry.split('-')[0], names.split(), good, bad, None)
    check_rejected(entry, prefix, bad, says, rc, msg)


def test_every_network_entry_is_listed():
    listed = set(PLAN_ENTRIES) | {e.split('-')[0] for e in FLAT_ENTRIES}
    assert listed == {'lgteun_forward', 'lgteun_backward', 'lgteun_dead_forward', 'lg_op_resample', 'lg_op_data_step', 'lg_op_lgt', 'lg_op_lgt_stages', 'lg_op_block',
                      'lg_op_block_bwd', 'lg_op_data_step_bwd', 'lg_op_lgt_bwd', 'lg_l1_loss', 'lg_l2_loss', 'lg_adam_step', 'lg_optim_step', 'lg_optim_step_ex',
                      'lg_dropout_mask'}
    assert {e.split('-')[0] for e, _, _ in FLAT_REJECTED} == {e.split('-')[0] for e in FLAT_ENTRIES}


# ------------------------------------------------------------------------------------------------------------------------
# the bound and the sizer
# ------------------------------------------------------------------------------------------------------------------------
def test_the_bound_is_what_the_header_says_at_the_shapes_it_quotes():
    assert net_max_batch(4, 1, 16, 16, 0) == 16383 and net_max_batch(8, 1, 16, 16, 0) == 8191        # the grid limit: B C <= 65535
    assert net_max_batch(4, 3, 16, 16, 0) == 16383 and net_max_batch(4, 16, 16, 16, 1) == 8191       # K = 16: 16 B samples in one launch, the element bound
    assert net_max_batch(4, 16, 16, 16, 2) == 16383                                                # chained: one stage per launch
    assert net_max_batch(4, 4, 128, 128, 1) == 511 and net_max_batch(4, 1, 1024, 1024, 0) == 31 and net_max_batch(8, 1, 1024, 1024, 0) == 15
    assert 16383 * 4 <= 65535 < 16384 * 4 and 8191 * 8 <= 65535 < 8192 * 8
    for C, K, H, W in PLAN_SHAPES:
        for train in (0, 1, 2):
            b = net_max_batch(C, K, H, W, train)
            S = K if (C == 4 and K >= 3 and H <= 128 and W <= 128 and train != 2) else 1
            assert b >= 1 and b * C <= 65535 and S * b * 16 * C * H * W < 2 ** 31
            assert (b + 1) * C > 65535 or S * (b + 1) * 16 * C * H * W >= 2 ** 31


@pytest.mark.parametrize('shape', PLAN_SHAPES, ids=lambda s: 'C%d-K%d-%dx%d' % s)
def test_sizer_is_positive_inside_the_range_zero_outside_and_never_shrinks(shape):
    p = plan(shape)
    for train in (0, 1, 2):
        b = p.bound(train)
        vals = [p.ws(B, train) for B in sorted({1, 2, b - 1, b} - {0})]
        assert vals[0] > 0 and all(x <= y for x, y in zip(vals, vals[1:])), (shape, train, vals)
        assert p.ws(b + 1, train) == 0 and p.ws(0, train) == 0 and p.ws(-1, train) == 0, (shape, train)
        assert p.ws(2 ** 31 - 1, train) == 0 and p.ws(-2 ** 31, train) == 0
    assert p.ws(1, 3) == 0 and p.ws(1, -1) == 0


MAX_REGIONS = 160          # carve() takes fewer regions than this for K = 16 (17 Z + 48 data-step + 5 tables + 16 X + 5 x 14 per block + 7)


@pytest.mark.parametrize('shape', PLAN_SHAPES, ids=lambda s: 'C%d-K%d-%dx%d' % s)
def test_the_carving_at_the_bound_is_the_exact_affine_value(shape):
    """the 32-bit-product check, in the exact form the module docstring derives"""
    p = plan(shape)
    for train in (0, 1, 2):
        b = p.bound(train)
        parts = {B: p.parts(B, train) for B in sorted({1, 2, b - 1, b})}
        for B, (fwd, bwd) in parts.items():
            assert fwd + bwd == p.ws(B, train) and fwd > 0 and (bwd > 0) == (train != 0), (shape, train, B, fwd, bwd)
        seq = [parts[B] for B in sorted(parts)]
        assert all(x[0] <= y[0] and x[1] <= y[1] for x, y in zip(seq, seq[1:])), (shape, train, seq)       # both parts never shrink
        if b < 192:       # 1024 x 1024 and the K = 16 slots at 128 x 128: the bound is below three multiples of 64; a multiple of 4 fills whole lines there
            unit = 4 if b >= 12 else 1
        else:
            unit = 64
        top = b // unit * unit
        f1, f2, ft = p.parts(unit, train)[0], p.parts(2 * unit, train)[0], p.parts(top, train)[0]
        slope = f2 - f1
        assert slope > 0
        line = lambda B: f1 * unit + (B - unit) * slope                                                  # unit x the affine value, in integers
        if unit > 1:
            assert ft * unit == line(top), (shape, train, unit, top, ft, line(top) / unit)
        fb = p.parts(b, train)[0]
        assert line(b) <= fb * unit <= line(b) + 256 * MAX_REGIONS * unit, (shape, train, b, fb, line(b) / unit)
        print(f'{shape} train {train}: bound {b}, carve({top}) = {ft} bytes exactly on the line, carve(bound) {fb - line(b) // unit} bytes above it')


@pytest.mark.parametrize('shape', PLAN_SHAPES, ids=lambda s: 'C%d-K%d-%dx%d' % s)
def test_the_backward_part_at_the_bound_is_the_exact_affine_value(shape):
    """the 32-bit-product check of the backward's part of a train workspace, in the exact form the module docstring derives"""
    p = plan(shape)
    for train in (1, 2):
        b = p.bound(train)
        assert b >= 12
        unit = 64 if b >= 256 else 4
        top = b // unit * unit
        bwd = lambda B: p.parts(B, train)[1]
        s = bwd(top) - bwd(top - unit)
        assert s > 0 and s == bwd(top - unit) - bwd(top - 2 * unit), (shape, train, top, s, bwd(top - unit) - bwd(top - 2 * unit))
        ladder, m = {top - 2 * unit, top - unit, top}, unit
        while m < top:
            ladder.add(m)
            m *= 2
        ladder = sorted(ladder)
        r = [bwd(m) - s * (m // unit) for m in ladder]
        assert all(x >= y for x, y in zip(r, r[1:])), (shape, train, list(zip(ladder, r)))
        assert r[-1] == r[-2] == r[-3] and 0 < r[-1] <= r[0] <= bwd(unit), (shape, train, list(zip(ladder, r)), bwd(unit))
        assert r[0] < 2 ** 32, (shape, train, r[0])          # a wrap lowers the remainder by a multiple of 4 GiB: it cannot hide inside it
        assert bwd(top) <= bwd(b) <= bwd(top) + s, (shape, train, b, top)
        print(f'{shape} train {train}: bound {b}, {s} bytes per {unit} samples, remainder {r[0]} -> {r[-1]} bytes over B = {ladder[0]} .. {top}')


def test_scene_auto_batch_keeps_to_the_plan_bound():
    """scene.auto_batch reads lg_workspace_bytes, which is 0 above the bound: with memory to spare, 64 tiles of 1024 x 1024 give the bound (31 at C = 4,
    15 at C = 8; 768 x 768, C = 4: 56), a batch the sizer and the entries accept, never the 64 it starts from; with little memory a smaller one that fits"""
    from types import SimpleNamespace
    from lgteun_amd import scene
    eng = SimpleNamespace(lib=L())
    for C, side, want in ((4, 1024, 31), (8, 1024, 15), (4, 768, 56), (4, 128, 64)):
        p = NetPlan(C, 2, side, side)
        B = scene.auto_batch(eng, p.handle, C, side, side, 64, 1 << 50)
        assert B == want == min(64, p.bound(0)) and p.ws(B, 0) > 0, (C, side, B, want)
        assert scene.auto_batch(eng, p.handle, C, side, side, 3, 1 << 50) == 3
        tight = 2 * (p.ws(2, 0) + 2 * 4 * (side * side + C * side * side // 16 + C * side * side))
        B = scene.auto_batch(eng, p.handle, C, side, side, 64, tight)
        assert B == 2 and p.ws(B, 0) > 0, (C, side, B)
        assert scene.auto_batch(eng, p.handle, C, side, side, 64, 0) == 1


def test_fake_pointers_are_what_the_docstring_says():
    assert P % 4096 == 0 and PW % 4096 == 0 and Q % 8 == 4 and (PW + 128) % 256 == 128 and ctypes.sizeof(ctypes.c_void_p) == 8
