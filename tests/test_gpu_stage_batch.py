"""The dead-stage LGT forwards of a faithful step as ONE pass over (K-1) B samples (include/lgteun_hip.h: LG_FLAG_STAGEWISE, lg_op_lgt_stages).

Every forward kernel of the C = 4 route is launched once over the samples of all dead stages and each workgroup picks its stage's weights by
its sample (csrc/kernels.h: StageSel).  The work and the arithmetic are those of the stage-by-stage order, so every comparison here is
BITWISE: torch.equal, no tolerance.  Shapes are the smallest that still run more than one workgroup per kernel and both plane sizes
(PAN 32: 32 x 32 and 16 x 16 planes; PAN 64: 64 x 64 and 32 x 32)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detweights as dw  # noqa: E402

T = torch.from_numpy


def _stages(ops, stage0, n, z, flags=0, seed=0, grid_cap=0):
    """lg_op_lgt_stages: z [n,B,C,H,W] -> out [n,B,C,H,W]"""
    from gpu_helpers import assert_guards_intact, guarded_empty
    from lgteun_amd import _lib
    from lgteun_amd.engine import _ptr, _stream_ptr
    B = z.shape[1]
    buf, out = guarded_empty(tuple(z.shape), z.device)
    ws = ops.ws(B)
    _lib.check(ops.lib.lg_op_lgt_stages(ops.plan, _ptr(ops.eng.flat), stage0, n, _ptr(z), _ptr(out), _ptr(ws), ws.numel(), B, flags, seed,
                                        grid_cap, _stream_ptr()), 'lg_op_lgt_stages')
    assert_guards_intact(buf, 'lg_op_lgt_stages')
    return out


def _z(n, B, C, pan, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, B, C, pan, pan, generator=g).cuda()


def _ops(C, K, pan):
    from gpu_helpers import Ops, make_module
    net = make_module(C, K)          # det_params weights: every tensor of every stage has its own values
    return net, Ops(net, pan, pan)


@pytest.mark.parametrize('drop', [False, True])
@pytest.mark.parametrize('C,pan,B,n', [(4, 32, 3, 3), (4, 64, 2, 3), (4, 32, 1, 2)])
def test_stages_pass_is_bitwise_the_stage_by_stage_lgts(C, pan, B, n, drop):
    """n stages in one pass against n lg_op_lgt calls, dropout off and on (same seed): bitwise"""
    from lgteun_amd import _lib
    net, ops = _ops(C, n + 1, pan)
    z = _z(n, B, C, pan, 11)
    flags, seed = (_lib.LG_FLAG_DROPOUT, 0x1234567) if drop else (0, 0)
    want = torch.stack([ops.lgt(s, z[s].contiguous(), flags, seed) for s in range(n)])
    got = _stages(ops, 0, n, z, flags, seed)
    assert torch.isfinite(want).all()
    assert not torch.equal(want[0], ops.lgt(1, z[0].contiguous(), flags, seed))     # the stages' weights do differ
    for s in range(n):
        assert torch.equal(got[s], want[s]), (s, float((got[s] - want[s]).abs().max()))
    if drop:
        assert not torch.equal(got, _stages(ops, 0, n, z, 0, 0))                    # and dropout did something


def _runs(units, grid):
    """the contiguous runs [u0, u1) the workgroups of a multi-stage launch take (csrc/k_ffn_xr.hip: run0, run1)"""
    return [(w * units // grid, (w + 1) * units // grid) for w in range(grid)]


def _crossing(units_per_stage, n, grid):
    """does some workgroup's run hold units of two stages?"""
    return any(u0 // units_per_stage != (u1 - 1) // units_per_stage for u0, u1 in _runs(units_per_stage * n, grid) if u1 > u0)


@pytest.mark.parametrize('drop', [False, True])
def test_restaging_at_a_stage_boundary(drop):
    """grid_cap = 5 makes the persistent kernels walk runs of strips / window quads that cross from one stage's samples into the next
    one's: the workgroup stages its tables again there.  Unit counts per stage at PAN 32, B = 3 (the launchers' geometry): k_ffn_xr 16-row
    strips of 16 columns, 3 x 2 x 2 = 12; k_ffn_x32 (16 x 16 planes) 3 x 1 x 1 = 3; k_attn_m window quads 3 x 16 / 4 = 12 and 3 x 4 / 4 = 3."""
    from lgteun_amd import _lib
    C, pan, B, n, cap = 4, 32, 3, 3, 5
    per_stage = {'k_ffn_xr': B * (pan // 16) * (pan // 16), 'k_ffn_x32': B * 1 * 1, 'k_attn_m<8>': B * (pan // 8) ** 2 // 4, 'k_attn_m<16>': B * (pan // 16) ** 2 // 4}
    for name, u in per_stage.items():
        grid = min(cap, u * n)
        assert _crossing(u, n, grid), (name, u, grid)
    net, ops = _ops(C, n + 1, pan)
    z = _z(n, B, C, pan, 12)
    flags, seed = (_lib.LG_FLAG_DROPOUT, 0xABCDEF) if drop else (0, 0)
    want = torch.stack([ops.lgt(s, z[s].contiguous(), flags, seed) for s in range(n)])
    got = _stages(ops, 0, n, z, flags, seed, grid_cap=cap)
    for s in range(n):
        assert torch.equal(got[s], want[s]), (s, float((got[s] - want[s]).abs().max()))
    assert torch.equal(got, _stages(ops, 0, n, z, flags, seed))          # the partition does not matter


def _deadout(eng, plan, B, K, C, pan):
    from lgteun_amd import _lib
    off, stride = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(eng.lib.lg_workspace_deadout(plan, B, 1, ctypes.byref(off), ctypes.byref(stride)), 'lg_workspace_deadout')
    ws = eng.workspace(plan, B, 1).view(torch.uint8).reshape(-1)
    nbytes = B * C * pan * pan * 4
    return [ws[off.value + i * stride.value: off.value + i * stride.value + nbytes].clone() for i in range(K - 1)], stride.value


def _steps(C, K, pan, B, stagewise, loss_type='l1', n_steps=2):
    from gpu_helpers import make_module
    from lgteun_amd import FusedAdam
    torch.manual_seed(4321)
    net = make_module(C, K)
    net.train()
    opt = FusedAdam(net.parameters(), lr=1e-3)
    eng = net.engine()
    eng.dead_stagewise = stagewise
    ms, pan_, gt = (T(a).cuda() for a in dw.make_inputs(B, C, pan // 4, pan // 4, seed=5, kind='dn'))
    losses = [eng.train_step(ms, pan_, gt, opt, loss_type=loss_type).item() for _ in range(n_steps)]
    torch.cuda.synchronize()
    dead, stride = _deadout(eng, eng.plan(pan, pan), B, K, C, pan)
    live = set(eng.live_idx)
    dead_grads = [eng.gflat[eng.offsets[i]:eng.offsets[i] + p.numel()] for i, p in enumerate(eng.params) if i not in live]
    return dict(losses=losses, g=eng.gflat.clone(), w=eng.flat.clone(), dead=dead, stride=stride, dead_grads=dead_grads)


@pytest.mark.parametrize('C,K,pan,B', [(4, 3, 32, 3), (4, 4, 32, 2)])
def test_train_step_batched_against_stagewise(C, K, pan, B):
    """Engine.train_step (dropout on), two steps, default against dead_stagewise: every live gradient, the weights after Adam and every
    dead stage's discarded output bitwise; dead-stage gradient slots zero.  The loss: lg_l1_loss adds one float per workgroup with atomics,
    in arrival order, so the l1 scalar of the SAME build repeats only to fp32 rounding (bench.py says so) -- it is compared to 2 ulp here,
    and bitwise under loss_type='l2', whose scalar takes ONE float add per launch (csrc/k_recloss.hip: k_l2)."""
    a, b = _steps(C, K, pan, B, False), _steps(C, K, pan, B, True)
    assert a['stride'] > 0 and b['stride'] > 0                      # this plan keeps every dead stage's output
    assert torch.equal(a['g'], b['g']) and float(a['g'].abs().max()) > 0
    assert torch.equal(a['w'], b['w'])
    for i in range(K - 1):
        assert torch.equal(a['dead'][i], b['dead'][i]), i
        assert bool(torch.isfinite(a['dead'][i].view(torch.float32)).all())
    assert not torch.equal(a['dead'][0], a['dead'][1])
    for g in a['dead_grads']:
        assert float(g.abs().max()) == 0.0
    assert len(a['dead_grads']) == 119 * (K - 1)
    for x, y in zip(a['losses'], b['losses']):
        assert abs(x - y) <= 2 * np.spacing(np.float32(abs(x))), (x, y)
    a2, b2 = _steps(C, K, pan, B, False, 'l2', 1), _steps(C, K, pan, B, True, 'l2', 1)
    assert a2['losses'] == b2['losses'] and torch.equal(a2['w'], b2['w'])


def test_k2_is_untouched():
    """K = 2 has one dead stage: no plan batches, one deadout slot, and the bit changes nothing (tests/test_route_cpu.py pins lg_workspace_bytes at K = 2)"""
    from gpu_helpers import Ops, make_module
    a, b = _steps(4, 2, 32, 2, False, n_steps=1), _steps(4, 2, 32, 2, True, n_steps=1)
    assert a['stride'] == 0 and b['stride'] == 0
    assert torch.equal(a['g'], b['g']) and torch.equal(a['w'], b['w']) and torch.equal(a['dead'][0], b['dead'][0])
    net = make_module(4, 2)
    ops = Ops(net, 32, 32)
    from lgteun_amd import _lib
    from lgteun_amd.engine import _ptr, _stream_ptr
    z = _z(2, 1, 4, 32, 3)
    out = torch.empty_like(z)
    ws = ops.ws(1)
    rc = ops.lib.lg_op_lgt_stages(ops.plan, _ptr(ops.eng.flat), 0, 2, _ptr(z), _ptr(out), _ptr(ws), ws.numel(), 1, 0, 0, 0, _stream_ptr())
    assert rc == -2 and b'one stage per pass' in ops.lib.lg_last_error()


def test_c8_plan_falls_back():
    """a C = 8 plan (k_ffn1/2_x64, k_attn_m<32,.>) has no batched form: identical results with and without the bit, one deadout slot"""
    a, b = _steps(8, 3, 32, 1, False, n_steps=1), _steps(8, 3, 32, 1, True, n_steps=1)
    assert a['stride'] == 0 and b['stride'] == 0
    assert torch.equal(a['g'], b['g']) and torch.equal(a['w'], b['w']) and float(a['g'].abs().max()) > 0


def test_prof_counts_stage_sized_launches():
    """lg_prof: a launch over the samples of S dead stages counts S, so the FFN slot's count per step is the same with and without the bit"""
    from gpu_helpers import make_module
    from lgteun_amd import FusedAdam, _lib
    L = _lib.lib()
    ms, pan, gt = (T(a).cuda() for a in dw.make_inputs(2, 4, 8, 8, seed=5, kind='dn'))
    counts = []
    for stagewise in (False, True):
        net = make_module(4, 4)
        net.train()
        opt = FusedAdam(net.parameters(), lr=1e-3)
        eng = net.engine()
        eng.dead_stagewise = stagewise
        eng.train_step(ms, pan, gt, opt)
        _lib.check(L.lg_prof_enable(_lib.KERNEL_IDS['ffn'], 256), 'lg_prof_enable')
        eng.train_step(ms, pan, gt, opt)
        torch.cuda.synchronize()
        tot, n = ctypes.c_double(), ctypes.c_int64()
        _lib.check(L.lg_prof_read(ctypes.byref(tot), ctypes.byref(n)), 'lg_prof_read')
        L.lg_prof_disable()
        counts.append(int(n.value))
    assert counts[0] == counts[1] == 4 * 5, counts
