"""Uneven runs for the two workgroups of a CU in the one-pass dead-stage forward (csrc/kernels.h: stage_run_halves, stage_run_chunk).

With the 512 resident workgroups and no grid cap, k_ffn_xr<.,.,true> walks runs of strip PAIRS (the first workgroup of a CU the tall strips,
the second the short ones) and k_attn_m<8|16,.,true> cuts a CU's chunk of window quads unevenly between its two workgroups.  The work and
the arithmetic per pixel are unchanged, so every comparison is BITWISE: against the stage-by-stage lg_op_lgt calls and against the same pass
under grid_cap = 5, which keeps the even runs.

The shape is the smallest at which all three kernels take the uneven form and a workgroup's run crosses a stage boundary: C = 4, PAN 64 x 64,
64 samples per stage, 3 stages.  k_ffn_xr: 32-row strips, 3 x 512 of them = 768 pairs on 256 workgroup pairs, 256 pairs per stage (pair 85
crosses).  k_attn_m<8>: 3072 quads, 12 per CU, 1024 per stage (no multiple of 12).  k_attn_m<16>: 768 quads, 3 per CU, 256 per stage (this
instance keeps its even runs in the default build, where they are the faster ones; the uneven form of the same template runs at <8>)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

C, PAN, B = 4, 64, 64


@functools.lru_cache(maxsize=None)
def _ops(K):
    from gpu_helpers import Ops, make_module
    net = make_module(C, K)          # det_params weights: every tensor of every stage has its own values
    return net, Ops(net, PAN, PAN)


@functools.lru_cache(maxsize=None)
def _z(n):
    g = torch.Generator().manual_seed(21)
    return torch.rand(n, B, C, PAN, PAN, generator=g).cuda()


def _stages(ops, n, z, flags=0, seed=0, grid_cap=0):
    """lg_op_lgt_stages into a guarded buffer: z [n,B,C,H,W] -> out [n,B,C,H,W]"""
    from gpu_helpers import assert_guards_intact, guarded_empty
    from lgteun_amd import _lib
    from lgteun_amd.engine import _ptr, _stream_ptr
    buf, out = guarded_empty(tuple(z.shape), z.device)
    ws = ops.ws(B)
    _lib.check(ops.lib.lg_op_lgt_stages(ops.plan, _ptr(ops.eng.flat), 0, n, _ptr(z), _ptr(out), _ptr(ws), ws.numel(), B, flags, seed,
                                        grid_cap, _stream_ptr()), 'lg_op_lgt_stages')
    torch.cuda.synchronize()
    assert_guards_intact(buf, 'lg_op_lgt_stages')
    return out


def _decision(kind, h, n, grid_cap=0):
    from lgteun_amd import _lib
    out = (ctypes.c_int32 * 8)()
    assert _lib.lib().lg_debug_stage_decision(kind, h, h, B, n, grid_cap, out) == 0
    return list(out)


def _crossing(kind, units, per_stage, grid, split):
    """workgroups whose run holds units of two stages"""
    from lgteun_amd import _lib
    out = (ctypes.c_int32 * (5 * (grid + 16)))()
    rows = _lib.lib().lg_debug_stage_runs(kind, units, per_stage, grid, split, out, grid + 16)
    assert grid <= rows <= grid + 16
    wgs = [out[5 * i] for i in range(rows)]
    return sorted({w for w in wgs if wgs.count(w) > 1})


def _check_geometry(n):
    """the counts of the module docstring, and the uneven decision of all three kernels"""
    uneven, dS, units, per_stage, grid, SH, tiles_x, strips_y = _decision(0, PAN, n)
    assert (uneven, units, per_stage, grid, SH, tiles_x, strips_y) == (1, 256 * n, 256, 512, 32, 4, 2) and 0 < dS < SH and dS % 8 == 0
    xr_cross = _crossing(0, units, per_stage, grid, dS)
    uneven8, u8, quads8, per8, grid8 = _decision(8, PAN, n)[:5]
    assert (uneven8, quads8, per8, grid8) == (1, 1024 * n, 1024, 512) and u8 != 4
    # k_attn_m<16>: 3 quads per CU.  The default build leaves this instance on even runs (its uneven launch measured slower: csrc/k_attn_m.hip,
    # am::MULTI_UNEVEN16); a build with that constant at 5 takes 2 : 1 here, and everything below holds for it unchanged
    uneven16, u16, quads16, per16, grid16 = _decision(16, PAN // 2, n)[:5]
    assert (quads16, per16, grid16) == (256 * n, 256, 512) and uneven16 == (u16 != 4)
    a8_cross, a16_cross = _crossing(1, quads8, per8, grid8, u8), _crossing(1, quads16, per16, grid16, u16)
    if n == 3:
        assert xr_cross == [85, 170, 85 + 256, 170 + 256] and a8_cross and a16_cross      # 3 pairs per workgroup pair: 255 | 256, 257 and 510, 511 | 512
    else:
        assert not xr_cross                                                              # 2 pairs per workgroup pair: no run crosses
    for kind, h in ((0, PAN), (8, PAN), (16, PAN // 2)):                                   # the cap keeps the even runs
        assert _decision(kind, h, n, 5)[0] == 0 and _decision(kind, h, n, 5)[4] == 5


@pytest.mark.parametrize('drop', [False, True])
@pytest.mark.parametrize('n', [3, 2])
def test_uneven_pass_is_bitwise_the_stage_by_stage_lgts(n, drop):
    """n stages in one pass (uneven runs) against n lg_op_lgt calls and against the capped pass (even runs), dropout off and on: bitwise"""
    from lgteun_amd import _lib
    _check_geometry(n)
    net, ops = _ops(n + 1)
    z = _z(n)
    flags, seed = (_lib.LG_FLAG_DROPOUT, 0x2468ACE) if drop else (0, 0)
    got = _stages(ops, n, z, flags, seed)
    assert bool(torch.isfinite(got).all())
    for s in range(n):
        want = ops.lgt(s, z[s].contiguous(), flags, seed)
        assert torch.equal(got[s], want), (s, float((got[s] - want).abs().max()))
    assert not torch.equal(got[0], got[1])
    assert torch.equal(got, _stages(ops, n, z, flags, seed, grid_cap=5))      # the partition does not matter
    if drop:
        assert not torch.equal(got, _stages(ops, n, z, 0, 0))                 # and dropout did something
