"""The parameter-gradient reductions of a backward pass in ONE launch for the LGT and ONE for the K data steps (csrc/bwd_kernels.h:
ReduceQueue, merged form) against the launch points of rounds 2 - 6 (lg_config.variant LG_VAR_REDUCE_PER_BLOCK: one launch per LGT block
and per data step).  Only the grouping of the launches differs -- every output is summed from the same slices in the same order, and the
K data steps' contributions to a shared parameter are added in the same order by one chain of jobs -- so the gradients are BITWISE equal."""
import ctypes

import pytest
import torch

from oracle import detweights as dw

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _stats(lib, reset):
    out = (ctypes.c_longlong * 6)()
    lib.lg_debug_reduce_stats.restype = ctypes.c_int
    lib.lg_debug_reduce_stats.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    assert lib.lg_debug_reduce_stats(out, int(reset)) == 0
    return {'launches': out[0], 'self_flushes': out[1], 'uploads': out[2], 'jobs_max': out[3], 'flush_host_us': out[4] / 1e3, 'chains_max': out[5]}


def _backward(C, K, n, B, flags, variant, seed=977, split=False, kind='smooth'):
    """gradient buffer (started from a non-zero fill: the reductions ADD) of one forward + backward of a fresh module"""
    from gpu_helpers import make_module
    from lgteun_amd.engine import LG_FLAG_BWD_DATA, LG_FLAG_BWD_LGT
    ms, pan, _ = (T(a).cuda() for a in dw.make_inputs(B, C, n // 4, n // 4, seed=21, kind=kind))
    net = make_module(C, K)
    eng = net.engine()
    eng.variant = variant
    y, saved = eng.forward_raw(ms, pan, flags, seed=seed)
    r = torch.randn(y.shape, generator=torch.Generator(device='cpu').manual_seed(8)).cuda()
    g = (1e-3 * torch.randn(eng.flat.shape, generator=torch.Generator(device='cpu').manual_seed(9))).cuda()
    _stats(eng.lib, True)
    if split:
        eng.backward_raw(saved, r, g, flags | LG_FLAG_BWD_LGT, seed=seed)
        eng.backward_raw(saved, r, g, flags | LG_FLAG_BWD_DATA, seed=seed)
    else:
        eng.backward_raw(saved, r, g, flags, seed=seed)
    torch.cuda.synchronize()
    return g, eng, _stats(eng.lib, False)


def _assert_bitwise(g0, g1, eng, what):
    from gpu_helpers import assert_bitwise
    assert_bitwise(g0, g1, eng, what)


@pytest.mark.parametrize('drop', [False, True])
@pytest.mark.parametrize('n', [32, 64])
@pytest.mark.parametrize('K', [2, 4])
@pytest.mark.parametrize('C', [4, 8])
def test_merged_reduce_launches_give_bitwise_the_per_block_gradients(C, K, n, drop):
    """every parameter of net_backward, the shared D / DT / R / RT ones the K data steps add into and the per-stage eta included"""
    from lgteun_amd import _lib
    from lgteun_amd.engine import LG_FLAG_DROPOUT, LG_FLAG_FAITHFUL, LG_FLAG_SAVE
    flags = LG_FLAG_SAVE | LG_FLAG_FAITHFUL | (LG_FLAG_DROPOUT if drop else 0)
    g_old, eng, st_old = _backward(C, K, n, 2, flags, _lib.LG_VAR_REDUCE_PER_BLOCK)
    g_new, _, st_new = _backward(C, K, n, 2, flags, 0)
    # per-block form: five blocks + K data steps (+ the launches a full table of 56 forces); merged form: the LGT, the K data steps
    assert st_old['launches'] == 5 + K + st_old['self_flushes'] and st_new['launches'] == 2 and st_new['self_flushes'] == 0, (st_old, st_new)
    _assert_bitwise(g_old, g_new, eng, (C, K, n, drop))
    # every live parameter did receive its sum: what is compared is not the fill
    fill = (1e-3 * torch.randn(eng.flat.shape, generator=torch.Generator(device='cpu').manual_seed(9))).cuda()
    for i in eng.live_idx:
        o, m = eng.offsets[i], eng.params[i].numel()
        assert not torch.equal(g_new[o:o + m], fill[o:o + m]), eng.names[i]


def test_merged_reduce_in_two_calls_and_in_chained_mode():
    """LG_FLAG_BWD_LGT then LG_FLAG_BWD_DATA (the two-bucket all-reduce form) = one call, bitwise; chained mode (every stage live: a launch per
    LGT and per data step in the merged form) = the per-block form, bitwise"""
    from lgteun_amd import _lib
    from lgteun_amd.engine import LG_FLAG_CHAINED, LG_FLAG_FAITHFUL, LG_FLAG_SAVE
    flags = LG_FLAG_SAVE | LG_FLAG_FAITHFUL
    g1, eng, _ = _backward(4, 4, 32, 2, flags, 0)
    g2, _, st = _backward(4, 4, 32, 2, flags, 0, split=True)
    assert st['launches'] == 2, st
    _assert_bitwise(g1, g2, eng, 'two calls')
    g_old, eng, _ = _backward(4, 2, 32, 2, LG_FLAG_SAVE | LG_FLAG_CHAINED, _lib.LG_VAR_REDUCE_PER_BLOCK)
    g_new, _, st = _backward(4, 2, 32, 2, LG_FLAG_SAVE | LG_FLAG_CHAINED, 0)
    assert st['launches'] == 4 and st['self_flushes'] == 0, st
    _assert_bitwise(g_old, g_new, eng, 'chained')


def test_job_tables_are_uploaded_once():
    """the job list of a (plan, batch, flags, workspace, gradient buffer) repeats from step to step: the second and third backward of a
    training loop find their two tables on the device (no host-to-device copy on the stream)"""
    from gpu_helpers import make_module
    from lgteun_amd.engine import LG_FLAG_FAITHFUL, LG_FLAG_SAVE
    ms, pan, _ = (T(a).cuda() for a in dw.make_inputs(2, 4, 8, 8, seed=21, kind='smooth'))
    net = make_module(4, 4)
    eng = net.engine()
    eng.variant = 0
    flags = LG_FLAG_SAVE | LG_FLAG_FAITHFUL
    g = torch.zeros_like(eng.flat)
    grads = []
    for it in range(3):
        y, saved = eng.forward_raw(ms, pan, flags)
        g.zero_()
        _stats(eng.lib, True)
        eng.backward_raw(saved, torch.ones_like(y), g, flags)
        torch.cuda.synchronize()
        st = _stats(eng.lib, False)
        assert st['launches'] == 2 and st['uploads'] <= (2 if it == 0 else 0), (it, st)   # (it = 0: an earlier test may have left the same tables)
        grads.append(g.clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


@pytest.mark.parametrize('C,K,n,B', [(4, 4, 128, 2), (4, 4, 128, 32), (8, 4, 128, 32), (8, 8, 256, 16)], ids=['c2-B2', 'c2', 'c3', 'c5'])
def test_launch_count_and_arena_at_the_bench_shapes(C, K, n, B):
    """one backward of the bench configurations (and of c2's shape at B = 2): at most 3 reduce launches (2: the LGT, the K data steps), and
    neither the arena nor the job table overflowed into a launch of its own"""
    from lgteun_amd.engine import LG_FLAG_SAVE
    g, eng, st = _backward(C, K, n, B, LG_FLAG_SAVE, 0, kind='smooth')
    assert st['launches'] <= 3 and st['self_flushes'] == 0, st
    print('reduce launches at', (C, K, n, B), st)   # (the job counts DESIGN.md quotes)
    assert st['launches'] == 2 and 0 < st['chains_max'] <= st['jobs_max'] <= 512, st   # the larger of the two tables (LG_RQ_MAX_JOBS)
    assert bool(torch.isfinite(g).all())
