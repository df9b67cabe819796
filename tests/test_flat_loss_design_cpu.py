"""The designed inputs of tests/test_gpu_flat_loss.py (tests/flat_loss_helpers.py) do what they claim, without a device: at every size the
sums of |d| and of d^2 over BOTH accumulating calls are integers of their unit (1/4, 1/16) below 2^24, and an fp32 accumulator that adds
the terms of both calls one by one, in three random orders, holds the fp64 sum after EVERY addition -- so any tree of fp32 additions
(per-thread sums, butterfly, wave meet, atomics in arrival order) is exact too, its partial sums being sums of subsets of the same
non-negative integers.  A dropped, doubled or stale element then moves the loss by at least (1/4) / 2^22 for l1 and (1/16) / 2^22 for l2,
except where d = 0 (every 97th element and a seventh of the rest): which is why the GPU test also checks dout element by element."""
import numpy as np
import pytest

from flat_loss_helpers import CALLS, K_MAX, N_GLOBAL, SIZES, designed, exact_loss


@pytest.mark.parametrize('n', SIZES)
def test_designed_inputs(n):
    out, gt, k = designed(n)
    assert out.dtype == gt.dtype == np.float32 and out.size == gt.size == n
    assert np.array_equal(gt * 4, np.rint(gt * 4)) and gt.min() >= 0 and gt.max() < 8
    assert np.abs(k).max() <= K_MAX and not k[96::97].any() and k[-8:].all()
    assert np.array_equal((out - gt).astype(np.float64) * 4, k.astype(np.float64))
    if n >= 1003:
        assert set(np.unique(k)) == set(range(-K_MAX, K_MAX + 1))          # both signs and zero: every branch of the l1 gradient


@pytest.mark.parametrize('kind', ['l1', 'l2'])
@pytest.mark.parametrize('n', SIZES)
def test_fp32_sums_in_any_order_are_the_fp64_sum(n, kind):
    out, gt, _ = designed(n)
    want = exact_loss(kind, out, gt)                     # asserts the bound over both calls
    d = out - gt                                         # fp32
    terms = np.abs(d) if kind == 'l1' else d * d
    both = np.concatenate([terms] * CALLS)
    rng = np.random.default_rng(n)
    for _ in range(3):
        order = rng.permutation(both.size)
        run32 = np.cumsum(both[order], dtype=np.float32)          # serial: one fp32 addition per element
        run64 = np.cumsum(both[order].astype(np.float64))
        assert np.array_equal(run32.astype(np.float64), run64)
        assert run64[-1] / N_GLOBAL == CALLS * want and np.float32(run32[-1] / np.float32(N_GLOBAL)) == np.float32(CALLS * want)


def test_worst_case_is_inside_the_bound_for_l1_and_the_draw_for_l2():
    """l1: even |k| = 3 everywhere stays below 2^24 quarters over two calls at the largest size.  l2: the worst case (9 sixteenths
    everywhere) would not, the draw's mean k^2 of 4 does, with room: which is why exact_loss asserts the bound on the data itself."""
    n = max(SIZES)
    assert CALLS * n * K_MAX < 2 ** 24 < CALLS * n * K_MAX * K_MAX
    k = designed(n)[2]
    assert CALLS * int((k * k).sum()) < 2 ** 24 - 10 ** 5
