"""Shared by tests/test_flat_loss_design_cpu.py and tests/test_gpu_flat_loss.py: inputs on which the l1 and the l2 loss are numbers with no
rounding in them, in ANY order of summation.

gt is a random multiple of 1/4 in [0, 8), out = gt + k/4 with integer |k| <= 3, k = 0 at every 97th element and k != 0 in the
last eight.  Every difference
out - gt = k/4 is exact in fp32; |d| is a multiple of 1/4 and d^2 a multiple of 1/16, so every partial sum of either is an integer
number of that unit.  While that integer stays below 2^24 an fp32 (or fp64) accumulator holds it exactly, whatever the order: per-thread
sums, the wave butterfly, the four-wave meet and the float atomics of the workgroups add without rounding.  n_global = 2^22 makes the 1 / n factor
a power of two, which only moves the exponent.  `exact_loss` is the precondition and the fp64 value in one."""
import numpy as np

SIZES = [1, 3, 4, 1003, 100003, 1179651, 2097155]      # the loops of rl_stream_diff (k_recloss.hip): see test_gpu_flat_loss.py
N_GLOBAL = 2 ** 22
SCALE = 0.5
K_MAX = 3
CALLS = 2                                                # the scalar is accumulated: the GPU test calls twice


def designed(n):
    """(out, gt, k) as float32, float32, int64"""
    rng = np.random.default_rng(1000 + n)
    gt = (rng.integers(0, 32, n) / 4.0).astype(np.float32)
    k = rng.integers(-K_MAX, K_MAX + 1, n)
    k[-8:][k[-8:] == 0] = 1          # the scalar tail and the last float4s count in the loss: a kernel that drops one of them moves it
    k[96::97] = 0
    out = (gt.astype(np.float64) + k / 4.0).astype(np.float32)
    return out, gt, k


def exact_loss(kind, out, gt, calls=CALLS):
    """the fp64 loss of ONE call (this rank's share, sum / N_GLOBAL) after asserting that the sum over `calls` calls is an integer number of
    its unit below 2^24"""
    d = out.astype(np.float64) - gt.astype(np.float64)
    unit, terms = (0.25, np.abs(d)) if kind == 'l1' else (0.0625, d * d)
    units = terms / unit
    assert np.array_equal(units, np.rint(units)) and units.max(initial=0.0) <= (K_MAX if kind == 'l1' else K_MAX * K_MAX)
    assert np.array_equal((out - gt).astype(np.float64), d)                  # the fp32 difference is the difference
    total = float(units.sum())                                              # integers below 2^53: exact
    assert calls * total < 2.0 ** 24, (kind, out.size, calls * total)
    return total * unit / N_GLOBAL
