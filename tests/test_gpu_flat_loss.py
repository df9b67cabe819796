"""-m gpu: `lg_l1_loss` and `lg_l2_loss` (k_l1 / k_l2 over rl_stream_diff, lgteun_amd/csrc/k_recloss.hip), the launch that ends the forward
half of every train step, per op.

Exactly.  On the designed inputs of tests/flat_loss_helpers.py (multiples of 1/4, n_global = 2^22, scale = 0.5; the design is proved on
the CPU by tests/test_flat_loss_design_cpu.py) no addition on any path rounds, so `loss_accum` must EQUAL the fp64 loss after one call
and twice it after a second.  A dropped, doubled or stale element with d != 0 moves it by at least (1/16) / 2^22.  The sizes reach each
loop of rl_stream_diff (grid = min(256, ceil(n4 / 256)) workgroups of 256 threads, n4 = n / 4 float4 per tensor):
    1, 3      the scalar tail only (n4 = 0)
    4         exactly one float4, no tail
    1003, 100003   the single-float4 loop, with threads that get nothing; tails of 3
    1179651   n4 = 4.5 strides of 65 536: one unrolled four-in-flight trip, the single loop for half of the threads, a tail of 3
    2097155   the headline's 2^21 elements + 3: two unrolled trips and a tail
`dout`: l1 element by element exactly sign(d) fl32(scale / fl32(n_global)), 0 where out == gt; l2 within one fp32 ulp of
2 (out - gt) scale / n_global in fp32 (the check of test_l2_loss_vs_mseloss).  Eight floats behind dout keep their value.

Rejected calls (a dout that is not 16-byte aligned, n_local = 0, a null pointer) return < 0 and leave dout and loss_accum alone.

Ordinary data for l1 (random fp32 in [0, 1), n_global = 2 n): dout exact as above, the loss against fp64 within the DERIVED relative bound
r 2^-24 / (1 - r 2^-24), r the number of roundings on the longest path: 4 ceil(n4 / (grid 256)) + 1 per-thread additions, 6 butterfly
levels, 3 wave adds, 1 multiply and `grid` atomics; every term is non-negative, so the relative bound holds.  Not a measurement: the measured
share of it is printed (MI355X: relative error 0 .. 1.0e-7, at most 6.8 % of the bound).

Measured on the MI355X: every case passes on the kernels as the parent commit has them.  The tests were themselves checked once, against a
scratch build that is not kept, with `j < n - 1` in the scalar tail of rl_stream_diff: all 12 designed cases with n % 4 != 0 went red on
the exact loss (n = 4 has no tail and stayed green), e.g. l1 at n = 2097155 gave 0.21209865808 for 0.21209883690, three quarters of
2^-22 short; the 6 ordinary-data cases with a tail went red too, four of them on the derived bound."""
import numpy as np
import pytest
import torch

from flat_loss_helpers import CALLS, N_GLOBAL, SCALE, SIZES, designed, exact_loss

pytestmark = pytest.mark.gpu
T = torch.from_numpy
KINDS = ['l1', 'l2']


def _call(kind, out, gt, dout, accum, n, n_global, scale):
    from lgteun_amd import _lib
    from lgteun_amd.engine import _stream_ptr
    import ctypes
    ptr = lambda t: None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())      # noqa: E731
    fn = getattr(_lib.lib(), f'lg_{kind}_loss')
    return fn(ptr(out), ptr(gt), ptr(dout), ptr(accum), n, n_global, scale, _stream_ptr())


def _l1_dout(out, gt, scale, n_global):
    """what k_l1 must write: sign(out - gt) * fl32(scale / fl32(n_global)), in numpy float32"""
    g = np.float32(scale) / np.float32(n_global)
    d = out - gt
    return np.where(d > 0, g, np.where(d < 0, -g, np.float32(0.0))).astype(np.float32)


def _grid(n):
    return min(256, max(1, (n // 4 + 255) // 256))          # rl_flat_grid


def test_sizes_reach_the_loops_they_are_named_for():
    assert [n // 4 for n in SIZES[:3]] == [0, 0, 1] and SIZES[2] % 4 == 0
    assert all(_grid(n) * 256 > n // 4 > 0 and n % 4 == 3 for n in (1003, 100003))                  # threads that get nothing
    n4, stride = 1179651 // 4, 256 * 256
    assert _grid(1179651) == 256 and 4 * stride < n4 < 5 * stride and n4 - 4 * stride == stride // 2 and 1179651 % 4 == 3
    n4 = 2097155 // 4
    assert n4 == 8 * stride and 2097155 % 4 == 3


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_designed_loss_is_exact(n, kind):
    out, gt, _ = designed(n)
    want = exact_loss(kind, out, gt)                      # fp64; asserts that no sum over both calls can round
    d_out, d_gt = T(out).cuda(), T(gt).cuda()
    dout = torch.full((n + 8,), 7.0, device='cuda')
    accum = torch.zeros(1, device='cuda')
    seen = []
    for _ in range(CALLS):
        rc = _call(kind, d_out, d_gt, dout, accum, n, N_GLOBAL, SCALE)
        assert rc == 0
        seen.append(float(accum.item()))
    print(f'{kind} n {n}: loss_accum {seen!r} against fp64 {want!r} and twice it')
    assert seen[0] == want and seen[1] == CALLS * want, (seen, want)
    g = dout[:n].cpu().numpy()
    if kind == 'l1':
        assert g.tobytes() == _l1_dout(out, gt, SCALE, N_GLOBAL).tobytes()
    else:
        ref = (2 * (out - gt) * np.float32(SCALE)) / np.float32(N_GLOBAL)       # fp32 on the host
        assert bool((np.abs(g - ref) <= np.spacing(np.abs(ref))).all()), float(np.abs(g - ref).max())
        assert np.array_equal(g == 0, out == gt)
    assert bool((dout[n:] == 7.0).all())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', ['misaligned-dout', 'n_local-0', 'null-out', 'null-accum'])
def test_rejected_calls_touch_nothing(case, kind):
    n = 1003
    out, gt, _ = designed(n)
    d_out, d_gt = T(out).cuda(), T(gt).cuda()
    dout = torch.full((n + 8,), 7.0, device='cuda')
    accum = torch.full((1,), 3.0, device='cuda')
    args = dict(out=d_out, gt=d_gt, dout=dout, accum=accum, n=n)
    if case == 'misaligned-dout':
        args['dout'] = dout.data_ptr() + 4
    elif case == 'n_local-0':
        args['n'] = 0
    else:
        args[case[5:]] = None
    rc = _call(kind, args['out'], args['gt'], args['dout'], args['accum'], args['n'], N_GLOBAL, SCALE)
    torch.cuda.synchronize()
    assert rc < 0
    assert bool((dout == 7.0).all()) and float(accum.item()) == 3.0


@pytest.mark.parametrize('n', SIZES)
def test_l1_loss_on_ordinary_data(n):
    gen = torch.Generator().manual_seed(n)
    out, gt = torch.rand(n, generator=gen).numpy(), torch.rand(n, generator=gen).numpy()
    n_global = 2 * n
    dout = torch.full((n + 8,), 7.0, device='cuda')
    accum = torch.zeros(1, device='cuda')
    assert _call('l1', T(out).cuda(), T(gt).cuda(), dout, accum, n, n_global, SCALE) == 0
    got = float(accum.item())
    want = float(np.abs(out.astype(np.float64) - gt.astype(np.float64)).sum()) / n_global
    grid = _grid(n)
    r = 4 * -(-(n // 4) // (grid * 256)) + 1 + 6 + 3 + 1 + grid
    bound = r * 2.0 ** -24 / (1 - r * 2.0 ** -24)
    rel = abs(got - want) / want
    print(f'l1 n {n}: loss {got!r} against fp64 {want!r}: relative error {rel:.3e}, derived bound {bound:.3e} (r = {r}), ratio {rel / bound:.4f}')
    assert rel <= bound, (got, want, rel, bound)
    assert dout[:n].cpu().numpy().tobytes() == _l1_dout(out, gt, SCALE, n_global).tobytes()
    assert bool((dout[n:] == 7.0).all())
