"""-m gpu: every distinct kernel route a plan can resolve launches.  The A/B tests elsewhere flip one switch at a time, mostly at fp32 and C = 4;
here the whole word set of tests/test_route_cpu.py's sweep runs a saving forward and a backward at both widths and both precisions, so that no
kernel instance the route can name is missing from the library."""
import re

import pytest
import torch

from oracle import detweights as dw
from test_route_cpu import Plan, ffn_impl_rejected, sweep_words

pytestmark = pytest.mark.gpu

# distinct routes among the sweep's words per (C, precision, n); n = 32: the smallest plan with whole strips at level 1, 48: the smallest whose
# level-1 width is 8 mod 16 (the tile fallback of the spatial FFN backward)
N_ROUTES = {(4, 0, 32): 93, (4, 0, 48): 77, (4, 1, 32): 26, (4, 1, 48): 18, (8, 0, 32): 32, (8, 0, 48): 32, (8, 1, 32): 10, (8, 1, 48): 10}

# variant word -> the error a route ALREADY failed to launch with before this test existed ((C, precision, n, word): text).  Empty: every route launches.
KNOWN_LAUNCH_FAILURES = {}

# largest relative L2 distance of a route's result to the default route's, by precision: (output, gradient buffer), measured over all 298 routes on
# the commit before this test (figures in the test's docstring).  The bound is 2 x these.
BOUNDS_MEASURED = {0: (1.919e-4, 5.408e-3), 1: (1.883e-3, 1.497e-1)}


def representatives(C, prec, n):
    """one word per distinct lg_plan_describe text (the variant field dropped), in ascending order of the words"""
    seen, reps = set(), []
    for v in sorted(sweep_words()):
        p = Plan(C, prec, n, n, v)
        if p.error is not None:
            assert ffn_impl_rejected(v, prec), (hex(v), p.error)
            continue
        text = re.sub(r' variant=0x[0-9a-f]+', '', p.describe())
        if text not in seen:
            seen.add(text)
            reps.append(v)
    return reps


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize('C,prec,n', sorted(N_ROUTES))
def test_every_route_launches_and_agrees_with_the_default(C, prec, n):
    """one plan per distinct route (K = 1, B = 1, fixed smooth inputs, dropout off): the saving forward and the backward return without error, output
    and gradient buffer are finite and lie within 2 x the largest distance to the default route's result that the commit before this test showed.
    The routes compute the same function in different arithmetic -- 1e-6-level rounding at precision = 0, one bf16 rounding per operand at
    precision = 1 -- while a wrong or missing kernel instance is off by orders of magnitude (relative distance near 1) or returns an error.
    Measured there, worst route per case, output / gradient:
        C=4 fp32 32: 4.835e-07 / 4.752e-04    C=4 fp32 48: 2.741e-07 / 1.089e-05    C=8 fp32 32: 3.225e-07 / 5.653e-05    C=8 fp32 48: 1.919e-04 / 5.408e-03
        C=4 bf16 32: 1.883e-03 / 6.330e-02    C=4 bf16 48: 1.525e-03 / 2.373e-02    C=8 bf16 32: 1.640e-03 / 1.497e-01    C=8 bf16 48: 1.363e-03 / 3.797e-02
    (C=8 fp32 48: every route whose forward arithmetic is not the default's f16 pairs sits at the same 1.919e-04 -- it is the default route's own
    distance to the exact-fp32 kernels on this input, not a spread among the A/B routes.)
    Bounds (2 x the maxima by precision): fp32 output 3.838e-04, gradient 1.082e-02; bf16 output 3.766e-03, gradient 2.994e-01.  No route failed to
    launch there: KNOWN_LAUNCH_FAILURES is empty."""
    from gpu_helpers import make_module
    from lgteun_amd import _lib
    reps = representatives(C, prec, n)
    assert len(reps) == N_ROUTES[(C, prec, n)] and reps[0] == 0, (len(reps), reps[:4])
    net = make_module(C, 1)
    if prec:
        net.precision = 'bf16'
    eng = net.engine()
    ms, pan, gt = (torch.from_numpy(a).cuda() for a in dw.make_inputs(1, C, n // 4, n // 4, seed=5, kind='smooth'))
    dout = (gt - gt.mean()).contiguous()

    def run(v):
        eng.variant = v
        out, saved = eng.forward_raw(ms, pan, _lib.LG_FLAG_SAVE)          # K = 1, no LG_FLAG_DROPOUT: one live stage, dropout off
        g = torch.zeros(eng.total, dtype=torch.float32, device=eng.device)
        eng.backward_raw(saved, dout, g, _lib.LG_FLAG_SAVE)
        return out.clone(), g

    out0, g0 = run(0)
    assert bool(torch.isfinite(out0).all()) and bool(torch.isfinite(g0).all()) and float(g0.norm()) > 0
    bound_out, bound_g = (2 * b for b in BOUNDS_MEASURED[prec])
    worst_out = worst_g = 0.0
    failures = []
    for v in reps[1:]:
        key = (C, prec, n, v)
        try:
            out, g = run(v)
        except _lib.LgteunHipError as err:                                  # a launcher that has no instance for the route returns an error code
            if key not in KNOWN_LAUNCH_FAILURES:
                failures.append((hex(v), str(err)))
            continue
        assert key not in KNOWN_LAUNCH_FAILURES, (hex(v), 'launches now: take it out of the table')
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all()), hex(v)
        d_out, d_g = rel(out, out0), rel(g, g0)
        print(f'route C={C} precision={prec} n={n} variant={v:#x}: output {d_out:.3e}, gradient {d_g:.3e}')
        worst_out, worst_g = max(worst_out, d_out), max(worst_g, d_g)
        if d_out > bound_out or d_g > bound_g:
            failures.append((hex(v), d_out, d_g))
    print(f'routes C={C} precision={prec} n={n}: {len(reps)} routes, worst distance to the default: output {worst_out:.3e}, gradient {worst_g:.3e}')
    assert not failures, failures
