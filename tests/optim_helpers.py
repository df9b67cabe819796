"""Shared by tests/test_gpu_fused_optim.py and tests/test_gpu_optim_bits.py: what a fused optimizer's step_flat needs of an Engine over
synthetic flat buffers, and bit-level comparisons of float tensors that say where and by how much two of them part."""
import types

import torch


def flat_engine(flat, gflat, ranges, grad_scale=None, calls=None):
    """the library, the buffers, the ranges and Engine's own launch methods, `max_range` as Engine.max_range computes it.
    grad_scale: handed to every lg_optim_step launch (step_flat itself never passes one); calls: a list that receives
    (step, algo, flags, h0, h1, weight_decay) of every lg_optim_step launch"""
    from lgteun_amd import _lib
    from lgteun_amd.engine import Engine
    assert all(0 <= a < b <= flat.numel() for a, b in ranges) and gflat.numel() == flat.numel()
    eng = types.SimpleNamespace(lib=_lib.lib(), flat=flat, gflat=gflat, total=flat.numel(), live_ranges=list(ranges),
                                ranges_dev=torch.tensor([v for r in ranges for v in r], dtype=torch.int64, device=flat.device),
                                max_range=max(b - a for a, b in ranges))
    eng.adam = types.MethodType(Engine.adam, eng)
    eng.optim_step_ex = types.MethodType(Engine.optim_step_ex, eng)

    def optim_step(states, step, algo, flags, lr, h0, h1, eps, weight_decay):
        if calls is not None:
            calls.append((step, int(algo), int(flags), float(h0), float(h1), float(weight_decay)))
        kw = {} if grad_scale is None else dict(grad_scale=grad_scale)
        Engine.optim_step(eng, states, step, algo, flags, lr, h0, h1, eps, weight_decay, **kw)

    eng.optim_step = optim_step
    return eng


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def ordered(t):
    """fp32 -> int64 that grows with the value: the distance of two of them is their distance in ulps (+0 and -0 coincide)"""
    b = bits(t).to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


def parting(got, want, where=None):
    """None when `got` has the bits of `want` (inside the mask `where`), else 'N elements differ, largest distance U ulps, first index I
    (got .. want ..)' -- the index into the whole tensor"""
    ne = bits(got) != bits(want)
    if where is not None:
        ne &= where
    n = int(ne.sum())
    if n == 0:
        return None
    d = (ordered(got) - ordered(want)).abs()[ne]
    first = int(ne.nonzero()[0])
    return (f'{n} elements differ, largest distance {int(d.max())} ulps, first index {first} '
            f'(got {float(got[first])!r} want {float(want[first])!r})')
