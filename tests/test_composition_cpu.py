"""The oracle's whole-network forward is the composition of its own resample, data_step and lgt that tests/test_gpu_composition.py composes from the
library's per-op entries -- written out by hand here and compared with torch.equal in fp64.  oracle.forward(mode='chained') is the checker of
tests/test_gpu_chained.py: this makes it provably the chain Z[i+1] = data_step(i, X[i]), X[i+1] = lgt(i, Z[i+1]), and the faithful / live forward
provably Z[i+1] = data_step(i, Z[i]), out = lgt(K-1, Z[K])."""
import pytest
import torch

from helpers import det_params
from oracle import detweights as dw
from oracle import lgteun_oracle as orc

T = torch.from_numpy


def _hand(P, ms, pan, K, chained):
    """the hand sequence of tests/test_gpu_composition.py on the oracle's functions: (output, [LGT_i(Z[i+1]) for every stage i])"""
    x = orc.resample(ms, 4)
    lgts = []
    for i in range(K):
        z = orc.data_step(P, x, ms, pan, P[f'eta.{i}'])
        lgts.append(orc.lgt(P, f'prior_module.{i}.', z))
        x = lgts[-1] if chained else z
    return lgts[-1], lgts


@pytest.mark.parametrize('C,K', [(4, 3), (8, 2)])
def test_oracle_forward_is_the_hand_composition(C, K):
    ms, pan, _ = (T(a).double() for a in dw.make_inputs(2, C, 4, 4, seed=31, kind='smooth'))     # PAN 16 x 16
    P = det_params(C, K, dtype=torch.float64)
    with torch.no_grad():
        chained, lg_c = _hand(P, ms, pan, K, True)
        plain, lg_p = _hand(P, ms, pan, K, False)
        assert torch.equal(orc.forward(P, ms, pan, K, mode='chained'), chained)
        assert torch.equal(orc.forward(P, ms, pan, K, mode='faithful'), plain)
        assert torch.equal(orc.forward(P, ms, pan, K, mode='live'), plain)
    # the two compositions are different networks from the second stage on, and the same one in the first
    assert torch.equal(lg_c[0], lg_p[0]) and not torch.equal(chained, plain)
    assert bool(torch.isfinite(chained).all()) and bool(torch.isfinite(plain).all())
