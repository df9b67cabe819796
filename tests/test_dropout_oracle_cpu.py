"""The oracle's train mode (no GPU): `drop_masks` threaded through oracle.lgb / lgt / forward.  The GPU tests
(tests/test_gpu_dropout_oracle.py) feed it the library's exported masks; here the plumbing itself is pinned -- that None and
all-ones change nothing, that block b of stage s asks for exactly (s, b) with its level's (h, w, e) and that this mask lands on
that block's mixer half, which stages' masks reach the output in each mode, and the element order of the mask tensor."""
import numpy as np
import pytest
import torch

from helpers import _dropout_mask_numpy, det_params, numpy_drop_masks
from oracle import detweights as dw
from oracle import lgteun_oracle as orc

T = torch.from_numpy
C, K, H, W, B = 4, 2, 16, 32, 2                # a rectangle: a transposed (h, w) cannot pass
BLOCKS = ['encoder_layers.0.0.blocks.0.', 'encoder_layers.0.0.blocks.1.', 'bottleneck.blocks.0.', 'decoder_layers.0.2.blocks.0.',
          'decoder_layers.0.2.blocks.1.']


@pytest.fixture(scope='module')
def setup():
    P = det_params(C, K, dtype=torch.float64)
    rng = np.random.default_rng(7)
    z = T(rng.uniform(0, 1, (B, C, H, W)))
    ms, pan, _ = (T(a).double() for a in dw.make_inputs(B, C, H // 4, W // 4, seed=31, kind='smooth'))
    return P, z, ms, pan


def _ones(stage, blk, B_, h, w, e):
    return torch.ones(B_, e, h, w, dtype=torch.float64)


def test_all_ones_masks_are_bitwise_the_eval_result(setup):
    P, z, ms, pan = setup
    with torch.no_grad():
        pre = 'prior_module.1.'
        want = orc.lgt(P, pre, z)
        assert torch.equal(orc.lgt(P, pre, z, drop_masks=_ones, stage=1), want)
        assert torch.equal(orc.lgt(P, pre, z, drop_masks=lambda blk, *a: _ones(1, blk, *a)), want)    # a callable bound to its stage
        assert torch.equal(orc.lgt(P, pre, z, drop_masks=None, stage=1), want)
        for mode in ('faithful', 'live', 'chained'):
            assert torch.equal(orc.forward(P, ms, pan, K, mode=mode, drop_masks=_ones), orc.forward(P, ms, pan, K, mode=mode)), mode


@pytest.mark.parametrize('blk', range(5))
def test_a_zero_mask_silences_exactly_that_blocks_mixer_half(setup, blk, monkeypatch):
    """block numbering 0, 1 encoder; 2 bottleneck; 3, 4 decoder, each asked for once with its level's (B, h, w, e) and its LGT's stage;
    with block blk's mask zero its mixer half-block is x + 0 -- the same result as a mixer that returns zeros for that block's
    parameters alone"""
    P, z, _, _ = setup
    stage, pre = 1, 'prior_module.1.'
    asked = []

    def masks(st, b, B_, h, w, e):
        asked.append((st, b, B_, h, w, e))
        return torch.zeros(B_, e, h, w, dtype=torch.float64) if b == blk else _ones(st, b, B_, h, w, e)
    with torch.no_grad():
        got = orc.lgt(P, pre, z, drop_masks=masks, stage=stage)
        E = 4 * C
        assert asked == [(stage, 0, B, H, W, E), (stage, 1, B, H, W, E), (stage, 2, B, H // 2, W // 2, 2 * E), (stage, 3, B, H, W, E),
                         (stage, 4, B, H, W, E)]
        real = orc.lg_mixer
        silenced = pre + BLOCKS[blk] + '0.fn.fn.'
        monkeypatch.setattr(orc, 'lg_mixer', lambda P_, p_, x, drop_mask=None: torch.zeros_like(x) if p_ == silenced else real(P_, p_, x, drop_mask))
        want = orc.lgt(P, pre, z)
        monkeypatch.setattr(orc, 'lg_mixer', real)
        assert torch.equal(got, want)
        assert not torch.equal(got, orc.lgt(P, pre, z))


def test_dead_stage_masks_never_reach_the_output_but_chained_ones_do(setup):
    P, _, ms, pan = setup
    m0 = numpy_drop_masks(1234)
    m1 = numpy_drop_masks(99)

    def other_stage0(stage, *a):
        return (m1 if stage == 0 else m0)(stage, *a)
    with torch.no_grad():
        faithful = orc.forward(P, ms, pan, K, mode='faithful', drop_masks=m0)
        assert torch.equal(faithful, orc.forward(P, ms, pan, K, mode='live', drop_masks=m0))
        assert torch.equal(faithful, orc.forward(P, ms, pan, K, mode='faithful', drop_masks=other_stage0))
        assert not torch.equal(faithful, orc.forward(P, ms, pan, K, mode='faithful'))
        chained = orc.forward(P, ms, pan, K, mode='chained', drop_masks=m0)
        moved = orc.forward(P, ms, pan, K, mode='chained', drop_masks=other_stage0)
        assert float((chained - moved).norm() / chained.norm()) > 1e-2


def test_mask_tensor_follows_the_headers_element_index():
    """include/lgteun_hip.h lg_dropout_mask: element i = pixel * e + channel, pixel = (b * h + y) * w + x over the whole batch"""
    seed, stage, blk, B_, h, w, e = 2 ** 63 + 77, 1, 2, 3, 4, 6, 8
    got = numpy_drop_masks(seed, torch.float32)(stage, blk, B_, h, w, e)
    assert got.shape == (B_, e, h, w) and got.dtype == torch.float32
    flat = _dropout_mask_numpy(seed, stage, blk, 0, B_ * h * w * e)
    assert 0 < (flat == 0).sum() < flat.size
    for b in range(B_):
        for y in range(h):
            for x in range(w):
                for c in range(e):
                    assert float(got[b, c, y, x]) == float(flat[((b * h + y) * w + x) * e + c]), (b, y, x, c)
    other = numpy_drop_masks(seed, torch.float32)(stage, blk + 1, B_, h, w, e)
    assert not torch.equal(got, other)
