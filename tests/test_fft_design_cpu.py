"""The inputs of test_gpu_fft_mixer.py are fit to judge a kernel by: for every one of its cases, on the CPU, from the fp64 oracle on
LayerNorm(feat) with the block's own deterministic weights.

The per-op shape files take the FFT mixer out of their element-wise figures because random features put bins next to angle()'s branch cut
(|Im F| down to 5e-7 of the plane's norm: one fp32 rounding away from a flip of 2 pi) and next to zero amplitude (the backward divides by it).
Both are properties of the input.  helpers.fft_designed_features draws the spectrum itself, so every case here has
  * cut margin   min |Im F| / ||plane||_2 over the non-structural bins with Re F < 0            >= 0.05
  * amplitude floor   min |F| / ||plane||_2 over all bins                                       >= 0.05
  * masked share   pixels where the fp64 output is below 1e-4 of its plane's RMS (dy = 0 there)  <= 1e-3
  * a clean fp32 oracle: the four gradients within 2e-6 of their tensor's largest entry, dx within 2e-6 of its plane's RMS element by element,
    the forward within 2e-6 of its plane's LARGEST entry element by element.  (Not of its RMS, the scale of the GPU file's forward figure: the
    edited spectrum's phases are nearly coherent -- conv_pha's weights are small -- so the output has a peak of 6 .. 450 x RMS around pixel (0, 0),
    and any fp32 evaluation is 2^-24 x that peak off there: 9e-7 .. 7e-5 of the RMS by the size of the plane, whatever the seed.)
and the fp32 oracle is a yardstick for the kernels.  These are conditions, not tolerances: a case that misses one gets another seed
(helpers.FFT_RESEED: one case, whose first draw had a DC bin nearly cancelled by the LayerNorm bias, amplitude floor 0.034), never another bound.
Measured over the 30 cases: cut margin 0.100 .. 0.137, amplitude floor 0.082 .. 0.361, masked share 0 .. 6.5e-4, 16 .. 560 negative structurally real
bins per case, fp32 oracle forward 1.5e-7 .. 1.0e-6, dx 6.4e-7 .. 1.5e-6, gradients <= 5.2e-7.  The file: 36 tests in 6 s."""
import numpy as np
import pytest
import torch

from helpers import FFT_CASES, FFT_FULL_CASES, fft_assert_preconditions, fft_designed_features, fft_kink_mask
from helpers import fft_mixer_refs, fft_plane
from oracle import lgteun_oracle as orc


@pytest.fixture(autouse=True)
def canonical_real_bins(monkeypatch):
    monkeypatch.setattr(orc, 'CANONICAL_REAL_BINS', True)


def test_full_cases_are_cases_of_the_main_list():
    """the LG_FFT=full cases reuse inputs whose preconditions the parametrised test below proves"""
    assert all(c in [k[1:] for k in FFT_CASES] for c in FFT_FULL_CASES)


@pytest.mark.parametrize('C,blk,h,w', [(4, 0, 16, 16), (4, 2, 8, 24), (8, 2, 40, 24), (8, 0, 32, 64)])
def test_designed_features_are_what_they_claim(C, blk, h, w):
    """every pixel has mean 0 and variance 1 over its channels (LayerNorm is one uniform scale), the global half's planes have std 0.5, phases
    stay 0.3 away from 0 and pi outside the four structural bins, and some structural bins are negative (the exact-pi branch)"""
    x = fft_designed_features(C, blk, 3, h, w).double()
    e = 8 * C if blk == 2 else 4 * C
    assert tuple(x.shape) == (3, h, w, e) and x.dtype == torch.float64
    assert float(x.mean(-1).abs().max()) < 1e-6 and float((x.pow(2).mean(-1) - 1).abs().max()) < 1e-6
    g = x[..., e // 2:].permute(0, 3, 1, 2)
    assert float((g.std(dim=(-2, -1), unbiased=False) - 0.5).abs().max()) < 1e-6
    F = torch.fft.rfft2(g)
    ang = torch.angle(F).abs()
    struct = torch.zeros(h, w // 2 + 1, dtype=torch.bool)
    for k0 in (0, h // 2):
        for kx in (0, w // 2):
            struct[k0, kx] = True
    assert float(ang[..., ~struct].min()) > 0.3 - 1e-5 and float(ang[..., ~struct].max()) < np.pi - 0.3 + 1e-5
    assert float((F.imag[..., struct].abs() / F.abs()[..., struct]).max()) < 1e-5
    assert bool((F.real[..., struct] < 0).any()) and bool((F.real[..., struct] > 0).any())
    amp = F.abs() / F.abs().max()
    assert float(amp.min()) > 0.2            # amplitudes uniform in [0.5, 2]: no bin below a quarter of the largest


def test_kink_mask_uses_the_rms_of_each_plane():
    out = torch.ones(1, 2, 4, 4, dtype=torch.float64)
    out[0, 0, 0, 0] = 1000.0                  # a peak: the RMS moves to ~250, the maximum to 1000
    out[0, 0, 1, 1] = 2e-2                    # below 1e-4 x RMS (2.5e-2), above nothing of plane 1
    out[0, 1, 2, 2] = 5e-5
    m = fft_kink_mask(out)
    assert m.dtype == torch.bool and int(m.sum()) == 2 and bool(m[0, 0, 1, 1]) and bool(m[0, 1, 2, 2])


@pytest.mark.parametrize('family,C,blk,B,H,W', FFT_CASES)
def test_preconditions_of_every_gpu_case(family, C, blk, B, H, W):
    tag = f'fft design {family} C={C} blk={blk} ({B},{H},{W})'
    ref = fft_mixer_refs(C, blk, B, H, W)
    pre = ref['pre']
    print(f'{tag}: cut margin {pre["cut"]:.3f}  amplitude floor {pre["floor"]:.3f}  masked {pre["masked"]:.1e}  negative real bins '
          f'{pre["neg_real_bins"]}  fp32 oracle forward {pre["clean_fwd"]:.1e} dx {pre["clean_dx"]:.1e} gradients '
          f'{max(pre["clean_grads"].values()):.1e}')
    fft_assert_preconditions(tag, pre)
    h, w = fft_plane(blk, H, W)
    assert tuple(ref['y64'].shape) == (B, ref['feat'].shape[-1] // 2, h, w) == tuple(ref['dx64'].shape) == tuple(ref['dy'].shape)
    assert float(ref['dy'][ref['mask']].abs().sum()) == 0.0
    assert pre['neg_real_bins'] > 0, (tag, 'no structurally real bin is negative: the exact-pi branch is not pinned')
