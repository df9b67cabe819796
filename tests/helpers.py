"""Shared test helpers: deterministic weights + shapes of the reference state_dict."""
import functools

import numpy as np
import torch

from oracle import detweights as dw
from oracle import lgteun_oracle as orc


def state_shapes(C, K):
    """Shapes of Pansharpening.state_dict() (reference models/unlg_former.py:22-48;
    measured key list in SURVEY.md §8b) -- rebuilt here from the architecture definition."""
    E = 4 * C
    s = {}
    for n in ('D.1', 'D.3', 'DT.1', 'DT.3'):
        s[n + '.weight'] = (C, 1, 3, 3)
        s[n + '.bias'] = (C,)
    s['R.weight'] = (1, C, 1, 1)
    s['R.bias'] = (1,)
    s['RT.weight'] = (C, 1, 1, 1)
    s['RT.bias'] = (C,)
    for i in range(K):
        s[f'eta.{i}'] = ()

    def block(pre, e):
        h = e // 2
        m = pre + '0.fn.'
        s[m + 'fn.local_mixer.pos_emb'] = (1, 2, 64, 64)
        s[m + 'fn.local_mixer.to_qkv.weight'] = (3 * h, h, 1, 1)
        s[m + 'fn.local_mixer.to_qkv.bias'] = (3 * h,)
        for n in ('conv_amp', 'conv_pha'):
            s[m + f'fn.global_mixer.{n}.0.weight'] = (h, 1, 1, 1)
            s[m + f'fn.global_mixer.{n}.0.bias'] = (h,)
        s[m + 'fn.proj.weight'] = (e, e, 1, 1)
        s[m + 'fn.proj.bias'] = (e,)
        s[m + 'norm.weight'] = (e,)
        s[m + 'norm.bias'] = (e,)
        f = pre + '1.fn.'
        s[f + 'fn.net.0.weight'] = (4 * e, e, 1, 1)
        s[f + 'fn.net.0.bias'] = (4 * e,)
        s[f + 'fn.net.2.point_conv.weight'] = (4 * e, 4 * e, 1, 1)
        s[f + 'fn.net.2.point_conv.bias'] = (4 * e,)
        s[f + 'fn.net.2.depth_conv.weight'] = (4 * e, 1, 3, 3)
        s[f + 'fn.net.2.depth_conv.bias'] = (4 * e,)
        s[f + 'fn.net.4.weight'] = (e, 4 * e, 1, 1)
        s[f + 'fn.net.4.bias'] = (e,)
        s[f + 'norm.weight'] = (e,)
        s[f + 'norm.bias'] = (e,)

    for i in range(K):
        p = f'prior_module.{i}.'
        s[p + 'patch_embed.proj.0.weight'] = (C, 1, 1, 1)
        s[p + 'patch_embed.proj.0.bias'] = (C,)
        s[p + 'patch_embed.proj.1.weight'] = (E, C, 1, 1)
        s[p + 'patch_embed.proj.1.bias'] = (E,)
        s[p + 'patch_embed.norm.weight'] = (E,)
        s[p + 'patch_embed.norm.bias'] = (E,)
        for j in range(2):
            block(p + f'encoder_layers.0.0.blocks.{j}.', E)
        s[p + 'encoder_layers.0.1.1.weight'] = (2 * E, E, 1, 1)
        s[p + 'encoder_layers.0.1.1.bias'] = (2 * E,)
        block(p + 'bottleneck.blocks.0.', 2 * E)
        s[p + 'decoder_layers.0.0.1.weight'] = (E, 2 * E, 1, 1)
        s[p + 'decoder_layers.0.0.1.bias'] = (E,)
        s[p + 'decoder_layers.0.1.weight'] = (E, 2 * E, 1, 1)
        s[p + 'decoder_layers.0.1.bias'] = (E,)
        for j in range(2):
            block(p + f'decoder_layers.0.2.blocks.{j}.', E)
        s[p + 'tail.1.weight'] = (C, E, 1, 1)
        s[p + 'tail.1.bias'] = (C,)
    return s


def det_params(C, K, salt=0, dtype=torch.float32, requires_grad=False):
    sd = dw.fill_state_dict(state_shapes(C, K), salt=salt, dtype=np.float64)
    P = {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}
    if requires_grad:
        for v in P.values():
            v.requires_grad_(True)
    return P


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _dropout_mask_numpy(seed, stage, blk, first, n):
    """numpy restatement of csrc/common.h mix_seed + dropout_scale (test infrastructure only)"""
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (stage * 8 + blk + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    idx = np.arange(first, first + n, dtype=np.uint64)
    pair = idx >> np.uint64(1)                 # round 5: one hash per PAIR of elements, 16 bits of it per element
    x = (pair + np.uint64(z & 0xffffffff)).astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d)
    x ^= np.uint32(z >> 32) ^ (pair >> np.uint64(32)).astype(np.uint32)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    h = np.where((idx & np.uint64(1)) == 1, x >> np.uint32(16), x & np.uint32(0xffff))
    return np.where(h < np.uint32(6554), np.float32(0), np.float32(1.0 / 0.9))


def mask_tensor(flat, B, h, w, e, dtype):
    """the B * h * w * e flat factors of one block, in the header's order (include/lgteun_hip.h lg_dropout_mask: element
    i = pixel * e + channel, pixel running over the whole batch in NHWC order), as the [B, e, h, w] tensor oracle.lg_mixer takes"""
    return flat.reshape(B, h, w, e).permute(0, 3, 1, 2).contiguous().to(dtype)


def numpy_drop_masks(seed, dtype=torch.float64):
    """the `drop_masks` callable of oracle.lgb / lgt / forward, drawn from the numpy restatement"""
    def masks(stage, blk, B, h, w, e):
        return mask_tensor(torch.from_numpy(_dropout_mask_numpy(seed, stage, blk, 0, B * h * w * e)), B, h, w, e, dtype)
    return masks


# ---- inputs and oracle restatements shared by the per-op shape files (test_gpu_forward_shapes.py, test_gpu_backward_shapes.py)
BLOCKS = {0: 'encoder_layers.0.0.blocks.0.', 1: 'encoder_layers.0.0.blocks.1.', 2: 'bottleneck.blocks.0.',
          3: 'decoder_layers.0.2.blocks.0.', 4: 'decoder_layers.0.2.blocks.1.'}


def block_prefix(blk):
    return 'prior_module.0.' + BLOCKS[blk]


@functools.lru_cache(maxsize=None)
def block_features(C, blk, B, H, W):
    """standard-normal NHWC features of block `blk` of a B x H x W PAN batch; the last sample's global half has a negative mean"""
    h, w, e = (H // 2, W // 2, 8 * C) if blk == 2 else (H, W, 4 * C)
    rng = np.random.default_rng(1000 + H + W + 7 * blk + C)
    x = torch.from_numpy(rng.standard_normal((B, h, w, e)).astype(np.float32))
    x[-1, ..., e // 2:] -= 0.7
    return x


def ffn_half_block(P, blk, x):
    p = block_prefix(blk)
    return x + orc.feed_forward(P, p + '1.fn.fn.', orc.layer_norm(x, P[p + '1.fn.norm.weight'], P[p + '1.fn.norm.bias']))


def mixer_half_block(P, blk, x):
    p = block_prefix(blk)
    return x + orc.lg_mixer(P, p + '0.fn.fn.', orc.layer_norm(x, P[p + '0.fn.norm.weight'], P[p + '0.fn.norm.bias']))


def mixer_restated(P, blk, x, x1, o2):
    """x + proj(cat(local_mixer(LN(x)[..., :e/2]), o2)): o2 planar [B, e/2, h, w], the build's own global-mixer output"""
    p = block_prefix(blk) + '0.fn.fn.'
    cat = torch.cat((x1, o2.permute(0, 2, 3, 1)), dim=-1).permute(0, 3, 1, 2)
    return x + orc.point_conv(cat, P[p + 'proj.weight'], P[p + 'proj.bias']).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def lgt_input(C, B, H, W):
    return torch.from_numpy(np.random.default_rng(H + W).uniform(0, 1, (B, C, H, W)).astype(np.float32))


# ---- the FFT (global) mixer on inputs designed in the frequency domain (test_fft_design_cpu.py, test_gpu_fft_mixer.py)
def fft_designed_features(C, blk, B, h, w, seed=0):
    """fp32 NHWC [B, h, w, e] features of block `blk` (e = 8C at block 2, else 4C; h x w the block's plane) whose LayerNorm-ed global half has,
    plane by plane, a spectrum away from everything that makes the reference's own fp32 arithmetic fragile:
      * global half: a half spectrum of amplitudes uniform in [0.5, 2] and phases +-uniform[0.3, pi - 0.3] (away from the branch cut of
        angle() at pi AND from 0, where a negative LayerNorm weight would put it on the cut), columns kx = 0 and kx = w/2 Hermitian in ky, the
        four structurally real bins real with a random sign (the negative ones pin the exact-pi branch); irfft2 in fp64, scaled to std 0.5;
      * local half (irrelevant to which = 0): per pixel, every other channel p, the rest q, with p and q solved so that the pixel's mean over
        all e channels is 0 and its variance 1 -- LayerNorm is then one uniform scale and a per-channel affine map, which touches the DC bin
        only."""
    e = 8 * C if blk == 2 else 4 * C
    half, wh = e // 2, w // 2 + 1
    rng = np.random.default_rng([7100, C, blk, B, h, w, seed])
    amp = rng.uniform(0.5, 2.0, (B, half, h, wh))
    pha = rng.uniform(0.3, np.pi - 0.3, (B, half, h, wh)) * rng.choice([-1.0, 1.0], (B, half, h, wh))
    F = amp * np.exp(1j * pha)
    ky = np.arange(1, h // 2)
    for kx in (0, w // 2):
        F[:, :, h - ky, kx] = np.conj(F[:, :, ky, kx])
        for k0 in (0, h // 2):
            F[:, :, k0, kx] = amp[:, :, k0, kx] * rng.choice([-1.0, 1.0], (B, half))
    g = np.fft.irfft2(F, s=(h, w))
    g *= 0.5 / g.std(axis=(-2, -1), keepdims=True)
    g = np.ascontiguousarray(g.transpose(0, 2, 3, 1))                 # [B, h, w, half]
    m = half // 2                                                     # m channels of p, m of q
    s, r = g.sum(-1), (g * g).sum(-1)
    S, Q = -s / m, (e - r) / m                                        # p + q, p^2 + q^2
    disc = 2.0 * Q - S * S                                            # (p - q)^2
    assert float(disc.min()) > 0.0, ('no real p, q: change the seed', float(disc.min()))
    p, q = 0.5 * (S + np.sqrt(disc)), 0.5 * (S - np.sqrt(disc))
    loc = np.empty((B, h, w, half))
    loc[..., 0::2], loc[..., 1::2] = p[..., None], q[..., None]
    return torch.from_numpy(np.concatenate((loc, g), axis=-1).astype(np.float32))


def fft_kink_mask(out64):
    """[B, c, h, w] bool: where the fp64 mixer output (= |t|) is below 1e-4 x its plane's RMS -- the kink of abs(), where the sign of a t that is zero
    to rounding decides dt.  (The RMS, not the maximum: the edited spectrum's bias puts a peak of 7 .. 450 x RMS at pixel (0, 0).)"""
    rms = out64.double().pow(2).mean(dim=(-2, -1), keepdim=True).sqrt()
    return out64.double() < 1e-4 * rms


FFT_GLOBAL = ('conv_amp.0.weight', 'conv_amp.0.bias', 'conv_pha.0.weight', 'conv_pha.0.bias')
# (family, C, blk, B, PAN H, PAN W); the plane is the PAN size at blocks 0 / 1 / 3 / 4, half of it at block 2.  Families: 'lds' k_fftmix_r (in LDS),
# 'split' (square 256 / 512), 'blue' / 'blue1k' the Bluestein path with both FFT lengths M <= 512 / one of them >= 1024 (M = the next power of
# two >= 2n - 1; L = min(16, 8192 / M) lines per workgroup)
FFT_CASES = [
    ('lds', 4, 2, 1, 16, 16), ('lds', 4, 2, 3, 16, 16),                  # planes 8 x 8
    ('lds', 4, 0, 2, 16, 16), ('lds', 4, 0, 2, 32, 32), ('lds', 4, 0, 2, 64, 64), ('lds', 4, 0, 2, 128, 128),
    ('lds', 8, 0, 16, 128, 128),                                         # 256 planes: the last count on k_fftmix_r<7, 1024>
    ('lds', 8, 0, 17, 128, 128),                                         # 272 planes: k_fftmix_r<7, 512>
    ('lds', 4, 1, 2, 32, 32), ('lds', 4, 3, 2, 32, 32), ('lds', 4, 4, 2, 32, 32),      # the other blocks' parameter offsets
    ('split', 4, 0, 1, 256, 256),                                        # 129 columns in groups of 32: the last group holds one
    ('split', 4, 0, 2, 256, 256), ('split', 4, 0, 1, 512, 512),          # 512: groups of 16
    ('blue', 4, 2, 3, 16, 48), ('blue', 4, 2, 3, 48, 16),                # planes 8 x 24 and 24 x 8: one ragged row group, M = 16 / 64
    ('blue', 4, 2, 3, 80, 48),                                           # plane 40 x 24: rows 16 + 16 + 8
    ('blue', 4, 0, 2, 48, 48), ('blue', 4, 0, 2, 32, 64), ('blue', 4, 0, 2, 64, 32),   # power-of-two sides of rectangles: M = 2n exactly
    ('blue', 4, 0, 1, 208, 176), ('blue', 4, 2, 1, 208, 176),
    ('blue', 4, 0, 2, 256, 16),                                          # n = 256: M = 512, the largest n on it
    ('blue1k', 4, 0, 2, 272, 16),                                        # M = 1024, L = 8
    ('blue1k', 4, 0, 1, 512, 16),                                        # M = 1024, the largest n on it
    ('blue1k', 4, 0, 1, 528, 16),                                        # M = 2048, L = 4
    ('blue1k', 4, 0, 1, 400, 400),                                       # 201 columns in groups of 8: the last holds one
    ('blue1k', 4, 0, 1, 32, 1024), ('blue1k', 4, 0, 1, 1024, 32),        # length-1024 lines as rows / as columns: 17 columns in groups of 16, 513 in groups of 4
    ('blue', 8, 0, 2, 80, 48),
]
FFT_FULL_CASES = [(4, 2, 1, 16, 16), (4, 0, 2, 32, 32), (4, 0, 2, 128, 128)]         # LG_FFT=full: k_fftmix / k_fftmix_bwd at planes 8, 32, 128
# (C, blk, B, H, W) -> seed of a case whose first draw missed a precondition (never a bound changed).  (4,2,3,16,48): amplitude floor 0.034, a DC bin
# nearly cancelled by the LayerNorm bias; seed 1: 0.082
FFT_RESEED = {(4, 2, 3, 16, 48): 1}
FFT_PRE = {'cut': 0.05, 'floor': 0.05, 'masked': 1e-3, 'clean': 2e-6}


def fft_plane(blk, H, W):
    return (H // 2, W // 2) if blk == 2 else (H, W)


def fft_plane_err(a, b64, scale='rms'):
    """max over planes of max |a - b64| / RMS(b64 plane) (scale='max': / max |b64 plane|): [B, c, h, w] tensors"""
    d = (a.double() - b64).abs().amax(dim=(-2, -1))
    den = b64.pow(2).mean(dim=(-2, -1)).sqrt() if scale == 'rms' else b64.abs().amax(dim=(-2, -1))
    return float((d / den).max())


def fft_local_err(a, b64):
    """max over all elements of |a - b64| / (|b64| + RMS(b64 plane)): the error on the scale of the element's own size where that is above the
    plane's RMS -- the forward output's peak around pixel (0, 0), whose rounding error (2^-24 x 6 .. 450 RMS) sets fft_plane_err and hides an
    error of a few 1e-6 RMS everywhere else"""
    rms = b64.pow(2).mean(dim=(-2, -1), keepdim=True).sqrt()
    return float(((a.double() - b64).abs() / (b64.abs() + rms)).max())


def fft_grad_err(a, b64):
    return float((a.double() - b64).abs().max()) / float(b64.abs().max())


_FFT_REFS = {}


def fft_mixer_refs(C, blk, B, H, W):
    """one case of the FFT mixer alone (lg_op_block / lg_op_block_bwd with which = 0): the designed features, the upstream gradient (standard
    normal, exactly 0 on the kink mask), the oracle in fp64 and fp32 -- the output y [B, e/2, h, w], dx = d/d LayerNorm(feat)'s global half
    (planar) and the four global_mixer gradients -- and the measured preconditions.  Computed once per case, shared, never written to."""
    key = (C, blk, B, H, W)
    if key in _FFT_REFS:
        return _FFT_REFS[key]
    assert orc.CANONICAL_REAL_BINS, 'the FFT mixer tests pin the +0 convention of the four purely-real bins'
    h, w = fft_plane(blk, H, W)
    feat = fft_designed_features(C, blk, B, h, w, FFT_RESEED.get(key, 0))
    half = feat.shape[-1] // 2
    bp = block_prefix(blk) + '0.fn.'
    names = [bp + 'fn.global_mixer.' + n for n in FFT_GLOBAL]
    res = {}
    dy = None
    for dtype in (torch.float64, torch.float32):
        P = _fft_params(C, dtype)
        with torch.no_grad():
            ln = orc.layer_norm(feat.to(dtype), P[bp + 'norm.weight'], P[bp + 'norm.bias'])
        xin = ln[..., half:].clone().requires_grad_(True)
        y = orc.global_mixer(P, bp + 'fn.global_mixer.', xin).permute(0, 3, 1, 2)
        if dy is None:
            mask = fft_kink_mask(y.detach())
            dy = torch.from_numpy(np.random.default_rng([7200, C, blk, B, H, W]).standard_normal(tuple(y.shape)).astype(np.float32))
            dy[mask] = 0.0
            pl = xin.detach().permute(0, 3, 1, 2)
            Fq = torch.fft.rfft2(pl)
            nrm = pl.pow(2).sum(dim=(-2, -1), keepdim=True).sqrt()
            struct = torch.zeros(h, w // 2 + 1, dtype=torch.bool)
            for k0 in (0, h // 2):
                for kx in (0, w // 2):
                    struct[k0, kx] = True
            cut = (Fq.imag.abs() / nrm)[(Fq.real < 0) & ~struct]
            pre = {'cut': float(cut.min()), 'floor': float((Fq.abs() / nrm).min()), 'masked': float(mask.double().mean()),
                   'neg_real_bins': int((Fq.real[..., struct] < 0).sum())}
        g = torch.autograd.grad((y * dy.to(dtype)).sum(), [xin] + [P[n] for n in names])
        res[dtype] = (y.detach().double(), g[0].permute(0, 3, 1, 2).double().contiguous(), {n: v.double() for n, v in zip(names, g[1:])})
    (y64, dx64, g64), (y32, dx32, g32) = res[torch.float64], res[torch.float32]
    # forward: on the plane's LARGEST entry.  The edited spectrum's phases are nearly coherent (conv_pha's weights are small), so the output has a
    # peak of 6 .. 450 x its RMS around pixel (0, 0) and ANY fp32 evaluation is off by 2^-24 x that peak there: on the RMS the fp32 oracle's
    # forward figure is 1e-6 .. 7e-5 by the size of the plane, whatever the seed.  dx has no such peak (4 .. 5 x RMS) and is held on its RMS.
    pre['clean_fwd'], pre['clean_dx'] = fft_plane_err(y32, y64, 'max'), fft_plane_err(dx32, dx64)
    pre['peak'] = float((y64.amax(dim=(-2, -1)) / y64.pow(2).mean(dim=(-2, -1)).sqrt()).max())
    pre['clean_grads'] = {n: fft_grad_err(g32[n], g64[n]) for n in names}
    ref = dict(feat=feat, dy=dy, mask=mask, names=names, y64=y64, y32=y32, dx64=dx64, dx32=dx32, g64=g64, g32=g32, pre=pre)
    if B * h * w * half <= 1 << 19:                      # (the large cases are used once)
        _FFT_REFS[key] = ref
    return ref


@functools.lru_cache(maxsize=None)
def _fft_params(C, dtype):
    return det_params(C, 1, dtype=dtype, requires_grad=True)


def fft_assert_preconditions(tag, pre):
    """conditions on the INPUT, not tolerances: a case that misses one gets another seed (FFT_RESEED), never another bound"""
    assert pre['cut'] >= FFT_PRE['cut'], (tag, 'a bin with Re F < 0 too close to the branch cut of angle(): change the seed', pre['cut'])
    assert pre['floor'] >= FFT_PRE['floor'], (tag, 'a bin amplitude too small for the backward division: change the seed', pre['floor'])
    assert pre['masked'] <= FFT_PRE['masked'], (tag, 'too many pixels on the kink of abs(): change the seed', pre['masked'])
    assert pre['clean_fwd'] <= FFT_PRE['clean'] and pre['clean_dx'] <= FFT_PRE['clean'], (tag, 'the fp32 oracle is not clean', pre)
    assert max(pre['clean_grads'].values()) <= FFT_PRE['clean'], (tag, 'the fp32 oracle is not clean', pre['clean_grads'])


LGT_CASES = [(4, 1, 16, 16), (4, 2, 16, 48), (4, 3, 80, 48), (8, 1, 48, 208), (8, 2, 48, 48), (8, 3, 80, 48)]                 # (C, B, H, W)
DSTEP_CASES = [(1, 4, 16, 16), (3, 4, 48, 16), (3, 8, 80, 48), (1, 4, 208, 176), (2, 8, 16, 48), (5, 4, 64, 64)]               # (B, C, H, W)
