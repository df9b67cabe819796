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


LGT_CASES = [(4, 1, 16, 16), (4, 2, 16, 48), (4, 3, 80, 48), (8, 1, 48, 208), (8, 2, 48, 48), (8, 3, 80, 48)]                 # (C, B, H, W)
DSTEP_CASES = [(1, 4, 16, 16), (3, 4, 48, 16), (3, 8, 80, 48), (1, 4, 208, 176), (2, 8, 16, 48), (5, 4, 64, 64)]               # (B, C, H, W)
