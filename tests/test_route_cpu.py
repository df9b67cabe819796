"""CPU (no GPU) checks of the kernel routes a plan resolves at creation (csrc/route.hip): lg_plan_create and lg_plan_describe are host code."""
import ctypes
import itertools
import json
import os

import pytest

from lgteun_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

K = 2
N_OFF = 12 + K + 119 * K
OFFS = (ctypes.c_int64 * N_OFF)(*[4 * i for i in range(N_OFF)])

# The resolver fills the FFN route, the mixer route and the net-level switches in three functions that read disjoint bit groups, except for the
# FFN implementation field and LG_VAR_FFN_BF16X3 (the local mixer's operand scales ride in the FFN's prep launch): both groups carry those two.
# test_bit_groups_are_independent checks the claim on the text; the sweeps below then iterate each group on its own instead of 4 * 3 * 2^14 words.
FFN_BITS = [_lib.LG_VAR_FFN_BWD32_PAIR, _lib.LG_VAR_FFN_DWBWD_TILE, _lib.LG_VAR_FFN_BF16X3, _lib.LG_VAR_FFN_BWD_BF16X3, _lib.LG_VAR_FFN_XS,
            _lib.LG_VAR_FFN_H3_RECOMPUTE]
MIXER_BITS = [_lib.LG_VAR_ATTN_BWD_R3, _lib.LG_VAR_ATTN_FWD_VALU, _lib.LG_VAR_FFN_BF16X3, _lib.LG_VAR_ATTN_BWD_CORE_M, _lib.LG_VAR_ATTN_BF16X3,
              _lib.LG_VAR_ATTN_BWD_RESTATS]
NET_BITS = [_lib.LG_VAR_DSTEP_TILES, _lib.LG_VAR_FFT_FULL, _lib.LG_VAR_REDUCE_PER_BLOCK]
SINGLE = [1, 2, 3, _lib.LG_VAR_FFN_SAVE3, _lib.LG_VAR_FFN_SAVE5] + [1 << b for b in range(4, 18)]


def subsets(bits):
    for r in range(len(bits) + 1):
        for c in itertools.combinations(bits, r):
            yield sum(c)


class Plan:
    """a plan of the library under test, or the message it was refused with"""

    def __init__(self, C, prec, H, W, variant):
        self.lib = _lib.lib()
        self.handle = ctypes.c_void_p()
        cfg = _lib.LgConfig(C, K, H, W, prec, variant)
        rc = self.lib.lg_plan_create(ctypes.byref(cfg), OFFS, N_OFF, ctypes.byref(self.handle))
        self.error = None if rc == 0 else self.lib.lg_last_error().decode()
        if rc:
            assert rc < 0 and self.error, (rc, self.error)
            self.handle = None

    def describe(self):
        buf = ctypes.create_string_buffer(2048)
        assert self.lib.lg_plan_describe(self.handle, buf, len(buf)) == 0, self.lib.lg_last_error()
        return buf.value.decode()

    def workspace_bytes(self):
        return [int(self.lib.lg_workspace_bytes(self.handle, B, t)) for B in (1, 2) for t in (0, 1, 2)]

    def __del__(self):
        if self.handle:
            self.lib.lg_plan_destroy(self.handle)


def parse(text):
    """{(level, mode): (ffn fields, mixer fields)} of the per-level lines -- a 'fwd' line carries a third group, the global mixer's {'fft': path} --
    and the net line"""
    lines = text.splitlines()
    assert lines[0].startswith('net ') and len(lines) == 7, text
    out = {}
    for line in lines[1:]:
        head, rest = line.split(': ', 1)
        mode = head.split()[-1]
        groups = tuple(dict(kv.split('=', 1) for kv in part.split()) for part in rest.split(' | '))
        assert len(groups) == (3 if mode == 'fwd' else 2) and (mode != 'fwd' or list(groups[2]) == ['fft']), line
        out[(int(head[1]), mode)] = groups
    assert sorted(out) == [(lvl, mode) for lvl in (0, 1) for mode in ('bwd', 'fwd', 'save')], text
    return lines[0], out


def check_reads_are_written(text):
    _, r = parse(text)
    for lvl in (0, 1):
        (fs, ms), (fb, mb) = r[(lvl, 'save')], r[(lvl, 'bwd')]
        # a slot is named with what it holds ('a3' gelu(h3), 'a3:h3' the pre-activation): the backward has to read the form that was written
        written, read = set(fs['writes'].split(',')), set(fb['reads'].split(','))
        assert read <= written, (lvl, text)
        assert (mb['stats'] == 'saved') <= (ms['writes'] == 'o,l'), (lvl, text)
        assert r[(lvl, 'fwd')][0]['ffn'] and fs['ffn'] and fb['ffn'] and mb['mixer'], text


def ffn_impl_rejected(v, prec):
    """the words lg_plan_create turns away: FFN implementation field 2 or 3 (retired kernels), or the fp32-only field value 1 with precision = 1"""
    impl = v & 3
    return impl >= 2 or (prec == 1 and impl != 0)


CONFIGS = [(C, prec, n) for C in (4, 8) for prec in (0, 1) for n in (32, 48, 128)]   # 48: the level-1 width is 8 mod 16 (no 16-wide strips)


def sweep_words():
    """the variant words of the sweeps (tests/test_gpu_routes_launch.py launches one plan per distinct route among them)"""
    words = {impl | save | rest for impl in range(4) for save in (0, _lib.LG_VAR_FFN_SAVE3, _lib.LG_VAR_FFN_SAVE5) for rest in subsets(FFN_BITS)}
    words |= {impl | rest for impl in range(4) for rest in subsets(MIXER_BITS)}
    words |= set(subsets(NET_BITS)) | set(SINGLE)
    return words


@pytest.mark.parametrize('C,prec,n', CONFIGS)
def test_every_backward_read_is_a_forward_write(C, prec, n):
    words = sweep_words()
    accepted = 0
    for v in sorted(words):
        p = Plan(C, prec, n, n, v)
        assert (p.error is not None) == ffn_impl_rejected(v, prec), (hex(v), p.error)   # every other word of the product is a valid one
        if p.error is not None:
            assert 'FFN implementation field' in p.error, (hex(v), p.error)
            continue
        accepted += 1
        check_reads_are_written(p.describe())
    assert accepted >= len(words) // 4


# PAN sizes whose level-1 plane (8 x 8, 40 x 24, 24 x 104) is no whole number of 8-row steps of 16-column strips: resolve_ffn turns the strip walk off there
FALLBACK_PLANES = [(16, 16), (80, 48), (48, 208)]


@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('prec', [0, 1])
@pytest.mark.parametrize('H,W', FALLBACK_PLANES)
def test_level_1_planes_without_whole_strips_fall_back_to_the_tile_kernel(C, prec, H, W):
    """the default plan at rectangles: every backward read is a forward write, and the level-1 FFN backward is the tile kernel k_ffn_dw_bwd (with its
    k_wgrad launch for dW3), not the strip walk k_ffn_dw_bwd_xs -- which level 0, whose planes are whole strips, keeps where it has one"""
    p = Plan(C, prec, H, W, 0)
    assert p.error is None
    text = p.describe()
    check_reads_are_written(text)
    _, r = parse(text)
    l1 = r[(1, 'bwd')][0]['ffn'].split('+')
    assert l1[0] == 'k_ffn_dw_bwd' and 'k_ffn_dw_bwd_xs' not in l1 and l1[-1] == 'k_wgrad(W3)', text
    assert l1[1] == ('k_ffn1_bwd_xs' if C == 4 else 'k_ffn1_bwd'), text
    assert r[(0, 'bwd')][0]['ffn'] == 'k_ffn_dw_bwd_xs+k_ffn1_bwd_xs', text
    # the same heights at a width of whole strips (level 1: 32 columns) keep the strip walk at e = 32 (C = 4); e = 64 has the tile kernel only
    whole = parse(Plan(C, prec, H, 64, 0).describe())[1]
    assert (whole[(1, 'bwd')][0]['ffn'].split('+')[0] == 'k_ffn_dw_bwd_xs') == (C == 4), (C, prec, H, W)


def test_bit_groups_are_independent():
    """a bit outside a group leaves that group's part of the text alone, on the default and on every single switch; the global mixer's path is part
    of the net group (LG_VAR_FFT_FULL alone moves it)"""
    def parts(text):
        net, r = parse(text)
        fft = [r[k][2] for k in sorted(r) if k[1] == 'fwd']
        return (net.split(': ')[1], fft), [r[k][0] for k in sorted(r)], [r[k][1] for k in sorted(r)]
    for C, prec in ((4, 0), (8, 0), (4, 1)):
        for base in [0] + SINGLE:
            p0 = Plan(C, prec, 128, 128, base)
            if p0.error is not None:
                continue
            net0, ffn0, mix0 = parts(p0.describe())
            for bit in set(FFN_BITS + MIXER_BITS + NET_BITS) - {base}:
                p1 = Plan(C, prec, 128, 128, base | bit)
                assert p1.error is None
                net1, ffn1, mix1 = parts(p1.describe())
                assert net1 == net0 or bit in NET_BITS
                assert ffn1 == ffn0 or bit in FFN_BITS
                assert mix1 == mix0 or bit in MIXER_BITS


def test_invalid_variant_words_are_rejected():
    for v in (1 << 18, 1 << 20, 1 << 31, _lib.LG_VAR_REDUCE_PER_BLOCK | 1 << 19):
        p = Plan(4, 0, 32, 32, v)
        assert p.error is not None and 'unknown variant bits' in p.error
    p = Plan(4, 0, 32, 32, _lib.LG_VAR_FFN_SAVE3 | _lib.LG_VAR_FFN_SAVE5)
    assert p.error is not None and 'invalid FFN save variant' in p.error


# the default plans at 128 x 128; the kernel names are the ones a kernel trace of the library before the route table shows for these configurations
DEFAULT_ROUTES = {
    (4, 0): """\
net C=4 128x128 precision=0 variant=0x0: dstep=fused fft=k_fftmix_r reduce=merged
L0 e=16 128x128 fwd: ffn=k_ffn_xr arith=f16x2 hidden=fp32 | mixer=k_attn_m arith=f16x2 | fft=k_fftmix_r
L0 e=16 128x128 save: ffn=k_ffn_xr writes=h2,a3:h3 | mixer=k_attn_m writes=o,l
L0 e=16 128x128 bwd: ffn=k_ffn_dw_bwd_xs+k_ffn1_bwd_xs arith=f16x2 reads=h2,a3:h3 | mixer=k_attn_bwd_f stats=saved
L1 e=32 64x64 fwd: ffn=k_ffn_x32 arith=f16x2 hidden=fp32 | mixer=k_attn_m arith=f16x2 | fft=k_fftmix_r
L1 e=32 64x64 save: ffn=k_ffn_x32 writes=h2,a3:h3 | mixer=k_attn_m writes=o,l
L1 e=32 64x64 bwd: ffn=k_ffn_dw_bwd_xs+k_ffn1_bwd_xs arith=f16x2 reads=h2,a3:h3 | mixer=k_attn_bwd_core+k_attn_bwd_epi stats=saved
""",
    (4, 1): """\
net C=4 128x128 precision=1 variant=0x0: dstep=fused fft=k_fftmix_r reduce=merged
L0 e=16 128x128 fwd: ffn=k_ffn_xr arith=bf16 hidden=bf16 | mixer=k_attn_m arith=bf16 | fft=k_fftmix_r
L0 e=16 128x128 save: ffn=k_ffn_xr writes=h2,a3:h3 | mixer=k_attn_m writes=-
L0 e=16 128x128 bwd: ffn=k_ffn_dw_bwd_xs+k_ffn1_bwd_xs arith=bf16 reads=h2,a3:h3 | mixer=k_attn_bwd_f stats=recomputed
L1 e=32 64x64 fwd: ffn=k_ffn_x32 arith=bf16 hidden=bf16 | mixer=k_attn_m arith=bf16 | fft=k_fftmix_r
L1 e=32 64x64 save: ffn=k_ffn_x32 writes=h2,a3:h3 | mixer=k_attn_m writes=-
L1 e=32 64x64 bwd: ffn=k_ffn_dw_bwd_xs+k_ffn1_bwd_xs arith=bf16 reads=h2,a3:h3 | mixer=k_attn_bwd_core+k_attn_bwd_epi stats=recomputed
""",
    (8, 0): """\
net C=8 128x128 precision=0 variant=0x0: dstep=fused fft=k_fftmix_r reduce=merged
L0 e=32 128x128 fwd: ffn=k_ffn_x32 arith=f16x2 hidden=fp32 | mixer=k_attn_m arith=f16x2 | fft=k_fftmix_r
L0 e=32 128x128 save: ffn=k_ffn_x32 writes=h2,a3:h3 | mixer=k_attn_m writes=o,l
L0 e=32 128x128 bwd: ffn=k_ffn_dw_bwd_xs+k_ffn1_bwd_xs arith=f16x2 reads=h2,a3:h3 | mixer=k_attn_bwd_core+k_attn_bwd_epi stats=saved
L1 e=64 64x64 fwd: ffn=k_ffn1_x64+k_ffn2_x64 arith=f16x2 hidden=fp32 | mixer=k_attn_m arith=f16x2 | fft=k_fftmix_r
L1 e=64 64x64 save: ffn=k_ffn1_x64+k_ffn2_x64 writes=a1,g1,h2,a3,g3 | mixer=k_attn_m writes=o,l
L1 e=64 64x64 bwd: ffn=k_ffn_dw_bwd+k_ffn1_bwd+k_wgrad(W2)+k_wgrad(W1)+k_wgrad(W3) arith=f32 reads=a1,g1,h2,a3,g3 | mixer=k_attn_bwd_core+k_attn_bwd_epi stats=saved
""",
    (8, 1): """\
net C=8 128x128 precision=1 variant=0x0: dstep=fused fft=k_fftmix_r reduce=merged
L0 e=32 128x128 fwd: ffn=k_ffn_x32 arith=bf16 hidden=bf16 | mixer=k_attn_m arith=bf16 | fft=k_fftmix_r
L0 e=32 128x128 save: ffn=k_ffn_x32 writes=h2,a3:h3 | mixer=k_attn_m writes=-
L0 e=32 128x128 bwd: ffn=k_ffn_dw_bwd_xs+k_ffn1_bwd_xs arith=bf16 reads=h2,a3:h3 | mixer=k_attn_bwd_core+k_attn_bwd_epi stats=recomputed
L1 e=64 64x64 fwd: ffn=k_ffn1_x64+k_ffn2_x64 arith=bf16x3 hidden=fp32 | mixer=k_attn_m arith=bf16 | fft=k_fftmix_r
L1 e=64 64x64 save: ffn=k_ffn1_x64+k_ffn2_x64 writes=a1,g1,h2,a3,g3 | mixer=k_attn_m writes=-
L1 e=64 64x64 bwd: ffn=k_ffn_dw_bwd+k_ffn1_bwd+k_wgrad(W2)+k_wgrad(W1)+k_wgrad(W3) arith=f32 reads=a1,g1,h2,a3,g3 | mixer=k_attn_bwd_core+k_attn_bwd_epi stats=recomputed
""",
}


@pytest.mark.parametrize('C,prec', sorted(DEFAULT_ROUTES))
def test_default_routes_are_pinned(C, prec):
    p = Plan(C, prec, 128, 128, 0)
    assert p.error is None
    assert p.describe() == DEFAULT_ROUTES[(C, prec)]


# PAN sizes on every path of the global (FFT) mixer, level 0 then level 1: in LDS on both (16, 32, 128); split, then in LDS (256); split on both (512);
# Bluestein, then split (1024); Bluestein on both (rectangles, sides that are no power of two).  24 x 8 is no multiple of 16: no plan takes it
FFT_SIZES = [(16, 16), (32, 32), (128, 128), (256, 256), (512, 512), (1024, 1024), (80, 48), (208, 176), (400, 400), (1024, 32), (24, 8)]


def fft_path_by_size(h, w, full):
    """the size rule of the global mixer, restated: a square power of two of 8 .. 512 stays radix-2 -- through HBM above 128, in LDS otherwise, where
    LG_VAR_FFT_FULL picks the kernel pair -- and everything else takes Bluestein lines"""
    if h == w and h & (h - 1) == 0 and 8 <= h <= 512:
        return 'split' if h > 128 else 'k_fftmix' if full else 'k_fftmix_r'
    return 'bluestein'


@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('H,W', FFT_SIZES)
def test_fft_path_follows_the_plane_size(C, H, W):
    """each level's fft= token of lg_plan_describe is the size rule's answer for that level's plane, with and without LG_VAR_FFT_FULL, and the switch
    changes the token of the in-LDS levels only"""
    tokens = {}
    for full in (False, True):
        p = Plan(C, 0, H, W, _lib.LG_VAR_FFT_FULL if full else 0)
        if H % 16 or W % 16:
            assert p.error is not None and 'multiples of 16' in p.error, (H, W, p.error)
            return
        assert p.error is None, p.error
        net, r = parse(p.describe())
        assert ('fft=k_fftmix' if full else 'fft=k_fftmix_r') in net.split(': ')[1].split(), net   # the net line: the switch, as before
        tokens[full] = [r[(lvl, 'fwd')][2]['fft'] for lvl in (0, 1)]
        assert tokens[full] == [fft_path_by_size(H >> lvl, W >> lvl, full) for lvl in (0, 1)], (C, H, W, full, tokens[full])
    for plain, switched in zip(tokens[False], tokens[True]):
        assert (plain, switched) == ('k_fftmix_r', 'k_fftmix') or (plain == switched and plain in ('split', 'bluestein')), tokens


def test_workspace_bytes_on_every_fft_path_are_those_before_the_fft_route():
    """lg_workspace_bytes at FFT_SIZES (both C, both precisions, with and without LG_VAR_FFT_FULL): the half-spectrum scratch of the split and the
    Bluestein path and the backward's partial rows, sized from FftRoute, against the figures of the library that derived them from the plane size"""
    with open(os.path.join(GOLD, 'workspace_bytes_fft.json')) as f:
        gold = json.load(f)
    assert gold['K'] == K
    seen = set()
    for c in gold['cases']:
        p = Plan(c['C'], c['precision'], c['H'], c['W'], c['variant'])
        assert p.error is None, (c, p.error)
        assert p.workspace_bytes() == c['bytes'], c
        seen.add((c['C'], c['precision'], c['H'], c['W'], c['variant']))
    assert seen == {(C, prec, H, W, v) for C in (4, 8) for prec in (0, 1) for H, W in FFT_SIZES if H % 16 == 0 and W % 16 == 0
                    for v in (0, _lib.LG_VAR_FFT_FULL)}


def test_describe_reports_a_short_buffer():
    p = Plan(4, 0, 128, 128, 0)
    buf = ctypes.create_string_buffer(64)
    assert p.lib.lg_plan_describe(p.handle, buf, len(buf)) == -3 and b'too small' in p.lib.lg_last_error()


def test_workspace_bytes_are_those_of_the_library_before_the_route_table():
    with open(os.path.join(GOLD, 'workspace_bytes.json')) as f:
        gold = json.load(f)
    assert gold['K'] == K
    seen = set()
    for c in gold['cases']:
        p = Plan(c['C'], c['precision'], c['H'], c['W'], c['variant'])
        assert (p.error is not None) == ffn_impl_rejected(c['variant'], c['precision']), (c, p.error)   # (recorded from a build that carried the retired words too)
        if p.error is not None:
            assert 'FFN implementation field' in p.error, (c, p.error)
            continue
        assert p.workspace_bytes() == c['bytes'], c
        seen.add(c['variant'])
    assert {0, 1, _lib.LG_VAR_FFN_SAVE3, _lib.LG_VAR_FFN_SAVE5} | {1 << b for b in range(4, 18)} <= seen
