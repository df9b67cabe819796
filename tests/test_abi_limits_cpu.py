"""No GPU needed: the argument checks and the workspace sizers of the satellite entries of include/lgteun_hip.h at the edges of their stated
ranges (tests/test_gpu_abi_limits.py runs the accepted side on the device).

The header promises that arguments are validated before any HIP call.  So a call with ONE argument just outside its range is safe with
pointers that are never dereferenced (limits_helpers.FAKE): every case below was read against its validator first, returns a negative
code, and leaves a message in lg_last_error that begins with the entry's name, names the argument and is no HIP error string.  The values one
step INSIDE the range go to the sizers only -- never to a launcher, neither here nor with fake pointers on a GPU box."""
import ctypes

import pytest

from limits_helpers import FAKE, TWO31
from lgteun_amd import _lib

P, PW, Q = FAKE, FAKE + (1 << 24), FAKE + 4          # two aligned fake pointers; one that is 4 bytes off every 8- and 16-byte alignment
WS = 1 << 40                                         # workspace_bytes that no sizer exceeds: a size check never fires before the one under test
U16, F32 = _lib.LG_DT_U16, _lib.LG_DT_F32
NULL = None


def L():
    return _lib.lib()


# entry -> (prefix of its messages, the argument names in ABI order, arguments every check accepts)
ENTRIES = {
    'lg_interp23_up4': ('interp23_up4', 'ms out B C h w stream', dict(ms=P, out=P, B=2, C=4, h=8, w=8)),
    'lg_sfim': ('sfim', 'ms pan out B C h w workspace workspace_bytes stream', dict(ms=P, pan=P, out=P, B=2, C=4, h=8, w=8, workspace=PW, workspace_bytes=WS)),
    'lg_gsa': ('gsa', 'ms pan out stats B C h w workspace workspace_bytes stream',
               dict(ms=P, pan=P, out=P, stats=P, B=2, C=4, h=8, w=8, workspace=PW, workspace_bytes=WS)),
    'lg_wavelet': ('wavelet', 'ms pan out B C h w stream', dict(ms=P, pan=P, out=P, B=2, C=4, h=8, w=8)),
    'lg_mtf_glp': ('mtf_glp', 'ms pan out stats taps n_filters n_taps mode B C h w workspace workspace_bytes stream',
                   dict(ms=P, pan=P, out=P, stats=P, taps=P, n_filters=1, n_taps=41, mode=0, B=2, C=4, h=8, w=8, workspace=PW, workspace_bytes=WS)),
    'lg_bdsd': ('bdsd', 'ms pan out stats taps_ms n_filters taps_pan n_taps block B C h w workspace workspace_bytes stream',
                dict(ms=P, pan=P, out=P, stats=P, taps_ms=P, n_filters=1, taps_pan=P, n_taps=41, block=0, B=2, C=4, h=8, w=8, workspace=PW,
                     workspace_bytes=WS)),
    'lg_iqa_ref': ('iqa', 'pred gt out B C H W scale workspace workspace_bytes stream',
                   dict(pred=P, gt=P, out=P, B=2, C=4, H=16, W=16, scale=1.0, workspace=PW, workspace_bytes=WS)),
    'lg_iqa_no_ref': ('iqa', 'pred pan ms out B C H W scale workspace workspace_bytes stream',
                      dict(pred=P, pan=P, ms=P, out=P, B=2, C=4, H=32, W=32, scale=1.0, workspace=PW, workspace_bytes=WS)),
    'lg_iqa_ref_ext': ('lg_iqa_ref_ext', 'pred gt out B C H W scale workspace workspace_bytes stream',
                       dict(pred=P, gt=P, out=P, B=2, C=4, H=32, W=32, scale=1.0, workspace=PW, workspace_bytes=WS)),
    'lg_iqa_q2n': ('lg_iqa_q2n', 'gt fused out B C H W scale workspace workspace_bytes stream',
                   dict(gt=P, fused=P, out=P, B=2, C=4, H=32, W=32, scale=1.0, workspace=PW, workspace_bytes=WS)),
    'lg_qnr_stats': ('qnr_stats', 'out pan ms pan_l q table B C H W workspace workspace_bytes stream',
                     dict(out=P, pan=P, ms=P, pan_l=P, q=P, table=P, B=2, C=4, H=8, W=8, workspace=PW, workspace_bytes=WS)),
    'lg_qnr_grad': ('qnr_grad', 'out pan table dout loss_accum indices B B_global C H W scale accumulate workspace workspace_bytes stream',
                    dict(out=P, pan=P, table=P, dout=P, loss_accum=P, indices=P, B=2, B_global=2, C=4, H=8, W=8, scale=1.0, accumulate=0, workspace=PW,
                         workspace_bytes=WS)),
    'lg_sam_loss': ('sam_loss', 'out gt dout loss_accum B B_global C H W scale accumulate workspace workspace_bytes stream',
                    dict(out=P, gt=P, dout=P, loss_accum=P, B=2, B_global=2, C=4, H=1, W=4, scale=1.0, accumulate=0, workspace=PW, workspace_bytes=WS)),
    'lg_ssim_loss': ('ssim_loss', 'out gt dout loss_accum B B_global C H W scale data_range accumulate workspace workspace_bytes stream',
                     dict(out=P, gt=P, dout=P, loss_accum=P, B=2, B_global=2, C=4, H=11, W=12, scale=1.0, data_range=1.0, accumulate=0, workspace=PW,
                          workspace_bytes=WS)),
    'lg_pyr_down2': ('pyr_down2', 'pan pan_l planes H W dtype stream', dict(pan=P, pan_l=P, planes=3, H=8, W=8, dtype=U16)),
    'lg_batch_assemble': ('batch_assemble', 'pan lr mul pan_l N idx idx_offset flips o_pan o_lr o_mul o_pan_l B C H W h w dtype divisor n_div post_scale stream',
                          dict(pan=P, lr=P, mul=P, pan_l=P, N=5, idx=P, idx_offset=0, flips=NULL, o_pan=P, o_lr=P, o_mul=P, o_pan_l=P, B=2, C=4, H=8, W=8,
                               h=2, w=2, dtype=U16, divisor=1.0, n_div=0, post_scale=1.0)),
    'lg_fir_decimate4': ('fir_decimate4', 'in out taps planes H W n_taps phase dtype out_f32 stream',
                         dict(out=P, taps=P, planes=3, H=8, W=8, n_taps=41, phase=2, dtype=U16, out_f32=1, **{'in': P})),
    'lg_window_assemble': ('window_assemble', 'pan lr mul origins n_windows first flips o_pan o_lr o_mul o_pan_l B C Hs Ws P Q dtype divisor n_div post_scale stream',
                           dict(pan=P, lr=P, mul=P, origins=P, n_windows=4, first=0, flips=NULL, o_pan=P, o_lr=P, o_mul=P, o_pan_l=P, B=2, C=4, Hs=64, Ws=64,
                                P=8, Q=8, dtype=U16, divisor=1.0, n_div=0, post_scale=1.0)),
    'lg_scene_gather': ('scene_gather', 'pan ms origins n_tiles first o_pan o_ms B C H W th tw dtype divisor n_div post_scale stream',
                        dict(pan=P, ms=P, origins=P, n_tiles=4, first=0, o_pan=P, o_ms=P, B=2, C=4, H=64, W=64, th=16, tw=16, dtype=U16, divisor=1.0, n_div=0,
                             post_scale=1.0)),
    'lg_scene_blend': ('scene_blend', 'tiles scene first B C H W th tw overlap stream',
                       dict(tiles=P, scene=P, first=0, B=2, C=4, H=64, W=64, th=16, tw=16, overlap=0)),       # a 4 x 4 grid of 16 tiles
    'lg_scene_to_u16': ('scene_to_u16', 'src dst n scale stream', dict(src=P, dst=P, n=8, scale=1.0)),
    'lg_grad_norm': ('grad_norm', 'grads ranges n_ranges max_range max_norm out workspace workspace_bytes stream',
                     dict(grads=P, ranges=P, n_ranges=2, max_range=100, max_norm=1.0, out=P, workspace=PW, workspace_bytes=WS)),
}

CLASSICAL = ('lg_interp23_up4', 'lg_sfim', 'lg_gsa', 'lg_wavelet', 'lg_mtf_glp', 'lg_bdsd')
B_ENTRIES = CLASSICAL + ('lg_iqa_ref', 'lg_iqa_no_ref', 'lg_iqa_ref_ext', 'lg_iqa_q2n', 'lg_qnr_stats', 'lg_qnr_grad', 'lg_sam_loss', 'lg_ssim_loss',
                         'lg_batch_assemble', 'lg_window_assemble', 'lg_scene_gather', 'lg_scene_blend')

# (entry, the one argument outside its range, what the message must say).  pyr_down2: 2^20 tiles of 8 x 8 outputs per 32768^2 plane, fir: 2^20 tiles of
# 16 x 16 per 65536^2 plane: 2048 planes make planes x tiles = 2^31.
REJECTED = [(e, dict(B=b), 'B must be') for e in B_ENTRIES for b in (0, 65536)]
REJECTED += [(e, dict([kv]), f'{kv[0]} must be') for e in CLASSICAL for kv in (('h', 4097), ('h', 3), ('w', 4097), ('w', 3), ('C', 1), ('C', 17))]
REJECTED += [(e, dict(ms=Q), 'ms must be 16-byte aligned') for e in CLASSICAL]
REJECTED += [(e, dict(workspace=Q), 'workspace must be 8-byte aligned') for e in ('lg_sfim', 'lg_gsa', 'lg_mtf_glp', 'lg_bdsd')]
REJECTED += [
    ('lg_gsa', dict(stats=Q), 'stats must be 8-byte aligned'), ('lg_mtf_glp', dict(taps=Q), 'taps must be 8-byte aligned'),
    ('lg_mtf_glp', dict(n_taps=65), 'n_taps must be'), ('lg_mtf_glp', dict(n_filters=2), 'n_filters must be'),
    ('lg_bdsd', dict(taps_pan=Q), 'taps_pan must be 8-byte aligned'), ('lg_bdsd', dict(block=48), 'block must be'),
    ('lg_bdsd', dict(h=4, w=4, C=8), 'h * w'), ('lg_bdsd', dict(n_taps=40), 'n_taps must be'),
    ('lg_iqa_ref', dict(C=1), 'C must be'), ('lg_iqa_ref', dict(C=17), 'C must be'), ('lg_iqa_ref', dict(H=10), 'H and W must be >= 11'),
    ('lg_iqa_ref', dict(W=8196), 'H and W must be <= 8192'), ('lg_iqa_ref', dict(workspace=Q), 'workspace must be 8-byte aligned'),
    ('lg_iqa_no_ref', dict(C=17), 'C must be'), ('lg_iqa_no_ref', dict(H=28), 'H and W >= 32'), ('lg_iqa_no_ref', dict(W=34), 'multiples of 4'),
    ('lg_iqa_no_ref', dict(H=8196), 'H and W must be <= 8192'),
    ('lg_iqa_ref_ext', dict(C=1), 'C must be'), ('lg_iqa_ref_ext', dict(C=9), 'C must be'), ('lg_iqa_ref_ext', dict(H=31), 'H and W must be >= 32'),
    ('lg_iqa_ref_ext', dict(W=8193), 'H and W must be <= 8192'), ('lg_iqa_ref_ext', dict(workspace=Q), 'workspace must be 8-byte aligned'),
    ('lg_iqa_q2n', dict(C=9), 'C must be'), ('lg_iqa_q2n', dict(W=31), 'H and W must be >= 32'), ('lg_iqa_q2n', dict(H=8193), 'H and W must be <= 8192'),
    ('lg_qnr_stats', dict(C=5), 'C must be 4 or 8'), ('lg_qnr_stats', dict(H=4), 'H and W must be multiples of 4 and at least 8'),
    ('lg_qnr_stats', dict(W=10), 'H and W must be multiples of 4 and at least 8'), ('lg_qnr_stats', dict(H=65540), 'H and W must be <= 65536'),
    ('lg_qnr_stats', dict(pan_l=Q), 'pan_l must be 16-byte aligned'), ('lg_qnr_stats', dict(table=Q), 'table must be 8-byte aligned'),
    ('lg_qnr_grad', dict(C=16), 'C must be 4 or 8'), ('lg_qnr_grad', dict(W=65540), 'H and W must be <= 65536'),
    ('lg_qnr_grad', dict(dout=Q), 'dout must be 16-byte aligned'), ('lg_qnr_grad', dict(B_global=1), 'B_global must be at least B'),
    ('lg_sam_loss', dict(C=2), 'C must be 4 or 8'), ('lg_sam_loss', dict(W=6), 'W must be a multiple of 4'), ('lg_sam_loss', dict(H=0), 'H at least 1'),
    ('lg_sam_loss', dict(H=65540), 'H and W must be <= 65536'), ('lg_sam_loss', dict(gt=Q), 'gt must be 16-byte aligned'),
    ('lg_ssim_loss', dict(C=6), 'C must be 4 or 8'), ('lg_ssim_loss', dict(H=10), 'H and W must be at least 11'),
    ('lg_ssim_loss', dict(W=8), 'H and W must be at least 11'), ('lg_ssim_loss', dict(W=65540), 'H and W must be <= 65536'),
    ('lg_ssim_loss', dict(workspace=Q), 'workspace must be 8-byte aligned'),
    ('lg_pyr_down2', dict(H=32772), 'H and W must be multiples of 4 in 8 .. 32768'), ('lg_pyr_down2', dict(W=4), 'H and W must be multiples of 4 in 8 .. 32768'),
    ('lg_pyr_down2', dict(W=10), 'H and W must be multiples of 4'), ('lg_pyr_down2', dict(planes=0), 'planes must be positive'),
    ('lg_pyr_down2', dict(planes=2048, H=32768, W=32768), 'planes x tiles below 2^31'),
    ('lg_batch_assemble', dict(C=0), 'C must be in 1 .. 16'), ('lg_batch_assemble', dict(C=17), 'C must be in 1 .. 16'),
    ('lg_batch_assemble', dict(N=0), 'N must be'), ('lg_batch_assemble', dict(N=TWO31), 'N must be'), ('lg_batch_assemble', dict(H=12), 'H and W must be 4 x'),
    ('lg_batch_assemble', dict(h=8193, H=4 * 8193), 'MS up to 8192'), ('lg_batch_assemble', dict(o_lr=Q), '16-byte aligned'),
    ('lg_fir_decimate4', dict(H=65540), 'H and W must be multiples of 4 in 8 .. 65536'), ('lg_fir_decimate4', dict(W=4), 'H and W must be multiples of 4 in 8 .. 65536'),
    ('lg_fir_decimate4', dict(n_taps=65), 'tap count'), ('lg_fir_decimate4', dict(n_taps=40), 'tap count'), ('lg_fir_decimate4', dict(phase=4), 'phase'),
    ('lg_fir_decimate4', dict(planes=0), 'planes must be positive'), ('lg_fir_decimate4', dict(planes=2048, H=65536, W=65536), 'planes x tiles below 2^31'),
    ('lg_fir_decimate4', dict(taps=Q), 'taps must be 8-byte aligned'), ('lg_fir_decimate4', {'in': P + 1}, 'aligned to their sample type'),
    ('lg_window_assemble', dict(C=17), 'C must be in 1 .. 16'), ('lg_window_assemble', dict(Hs=65540, Ws=65540), 'Hs and Ws must be multiples of 4 in 8 .. 65536'),
    ('lg_window_assemble', dict(P=4100, Hs=8192), 'window sides must be multiples of 4 in 8 .. 4096'), ('lg_window_assemble', dict(Q=4), 'window sides'),
    ('lg_window_assemble', dict(P=128), 'must not exceed the scene side'), ('lg_window_assemble', dict(first=3), 'first + B - 1 must lie inside'),
    ('lg_window_assemble', dict(o_pan_l=Q), '16-byte aligned'),
    ('lg_scene_gather', dict(C=0), 'C must be in 1 .. 16'), ('lg_scene_gather', dict(H=65540), 'H and W must be multiples of 4 in 16 .. 65536'),
    ('lg_scene_gather', dict(W=12), 'H and W must be multiples of 4 in 16 .. 65536'), ('lg_scene_gather', dict(th=1040, H=2048), 'tile sides must be multiples of 16'),
    ('lg_scene_gather', dict(tw=24), 'tile sides must be multiples of 16'), ('lg_scene_gather', dict(first=3), 'first + B - 1 must lie inside'),
    ('lg_scene_gather', dict(o_ms=Q), '16-byte aligned'),
    ('lg_scene_blend', dict(C=17), 'C must be in 1 .. 16'), ('lg_scene_blend', dict(W=65540), 'H and W must be multiples of 4 in 16 .. 65536'),
    ('lg_scene_blend', dict(overlap=12), 'overlap'), ('lg_scene_blend', dict(first=15), 'first + B - 1 must lie inside the grid'),
    ('lg_scene_blend', dict(scene=Q), '16-byte aligned'),
    ('lg_scene_to_u16', dict(n=6), 'multiple of 4'), ('lg_scene_to_u16', dict(n=0), 'positive multiple of 4'), ('lg_scene_to_u16', dict(src=Q), '16-byte'),
    ('lg_scene_to_u16', dict(dst=Q), '8-byte aligned'),
    ('lg_grad_norm', dict(n_ranges=0), 'n_ranges must be in 1 .. 65535'), ('lg_grad_norm', dict(n_ranges=65536), 'n_ranges must be in 1 .. 65535'),
    ('lg_grad_norm', dict(max_range=0), 'max_range must be positive'), ('lg_grad_norm', dict(workspace=Q), 'workspace must be 8-byte aligned'),
]
HIP_WORDS = ('hip', 'invalid device', 'no rocm', 'illegal', 'launch fail', 'out of memory')


def call_rejected(entry, bad):
    prefix, names, good = ENTRIES[entry]
    names = names.split()
    args = dict(good, stream=NULL)
    assert set(bad) <= set(names) and set(args) == set(names), (entry, bad)
    args.update(bad)
    L().lg_batch_assemble(NULL, NULL, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, 0, 0, 0, 1.0, 0, 1.0, NULL)     # leaves another entry's message
    rc = getattr(L(), entry)(*[args[n] for n in names])
    return rc, L().lg_last_error().decode(), prefix


@pytest.mark.parametrize('entry,bad,says', REJECTED, ids=[f'{e}-{"-".join(f"{k}={v}" for k, v in b.items())}' for e, b, _ in REJECTED])
def test_one_argument_outside_its_range_is_rejected_by_name(entry, bad, says):
    rc, msg, prefix = call_rejected(entry, bad)
    assert rc < 0, (entry, bad, rc, msg)
    assert msg.startswith(prefix + ':'), (entry, bad, msg)
    assert says in msg, (entry, bad, msg)
    assert not any(w in msg.lower() for w in HIP_WORDS), (entry, bad, msg)


def test_every_listed_entry_has_its_b_range_and_a_shape_case():
    seen = {}
    for e, bad, _ in REJECTED:
        seen.setdefault(e, set()).update(bad)
    assert set(seen) == set(ENTRIES)
    for e in B_ENTRIES:
        assert 'B' in seen[e] and len(seen[e]) >= 3, (e, seen[e])
    assert len(B_ENTRIES) == 18                 # the six classical calls (lg_mtf_glp's three modes and lg_bdsd's two forms share theirs) and the twelve others


# ------------------------------------------------------------------------------------------------------------------------
# sizers: one step inside the range is sized, one step outside is 0
# ------------------------------------------------------------------------------------------------------------------------
def classical_sizers():
    """name -> f(B, C, h, w) at fixed further arguments"""
    lib = L()
    return {
        'classical/sfim': lambda B, C, h, w: lib.lg_classical_workspace_bytes(B, C, h, w, _lib.LG_CLASSICAL_SFIM),
        'classical/gsa': lambda B, C, h, w: lib.lg_classical_workspace_bytes(B, C, h, w, _lib.LG_CLASSICAL_GSA),
        'mtfglp/glp': lambda B, C, h, w: lib.lg_mtfglp_workspace_bytes(B, C, h, w, 1, _lib.LG_MTFGLP_GLP),
        'mtfglp/cbd per band': lambda B, C, h, w: lib.lg_mtfglp_workspace_bytes(B, C, h, w, C, _lib.LG_MTFGLP_CBD),
        'bdsd/global': lambda B, C, h, w: lib.lg_bdsd_workspace_bytes(B, C, h, w, 0),
        'bdsd/32': lambda B, C, h, w: lib.lg_bdsd_workspace_bytes(B, C, h, w, 32),
    }


def image_sizers():
    """name -> (f(B, C, H, W), C range, smallest side, largest side, step of the sides)"""
    lib = L()
    return {
        'iqa/ref': (lambda B, C, H, W: lib.lg_iqa_workspace_bytes(B, C, H, W, 0), (2, 16), 11, 8192, 1),
        'iqa/no_ref': (lambda B, C, H, W: lib.lg_iqa_workspace_bytes(B, C, H, W, 1), (2, 16), 32, 8192, 4),
        'iqa_ext': (lambda B, C, H, W: lib.lg_iqa_ext_workspace_bytes(B, C, H, W), (2, 8), 32, 8192, 1),
        'qnr': (lambda B, C, H, W: lib.lg_qnr_workspace_bytes(B, C, H, W), (4, 8), 8, 65536, 4),
        'recloss': (lambda B, C, H, W: lib.lg_recloss_workspace_bytes(B, C, H, W), (4, 8), 4, 65536, 4),
    }


def test_sizers_accept_the_last_value_inside_and_return_zero_outside():
    for name, f in classical_sizers().items():
        small = 8 if name == 'bdsd/32' else 4                        # block 32 has to divide 4 h and 4 w
        for B, C, h, w in ((1, 2, small, small), (65535, 2, small, small), (1, 16, 4096, 4096), (65535, 16, 4096, 4096), (1, 2, small, 4096), (1, 2, 4096, small)):
            assert f(B, C, h, w) > 0, (name, B, C, h, w)
        for B, C, h, w in ((0, 4, 8, 8), (65536, 4, 8, 8), (2, 1, 8, 8), (2, 17, 8, 8), (2, 4, 3, 8), (2, 4, 8, 3), (2, 4, 4097, 8), (2, 4, 8, 4097)):
            assert f(B, C, h, w) == 0, (name, B, C, h, w)
    for name, (f, (c0, c1), lo, hi, step) in image_sizers().items():
        for B, C, H, W in ((1, c0, lo, lo), (65535, c0, lo, lo), (1, c1, hi, hi), (65535, c1, hi, hi), (1, c0, lo, hi), (1, c0, hi, lo)):
            assert f(B, C, H, W) > 0, (name, B, C, H, W)
        outside = [(0, c0, lo, lo), (65536, c0, lo, lo), (2, c0 - 1, lo, lo), (2, c1 + 1, lo, lo), (2, c0, hi + step, lo), (2, c0, lo, hi + step)]
        if name != 'recloss':                                        # lg_sam_loss takes any H >= 1 and W >= 4; below that the next line
            outside += [(2, c0, lo - step, lo), (2, c0, lo, lo - step)]
        for B, C, H, W in outside:
            assert f(B, C, H, W) == 0, (name, B, C, H, W)
    rl = image_sizers()['recloss'][0]
    assert rl(2, 4, 0, 4) == 0 and rl(2, 4, 1, 0) == 0 and rl(2, 4, 1, 6) == 0
    gn = L().lg_grad_norm_workspace_bytes
    assert gn(1, 1) > 0 and gn(65535, 1 << 40) > 0 and gn(0, 8) == 0 and gn(65536, 8) == 0 and gn(8, 0) == 0


BS = (1, 2, 3, 255, 256, 32768, 65535)


def _non_decreasing(vals):
    return all(a <= b for a, b in zip(vals, vals[1:]))


def all_sizers():
    """name -> (f(B) at the largest accepted shape, [three ladders of f at B = 65535 over the sides])"""
    out = {}
    for name, f in classical_sizers().items():
        sides = [8, 16, 32, 64, 96, 128, 512, 1024, 2048, 4064, 4096]
        out[name] = (lambda B, f=f: f(B, 16, 4096, 4096),
                     lambda f=f, sides=sides: ([f(65535, 16, s, 4096) for s in sides], [f(65535, 16, 4096, s) for s in sides], [f(65535, 16, s, s) for s in sides]))
    for name, (f, (c0, c1), lo, hi, step) in image_sizers().items():
        sides = sorted({lo, lo + step, 32, 36, 64, 128, 256, 1024, 4096, hi - step, hi})
        out[name] = (lambda B, f=f, c1=c1, hi=hi: f(B, c1, hi, hi),
                     lambda f=f, c1=c1, hi=hi, sides=sides: ([f(65535, c1, s, hi) for s in sides], [f(65535, c1, hi, s) for s in sides],
                                                             [f(65535, c1, s, s) for s in sides]))
    gn = L().lg_grad_norm_workspace_bytes                      # no batch: its two counts take the batch's place
    out['grad_norm'] = (lambda n: gn(n, 1 << 40), lambda: ([gn(65535, 1 << k) for k in range(0, 48, 4)],))
    return out


SIZER_NAMES = ('classical/sfim', 'classical/gsa', 'mtfglp/glp', 'mtfglp/cbd per band', 'bdsd/global', 'bdsd/32', 'iqa/ref', 'iqa/no_ref', 'iqa_ext', 'qnr',
               'recloss', 'grad_norm')


@pytest.mark.parametrize('name', SIZER_NAMES)
def test_sizers_never_shrink_with_the_batch_or_with_the_sides(name):
    """at the largest accepted shape over B in {1, 2, 3, 255, 256, 32768, 65535}, and over the sides at B = 65535"""
    at_b, ladders = all_sizers()[name]
    top = [at_b(B) for B in BS]
    assert top[0] > 0 and _non_decreasing(top), (name, top)
    for vals in ladders():
        assert vals[0] > 0 and _non_decreasing(vals), (name, vals)


@pytest.mark.parametrize('name', SIZER_NAMES)
def test_the_largest_batch_needs_65535_over_2_times_what_two_samples_need(name):
    """the value at (65535, largest shape) is at least 65535 / 2 times the value at B = 2: a 32-bit product breaks this.

    This case found the one thing the file found.  ws_layout (csrc/reduce.h) starts every region of a workspace on a 256-byte boundary, so a region's
    end used to round up by as many as 255 bytes whatever B was: a visible share of a two-sample workspace (lg_sfim's coefficients: 2 x 49 doubles =
    784 bytes took 1024), nothing at B = 65535, and the quotient of the two totals fell below 32767.5 for six sizers -- classical/sfim 32711.44,
    classical/gsa 32761.89, mtfglp/glp 32767.47, mtfglp/cbd per band 32767.4996, iqa_ext 32767.46, qnr 32735.88 -- though no product had wrapped.
    Those four size functions now reserve every sample's share of a region in whole 128-byte units (ws_region): two samples fill whole 256-byte
    lines, the total is proportional to B from B = 2 on, and all twelve quotients are 32767.50.  The kernels index as before; workspaces grow by at
    most 127 bytes per sample and region."""
    at_b = all_sizers()[name][0]
    two, top = at_b(2), at_b(65535)
    print(f'{name}: B = 2 {two} bytes, B = 65535 {top} bytes, ratio {top / two:.2f} (65535 / 2 = 32767.5)')
    assert top * 2 >= 65535 * two, (name, two, top)


def test_fake_pointers_are_what_the_docstring_says():
    assert P % 4096 == 0 and PW % 4096 == 0 and Q % 8 == 4 and ctypes.sizeof(ctypes.c_void_p) == 8
