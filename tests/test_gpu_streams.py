"""-m gpu: the stream contract of include/lgteun_hip.h -- "all work is enqueued on `stream`", "calls on different streams do not interact" -- which
the rest of the suite cannot see: it runs on torch's current default stream, where everything is ordered by construction.

A. every C entry that takes a stream, by the late-input protocol of tests/stream_helpers.py (one case per entry at the smallest shape its own
   test file uses), one case through Engine.train_step with deferred dead stages (its own side stream included), and one control that hands
   lg_interp23_up4 the null stream: the protocol must see it.
B. two streams, one host thread: two independent trainings through the C ABI enqueued call by call in turns, 130 lg_l2_loss launches over the
   64-slot ring, and the Python wrappers of the classical methods, same method and shape on two streams with different data.
D. a second device in the same process (skipped on a box with one GPU).

Every case prints `[streams] ...` lines: the calibrated sleep, the host time of its warm call and the longest so far.
Measured on an MI355X (the whole file 10.5 s, the slowest test 1.6 s, D skipped: one GPU in the process): calibrated sleep 99.6 ms; host time of a
warm call 0.004 - 0.35 ms (lgteun_forward 0.18, lgteun_backward with its forward 0.31, the split step of lgteun_dead_forward 0.35, Engine.train_step
0.42; one outlier of 0.73 ms on a 0.012 ms call), so the sleep is 130 times the longest.  Every late run equals its quiet run with the event still
pending; the control differs.
Found: the Python wrappers of the classical methods (classical.py, mtf_glp.py, bdsd.py, cs.py) kept ONE scratch buffer per (device, method, shape) in a
module-level dict, whatever the stream.  On two streams, outputs that differ from their quiet result out of 40: mtf_glp 'glp' 38, 'hpm' 39, 'cbd' 39,
cs.fuse 'pca' 17 (sfim, gsa, bdsd and the other three cs modes 0 in that run: their passes did not happen to interleave).  The wrappers now take their
scratch per call from torch's caching allocator, which never hands a block to two streams: 0 of 40 for all eleven.  No entry of the C ABI was found
on a wrong stream, waiting for the device on a warm call, or racing under four threads."""
import ctypes
import time

import numpy as np
import pytest
import torch

import mtf_glp_ref as mr
import qnr_helpers as qh
import stream_helpers as sh
from gpu_helpers import make_module
from lgteun_amd import _lib, bdsd, classical, cs, mtf_glp
from lgteun_amd import scene as sc
from oracle import detweights as dw
from stream_helpers import Case, L, handle, ptr, uniform

pytestmark = pytest.mark.gpu

F = _lib
U16 = _lib.LG_DT_U16
DIV = 2047.5
POST = float(np.float32(1.0) / np.float32(DIV))
C, K, H, W, B = 4, 2, 32, 32, 2              # the network cases: faithful mode, dropout on
NET_FLAGS = sh.NET_FLAGS
SEED = 0x5EED
f64, i16, i32 = torch.float64, torch.int16, torch.int32


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """if the device reports an error behind a case, the session ends there: nothing more is launched on a card that may have faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'the device reports an error behind this test; nothing more is launched: {e}', returncode=3)


@pytest.fixture(scope='module')
def net():
    m = make_module(C, K)
    eng = m.engine()
    return m, eng, eng.plan(H, W)


def rand_i16(shape, seed, mask=0x07FF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 65536, shape, generator=g, dtype=torch.int32) & mask).to(i16)


def inp_i16(case, shape, seed):
    return case.inp(rand_i16(shape, seed), rand_i16(shape, seed + 1))


def accum(case, n=1):
    """a scalar (or buffer) an entry adds into: zeros in the true run, 0.25 in the decoy"""
    return case.inp(torch.zeros(n), torch.full((n,), 0.25), inout=True)


def net_inputs(case, seed=5):
    """ms, pan, gt / dout on the device: the smooth fields of the oracle's input maker, the decoy from another seed"""
    t, d = dw.make_inputs(B, C, H // 4, W // 4, seed=seed, kind='smooth'), dw.make_inputs(B, C, H // 4, W // 4, seed=seed + 1, kind='smooth')
    return [case.inp(torch.from_numpy(a), torch.from_numpy(b)) for a, b in zip(t, d)]


def net_params(case, eng):
    return case.inp(eng.flat.detach().clone(), eng.flat.detach() * 0.9)


# ========================================================================================================================
# A. the cases: name -> builder(net fixture) -> Case
# ========================================================================================================================
CASES = {}


def case(name):
    def deco(f):
        CASES[name] = f
        return f
    return deco


@case('lgteun_forward')
def _(net):
    _, eng, plan = net
    c = Case('lgteun_forward')
    p = net_params(c, eng)
    ms, pan, _ = net_inputs(c)
    out = c.out(B, C, H, W)
    ws, nb = c.ws(L().lg_workspace_bytes(plan, B, 1))
    c.call = lambda s: L().lgteun_forward(plan, ptr(p), ptr(ms), ptr(pan), ptr(out), ptr(ws), nb, B, NET_FLAGS, SEED, s)
    return c


@case('lgteun_backward')
def _(net):
    """forward with LG_FLAG_SAVE, then the backward, on one workspace and one gradient buffer in every run (the reduce-image cache key holds both pointers)"""
    _, eng, plan = net
    c = Case('lgteun_backward')
    p = net_params(c, eng)
    ms, pan, dout = net_inputs(c)
    grads = accum(c, eng.total)
    out = c.out(B, C, H, W)
    ws, nb = c.ws(L().lg_workspace_bytes(plan, B, 1))
    c.call = lambda s: [L().lgteun_forward(plan, ptr(p), ptr(ms), ptr(pan), ptr(out), ptr(ws), nb, B, NET_FLAGS, SEED, s),
                        L().lgteun_backward(plan, ptr(p), ptr(grads), ptr(ms), ptr(pan), ptr(dout), ptr(ws), nb, B, NET_FLAGS, SEED, s)]
    return c


@case('lgteun_dead_forward')
def _(net):
    """the split step: forward with LG_FLAG_DEFER_DEAD, the LGT backward, the dead-stage forward, the data-step backward; the discarded LGT
    output (lg_workspace_deadout) counts as an output"""
    _, eng, plan = net
    c = Case('lgteun_dead_forward')
    p = net_params(c, eng)
    ms, pan, dout = net_inputs(c)
    grads = accum(c, eng.total)
    out = c.out(B, C, H, W)
    ws, nb = c.ws(L().lg_workspace_bytes(plan, B, 1))
    off, stride = ctypes.c_size_t(), ctypes.c_size_t()
    assert L().lg_workspace_deadout(plan, B, 1, ctypes.byref(off), ctypes.byref(stride)) == 0
    n_dead = (K - 1 if stride.value else 1) * B * C * H * W * 4
    assert off.value + n_dead <= nb
    c.watch(ws.view(torch.uint8)[off.value:off.value + n_dead])
    fl = NET_FLAGS | F.LG_FLAG_DEFER_DEAD
    c.call = lambda s: [L().lgteun_forward(plan, ptr(p), ptr(ms), ptr(pan), ptr(out), ptr(ws), nb, B, fl, SEED, s),
                        L().lgteun_backward(plan, ptr(p), ptr(grads), ptr(ms), ptr(pan), ptr(dout), ptr(ws), nb, B, fl | F.LG_FLAG_BWD_LGT, SEED, s),
                        L().lgteun_dead_forward(plan, ptr(p), ptr(ws), nb, B, fl, SEED, s),
                        L().lgteun_backward(plan, ptr(p), ptr(grads), ptr(ms), ptr(pan), ptr(dout), ptr(ws), nb, B, fl | F.LG_FLAG_BWD_DATA, SEED, s)]
    return c


def _flat_loss(name, fn):
    """n = 1003 elements: one workgroup, so lg_l1_loss's float atomic repeats its bits; a tail that is no multiple of 4"""
    @case(name)
    def _(net):
        c, n = Case(name), 1003
        out, gt = c.rand((n,), 11), c.rand((n,), 13)
        loss = accum(c)
        dout = c.out(n)
        c.call = lambda s: getattr(L(), fn)(ptr(out), ptr(gt), ptr(dout), ptr(loss), n, n, 1.0, s)
        return c


_flat_loss('lg_l1_loss', 'lg_l1_loss')
_flat_loss('lg_l2_loss', 'lg_l2_loss')


def _rec_loss(name):
    @case(name)
    def _(net):
        c, h, w = Case(name), 11, 12
        out, gt = c.rand((B, C, h, w), 21), c.rand((B, C, h, w), 23)
        loss = accum(c)
        dout = c.out(B, C, h, w)
        ws, nb = c.ws(L().lg_recloss_workspace_bytes(B, C, h, w))
        if name == 'lg_sam_loss':
            c.call = lambda s: L().lg_sam_loss(ptr(out), ptr(gt), ptr(dout), ptr(loss), B, B, C, h, w, 1.0, 0, ptr(ws), nb, s)
        else:
            c.call = lambda s: L().lg_ssim_loss(ptr(out), ptr(gt), ptr(dout), ptr(loss), B, B, C, h, w, 1.0, 1.0, 0, ptr(ws), nb, s)
        return c


_rec_loss('lg_sam_loss')
_rec_loss('lg_ssim_loss')


def _optim(name):
    @case(name)
    def _(net):
        _, eng, _ = net
        c, n = Case(name), eng.total
        p = c.rand((n,), 31, -0.5, 0.5, inout=True)
        g = c.rand((n,), 33, -0.1, 0.1)
        m = c.rand((n,), 35, -0.01, 0.01, inout=True)
        v = c.rand((n,), 37, 1e-5, 1e-3, inout=True)
        rg, nr, mx = eng.ranges_dev, len(eng.live_ranges), eng.max_range
        if name == 'lg_adam_step':
            c.call = lambda s: L().lg_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(rg), nr, mx, 3, 1.5e-3, 0.9, 0.999, 1e-8, 1.0, s)
        elif name == 'lg_optim_step':
            c.call = lambda s: L().lg_optim_step(ptr(p), ptr(g), ptr(m), ptr(v), None, ptr(rg), nr, mx, 3, F.LG_OPT_ADAMW, 0, 1.5e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, s)
        else:
            clip = c.inp(torch.tensor([0.5]), torch.tensor([1.0]))
            ema = c.rand((n,), 39, -0.5, 0.5, inout=True)
            c.call = lambda s: L().lg_optim_step_ex(ptr(p), ptr(g), ptr(m), ptr(v), None, ptr(rg), nr, mx, 3, F.LG_OPT_ADAMW, 0, 1.5e-3, 0.9, 0.999, 1e-8, 1e-2,
                                                    1.0, ptr(clip), ptr(ema), 0.99, 0, s)
        return c


for _n in ('lg_adam_step', 'lg_optim_step', 'lg_optim_step_ex'):
    _optim(_n)


@case('lg_grad_norm')
def _(net):
    _, eng, _ = net
    c = Case('lg_grad_norm')
    g = c.rand((eng.total,), 41, -0.1, 0.1)
    rg, nr, mx = eng.ranges_dev, len(eng.live_ranges), eng.max_range
    out = c.out(2)
    ws, nb = c.ws(L().lg_grad_norm_workspace_bytes(nr, mx))
    c.call = lambda s: L().lg_grad_norm(ptr(g), ptr(rg), nr, mx, 1.0, ptr(out), ptr(ws), nb, s)
    return c


@case('lg_dropout_mask')
def _(net):
    """no input: a launch on another stream is caught by the fill that the side stream puts over the output behind the sleep"""
    c, n = Case('lg_dropout_mask'), 1000
    out = c.out(n)
    c.call = lambda s: L().lg_dropout_mask(SEED, 1, 2, 5, n, ptr(out), s)
    return c


# ---- the per-op entries ----
@case('lg_op_resample')
def _(net):
    c = Case('lg_op_resample')
    x = c.rand((B * C, 8, 8), 51)
    y = c.out(B * C, 32, 32)
    c.call = lambda s: L().lg_op_resample(ptr(x), ptr(y), B * C, 8, 8, 2, s)
    return c


@case('lg_op_data_step')
def _(net):
    _, eng, plan = net
    c = Case('lg_op_data_step')
    p = net_params(c, eng)
    ms, pan, z = net_inputs(c)
    out = c.out(B, C, H, W)
    tmp = c.out(3 * B * C * H * W // 4 + B * H * W)
    c.call = lambda s: L().lg_op_data_step(plan, ptr(p), 1, ptr(z), ptr(ms), ptr(pan), ptr(out), ptr(tmp), B, s)
    return c


@case('lg_op_data_step_bwd')
def _(net):
    _, eng, plan = net
    c = Case('lg_op_data_step_bwd')
    p = net_params(c, eng)
    ms, pan, z = net_inputs(c)
    dz_out = c.rand((B, C, H, W), 53, -1, 1)
    grads = accum(c, eng.total)
    dz = c.out(B, C, H, W)
    ws, nb = c.ws(L().lg_workspace_bytes(plan, B, 1))
    c.call = lambda s: L().lg_op_data_step_bwd(plan, ptr(p), ptr(grads), 1, ptr(z), ptr(ms), ptr(pan), ptr(dz_out), ptr(dz), ptr(ws), nb, B, s)
    return c


def _lgt(name):
    @case(name)
    def _(net):
        _, eng, plan = net
        c = Case(name)
        p = net_params(c, eng)
        z = c.rand((B, C, H, W), 55)
        out = c.out(B, C, H, W)
        train = name == 'lg_op_lgt_bwd'
        ws, nb = c.ws(L().lg_workspace_bytes(plan, B, int(train)))
        if name == 'lg_op_lgt':
            c.call = lambda s: L().lg_op_lgt(plan, ptr(p), 1, ptr(z), ptr(out), ptr(ws), nb, B, F.LG_FLAG_DROPOUT, SEED, s)
        elif name == 'lg_op_lgt_stages':
            c.call = lambda s: L().lg_op_lgt_stages(plan, ptr(p), 0, 1, ptr(z), ptr(out), ptr(ws), nb, B, F.LG_FLAG_DROPOUT, SEED, 0, s)
        else:
            dout = c.rand((B, C, H, W), 57, -1, 1)
            grads = accum(c, eng.total)
            c.call = lambda s: L().lg_op_lgt_bwd(plan, ptr(p), ptr(grads), 1, ptr(z), ptr(dout), ptr(out), ptr(ws), nb, B, F.LG_FLAG_DROPOUT, SEED, s)
        return c


for _n in ('lg_op_lgt', 'lg_op_lgt_stages', 'lg_op_lgt_bwd'):
    _lgt(_n)


def _block(which, blk, bwd):
    """which 0: the FFT mixer (planar output), 1: the local mixer half-block, 2: the FFN half-block; blk 0 is level 0 (e = 4C at H x W), blk 2 level 1"""
    name = f'lg_op_block{"_bwd" if bwd else ""}[which={which},blk={blk}]'

    @case(name)
    def _(net):
        _, eng, plan = net
        c = Case(name)
        h, w, e = (H, W, 4 * C) if blk in (0, 1, 3, 4) else (H // 2, W // 2, 8 * C)
        p = net_params(c, eng)
        x = c.rand((B, h, w, e), 61 + which, -1, 1)
        yshape = (B, e // 2, h, w) if which == 0 else (B, h, w, e)
        y = c.out(*yshape)
        ws, nb = c.ws(L().lg_workspace_bytes(plan, B, int(bwd)))
        if not bwd:
            c.call = lambda s: L().lg_op_block(plan, ptr(p), 1, blk, which, ptr(x), ptr(y), ptr(ws), nb, B, s)
        else:
            dy = c.rand(yshape, 67 + which, -1, 1)
            grads = accum(c, eng.total)
            c.call = lambda s: L().lg_op_block_bwd(plan, ptr(p), ptr(grads), 1, blk, which, ptr(x), ptr(dy), ptr(y), ptr(ws), nb, B, s)
        return c


for _which, _blk in ((0, 0), (1, 0), (2, 0), (0, 2)):
    _block(_which, _blk, False)
    _block(_which, _blk, True)


# ---- the classical methods: C = 4, 5 x 7, B = 2 ----
CH, CW = 5, 7


def classical_inputs(c, h=CH, w=CW, seed=3):
    (ms, pan), (ms_d, pan_d) = sh.classical_scene(B, C, h, w, seed), sh.classical_scene(B, C, h, w, seed + 1)
    return c.inp(ms, ms_d), c.inp(pan, pan_d)


def _classical(name, h=CH, w=CW, **kw):
    @case(name)
    def _(net):
        c = Case(name)
        ms, pan = classical_inputs(c, h, w)
        out = c.out(B, C, 4 * h, 4 * w)
        lib = L()
        entry = name.split('[')[0]
        if entry == 'lg_interp23_up4':
            c.call = lambda s: lib.lg_interp23_up4(ptr(ms), ptr(out), B, C, h, w, s)
        elif entry == 'lg_wavelet':
            c.call = lambda s: lib.lg_wavelet(ptr(ms), ptr(pan), ptr(out), B, C, h, w, s)
        elif entry == 'lg_sfim':
            ws, nb = c.ws(lib.lg_classical_workspace_bytes(B, C, h, w, F.LG_CLASSICAL_SFIM))
            c.call = lambda s: lib.lg_sfim(ptr(ms), ptr(pan), ptr(out), B, C, h, w, ptr(ws), nb, s)
        elif entry == 'lg_gsa':
            ws, nb = c.ws(lib.lg_classical_workspace_bytes(B, C, h, w, F.LG_CLASSICAL_GSA))
            stats = c.out(B, 2 * C + 1, dtype=f64)
            c.call = lambda s: lib.lg_gsa(ptr(ms), ptr(pan), ptr(out), ptr(stats), B, C, h, w, ptr(ws), nb, s)
        elif entry == 'lg_mtf_glp':
            mode = kw['mode']
            taps = c.const(torch.from_numpy(mr.taps(0.3)[None]))
            ws, nb = c.ws(lib.lg_mtfglp_workspace_bytes(B, C, h, w, 1, mode))
            stats = c.out(B, 2 * C, dtype=f64)
            c.call = lambda s: lib.lg_mtf_glp(ptr(ms), ptr(pan), ptr(out), ptr(stats), ptr(taps), 1, 41, mode, B, C, h, w, ptr(ws), nb, s)
        elif entry == 'lg_bdsd':
            blk = kw['block']
            taps_ms, taps_pan = c.const(torch.from_numpy(mr.taps(0.3)[None])), c.const(torch.from_numpy(mr.taps(0.15)[None]))
            ws, nb = c.ws(lib.lg_bdsd_workspace_bytes(B, C, h, w, blk))
            stats = c.out(B, (4 * h // blk) * (4 * w // blk) if blk else 1, C, C + 1, dtype=f64)
            c.call = lambda s: lib.lg_bdsd(ptr(ms), ptr(pan), ptr(out), ptr(stats), ptr(taps_ms), 1, ptr(taps_pan), 41, blk, B, C, h, w, ptr(ws), nb, s)
        else:
            mode = kw['mode']
            ws, nb = c.ws(lib.lg_cs_workspace_bytes(B, C, h, w))
            stats = c.out(B, 2 * C + 2, dtype=f64)
            c.call = lambda s: lib.lg_cs(ptr(ms), ptr(pan), ptr(out), ptr(stats), None, mode, B, C, h, w, ptr(ws), nb, s)
        return c


for _n in ('lg_interp23_up4', 'lg_sfim', 'lg_gsa', 'lg_wavelet'):
    _classical(_n)
for _m, _code in (('glp', F.LG_MTFGLP_GLP), ('hpm', F.LG_MTFGLP_HPM), ('cbd', F.LG_MTFGLP_CBD)):
    _classical(f'lg_mtf_glp[{_m}]', mode=_code)
_classical('lg_bdsd[global]', block=0)
_classical('lg_bdsd[block=32]', h=8, w=8, block=32)
for _m, _code in (('ihs', F.LG_CS_IHS), ('brovey', F.LG_CS_BROVEY), ('gs', F.LG_CS_GS), ('pca', F.LG_CS_PCA)):
    _classical(f'lg_cs[{_m}]', mode=_code)


# ---- the metrics and QNR ----
def _iqa(name, side):
    @case(name)
    def _(net):
        c, lib = Case(name), L()
        pred, gt = c.rand((B, C, side, side), 71), c.rand((B, C, side, side), 73)
        if name == 'lg_iqa_ref':
            out = c.out(B, 5, dtype=f64)
            ws, nb = c.ws(lib.lg_iqa_workspace_bytes(B, C, side, side, 0))
            c.call = lambda s: lib.lg_iqa_ref(ptr(pred), ptr(gt), ptr(out), B, C, side, side, DIV, ptr(ws), nb, s)
        elif name == 'lg_iqa_no_ref':
            pan, ms = c.rand((B, 1, side, side), 75), c.rand((B, C, side // 4, side // 4), 77)
            out = c.out(B, 3, dtype=f64)
            ws, nb = c.ws(lib.lg_iqa_workspace_bytes(B, C, side, side, 1))
            c.call = lambda s: lib.lg_iqa_no_ref(ptr(pred), ptr(pan), ptr(ms), ptr(out), B, C, side, side, DIV, ptr(ws), nb, s)
        else:
            k = 3 if name == 'lg_iqa_ref_ext' else 1
            out = c.out(B, k, dtype=f64)
            ws, nb = c.ws(lib.lg_iqa_ext_workspace_bytes(B, C, side, side))
            c.call = lambda s: getattr(lib, name)(ptr(pred), ptr(gt), ptr(out), B, C, side, side, DIV, ptr(ws), nb, s)
        return c


_iqa('lg_iqa_ref', 16)
_iqa('lg_iqa_no_ref', 32)
_iqa('lg_iqa_ref_ext', 32)
_iqa('lg_iqa_q2n', 32)


def _qnr(name):
    @case(name)
    def _(net):
        """lg_qnr_grad reads what lg_qnr_stats left in the workspace, so its case is the pair; lg_qnr_stats also stands alone"""
        c, lib, hq = Case(name), L(), 8
        x = [c.inp(t, d) for t, d in zip(qh.make_inputs(B, C, hq, hq, seed=81), qh.make_inputs(B, C, hq, hq, seed=82))]
        P = C * (C - 1) // 2 + C
        q, table = c.out(B, 2, P, dtype=f64), c.out(P, dtype=f64)
        ws, nb = c.ws(lib.lg_qnr_workspace_bytes(B, C, hq, hq))
        stats = lambda s: lib.lg_qnr_stats(*[ptr(t) for t in x], ptr(q), ptr(table), B, C, hq, hq, ptr(ws), nb, s)        # noqa: E731
        if name == 'lg_qnr_stats':
            c.call = stats
        else:
            dout, ind = c.out(B, C, hq, hq), c.out(3, dtype=f64)
            loss = accum(c)
            c.call = lambda s: [stats(s), lib.lg_qnr_grad(ptr(x[0]), ptr(x[1]), ptr(table), ptr(dout), ptr(loss), ptr(ind), B, B, C, hq, hq, 1.0, 0, ptr(ws), nb, s)]
        return c


_qnr('lg_qnr_stats')
_qnr('lg_qnr_grad')


# ---- data preparation ----
@case('lg_pyr_down2')
def _(net):
    c = Case('lg_pyr_down2')
    pan = inp_i16(c, (3, 8, 8), 91)
    out = c.out(3, 2, 2)
    c.call = lambda s: L().lg_pyr_down2(ptr(pan), ptr(out), 3, 8, 8, U16, s)
    return c


@case('lg_fir_decimate4')
def _(net):
    c = Case('lg_fir_decimate4')
    x = inp_i16(c, (3, 8, 8), 93)
    taps = c.const(torch.from_numpy(np.stack([mr.taps(g) for g in (0.3, 0.25, 0.2)])))
    out = c.out(3, 2, 2)
    c.call = lambda s: L().lg_fir_decimate4(ptr(x), ptr(out), ptr(taps), 3, 8, 8, 41, 2, U16, 1, s)
    return c


@case('lg_batch_assemble')
def _(net):
    c, N, hh = Case('lg_batch_assemble'), 5, 8
    pan, lr, mul = inp_i16(c, (N, 1, hh, hh), 95), inp_i16(c, (N, C, 2, 2), 97), inp_i16(c, (N, C, hh, hh), 99)
    pan_l = c.rand((N, 1, 2, 2), 101, 0, 2047)
    idx = c.const(torch.tensor([3, 1], dtype=i32))
    flips = c.const(torch.tensor([2], dtype=i32))
    o = [c.out(B, 1, hh, hh), c.out(B, C, 2, 2), c.out(B, C, hh, hh), c.out(B, 1, 2, 2)]
    c.call = lambda s: L().lg_batch_assemble(ptr(pan), ptr(lr), ptr(mul), ptr(pan_l), N, ptr(idx), 0, ptr(flips), *[ptr(t) for t in o], B, C, hh, hh, 2, 2, U16,
                                             DIV, 1, POST, s)
    return c


@case('lg_window_assemble')
def _(net):
    c, S, P = Case('lg_window_assemble'), 64, 8
    pan, lr, mul = inp_i16(c, (1, S, S), 103), inp_i16(c, (C, S // 4, S // 4), 105), inp_i16(c, (C, S, S), 107)
    org = c.const(torch.tensor([[4, 12], [56, 0], [20, 40]], dtype=i32))
    flips = c.const(torch.tensor([1], dtype=i32))
    o = [c.out(B, 1, P, P), c.out(B, C, P // 4, P // 4), c.out(B, C, P, P), c.out(B, 1, P // 4, P // 4)]
    c.call = lambda s: L().lg_window_assemble(ptr(pan), ptr(lr), ptr(mul), ptr(org), 3, 1, ptr(flips), *[ptr(t) for t in o], B, C, S, S, P, P, U16, DIV, 1, POST, s)
    return c


# ---- the scene entries ----
@case('lg_scene_gather')
def _(net):
    c, S, t = Case('lg_scene_gather'), 64, 16
    pan, ms = inp_i16(c, (1, S, S), 109), inp_i16(c, (C, S // 4, S // 4), 111)
    org = c.const(torch.tensor([[0, 0], [48, 16], [12, 44]], dtype=i32))
    o_pan, o_ms = c.out(B, 1, t, t), c.out(B, C, t // 4, t // 4)
    c.call = lambda s: L().lg_scene_gather(ptr(pan), ptr(ms), ptr(org), 3, 1, ptr(o_pan), ptr(o_ms), B, C, S, S, t, t, U16, DIV, 1, POST, s)
    return c


@case('lg_scene_blend')
def _(net):
    """every tile of the 5 x 5 grid of a 64 x 64 scene (tiles 16 x 16, overlap 4) in one launch"""
    c, S, t, ov = Case('lg_scene_blend'), 64, 16, 4
    ys, xs = sc.tile_grid(S, S, t, ov)
    n = len(ys) * len(xs)
    tiles = c.rand((n, C, t, t), 113)
    scene = c.out(C, S, S)
    c.call = lambda s: L().lg_scene_blend(ptr(tiles), ptr(scene), 0, n, C, S, S, t, t, ov, s)
    return c


@case('lg_scene_to_u16')
def _(net):
    c, n = Case('lg_scene_to_u16'), 1000
    src = c.rand((n,), 115, -0.1, 1.1)
    dst = c.out(n, dtype=i16)
    c.call = lambda s: L().lg_scene_to_u16(ptr(src), ptr(dst), n, DIV, s)
    return c


@pytest.mark.parametrize('name', list(CASES))
def test_entry_enqueues_on_the_stream_it_is_given(name, net):
    sh.check_entry_runs_on_its_stream(CASES[name](net))


def test_every_entry_with_a_stream_argument_has_a_case():
    """the binding's table of signatures: an entry of five or more arguments whose last one is a void* takes a stream there (the sizers end in an
    integer, the host-only entries in a typed pointer) -- every one of them has a case above, and no case names anything else"""
    with_stream = {n for n, (_, args) in _lib.SIGNATURES.items() if len(args) >= 5 and args[-1] is ctypes.c_void_p}
    assert len(with_stream) == 40, sorted(with_stream)
    covered = {n.split('[')[0] for n in CASES}
    assert with_stream == covered, sorted(with_stream ^ covered)


def test_control_a_launch_on_the_null_stream_is_seen(net):
    """the protocol can see a wrong stream: lg_interp23_up4 handed the null stream's handle while the side stream sleeps in front of the late copy runs at
    once, on the decoy, and the side stream's fill lands on what it wrote.  Reads and writes only the case's own buffers."""
    c = CASES['lg_interp23_up4'](net)
    c.quiet()
    r0, _ = c.quiet()
    s, = sh.side_streams(1)
    r1, _, pending = c.late(s, call_stream=ctypes.c_void_p(0))
    assert pending
    assert sh.same(r0, r1) == [0], 'the late run equals the quiet one although its launch went to the null stream'
    c.guards_intact()


def test_engine_train_step_with_deferred_dead_stages():
    """Engine.train_step in faithful mode with overlap_dead: forward with LG_FLAG_DEFER_DEAD, l1 loss, the LGT backward, the dead-stage forwards on the
    engine's own side stream, the data-step backward, Adam.  Everything the step enqueues follows torch's current stream, so under torch.cuda.stream(s)
    it must wait behind s's sleep for the late inputs, the side stream's part included."""
    import lgteun_amd
    m = make_module(C, K)
    eng = m.engine()
    eng.overlap_dead = True
    opt = lgteun_amd.FusedAdam(m.parameters(), lr=1.5e-3)
    c = Case('Engine.train_step')
    ms, pan, gt = net_inputs(c)
    flat0 = eng.flat.detach().clone()

    def step():
        eng._seed_ctr = 0
        opt._step = 0
        loss = eng.train_step(ms, pan, gt, opt)
        return loss

    def reset():
        eng.flat.copy_(flat0)
        for t in (opt._state or {}).values():
            t.zero_()

    def results():
        return [sh.bits(t) for t in (eng.flat, eng._gbuf, opt._state['exp_avg'], opt._state['exp_avg_sq'])]

    def quiet():
        torch.cuda.synchronize()
        c._load(decoy=False)
        reset()
        torch.cuda.synchronize()
        step()
        torch.cuda.synchronize()
        return results()
    cold, r0 = quiet(), quiet()
    assert not sh.same(cold[:1] + cold[2:], r0[:1] + r0[2:]), 'two quiet train steps differ in weights or optimizer state'
    s, = sh.side_streams(1)
    with torch.cuda.stream(s):                      # the step's torch.empty calls find blocks in s's pool: no allocation behind the sleep
        warm = [torch.empty_like(gt) for _ in range(4)]
        del warm
    cycles = sh.sleep_cycles()
    torch.cuda.synchronize()
    c._load(decoy=True)
    reset()
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        ev.record()
        for buf, true, _ in c.ins:
            buf.copy_(true, non_blocking=True)
        t0 = time.perf_counter()
        step()
        host_ms = 1e3 * (time.perf_counter() - t0)
        pending = not ev.query()
    s.synchronize()
    torch.cuda.synchronize()
    r1 = results()
    print(f'[streams] Engine.train_step: host {host_ms:.3f} ms; sleep {sh.STATS["sleep_ms"]:.1f} ms')
    assert sh.STATS['sleep_ms'] >= sh.HOST_FACTOR * host_ms, f'the sleep of {sh.STATS["sleep_ms"]:.1f} ms is not 10 times the step\'s host time of {host_ms:.3f} ms'
    assert pending, 'train_step returned only after its stream had passed the sleep'
    # the loss scalar of the step sums |out - gt| of 8192 elements over 8 workgroups with float atomics in the order they arrive: seven adds, each
    # rounding by at most 2^-24 of the total, so two orders differ by at most 14 x 2^-24 of it (16 below).  Weights, gradients and state do not move.
    n = eng.total
    assert torch.equal(r0[1][:4 * n], r1[1][:4 * n]), 'gradients differ from the quiet step'
    assert not sh.same(r0[:1] + r0[2:], r1[:1] + r1[2:]), 'weights or optimizer state differ from the quiet step'
    l0, l1 = r0[1][4 * n:4 * n + 4].view(torch.float32).item(), r1[1][4 * n:4 * n + 4].view(torch.float32).item()
    assert abs(l0 - l1) <= 16 * 2.0 ** -24 * abs(l0), (l0, l1)


# ========================================================================================================================
# B. two streams, one host thread
# ========================================================================================================================
def test_two_trainings_enqueued_in_turns_on_two_streams():
    """two parameter sets, data sets and workspaces; three train steps each (forward, l1 loss, backward, AdamW through lg_optim_step), enqueued call by
    call in turns with no synchronisation in between: weights, optimizer state and losses bitwise those of the two runs done one after the other"""
    steps = 3
    rigs = [sh.TrainRig(salt=k, seed=40 + k, steps=steps) for k in range(2)]
    s = sh.side_streams(2)
    alone = [rig.run_alone(s[k]) for k, rig in enumerate(rigs)]
    again = [rig.run_alone(s[k]) for k, rig in enumerate(rigs)]
    for k in range(2):
        assert not sh.differing(alone[k], again[k]), (k, 'a training alone does not repeat its bits', sh.differing(alone[k], again[k]))
    assert sh.differing(alone[0], alone[1]), 'the two trainings are the same one'
    for rig in rigs:
        rig.reset()
    torch.cuda.synchronize()
    for step in range(steps):
        for f0, f1 in zip(rigs[0].calls(step), rigs[1].calls(step)):
            f0(s[0])
            f1(s[1])
    for st in s:
        st.synchronize()
    for k, rig in enumerate(rigs):
        got = rig.results()
        assert not sh.differing(alone[k], got), (k, 'differs from the run alone', sh.differing(alone[k], got))
        assert bool(torch.isfinite(rig.losses).all()) and bool((rig.losses > 0).all())


def test_l2_loss_slots_over_two_streams():
    """130 lg_l2_loss launches in turns over two streams -- the ring of 64 accumulator slots wraps twice -- n = 4099, a loss scalar per launch: every
    loss and every dout bitwise that of the same launch on one stream"""
    n, launches = 4099, 130
    out = torch.stack([uniform((n + 1,), 200 + k) for k in range(2)]).cuda()       # rows stay 16-byte aligned: 4100 floats
    gt = torch.stack([uniform((n + 1,), 210 + k) for k in range(2)]).cuda()
    scale = [1.0 + 0.01 * i for i in range(launches)]

    def run(streams):
        loss = torch.zeros(launches, device='cuda')
        dout = torch.full((launches, n + 1), float('nan'), device='cuda')
        torch.cuda.synchronize()
        for i in range(launches):
            k = i % 2
            _lib.check(L().lg_l2_loss(ptr(out[k]), ptr(gt[k]), ptr(dout[i]), ptr(loss[i:]), n, n, scale[i], handle(streams[k % len(streams)])), 'lg_l2_loss')
        torch.cuda.synchronize()
        return loss, dout
    s = sh.side_streams(2)
    loss1, dout1 = run(s[:1])
    loss2, dout2 = run(s)
    want = [float(((out[k, :n].double() - gt[k, :n].double()) ** 2).sum() / n) for k in range(2)]
    for i in range(launches):
        assert abs(float(loss1[i]) - want[i % 2]) <= 2.0 ** -23 * want[i % 2], (i, float(loss1[i]), want[i % 2])
    assert torch.equal(loss1.view(torch.int32), loss2.view(torch.int32)), (loss1 != loss2).nonzero().flatten().tolist()
    assert torch.equal(dout1[:, :n].view(torch.int32), dout2[:, :n].view(torch.int32))
    assert bool(torch.isnan(dout2[:, n]).all())


def wrapper_methods():
    return {
        'classical.sfim': classical.sfim, 'classical.gsa': classical.gsa,
        'mtf_glp[glp]': lambda m, p: mtf_glp.mtf_glp(m, p, 'glp'), 'mtf_glp[hpm]': lambda m, p: mtf_glp.mtf_glp(m, p, 'hpm'),
        'mtf_glp[cbd]': lambda m, p: mtf_glp.mtf_glp(m, p, 'cbd'),
        'bdsd[global]': lambda m, p: bdsd.bdsd(m, p), 'bdsd[block=32]': lambda m, p: bdsd.bdsd(m, p, block=32),
        'cs.fuse[ihs]': lambda m, p: cs.fuse(m, p, 'ihs'), 'cs.fuse[brovey]': lambda m, p: cs.fuse(m, p, 'brovey'),
        'cs.fuse[gs]': lambda m, p: cs.fuse(m, p, 'gs'), 'cs.fuse[pca]': lambda m, p: cs.fuse(m, p, 'pca'),
    }


ROUNDS = 20
_scenes = {}


def wrapper_scenes():
    """two different batches at C = 4, 64 x 64 (PAN 256 x 256), B = 2: made once, read only"""
    if not _scenes:
        _scenes['x'] = [sh.classical_scene(2, 4, 64, 64, seed=7 + k) for k in range(2)]
    return _scenes['x']


def wrapper_mismatches(fn):
    """the quiet result of fn on each of the two batches, then ROUNDS rounds of (batch 0 on stream 0, batch 1 on stream 1) with no synchronisation
    between the calls -> how many of the 2 x ROUNDS outputs differ from their quiet result"""
    data = wrapper_scenes()
    s = sh.side_streams(2)
    quiet = []
    for k in range(2):
        with torch.cuda.stream(s[k]):
            quiet.append(fn(*data[k]))
        s[k].synchronize()
    assert not torch.equal(quiet[0], quiet[1])
    torch.cuda.synchronize()
    outs = []
    for _ in range(ROUNDS):
        for k in range(2):
            with torch.cuda.stream(s[k]):
                outs.append((k, fn(*data[k])))
    for st in s:
        st.synchronize()
    torch.cuda.synchronize()
    return sum(0 if torch.equal(o.view(torch.int32), quiet[k].view(torch.int32)) else 1 for k, o in outs)


@pytest.mark.parametrize('method', list(wrapper_methods()))
def test_wrapper_on_two_streams_with_different_data(method):
    """the same method at the same shape on two streams with different data, 20 rounds in turns: every output bitwise its quiet result.  One-sided: it cannot
    fail on correct code.  With the wrappers' former module-level workspace cache (one buffer per shape, whatever the stream) it did fail: the statistics pass
    of one stream overwrote the partial sums and coefficients the other stream's apply pass was about to read."""
    # (before the fix: mtf_glp glp / hpm / cbd 38 / 39 / 39 and cs.fuse pca 17 of 40, the others 0)
    bad = wrapper_mismatches(wrapper_methods()[method])
    print(f'[streams] {method}: {bad} of {2 * ROUNDS} outputs differ from their quiet result')
    assert bad == 0, (method, bad)


# ========================================================================================================================
# D. a second device in the same process
# ========================================================================================================================
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs a second GPU in the process')
def test_second_device_gives_the_bits_of_the_first():
    """device 0 warm, then on device 1 in the same process: the forward, the FFT-mixer op at 128 x 128 (plane in LDS) and 256 x 256 (split path), a
    train step (forward, lg_l2_loss, backward) and lg_gsa -- bitwise device 0's.  The first use of the per-device twiddle upload, LDS-attribute bits and
    reduce-image cache with a device other than 0."""
    def run(dev):
        res = {}
        with torch.cuda.device(dev):
            device = f'cuda:{dev}'
            s = torch.cuda.current_stream()
            rig = sh.TrainRig(salt=0, seed=50, steps=1, device=device)
            rig.reset()
            zero, fwd, _, bwd, _ = rig.calls(0)
            zero(s)
            fwd(s)
            n = rig.out.numel()
            _lib.check(L().lg_l2_loss(ptr(rig.out), ptr(rig.gt), ptr(rig.dout), ptr(rig.losses), n, n, 1.0, handle(s)), 'lg_l2_loss')
            bwd(s)
            torch.cuda.synchronize()
            res.update(out=sh.bits(rig.out), loss=sh.bits(rig.losses), grads=sh.bits(rig.grads))
            for side in (128, 256):
                m = make_module(C, K, device=device)
                eng = m.engine()
                plan = eng.plan(side, side)
                x = uniform((1, side, side, 4 * C), 300 + side, -1, 1).to(device)
                y = torch.empty(1, 2 * C, side, side, device=device)
                nb = int(L().lg_workspace_bytes(plan, 1, 0))
                ws = torch.empty(nb, dtype=torch.uint8, device=device)
                _lib.check(L().lg_op_block(plan, ptr(eng.flat), 0, 0, 0, ptr(x), ptr(y), ptr(ws), nb, 1, handle(s)), 'lg_op_block')
                torch.cuda.synchronize()
                res[f'fft{side}'] = sh.bits(y)
                del m, eng
            ms, pan = sh.classical_scene(2, 4, 5, 7, seed=9, device=device)
            out, stats = torch.empty(2, 4, 20, 28, device=device), torch.empty(2, 9, dtype=f64, device=device)
            ws = torch.empty(int(L().lg_classical_workspace_bytes(2, 4, 5, 7, _lib.LG_CLASSICAL_GSA)) // 8 + 1, dtype=f64, device=device)
            sh.gsa_call(ms, pan, out, stats, ws, s)
            torch.cuda.synchronize()
            res.update(gsa=sh.bits(out), gsa_stats=sh.bits(stats))
        return {k: v.cpu() for k, v in res.items()}
    first, second = run(0), run(1)
    assert not sh.differing(first, second), sh.differing(first, second)
