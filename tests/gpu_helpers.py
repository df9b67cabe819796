"""Helpers for the -m gpu parity tests: build the product module with deterministic weights and call the
C ABI per-op entry points."""
import ctypes

import numpy as np
import torch

import lgteun_amd
from lgteun_amd import _lib
from lgteun_amd.compat import Config
from lgteun_amd.engine import _ptr, _stream_ptr
from oracle import detweights as dw

from helpers import mask_tensor, state_shapes


def make_module(C, K, salt=0, device='cuda'):
    net = lgteun_amd.Pansharpening(Config(ms_chans=C), None, stage=K)
    sd = dw.fill_state_dict(state_shapes(C, K), salt=salt, dtype=np.float32)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(device)
    net.eval()
    return net


def device_drop_masks(seed, dtype=torch.float64):
    """the `drop_masks` callable of oracle.lgb / lgt / forward, drawn from the LIBRARY's export lg_dropout_mask (host tensors)"""
    lib = _lib.lib()

    def masks(stage, blk, B, h, w, e):
        out = torch.empty(B * h * w * e, device='cuda')
        _lib.check(lib.lg_dropout_mask(seed, stage, blk, 0, out.numel(), _ptr(out), _stream_ptr()), 'lg_dropout_mask')
        return mask_tensor(out.cpu(), B, h, w, e, dtype)
    return masks


def make_ops(C, H, W, K=1, precision=None, ws_fill=None):
    """Ops on a fresh module with the deterministic weights (a fresh module builds a fresh plan); precision: None or 'bf16'; ws_fill: see Ops"""
    net = make_module(C, K)
    if precision is not None:
        net.precision = precision
    return Ops(net, H, W, ws_fill=ws_fill)


GUARD = 1024        # floats of NaN band on each side of a guarded output (4 KiB: the output keeps its 16-byte alignment)


def guarded_empty(shape, device):
    """(buffer, out): `out` is a view of `shape` into a larger buffer filled with NaN -- `out` itself and GUARD floats on each side"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def assert_guards_intact(buf, what):
    """both bands of a guarded_empty buffer are still all-NaN: nothing next to the output was written"""
    lo, hi = torch.isnan(buf[:GUARD]), torch.isnan(buf[-GUARD:])
    assert bool(lo.all()) and bool(hi.all()), (what, 'written outside the output', int((~lo).sum()), int((~hi).sum()))


WS_GUARD_BYTES = 1 << 20      # NaN band on each side of a guarded workspace: the level-0 slabs are megabytes, a band of 4 KiB would only catch near misses
# what a workspace holds on entry: every byte 0x00, 0xFF (every float a NaN) or 0x5A (every float a finite 1.5e16, every bf16 the same)
WS_FILLS = {'zero': 0x00, 'nan': 0xFF, 'big': 0x5A}


def guarded_workspace(need_bytes, fill, device='cuda'):
    """(buffer, ws_view): ws_view is a uint8 view of exactly need_bytes that starts 256-byte aligned (the granule of carve()) inside a larger
    float buffer, WS_GUARD_BYTES of NaN floats on each side, and is filled with `fill` (a key of WS_FILLS or a byte)"""
    need_bytes = int(need_bytes)
    inner = (need_bytes + 3) // 4 * 4
    buf = torch.full(((2 * WS_GUARD_BYTES + inner) // 4,), float('nan'), device=device)
    view = buf.view(torch.uint8)[WS_GUARD_BYTES:WS_GUARD_BYTES + need_bytes]
    assert view.data_ptr() % 256 == 0, view.data_ptr()
    fill_workspace(view, fill)
    return buf, view


def fill_workspace(ws_view, fill):
    ws_view.fill_(WS_FILLS.get(fill, fill))


def assert_workspace_guards(buf, what):
    """both bands of a guarded_workspace buffer are still all-NaN: nothing was written in front of or behind the workspace"""
    n = WS_GUARD_BYTES // 4
    lo, hi = torch.isnan(buf[:n]), torch.isnan(buf[-n:])
    assert bool(lo.all()) and bool(hi.all()), (what, 'written outside the workspace', int((~lo).sum()), int((~hi).sum()))


def assert_bitwise(g0, g1, eng, what):
    """two flat gradient buffers of `eng`'s layout are equal float by float, the padding between the tensors included; names the tensors that differ"""
    if torch.equal(g0, g1):
        return
    bad = [eng.names[i] for i, (o, p) in enumerate(zip(eng.offsets, eng.params)) if not torch.equal(g0[o:o + p.numel()], g1[o:o + p.numel()])]
    raise AssertionError((what, 'gradients differ in', bad[:12], len(bad)))


class Ops:
    def __init__(self, net, H, W, ws_fill=None):
        """ws_fill=None: the engine's cached torch.empty workspace.  A key of WS_FILLS: every call runs on a guarded workspace of the test's own
        (guarded_workspace, allocated once per (B, train)) that is re-filled before the call, and whose bands are checked behind it.
        'stale': the same workspace, NOT re-filled: exactly what the previous call on it left (set `ops.ws_fill` between calls)"""
        self.net = net
        self.eng = net.engine()
        self.lib = self.eng.lib
        self.plan = self.eng.plan(H, W)   # precision follows net.precision
        self.H, self.W = H, W
        self.ws_fill = ws_fill
        self._guarded = {}

    def ws(self, B, train=False):
        if self.ws_fill is None:
            return self.eng.workspace(self.plan, B, train)
        key = (B, int(train))
        if key not in self._guarded:
            need = int(self.lib.lg_workspace_bytes(self.plan, B, int(train)))
            assert need > 0, key
            self._guarded[key] = guarded_workspace(need, 'nan' if self.ws_fill == 'stale' else self.ws_fill, self.eng.device)
        elif self.ws_fill != 'stale':
            fill_workspace(self._guarded[key][1], self.ws_fill)
        return self._guarded[key][1]

    def _ws_intact(self, what):
        """behind a call: the bands of every guarded workspace handed out so far (nothing to do without ws_fill)"""
        for key, (buf, _) in self._guarded.items():
            assert_workspace_guards(buf, (what, key))

    @staticmethod
    def _out(shape, device, guard):
        """guard=True: the output is a view into a NaN-filled buffer (itself included) with GUARD floats of band on each side; the caller
        hands the buffer to assert_guards_intact behind the launch"""
        if guard:
            return guarded_empty(tuple(shape), device)
        return None, torch.empty(tuple(shape), device=device)

    def resample(self, x, mode, guard=False):
        planes = x.shape[0] * x.shape[1]
        hi, wi = x.shape[2], x.shape[3]
        f = {0: 0.5, 1: 2, 2: 4}[mode]
        buf, y = self._out((x.shape[0], x.shape[1], int(hi * f), int(wi * f)), x.device, guard)
        _lib.check(self.lib.lg_op_resample(_ptr(x), _ptr(y), planes, hi, wi, mode, _stream_ptr()), 'lg_op_resample')
        if guard:
            assert_guards_intact(buf, 'lg_op_resample')
        return y

    def data_step(self, stage, z, ms, pan, guard=False):
        B = z.shape[0]
        buf, out = self._out(z.shape, z.device, guard)
        tmp = torch.empty(3 * z.numel() // 4 + z.numel() // z.shape[1], device=z.device)   # include/lgteun_hip.h: lg_op_data_step
        _lib.check(self.lib.lg_op_data_step(self.plan, _ptr(self.eng.flat), stage, _ptr(z), _ptr(ms), _ptr(pan), _ptr(out),
                                            _ptr(tmp), B, _stream_ptr()), 'lg_op_data_step')
        if guard:
            assert_guards_intact(buf, 'lg_op_data_step')
        return out

    def dropout_masks(self, seed, dtype=torch.float64):
        return device_drop_masks(seed, dtype)

    def lgt(self, stage, z, flags=0, seed=0, guard=False):
        B = z.shape[0]
        buf, out = self._out(z.shape, z.device, guard)
        ws = self.ws(B, train=bool(flags & _lib.LG_FLAG_SAVE))                 # LG_FLAG_SAVE writes the training workspace's save slots
        _lib.check(self.lib.lg_op_lgt(self.plan, _ptr(self.eng.flat), stage, _ptr(z), _ptr(out), _ptr(ws), ws.numel(), B, flags, seed,
                                      _stream_ptr()), 'lg_op_lgt')
        self._ws_intact('lg_op_lgt')
        if guard:
            assert_guards_intact(buf, 'lg_op_lgt')
        return out

    def lgt_stages(self, stage0, n, z, flags=0, seed=0, grid_cap=0, guard=False):
        """lg_op_lgt_stages: z [n,B,C,H,W] -> out [n,B,C,H,W], the stages stage0 .. stage0 + n - 1 as one pass"""
        B = z.shape[1]
        buf, out = self._out(z.shape, z.device, guard)
        ws = self.ws(B)
        _lib.check(self.lib.lg_op_lgt_stages(self.plan, _ptr(self.eng.flat), stage0, n, _ptr(z), _ptr(out), _ptr(ws), ws.numel(), B, flags, seed,
                                             grid_cap, _stream_ptr()), 'lg_op_lgt_stages')
        self._ws_intact('lg_op_lgt_stages')
        if guard:
            assert_guards_intact(buf, 'lg_op_lgt_stages')
        return out

    def block(self, stage, blk, which, x, guard=False):
        """x NHWC [B,h,w,e]; which 0: global mixer (planar out), 1: mixer half-block, 2: ffn half-block"""
        B, h, w, e = x.shape
        buf, y = self._out((B, e // 2, h, w) if which == 0 else x.shape, x.device, guard)
        ws = self.ws(B)
        _lib.check(self.lib.lg_op_block(self.plan, _ptr(self.eng.flat), stage, blk, which, _ptr(x), _ptr(y), _ptr(ws),
                                        ws.numel(), B, _stream_ptr()), 'lg_op_block')
        self._ws_intact('lg_op_block')
        if guard:
            assert_guards_intact(buf, 'lg_op_block')
        return y

    def _grads(self, owned, grads=None):
        """the flat gradient buffer of a per-op backward.  grads=<tensor>: the caller's own buffer, carried from call to call (the entries ADD into
        it); it is used as it is, without sentinel.  owned=None: plain zeros.  owned=[names]: a guarded view whose owned tensors start at
        zero and whose every other float (the 16-byte padding between tensors included) starts as a finite sentinel of tiny magnitude,
        2^-100 x (1 + index mod 251): a stray store or a stray `+=` of anything non-zero changes its bits, where NaN would hide the `+=`"""
        flat = self.eng.flat
        if grads is not None:
            assert owned is None and grads.shape == flat.shape and grads.dtype == flat.dtype and grads.device == flat.device and grads.is_contiguous()
            return None, grads
        if owned is None:
            return None, torch.zeros_like(flat)
        buf, grads = guarded_empty((flat.numel(),), flat.device)
        sentinel = (torch.arange(flat.numel(), device=flat.device) % 251 + 1).float() * 2.0 ** -100
        foreign = torch.ones(flat.numel(), dtype=torch.bool, device=flat.device)
        for name in owned:
            i = self.eng.names.index(name)
            foreign[self.eng.offsets[i]:self.eng.offsets[i] + self.eng.params[i].numel()] = False
        grads.copy_(torch.where(foreign, sentinel, torch.zeros_like(sentinel)))
        return (buf, sentinel, foreign), grads

    def _grads_intact(self, state, grads, what):
        """behind the launch: every float that is not an owned tensor's is bitwise the sentinel, both bands of the buffer are NaN"""
        if state is None:
            return
        buf, sentinel, foreign = state
        assert_guards_intact(buf, what + ' (gradient buffer)')
        moved = foreign & (grads.view(torch.int32) != sentinel.view(torch.int32))
        if bool(moved.any()):
            at = [int(i) for i in moved.nonzero().flatten()[:8]]
            owners = sorted({self.eng.names[max(j for j, o in enumerate(self.eng.offsets) if o <= i)] for i in at})
            assert False, (what, 'gradient floats that are not its own were written', int(moved.sum()), at, owners)

    def block_bwd(self, stage, blk, which, x, dy, guard=False, owned=None, grads=None):
        """returns (dx, flat_param_grads).  which 0: dy/dx planar [B,e/2,h,w]; 1,2: NHWC.  guard / owned: see _out / _grads"""
        B = x.shape[0]
        buf, dx = self._out(dy.shape, dy.device, guard)
        state, grads = self._grads(owned, grads)
        ws = self.ws(B, train=True)
        _lib.check(self.lib.lg_op_block_bwd(self.plan, _ptr(self.eng.flat), _ptr(grads), stage, blk, which, _ptr(x), _ptr(dy),
                                            _ptr(dx), _ptr(ws), ws.numel(), B, _stream_ptr()), 'lg_op_block_bwd')
        self._ws_intact('lg_op_block_bwd')
        if guard:
            assert_guards_intact(buf, 'lg_op_block_bwd')
        self._grads_intact(state, grads, 'lg_op_block_bwd')
        return dx, grads

    def data_step_bwd(self, stage, z, ms, pan, dz_out, guard=False, owned=None, grads=None):
        """returns (dz_in, flat_param_grads) of one data step"""
        B = z.shape[0]
        buf, dz = self._out(z.shape, z.device, guard)
        state, grads = self._grads(owned, grads)
        ws = self.ws(B, train=True)
        _lib.check(self.lib.lg_op_data_step_bwd(self.plan, _ptr(self.eng.flat), _ptr(grads), stage, _ptr(z), _ptr(ms), _ptr(pan),
                                                _ptr(dz_out), _ptr(dz), _ptr(ws), ws.numel(), B, _stream_ptr()), 'lg_op_data_step_bwd')
        self._ws_intact('lg_op_data_step_bwd')
        if guard:
            assert_guards_intact(buf, 'lg_op_data_step_bwd')
        self._grads_intact(state, grads, 'lg_op_data_step_bwd')
        return dz, grads

    def lgt_bwd(self, stage, z, dout, flags=0, seed=0, guard=False, owned=None, grads=None):
        """returns (dz, flat_param_grads) of one LGT; flags: 0 or LG_FLAG_DROPOUT (with seed)"""
        B = z.shape[0]
        buf, dz = self._out(z.shape, z.device, guard)
        state, grads = self._grads(owned, grads)
        ws = self.ws(B, train=True)
        _lib.check(self.lib.lg_op_lgt_bwd(self.plan, _ptr(self.eng.flat), _ptr(grads), stage, _ptr(z), _ptr(dout), _ptr(dz), _ptr(ws),
                                          ws.numel(), B, flags, seed, _stream_ptr()), 'lg_op_lgt_bwd')
        self._ws_intact('lg_op_lgt_bwd')
        if guard:
            assert_guards_intact(buf, 'lg_op_lgt_bwd')
        self._grads_intact(state, grads, 'lg_op_lgt_bwd')
        return dz, grads

    def grad_of(self, flat_grads, name):
        i = self.eng.names.index(name)
        o, p = self.eng.offsets[i], self.eng.params[i]
        return flat_grads[o:o + p.numel()].view(p.shape)
