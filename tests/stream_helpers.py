"""Helper, not a test: what tests/test_gpu_streams.py and tests/test_gpu_threads.py share -- the late-input protocol that shows on which stream an
entry of include/lgteun_hip.h really enqueues its work, a calibrated device sleep, and a train-step rig on raw C-ABI calls whose every call takes
the stream it is given.

The late-input protocol (check_entry_runs_on_its_stream), for one Case = the buffers of one entry call:
  1. quiet run: device synchronised, inputs hold the true data, outputs and workspace hold the byte FILL, the call goes to the current stream;
     the outputs, as bits, are R0.  Run twice: the first warms the entry (LDS attributes, twiddles, code objects, the reduce-image cache, whose
     key includes the workspace and gradient pointers -- a Case keeps its buffers, so the late call is a hit), the second must repeat its bits.
  2. late run on a side stream s (torch's side streams are non-blocking: the null stream does not order against them).  The inputs hold a decoy
     (another seed, finite, in range), outputs and workspace hold FILL.  Then, on s: a sleep of at least 50 ms, an event, device-to-device copies of
     the true data into the inputs, FILL into outputs and workspace once more, the entry call with s's handle.
  3. when the call returns on the host the event must still be pending: the call neither waited for the device nor drained it.
  4. after s.synchronize() every output equals R0 bit for bit and the guard bands of the float outputs are intact.
A launch that went to any other stream runs during the sleep: it reads the decoy or a FILLed workspace, and what it wrote is FILLed over by s.

The sleep is a condition of the test, not a tolerance on the library: it is calibrated once per process with two events to last at least 50 ms and
must be at least ten times the longest host-side duration of the warm call, or the case fails saying so."""
import ctypes
import time

import numpy as np
import torch

from gpu_helpers import assert_guards_intact, guarded_empty, make_module
from lgteun_amd import _lib
from oracle import detweights as dw

FILL = 0x5A                 # every float a finite 1.5e16, every double 3.6e127: a kernel that reads it cannot give R0
MIN_SLEEP_MS = 50.0
HOST_FACTOR = 10.0
STATS = dict(cycles=None, sleep_ms=None, max_host_ms=0.0, max_host_case=None)
_streams = []


def L():
    return _lib.lib()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def handle(s):
    """the hipStream_t of a torch stream, as the void* the C ABI takes"""
    return ctypes.c_void_p(s.cuda_stream)


def current():
    return handle(torch.cuda.current_stream())


def side_streams(n, device=None):
    """the first n of the (at most four) side streams of this process on the current device"""
    assert 1 <= n <= 4
    dev = torch.cuda.current_device() if device is None else device
    mine = [s for s in _streams if s.device.index == dev]
    while len(mine) < n:
        s = torch.cuda.Stream(device=dev)
        assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        _streams.append(s)
        mine.append(s)
    return mine[:n]


def bits(t):
    """a copy of t's bytes"""
    return t.contiguous().view(-1).view(torch.uint8).clone()


def fill(t):
    t.view(-1).view(torch.uint8).fill_(FILL)


def uniform(shape, seed, lo=0.05, hi=0.95, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


def sleep_cycles():
    """the argument of torch.cuda._sleep that lasts at least MIN_SLEEP_MS on this device, measured once with two events"""
    if STATS['cycles'] is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        probe = 2_000_000
        torch.cuda.synchronize()
        torch.cuda._sleep(probe)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        per = a.elapsed_time(b) / probe
        assert per > 0, 'the sleep kernel took no measurable time'
        cycles = int(2.0 * MIN_SLEEP_MS / per)             # aims at twice the minimum: room for a host that is busy with other work
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms >= MIN_SLEEP_MS, f'calibrated sleep of {cycles} cycles lasted {ms:.1f} ms, below {MIN_SLEEP_MS} ms'
        STATS.update(cycles=cycles, sleep_ms=ms)
        print(f'[streams] calibrated sleep: {cycles} cycles = {ms:.1f} ms')
    return STATS['cycles']


class Case:
    """the buffers of one entry call.  inp(): a buffer the entry reads, with its true data and a decoy (inout=True: the entry also writes it, and it
    counts as an output); out(): a buffer the entry only writes (float32 ones between guard bands); ws(): a workspace.  `call(stream)` makes the
    call with the given void* stream and returns the entry's return code (or a list of them)."""

    def __init__(self, name, device='cuda'):
        self.name, self.device = name, device
        self.ins, self.outs, self.fills, self.guards = [], [], [], []
        self.call = None

    def inp(self, true, decoy, inout=False):
        true, decoy = true.to(self.device).contiguous(), decoy.to(self.device).contiguous()
        assert true.shape == decoy.shape and true.dtype == decoy.dtype and not torch.equal(true, decoy), self.name
        assert bool(torch.isfinite(decoy.double()).all()), self.name
        buf = torch.empty_like(true)
        self.ins.append((buf, true, decoy))
        if inout:
            self.outs.append(buf)
        return buf

    def rand(self, shape, seed, lo=0.05, hi=0.95, inout=False):
        """an input of uniform float32 noise: the true data from `seed`, the decoy from seed + 1"""
        return self.inp(uniform(shape, seed, lo, hi), uniform(shape, seed + 1, lo, hi), inout)

    def const(self, t):
        """a small table (ranges, taps, origins, indices) that stays as it is in every run"""
        return t.to(self.device).contiguous()

    def out(self, *shape, dtype=torch.float32):
        if dtype == torch.float32:
            buf, view = guarded_empty(tuple(shape), self.device)
            self.guards.append(buf)
        else:
            view = torch.empty(tuple(shape), dtype=dtype, device=self.device)
        self.outs.append(view)
        self.fills.append(view)
        return view

    def ws(self, nbytes):
        nbytes = int(nbytes)
        assert nbytes > 0, (self.name, 'the sizer rejects the shape')
        t = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        self.fills.append(t)
        return t, nbytes

    def watch(self, view):
        """a region of a workspace that counts as an output"""
        self.outs.append(view)

    def _load(self, decoy):
        for buf, true, dec in self.ins:
            buf.copy_(dec if decoy else true)
        for t in self.fills:
            fill(t)

    def _call(self, stream):
        t0 = time.perf_counter()
        rcs = self.call(stream)
        host_ms = 1e3 * (time.perf_counter() - t0)
        for rc in (rcs if isinstance(rcs, (list, tuple)) else [rcs]):
            _lib.check(rc, self.name)
        return host_ms

    def quiet(self):
        """-> (the outputs as bits, the call's host time in ms)"""
        torch.cuda.synchronize()
        self._load(decoy=False)
        torch.cuda.synchronize()
        host_ms = self._call(current())
        torch.cuda.synchronize()
        return [bits(o) for o in self.outs], host_ms

    def late(self, s, call_stream=None):
        """-> (the outputs as bits, host time in ms, whether the sleep's event was still pending when the call returned).  call_stream: the handle
        the entry is given instead of s's (the control: a wrong stream)"""
        cycles = sleep_cycles()
        torch.cuda.synchronize()
        self._load(decoy=True)
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            ev.record()
            for buf, true, _ in self.ins:
                buf.copy_(true, non_blocking=True)
            for t in self.fills:
                fill(t)
            host_ms = self._call(handle(s) if call_stream is None else call_stream)
            pending = not ev.query()
        s.synchronize()
        torch.cuda.synchronize()
        return [bits(o) for o in self.outs], host_ms, pending

    def guards_intact(self):
        for buf in self.guards:
            assert_guards_intact(buf, self.name)


def same(r0, r1):
    """which outputs of two runs differ, by index"""
    assert len(r0) == len(r1)
    return [k for k, (a, b) in enumerate(zip(r0, r1)) if not torch.equal(a, b)]


def check_entry_runs_on_its_stream(case):
    cold, _ = case.quiet()
    r0, host0 = case.quiet()
    assert not same(cold, r0), (case.name, 'two quiet runs differ: the protocol needs an entry that repeats its bits', same(cold, r0))
    for k, o in enumerate(r0):
        assert not bool((o == FILL).all()), (case.name, 'output', k, 'still holds the fill after the quiet run')
    s, = side_streams(1)
    r1, host1, pending = case.late(s)
    host_ms = max(host0, host1)
    if host_ms > STATS['max_host_ms']:
        STATS.update(max_host_ms=host_ms, max_host_case=case.name)
    print(f'[streams] {case.name}: host {host0:.3f} ms quiet, {host1:.3f} ms late; sleep {STATS["sleep_ms"]:.1f} ms; longest warm call so far '
          f'{STATS["max_host_ms"]:.3f} ms ({STATS["max_host_case"]})')
    assert STATS['sleep_ms'] >= HOST_FACTOR * host_ms, (f'{case.name}: the sleep of {STATS["sleep_ms"]:.1f} ms is not {HOST_FACTOR:.0f} times the call\'s host '
                                                       f'time of {host_ms:.3f} ms: the case proves nothing')
    assert pending, (case.name, 'returned only after its stream had passed the sleep: the call waited for the device')
    assert not same(r0, r1), (case.name, 'outputs differ from the quiet run: work went to another stream', same(r0, r1))
    case.guards_intact()
    return r0


# ------------------------------------------------------------------------------------------------------------------------
# a train step on raw C-ABI calls: forward, l1 loss, backward, AdamW through lg_optim_step -- every call on the stream it is handed
# ------------------------------------------------------------------------------------------------------------------------
NET_FLAGS = _lib.LG_FLAG_FAITHFUL | _lib.LG_FLAG_SAVE | _lib.LG_FLAG_DROPOUT


class TrainRig:
    """one parameter set (module `salt`), data set (`seed`), plan, workspace, gradient and optimizer buffers of its own.  PAN 16 x 16, B = 2, C = 4: the output
    has 2048 floats, so lg_l1_loss runs two workgroups and its two float atomics on a zeroed scalar commute -- the loss repeats its bits."""

    def __init__(self, salt, seed, steps, C=4, K=2, H=16, W=16, B=2, device='cuda'):
        self.net = make_module(C, K, salt=salt, device=device)
        self.eng = self.net.engine()
        self.plan = self.eng.plan(H, W)
        self.B, self.steps, self.seed = B, steps, seed
        self.flat = self.eng.flat
        self.flat0 = self.flat.clone()
        self.grads, self.m, self.v = (torch.zeros_like(self.flat) for _ in range(3))
        ms, pan, gt = dw.make_inputs(B, C, H // 4, W // 4, seed=seed, kind='smooth')
        self.ms, self.pan, self.gt = (torch.from_numpy(a).to(device).contiguous() for a in (ms, pan, gt))
        self.ws_bytes = int(L().lg_workspace_bytes(self.plan, B, 1))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.out, self.dout = torch.empty_like(self.gt), torch.empty_like(self.gt)
        self.losses = torch.zeros(steps, device=device)
        assert self.out.numel() <= 2048
        self.n_ranges, self.max_range, self.ranges = len(self.eng.live_ranges), self.eng.max_range, self.eng.ranges_dev

    def reset(self):
        self.flat.copy_(self.flat0)
        for t in (self.grads, self.m, self.v, self.losses):
            t.zero_()
        fill(self.ws)
        fill(self.out)
        fill(self.dout)

    def calls(self, step):
        """the five calls of train step `step` (0-based), each a function of the torch stream it goes to"""
        lib, sd, n = L(), self.seed * 1000 + step, self.out.numel()

        def zero(s):
            with torch.cuda.stream(s):
                self.grads.zero_()

        def fwd(s):
            _lib.check(lib.lgteun_forward(self.plan, ptr(self.flat), ptr(self.ms), ptr(self.pan), ptr(self.out), ptr(self.ws), self.ws_bytes, self.B, NET_FLAGS, sd,
                                          handle(s)), 'lgteun_forward')

        def loss(s):
            _lib.check(lib.lg_l1_loss(ptr(self.out), ptr(self.gt), ptr(self.dout), ptr(self.losses[step:]), n, n, 1.0, handle(s)), 'lg_l1_loss')

        def bwd(s):
            _lib.check(lib.lgteun_backward(self.plan, ptr(self.flat), ptr(self.grads), ptr(self.ms), ptr(self.pan), ptr(self.dout), ptr(self.ws), self.ws_bytes,
                                           self.B, NET_FLAGS, sd, handle(s)), 'lgteun_backward')

        def opt(s):
            _lib.check(lib.lg_optim_step(ptr(self.flat), ptr(self.grads), ptr(self.m), ptr(self.v), None, ptr(self.ranges), self.n_ranges, self.max_range, step + 1,
                                         _lib.LG_OPT_ADAMW, 0, 1.5e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, handle(s)), 'lg_optim_step')
        return [zero, fwd, loss, bwd, opt]

    def run_alone(self, s):
        """all steps on stream s, then synchronised -> results()"""
        self.reset()
        torch.cuda.synchronize()
        for step in range(self.steps):
            for f in self.calls(step):
                f(s)
        s.synchronize()
        return self.results()

    def results(self):
        return {k: bits(t) for k, t in (('weights', self.flat), ('exp_avg', self.m), ('exp_avg_sq', self.v), ('losses', self.losses), ('grads', self.grads))}


def differing(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


# ------------------------------------------------------------------------------------------------------------------------
# classical scenes and raw calls with a workspace of the caller's
# ------------------------------------------------------------------------------------------------------------------------
def classical_scene(B, C, h, w, seed, device='cuda'):
    """ms [B, C, h, w], pan [B, 1, 4h, 4w] float32 on the device: classical_ref.make_scene per sample"""
    import classical_ref as cr
    pairs = [cr.make_scene(C, h, w, seed * 100 + b) for b in range(B)]
    ms = torch.from_numpy(np.stack([p[0] for p in pairs])).to(device)
    pan = torch.from_numpy(np.stack([p[1][None] for p in pairs])).to(device)
    return ms.contiguous(), pan.contiguous()


def gsa_call(ms, pan, out, stats, ws, s):
    B, C, h, w = ms.shape
    _lib.check(L().lg_gsa(ptr(ms), ptr(pan), ptr(out), ptr(stats), B, C, h, w, ptr(ws), ws.numel() * 8, handle(s)), 'lg_gsa')


def iqa_ref_call(pred, gt, out, ws, s, scale=2047.5):
    B, C, H, W = pred.shape
    _lib.check(L().lg_iqa_ref(ptr(pred), ptr(gt), ptr(out), B, C, H, W, scale, ptr(ws), ws.numel() * 8, handle(s)), 'lg_iqa_ref')
