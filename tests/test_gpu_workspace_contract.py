"""-m gpu: the workspace contract of the network's C entry points -- lgteun_forward, lgteun_backward, lgteun_dead_forward and the lg_op_* entries.

Every other test of these entries runs on Engine.workspace(): a torch.empty buffer cached per (plan, B, train), which almost always holds what the same
kernels left there on a previous, near-identical run.  A kernel that reads a slot nobody wrote in THIS call gets a plausible value and passes every
accuracy gate.  Here the workspace is the test's own (ctypes on eng.lib; gpu_helpers.guarded_workspace): a view of exactly lg_workspace_bytes bytes
between two bands of 1 MiB of NaN floats, in one of four states on entry --
    'zero'  every byte 0x00          'nan'  every byte 0xFF: every float a NaN          'big'  every byte 0x5A: every float a finite 1.5e16
    'stale' exactly as left by the SAME call sequence on different inputs, a different dropout seed and, for the backward, a dout 2^10 times larger
-- and ONE assertion throughout: the results of a call sequence (out, the gradient buffer, dz / dx where there is one) are BIT FOR BIT the same for
every state, and both bands are still NaN afterwards.  No tolerance: the kernels use no floating-point atomics on results, and accuracy against the
oracle stays where it is; this file adds none.

Read before the first run (carve() in workspace.h, carve_bwd() in k_bwd.hip): every workspace region holds data -- floats, bf16, dropout keep-bit
words, the float bits of max |dh2| -- and no index, offset or pointer; the reduce queue's job tables live in the library's own allocation.  Poison
can change numbers, it cannot send a kernel to a wild address.

Sections (PAN sizes; the smallest that reach each region):
  (a) whole net, training: saving forward + backward, four states, 13 cases -- baseline with dropout on and off; K = 3 batched dead pass and the same
      stagewise; K = 4 at 16 x 16; the level-1 plane 24 x 40 (tile fallback, Bluestein mixer); C = 8; chained; bf16; 256 x 256 (fft_scratch)
  (b) whole net, inference (train = 0): four states, and workspace_bytes = need + 4096 with the band behind the slack
  (c) split calls: forward with LG_FLAG_DEFER_DEAD, LG_FLAG_BWD_LGT, lgteun_dead_forward, LG_FLAG_BWD_DATA against the one-call pair, the
      lg_workspace_deadout region included
  (d) every route of tests/test_gpu_routes_launch.py, each on a workspace of its own, 'nan' against 'big': the check of route.hip's f.saves against
      what each route's backward reads -- no other route ever wrote the workspace
  (e) the per-op entries at the shapes of test_gpu_forward_shapes.py / test_gpu_backward_shapes.py that name a capped grid or a ragged tail
  (f) lgteun_backward twice on one saved forward (retain_graph): the second result is that of a fresh forward + backward
  (g) rejections: workspace_bytes = need - 1 and a null workspace launch nothing

Measured on an MI355X (every figure below was measured there; nothing in this file was run anywhere else):
  the file: 51 tests in 7.4 s; the slowest case 0.80 s (the retain_graph test), the slowest parametrized case 0.61 s (the first test of the
  file), the largest route case 0.47 s ((4, fp32, 48): 77 routes), (9, 128, 128) at C = 8 0.17 s; the 256 x 256 cases are not among the 20 slowest (0.05 s and below).
  lg_workspace_bytes of (4, 1, 256, 256, 1), train = 1: 1 090 388 480 bytes (1.02 GiB); filling and comparing it is no issue, all four states run.
  cases: (a) 13, (b) 4 (each also with slack), (c) 1, (d) 8 = 298 routes, (e) 18 (10 half-block cases x their which list, forward and backward; 3 LGT
  cases x three entries; 3 data steps; lg_op_lgt_stages at two grid caps), (f) 5, (g) 2.
  RED BEFORE A FIX: (f), all five.  On the commit before this file the second lgteun_backward on one saved forward with dout2 = dout1 * 2^-20 was not
  a fresh backward: 97 106 of 202 192 gradient floats differ at (4, 2, 32, 32, 2) and 254 167 at (8, 2, 32, 32, 1), dropout on or off; first differing
  tensor D.1.weight (the first of the buffer) at a relative L2 of 6.7e-8 ... 1.3e-7; through _LgteunFn with retain_graph 126 live tensors differ.  (The
  pair with an unrelated dout2 of the same scale was not reached there: the 2^-20 pair fails first.)  Cause: word 6 of a block's ffn_scales row, max |dh2|,
  is an atomic max that only the forward's k_ffn_scales set to zero, so a second backward began at the first one's maximum and k_ffn1_bwd_xs scaled its
  f16 pairs 2^20 too coarsely.  Fix: the transpose launch at the head of the LGT backward (k_bwd.hip: ffn_transposes) sets the word to zero; no launch
  added.  A single backward's bits did not move: sha256 of out + gradient buffer of the 13 cases of (a) is the same under both builds.  Every other
  section was green from its first run: no read-before-write was found in the route tables, the slab rows, the dead-stage pass or the regions that exist
  only sometimes, and the 0xFF fill produced no NaN anywhere.

What it sees, checked once with throw-away builds loaded through LGTEUN_HIP_LIB (in-bounds, arithmetic-only edits; nothing of them is kept):
  (i)  the start value of word 6 not part of the backward (= the commit before this file).  RED: (f), all five; GREEN: the other 46.  With the fix in, the
       edit the other way round -- k_ffn_scales in the forward no longer clears the word -- leaves all 51 green on poisoned workspaces: the backward owns
       the word's start value now.
  (ii) k_ffn_xr's saving forward (the default e = 16 route) skips its a3 (h3) store while k_ffn_dw_bwd_xs still reads it.  RED, 23 tests: (d) the four
       C = 4 cases, from the default route on (gradients not finite under 0xFF); (e) lg_op_block_bwd which = 2 at C = 4 blocks 0, 1, 3, 4 (five cases) and
       lg_op_lgt_bwd at C = 4 (two cases); also (a) the nine C = 4 cases ('nan' against 'zero': 101 094 ... 202 099 gradient floats differ), (c), and (f)
       at C = 4.  GREEN, 28: every C = 8 case, (b), (g), the forward entries, the mixer and data-step entries, lg_op_lgt_stages, the level-1 FFN cases, the retain_graph test (it runs on the engine's own workspace).
       tests/test_gpu_routes_launch.py on the same build: 3 of its 8 cases red as well, 5 green ((4, fp32, 32) and (4, fp32, 48): the default route's
       gradients, read from whatever torch.empty handed out, lie 0.11 ... 0.12 from the routes that store their own a3, against a bound of 1.1e-2;
       (4, bf16, 48): route 0x10 not finite; (4, bf16, 32) stayed GREEN with the same missing store) -- it notices the default route there by
       disagreement with the others, not the missing store itself, and not on every case.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import detweights as dw

pytestmark = pytest.mark.gpu

FAITHFUL, SAVE, DROPOUT, BWD_LGT, BWD_DATA, CHAINED, DEFER_DEAD, STAGEWISE = 1, 2, 4, 8, 16, 32, 64, 128
MODES = {'faithful': FAITHFUL, 'live': 0, 'chained': CHAINED}
SEED, SEED_STALE = 0x5EED1234, 0x0DDBA11
STATES = ('zero', 'nan', 'big', 'stale')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Net:
    """one engine, one plan, one guarded workspace (allocated once, re-filled per state) and the raw C calls on it"""

    def __init__(self, C, K, H, W, B, train, precision=None, variant=None, slack=0, module=None):
        from gpu_helpers import guarded_workspace, make_module
        self.net = make_module(C, K) if module is None else module      # (module: one engine for many variants -- each variant is a plan of its own)
        if precision is not None:
            self.net.precision = precision
        self.eng = self.net.engine()
        if variant is not None:
            self.eng.variant = variant
        self.lib = self.eng.lib
        self.C, self.K, self.H, self.W, self.B, self.train = C, K, H, W, B, train
        self.plan = self.eng.plan(H, W)
        self.need = int(self.lib.lg_workspace_bytes(self.plan, B, train))
        print(f'lg_workspace_bytes C={C} K={K} {H}x{W} B={B} train={train} precision={precision} variant={variant}: {self.need}')
        assert self.need > 0
        self.nbytes = self.need + slack
        self.buf, self.ws = guarded_workspace(self.nbytes, 'nan', self.eng.device)
        self.grads = torch.zeros(self.eng.total, dtype=torch.float32, device=self.eng.device)   # one buffer: the reduce queue's table cache is keyed by it

    def inputs(self, seed=5, dout_scale=1.0):
        ms, pan, gt = (torch.from_numpy(a).cuda() for a in dw.make_inputs(self.B, self.C, self.H // 4, self.W // 4, seed=seed, kind='smooth'))
        return ms, pan, ((gt - gt.mean()) * dout_scale).contiguous()

    def fill(self, state):
        from gpu_helpers import fill_workspace
        fill_workspace(self.ws, state)

    def guards(self, what):
        from gpu_helpers import assert_workspace_guards
        assert_workspace_guards(self.buf, what)

    def forward(self, ms, pan, flags, seed=SEED, nbytes=None, ws=True):
        from gpu_helpers import assert_guards_intact, guarded_empty
        from lgteun_amd.engine import _ptr, _stream_ptr
        obuf, out = guarded_empty((self.B, self.C, self.H, self.W), self.eng.device)
        rc = self.lib.lgteun_forward(self.plan, _ptr(self.eng.flat), _ptr(ms), _ptr(pan), _ptr(out), _ptr(self.ws) if ws else None,
                                     self.nbytes if nbytes is None else nbytes, self.B, flags, seed, _stream_ptr())
        assert_guards_intact(obuf, 'lgteun_forward')
        self.guards('lgteun_forward')
        return rc, out

    def backward(self, ms, pan, dout, flags, seed=SEED, zero=True, nbytes=None, ws=True, grads=None):
        from lgteun_amd.engine import _ptr, _stream_ptr
        g = self.grads if grads is None else grads
        if zero:
            g.zero_()
        rc = self.lib.lgteun_backward(self.plan, _ptr(self.eng.flat), _ptr(g), _ptr(ms), _ptr(pan), _ptr(dout), _ptr(self.ws) if ws else None,
                                      self.nbytes if nbytes is None else nbytes, self.B, flags, seed, _stream_ptr())
        self.guards('lgteun_backward')
        return rc

    def dead_forward(self, flags, seed=SEED, nbytes=None, ws=True):
        from lgteun_amd.engine import _ptr, _stream_ptr
        rc = self.lib.lgteun_dead_forward(self.plan, _ptr(self.eng.flat), _ptr(self.ws) if ws else None, self.nbytes if nbytes is None else nbytes,
                                          self.B, flags, seed, _stream_ptr())
        self.guards('lgteun_dead_forward')
        return rc

    def step(self, inp, flags, seed=SEED):
        """saving forward + backward into the zeroed gradient buffer -> {'out', 'grads'} (copies)"""
        ms, pan, dout = inp
        rc, out = self.forward(ms, pan, flags | SAVE, seed)
        assert rc == 0, (rc, self.lib.lg_last_error())
        rc = self.backward(ms, pan, dout, flags | SAVE, seed)
        assert rc == 0, (rc, self.lib.lg_last_error())
        return {'out': out.clone(), 'grads': self.grads.clone()}

    def infer(self, inp, flags):
        rc, out = self.forward(inp[0], inp[1], flags, 0)
        assert rc == 0, (rc, self.lib.lg_last_error())
        return {'out': out.clone()}

    def first_difference(self, a, b):
        """name of the first gradient tensor whose bits differ, and its relative L2 distance"""
        d = (_bits(a) != _bits(b)).nonzero().flatten()
        if d.numel() == 0:
            return None
        i = int(d[0])
        j = max(k for k, o in enumerate(self.eng.offsets) if o <= i)
        o, n = self.eng.offsets[j], self.eng.params[j].numel()
        ta, tb = a[o:o + n].double(), b[o:o + n].double()
        return self.eng.names[j], int(d.numel()), float((ta - tb).norm() / tb.norm()) if bool(torch.isfinite(ta).all()) else float('nan')


def _compare(net, tag, ref_state, ref, state, got):
    for k in ref:
        if not _same(ref[k], got[k]):
            where = net.first_difference(got[k], ref[k]) if k == 'grads' else None
            nd = int((_bits(ref[k]) != _bits(got[k])).sum())
            assert False, (tag, f"'{k}' differs between workspace states '{state}' and '{ref_state}'", nd, 'of', ref[k].numel(),
                           'first gradient tensor, floats, rel-L2', where, 'finite', bool(torch.isfinite(got[k]).all()))


def _run_states(net, tag, run, inp, stale_inp, states=STATES):
    """run(inputs, seed) once per state; 'stale' = the workspace as the same sequence on stale_inp left it.  Bitwise equal, bands intact, finite."""
    ref_state = ref = None
    for st in states:
        if st == 'stale':
            run(stale_inp, SEED_STALE)                      # on whatever the previous state left: its result is not looked at
        else:
            net.fill(st)
        got = run(inp, SEED)
        net.guards((tag, st))
        if ref is None:
            ref_state, ref = st, got
            for k, v in got.items():
                assert bool(torch.isfinite(v).all()), (tag, st, k, 'not finite')
            if 'grads' in got:
                assert float(got['grads'].norm()) > 0
        else:
            _compare(net, tag, ref_state, ref, st, got)
    return ref


# ---- (a) whole net, training
A_CASES = [  # C, K, H, W, B, mode, extra flags, dropout, precision
    (4, 2, 32, 32, 2, 'faithful', 0, 1, None), (4, 2, 32, 32, 2, 'faithful', 0, 0, None),            # baseline
    (4, 3, 32, 32, 2, 'faithful', 0, 1, None), (4, 3, 32, 32, 2, 'faithful', STAGEWISE, 1, None),    # one dead pass over 2 B samples | stage by stage
    (4, 4, 16, 16, 1, 'faithful', 0, 1, None),                                                       # smallest plan, three dead stages
    (4, 2, 48, 80, 1, 'live', 0, 1, None),                                                           # level-1 plane 24 x 40: tile fallback, Bluestein mixer
    (8, 2, 32, 32, 2, 'faithful', 0, 1, None), (8, 2, 48, 48, 1, 'live', 0, 1, None),                # e = 32 / 64 kernels, wsplit slots, no stage batching
    (4, 2, 32, 32, 2, 'chained', 0, 1, None), (8, 2, 32, 32, 1, 'chained', 0, 1, None),              # train = 2: K activation sets
    (4, 2, 32, 32, 2, 'faithful', 0, 1, 'bf16'), (8, 2, 32, 32, 1, 'faithful', 0, 1, 'bf16'),        # bf16 storage of the hidden tensors
    (4, 1, 256, 256, 1, 'live', 0, 1, None),                                                         # the only size with fft_scratch (split FFT path)
]


@pytest.mark.parametrize('C,K,H,W,B,mode,extra,drop,precision', A_CASES)
def test_training_step_bits_do_not_depend_on_the_workspace_on_entry(C, K, H, W, B, mode, extra, drop, precision):
    """lgteun_forward(LG_FLAG_SAVE | mode | dropout) + lgteun_backward into a zeroed gradient buffer: out and the gradient buffer have the same bits
    for the four workspace states.  (4, 1, 256, 256, 1): lg_workspace_bytes = see RESULTS in the module docstring; all four states run."""
    flags = MODES[mode] | extra | (DROPOUT if drop else 0)
    net = Net(C, K, H, W, B, 2 if mode == 'chained' else 1, precision)
    tag = f'train C={C} K={K} {H}x{W} B={B} {mode} extra={extra} dropout={drop} precision={precision}'
    _run_states(net, tag, lambda inp, seed: net.step(inp, flags, seed), net.inputs(5), net.inputs(6, 1024.0))


# ---- (b) whole net, inference
B_CASES = [(4, 2, 32, 32, 3, 0), (4, 3, 32, 32, 2, FAITHFUL), (8, 2, 48, 48, 1, 0), (4, 1, 256, 256, 1, 0)]


@pytest.mark.parametrize('C,K,H,W,B,flags', B_CASES)
def test_inference_bits_do_not_depend_on_the_workspace_on_entry(C, K, H, W, B, flags):
    """train = 0: the shared h2 and the transient-only carving; LG_FLAG_FAITHFUL at K = 3 runs the batched dead pass at inference.  Then the same on
    need + 4096 bytes, the band behind the slack: slack changes nothing"""
    net = Net(C, K, H, W, B, 0)
    tag = f'infer C={C} K={K} {H}x{W} B={B} flags={flags}'
    inp, stale = net.inputs(5), net.inputs(6)
    ref = _run_states(net, tag, lambda i, seed: net.infer(i, flags), inp, stale)
    wide = Net(C, K, H, W, B, 0, slack=4096)
    assert wide.nbytes == net.need + 4096
    got = _run_states(wide, tag + ' slack', lambda i, seed: wide.infer(i, flags), inp, stale, states=('nan', 'big'))
    assert _same(ref['out'], got['out']), (tag, 'slack behind the workspace changed the output')


# ---- (c) split calls
def test_split_calls_give_the_bits_of_the_one_call_pair_on_a_poisoned_workspace():
    """(4, 3, 32, 32, 2, faithful) with dropout: forward with LG_FLAG_DEFER_DEAD, backward LG_FLAG_BWD_LGT, lgteun_dead_forward, backward LG_FLAG_BWD_DATA
    on a poisoned workspace = the one-call forward + backward of (a): out, the gradient buffer and the lg_workspace_deadout region, bit for bit"""
    C, K, H, W, B = 4, 3, 32, 32, 2
    net = Net(C, K, H, W, B, 1)
    flags = FAITHFUL | DROPOUT | SAVE
    ms, pan, dout = net.inputs(5)
    off, stride = ctypes.c_size_t(), ctypes.c_size_t()
    assert net.lib.lg_workspace_deadout(net.plan, B, 1, ctypes.byref(off), ctypes.byref(stride)) == 0
    n_dead = (K - 1 if stride.value else 1) * B * C * H * W * 4
    assert stride.value == B * C * H * W * 4, stride.value            # this plan batches its dead stages: one slot per dead stage
    assert off.value + n_dead <= net.need

    def deadout():
        return net.ws[off.value:off.value + n_dead].clone()

    results = {}
    for st in ('nan', 'big'):
        net.fill(st)
        one = net.step((ms, pan, dout), FAITHFUL | DROPOUT)
        one['deadout'] = deadout()
        net.fill(st)
        rc, out = net.forward(ms, pan, flags | DEFER_DEAD)
        assert rc == 0, net.lib.lg_last_error()
        assert net.backward(ms, pan, dout, flags | DEFER_DEAD | BWD_LGT) == 0, net.lib.lg_last_error()
        assert net.dead_forward(flags | DEFER_DEAD) == 0, net.lib.lg_last_error()
        assert net.backward(ms, pan, dout, flags | DEFER_DEAD | BWD_DATA, zero=False) == 0, net.lib.lg_last_error()
        split = {'out': out.clone(), 'grads': net.grads.clone(), 'deadout': deadout()}
        for k, v in one.items():
            assert bool(torch.isfinite(v.view(torch.float32) if k == 'deadout' else v).all()), (st, k)
        _compare(net, f'split calls on {st}', 'one call', one, 'split', split)
        results[st] = split
    _compare(net, 'split calls', 'nan', results['nan'], 'big', results['big'])


# ---- (d) every route on a workspace of its own
def _route_cases():
    from test_gpu_routes_launch import N_ROUTES
    return sorted(N_ROUTES)


@pytest.mark.parametrize('C,prec,n', _route_cases())
def test_every_route_reads_only_what_its_own_saving_forward_wrote(C, prec, n):
    """per distinct route (the representatives of test_gpu_routes_launch.py; K = 1, B = 1, dropout off): a fresh plan on a guarded workspace of its own,
    saving forward + backward from 'nan' and from 'big'.  Equal bits, intact bands, finite output and gradients.  test_gpu_routes_launch.py walks the
    routes on ONE engine workspace, default route first, so every save slot a later route might wrongly read was just written by an earlier one"""
    from test_gpu_routes_launch import N_ROUTES, representatives
    reps = representatives(C, prec, n)
    assert len(reps) == N_ROUTES[(C, prec, n)] and reps[0] == 0, (len(reps), reps[:4])
    from gpu_helpers import make_module
    failures, module = [], make_module(C, 1)
    for v in reps:
        net = Net(C, 1, n, n, 1, 1, 'bf16' if prec else None, variant=v, module=module)
        inp = net.inputs(5)
        got = {}
        for st in ('nan', 'big'):
            net.fill(st)
            got[st] = net.step(inp, 0)
        text = re.sub(r' variant=0x[0-9a-f]+', '', net.eng.describe(n, n))
        for k in ('out', 'grads'):
            if not bool(torch.isfinite(got['nan'][k]).all()) or not bool(torch.isfinite(got['big'][k]).all()):
                failures.append((hex(v), k, 'not finite', text))
            elif not _same(got['nan'][k], got['big'][k]):
                failures.append((hex(v), k, 'bits differ between the fills 0xFF and 0x5A',
                                 net.first_difference(got['nan'][k], got['big'][k]) if k == 'grads' else None, text))
    print(f'routes C={C} precision={prec} n={n}: {len(reps)} routes on a poisoned workspace each, {len(failures)} failures')
    assert not failures, failures


# ---- (e) per-op entries at the shapes that name a capped grid or a ragged tail
def _ops(C, H, W, K=1):
    from gpu_helpers import make_ops
    return make_ops(C, H, W, K, ws_fill='nan')


def _fwd_route(ops, H, W, level, e):
    lines = [ln for ln in ops.eng.describe(H, W).splitlines() if ln.startswith(f'L{level} ') and ' fwd: ' in ln]
    assert len(lines) == 1, lines
    ffn = {16: 'k_ffn_xr', 32: 'k_ffn_x32', 64: 'k_ffn1_x64+k_ffn2_x64'}[e]
    from test_route_cpu import fft_path_by_size
    fft = fft_path_by_size(H >> level, W >> level, False)
    assert lines[0].split(' fwd: ')[1] == f'ffn={ffn} arith=f16x2 hidden=fp32 | mixer=k_attn_m arith=f16x2 | fft={fft}', lines[0]


def _fills_agree(ops, tag, call, stale_call=None):
    """call() on the 'nan' and the 'big' fill, then (backward entries) on what stale_call() left: equal bits, finite"""
    ref = None
    for st in ('nan', 'big') + (('stale',) if stale_call is not None else ()):
        if st == 'stale':
            ops.ws_fill = 'big'
            stale_call()
        ops.ws_fill = st
        got = [t.clone() for t in call()]
        if ref is None:
            ref = got
            assert all(bool(torch.isfinite(t).all()) for t in got), (tag, st, 'not finite')
        else:
            for i, (a, b) in enumerate(zip(ref, got)):
                if not _same(a, b):
                    name = None
                    if i == 1:        # the flat gradient buffer
                        j = int((_bits(a) != _bits(b)).nonzero().flatten()[0])
                        name = ops.eng.names[max(k for k, o in enumerate(ops.eng.offsets) if o <= j)]
                    assert False, (tag, f"result {i} differs between the workspace states '{st}' and 'nan'", int((_bits(a) != _bits(b)).sum()), name,
                                   'finite', bool(torch.isfinite(b).all()))
    ops.ws_fill = 'nan'


# (C, blk, B, H, W, which): FFN (2) -- one strip only; 576 strips on a grid of 512 (e = 16) and 288 on 256 (e = 32); the level-1 fallback planes 8 x 24 and
# 40 x 24.  Mixer (0: global, 1: half-block) -- 45 level-1 windows (a last group of one); 1280 windows on 256 workgroups.  Blocks 1 / 3 / 4 at (3, 48, 32)
BLOCK_CASES = ([(4, 0, 1, 16, 16, (2,)), (4, 0, 9, 128, 128, (2,)), (8, 0, 9, 128, 128, (2,)), (4, 2, 3, 16, 48, (2,)), (4, 2, 3, 80, 48, (0, 1, 2)),
                (4, 0, 5, 128, 128, (0, 1)), (8, 0, 5, 128, 128, (0, 1))] + [(4, blk, 3, 48, 32, (0, 1, 2)) for blk in (1, 3, 4)])


@pytest.mark.parametrize('C,blk,B,H,W,whiches', BLOCK_CASES)
def test_half_block_entries_on_a_poisoned_workspace(C, blk, B, H, W, whiches):
    """lg_op_block and lg_op_block_bwd (which = 0, 1, 2 as listed): route first, then 'nan' against 'big', and for the backward against 'stale' (the same
    entry on another x and a dy 2^10 times larger)"""
    from helpers import block_features
    from test_gpu_backward_shapes import _assert_route, _ffn_route, _level, _mixer_route, _width
    ops = _ops(C, H, W)
    _fwd_route(ops, H, W, _level(blk), _width(C, blk))
    _assert_route(ops, H, W, _level(blk), ffn=_ffn_route(C, blk, H, W), mixer=_mixer_route(C, blk))
    x = block_features(C, blk, B, H, W).cuda()
    rng = np.random.default_rng([77, C, blk, H, W])
    x_stale = torch.from_numpy(rng.standard_normal(tuple(x.shape)).astype(np.float32)).cuda()
    for which in whiches:
        shape = (B, x.shape[3] // 2, x.shape[1], x.shape[2]) if which == 0 else tuple(x.shape)
        dy = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
        dy_stale = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) * 1024.0).cuda()
        tag = f'C={C} blk={blk} ({B},{H},{W}) which={which}'
        _fills_agree(ops, 'lg_op_block ' + tag, lambda: [ops.block(0, blk, which, x, guard=True)])
        _fills_agree(ops, 'lg_op_block_bwd ' + tag, lambda: ops.block_bwd(0, blk, which, x, dy, guard=True),
                     lambda: ops.block_bwd(0, blk, which, x_stale, dy_stale))


@pytest.mark.parametrize('C,B,H,W', [(4, 2, 16, 48), (4, 3, 80, 48), (8, 2, 48, 48)])
def test_lgt_entries_on_a_poisoned_workspace(C, B, H, W):
    """lg_op_lgt with and without LG_FLAG_SAVE, lg_op_lgt_bwd (stage 1 of K = 2, dropout on): ragged window groups and the level-1 fallback planes
    8 x 24 / 40 x 24 inside one LGT"""
    from helpers import lgt_input
    from lgteun_amd import _lib
    from test_gpu_backward_shapes import _assert_route, _ffn_route, _mixer_route
    ops = _ops(C, H, W, K=2)
    for level, blk in ((0, 0), (1, 2)):
        _assert_route(ops, H, W, level, ffn=_ffn_route(C, blk, H, W), mixer=_mixer_route(C, blk))
    z = lgt_input(C, B, H, W).cuda()
    rng = np.random.default_rng([78, C, H, W])
    dy = torch.from_numpy(rng.standard_normal(tuple(z.shape)).astype(np.float32)).cuda()
    z_stale = torch.from_numpy(rng.uniform(0, 1, tuple(z.shape)).astype(np.float32)).cuda()
    tag = f'C={C} ({B},{H},{W})'
    _fills_agree(ops, 'lg_op_lgt ' + tag, lambda: [ops.lgt(1, z, guard=True)])
    _fills_agree(ops, 'lg_op_lgt SAVE ' + tag, lambda: [ops.lgt(1, z, flags=_lib.LG_FLAG_SAVE | _lib.LG_FLAG_DROPOUT, seed=SEED, guard=True)])
    _fills_agree(ops, 'lg_op_lgt_bwd ' + tag, lambda: ops.lgt_bwd(1, z, dy, flags=_lib.LG_FLAG_DROPOUT, seed=SEED, guard=True),
                 lambda: ops.lgt_bwd(1, z_stale, dy * 1024.0, flags=_lib.LG_FLAG_DROPOUT, seed=SEED_STALE))


@pytest.mark.parametrize('B,C,H,W', [(1, 4, 16, 16), (3, 8, 80, 48), (5, 4, 64, 64)])
def test_data_step_backward_entry_on_a_poisoned_workspace(B, C, H, W):
    """lg_op_data_step_bwd (stage 1 of K = 2): the 4 x 4 MS plane, tiles on a plane that is no multiple of 32, the one-launch form at an odd batch"""
    ops = _ops(C, H, W, K=2)
    net_line = ops.eng.describe(H, W).splitlines()[0]
    assert ('dstep=fused' if (H, W) == (64, 64) else 'dstep=tiles') in net_line.split(': ')[1].split(), net_line
    rng = np.random.default_rng([79, C, H, W])

    def draw(scale=1.0):
        z = torch.from_numpy(rng.uniform(0, 1, (B, C, H, W)).astype(np.float32)).cuda()
        ms = torch.from_numpy(rng.uniform(0, 1, (B, C, H // 4, W // 4)).astype(np.float32)).cuda()
        pan = torch.from_numpy(rng.uniform(0, 1, (B, 1, H, W)).astype(np.float32)).cuda()
        return z, ms, pan, (torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32)) * scale).cuda()
    real, stale = draw(), draw(1024.0)
    _fills_agree(ops, f'lg_op_data_step_bwd C={C} ({B},{H},{W})', lambda: ops.data_step_bwd(1, *real, guard=True), lambda: ops.data_step_bwd(1, *stale))


@pytest.mark.parametrize('grid_cap', [0, 5])
def test_lgt_stages_entry_on_a_poisoned_workspace(grid_cap):
    """lg_op_lgt_stages, n = 2 of K = 3 at (4, 32, 32), B = 3, dropout on: the transient buffers carved for (K-1) B samples.  grid_cap = 5 gives a workgroup
    of the persistent kernels samples of two stages (tests/test_gpu_stage_batch.py)"""
    from lgteun_amd import _lib
    ops = _ops(4, 32, 32, K=3)
    z = torch.from_numpy(np.random.default_rng(80).uniform(0, 1, (2, 3, 4, 32, 32)).astype(np.float32)).cuda()
    _fills_agree(ops, f'lg_op_lgt_stages grid_cap={grid_cap}',
                 lambda: [ops.lgt_stages(0, 2, z, flags=_lib.LG_FLAG_DROPOUT, seed=SEED, grid_cap=grid_cap, guard=True)])


# ---- (f) backward twice on one saved forward
@pytest.mark.parametrize('C,B', [(4, 2), (8, 1)])
@pytest.mark.parametrize('drop', [0, 1])
def test_second_backward_on_one_forward_is_a_fresh_backward(C, B, drop):
    """default route, K = 2, 32 x 32: backward(dout1) then backward(dout2) on the same saved forward, each into a zeroed gradient buffer; the second result
    is bit for bit that of a fresh forward + backward(dout2).  dout2 = dout1 * 2^-20 (word 6 of ffn_scales, max |dh2|, is an atomic max: it must start
    at zero in every backward, not at the first backward's maximum) and dout2 an unrelated draw of the same scale"""
    net = Net(C, 2, 32, 32, B, 1)
    flags = FAITHFUL | SAVE | (DROPOUT if drop else 0)
    ms, pan, dout1 = net.inputs(5)
    unrelated = net.inputs(11)[2]
    for name, dout2 in (('dout1 * 2^-20', (dout1 * 2.0 ** -20).contiguous()), ('an unrelated draw', unrelated)):
        net.fill('nan')
        rc, _ = net.forward(ms, pan, flags)
        assert rc == 0, net.lib.lg_last_error()
        assert net.backward(ms, pan, dout1, flags) == 0, net.lib.lg_last_error()
        assert net.backward(ms, pan, dout2, flags) == 0, net.lib.lg_last_error()
        second = net.grads.clone()
        net.fill('nan')
        rc, _ = net.forward(ms, pan, flags)
        assert rc == 0, net.lib.lg_last_error()
        assert net.backward(ms, pan, dout2, flags) == 0, net.lib.lg_last_error()
        fresh = net.grads.clone()
        assert bool(torch.isfinite(fresh).all()) and float(fresh.norm()) > 0
        assert _same(second, fresh), (f'C={C} B={B} dropout={drop}: the second backward ({name}) is not a fresh backward',
                                      'first gradient tensor, floats, rel-L2', net.first_difference(second, fresh))


def test_retain_graph_second_backward_is_a_fresh_backward():
    """the same through the autograd bridge (_LgteunFn) with retain_graph=True"""
    from gpu_helpers import make_module
    net = make_module(4, 2)
    eng = net.engine()
    ms, pan, gt = (torch.from_numpy(a).cuda() for a in dw.make_inputs(2, 4, 8, 8, seed=5, kind='smooth'))
    dout1 = (gt - gt.mean()).contiguous()
    dout2 = (dout1 * 2.0 ** -20).contiguous()
    live = [eng.params[i] for i in eng.live_idx]
    with torch.enable_grad():
        out = eng.forward_autograd(ms, pan, False)
        assert out.requires_grad
        torch.autograd.grad(out, live, dout1, retain_graph=True)
        second = torch.autograd.grad(out, live, dout2)
        fresh = torch.autograd.grad(eng.forward_autograd(ms, pan, False), live, dout2)
    bad = [eng.names[i] for i, a, b in zip(eng.live_idx, second, fresh) if not _same(a, b)]
    assert not bad, ('the second backward of a retained graph is not a fresh backward', len(bad), bad[:4])


# ---- (g) rejections
@pytest.mark.parametrize('how', ['one byte short', 'null workspace'])
def test_rejected_calls_launch_nothing(how):
    """lgteun_forward / lgteun_backward / lgteun_dead_forward with workspace_bytes = need - 1 or a null workspace: an error code, a message in
    lg_last_error, and out, the gradient buffer and the poisoned workspace untouched"""
    net = Net(4, 3, 32, 32, 2, 1)
    ms, pan, dout = net.inputs(5)
    flags = FAITHFUL | SAVE | DEFER_DEAD
    kw = dict(nbytes=net.need - 1) if how == 'one byte short' else dict(ws=False)
    sentinel = (torch.arange(net.eng.total, device=net.eng.device) % 251 + 1).float() * 2.0 ** -100
    net.fill('big')

    def untouched(what):
        torch.cuda.synchronize()
        assert bool((net.ws == 0x5A).all()), (what, 'the workspace was written')
        assert _same(grads, sentinel), (what, 'the gradient buffer was written')
        net.guards(what)

    grads = sentinel.clone()
    rc, out = net.forward(ms, pan, flags, **kw)
    assert rc != 0 and net.lib.lg_last_error(), ('lgteun_forward', how, rc)
    assert bool(torch.isnan(out).all()), ('lgteun_forward', how, 'out was written')
    untouched('lgteun_forward')
    rc = net.backward(ms, pan, dout, flags, zero=False, grads=grads, **kw)
    assert rc != 0 and net.lib.lg_last_error(), ('lgteun_backward', how, rc)
    untouched('lgteun_backward')
    rc = net.dead_forward(flags, **kw)
    assert rc != 0 and net.lib.lg_last_error(), ('lgteun_dead_forward', how, rc)
    untouched('lgteun_dead_forward')
