"""The live stage's slot of the transient forward buffers (csrc/workspace.h: carve, live_view), read from the host through lg_debug_live_slot.  No device.

A plan that batches its dead stages (C = 4, K - 1 >= 2) carves xin / xmid / xout / g / o2 of every block for K slots of B samples; the live stage owns
slot K-1 on every path.  Any other plan (K = 2, C = 8) keeps one slot, and chained training (train = 2) one set per stage: their live view is the
buffers themselves and their sizes are what they were (tests/golden/workspace_bytes.json, K = 2: tests/test_route_cpu.py)."""
import ctypes
import json
import os

import pytest

from lgteun_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIELDS = ('xin', 'xmid', 'xout', 'g', 'o2')


class Plan:
    def __init__(self, C, K, H, W, prec=0):
        self.lib = _lib.lib()
        self.handle = ctypes.c_void_p()
        n_off = 12 + K + 119 * K
        offs = (ctypes.c_int64 * n_off)(*[4 * i for i in range(n_off)])
        cfg = _lib.LgConfig(C, K, H, W, prec, 0)
        assert self.lib.lg_plan_create(ctypes.byref(cfg), offs, n_off, ctypes.byref(self.handle)) == 0, self.lib.lg_last_error()
        self.C, self.K, self.H, self.W = C, K, H, W

    def slot(self, B, train):
        out = (ctypes.c_size_t * 53)()
        assert self.lib.lg_debug_live_slot(self.handle, B, train, out) == 0, self.lib.lg_last_error()
        bufs = {}
        for j in range(5):
            for f, name in enumerate(FIELDS):
                bufs[(j, name)] = (out[3 + 10 * j + 2 * f], out[3 + 10 * j + 2 * f + 1])
        return {'end': out[0], 'bwd': out[1], 's0': out[2], 'bufs': bufs}

    def sample_bytes(self, j, name):
        """bytes of one sample of block j's buffer: level 1 (block 2) has e = 8 C channels on H/2 x W/2, the planar halves e / 2"""
        e, h, w = (8 * self.C, self.H // 2, self.W // 2) if j == 2 else (4 * self.C, self.H, self.W)
        return h * w * (e // 2 if name in ('g', 'o2') else e) * 4

    def bytes(self, B, train):
        return int(self.lib.lg_workspace_bytes(self.handle, B, train))

    def __del__(self):
        if self.handle:
            self.lib.lg_plan_destroy(self.handle)


@pytest.mark.parametrize('K', [3, 4])
@pytest.mark.parametrize('B,n', [(1, 32), (3, 64), (2, 128)])
@pytest.mark.parametrize('train', [0, 1])
def test_k_slots_and_the_live_stage_in_the_last(K, B, n, train):
    p = Plan(4, K, n, n)
    s = p.slot(B, train)
    assert p.bytes(B, train) == s['end'] + s['bwd'] and (s['bwd'] > 0) == bool(train)
    assert s['s0'] == (K - 1) * B
    starts = sorted({base for base, _ in s['bufs'].values()}) + [s['end']]
    for (j, name), (base, live) in s['bufs'].items():
        per = p.sample_bytes(j, name)
        assert base % 256 == 0 and live == base + (K - 1) * B * per, (j, name)
        nxt = min(x for x in starts if x > base)          # the next buffer of the carving (blocks 1 and 4 read their predecessor's xout: same start)
        assert base + K * B * per <= nxt, (j, name, 'K slots overlap the next buffer')
        assert live + B * per <= s['end']
    assert s['bufs'][(1, 'xin')] == s['bufs'][(0, 'xout')] and s['bufs'][(4, 'xin')] == s['bufs'][(3, 'xout')]


@pytest.mark.parametrize('C,K,train', [(4, 2, 0), (4, 2, 1), (8, 2, 1), (8, 3, 0), (8, 4, 1), (4, 3, 2), (4, 4, 2), (4, 1, 1)])
def test_other_plans_keep_one_slot(C, K, train):
    """K = 2 (one dead stage), C = 8 (stage by stage) and chained training: no slots, the live view is the carving itself"""
    p = Plan(C, K, 64, 64)
    s = p.slot(2, train)
    assert s['s0'] == 0 and all(base == live for base, live in s['bufs'].values())
    assert p.bytes(2, train) == s['end'] + s['bwd']


def test_k2_sizes_are_the_recorded_ones():
    with open(os.path.join(GOLD, 'workspace_bytes.json')) as f:
        gold = json.load(f)
    assert gold['K'] == 2
    n = 0
    for c in gold['cases']:
        if c['variant'] != 0:
            continue
        p = Plan(c['C'], 2, c['H'], c['W'], c['precision'])
        assert [p.bytes(B, t) for B in (1, 2) for t in (0, 1, 2)] == c['bytes'], c
        n += 1
    assert n > 0


def test_invalid_arguments_are_refused():
    p = Plan(4, 3, 32, 32)
    out = (ctypes.c_size_t * 53)()
    assert p.lib.lg_debug_live_slot(p.handle, 0, 0, out) == -1 and p.lib.lg_debug_live_slot(p.handle, 1, 3, out) == -1
    assert p.lib.lg_debug_live_slot(None, 1, 0, out) == -1 and p.lib.lg_debug_live_slot(p.handle, 1, 0, None) == -1
