"""The partition of a persistent multi-stage launch (csrc/kernels.h: stage_run_halves / stage_run_chunk, stage_seg_end), read from the host
through lg_debug_stage_runs, and the launchers' decision for a shape (lg_debug_stage_decision).  No device: the entries launch nothing.

k_ffn_xr (kind 0): split 0 = `units` strips in even runs; split != 0 = `units` strip PAIRS, workgroups j and j + grid/2 on the same run of
pairs, the second at strip base `units`.  k_attn_m (kind 1): `units` window quads; split = eighths of a CU's chunk to its first workgroup
(workgroup c of the first half of the grid; c + grid/2 takes the rest), 4 = even runs."""
import ctypes

import pytest

XR, ATTN = 0, 1


def _lib():
    from lgteun_amd import _lib as lib_mod
    return lib_mod.lib()


def _segments(kind, units, per_stage, grid, split):
    """{workgroup: [(seg0, seg1, stage, base), ...]} in the order the entry reports them"""
    L = _lib()
    cap = grid + units // per_stage * 2 + 8
    out = (ctypes.c_int32 * (5 * cap))()
    rows = L.lg_debug_stage_runs(kind, units, per_stage, grid, split, out, cap)
    assert 0 < rows <= cap, (rows, L.lg_last_error())
    segs = {}
    last_wg = -1
    for i in range(rows):
        wg, s0, s1, st, base = out[5 * i:5 * i + 5]
        assert wg >= last_wg
        last_wg = wg
        segs.setdefault(wg, []).append((s0, s1, st, base))
    assert sorted(segs) == list(range(grid))
    return segs


def _runs(segs):
    """{workgroup: (run0, run1, base)}; the segments of a run are contiguous and ascend"""
    runs = {}
    for wg, ss in segs.items():
        for (a0, a1, _, ba), (b0, _, _, bb) in zip(ss, ss[1:]):
            assert a1 == b0 and ba == bb
        assert all(s0 < s1 for s0, s1, _, _ in ss), (wg, ss)                 # no empty segment, so no empty run: units ascend
        runs[wg] = (ss[0][0], ss[-1][1], ss[0][3])
    return runs


def _check_segments(segs, per_stage, n):
    for wg, ss in segs.items():
        stages = [st for _, _, st, _ in ss]
        assert stages == sorted(set(stages)), (wg, ss)                       # one segment per stage, ascending
        for s0, s1, st, _ in ss:
            assert 0 <= st < n and st * per_stage <= s0 < s1 <= (st + 1) * per_stage, (wg, s0, s1, st)


# (units, per_stage, grid): configs[1]'s strips (1536 on 512), chunk sizes that are no whole number, 2 - 3 stages, a grid of 5 (the test cap)
EVEN = [(1536, 512, 512), (6144, 2048, 512), (2304, 768, 512), (36, 12, 5), (36, 12, 36), (24, 12, 24), (3072, 1024, 500), (1000, 500, 7),
        (768, 256, 512), (9, 3, 5)]


@pytest.mark.parametrize('kind', [XR, ATTN])
@pytest.mark.parametrize('units,per_stage,grid', EVEN)
def test_even_split_is_the_strip_run_partition(kind, units, per_stage, grid):
    """split at 'even': exactly (w units // grid, (w + 1) units // grid), base 0 -- the partition every multi-stage launch had before"""
    segs = _segments(kind, units, per_stage, grid, 0 if kind == XR else 4)
    runs = _runs(segs)
    assert runs == {w: (w * units // grid, (w + 1) * units // grid, 0) for w in range(grid)}
    _check_segments(segs, per_stage, units // per_stage)


# (pairs, pairs per stage, grid): configs[1] (768 pairs over 256 workgroup pairs, 3 stages), the GPU test's shape (the same counts at PAN 64, and
# 2 stages: 512 pairs), grids whose chunk is no whole number of pairs
PAIRS = [(768, 256, 512), (512, 256, 512), (768, 256, 500), (1000, 500, 14), (999, 333, 200), (6, 3, 4), (256, 128, 512)]


@pytest.mark.parametrize('dS', [8, 16, 24])
@pytest.mark.parametrize('units,per_stage,grid', PAIRS)
def test_ffn_pairs(units, per_stage, grid, dS):
    segs = _segments(XR, units, per_stage, grid, dS)
    runs = _runs(segs)
    hg = grid // 2
    taken = [0] * (2 * units)
    for j in range(hg):
        a, b = runs[j], runs[j + hg]
        assert a[:2] == b[:2] == (j * units // hg, (j + 1) * units // hg)    # the two workgroups of a CU: the same run of pairs ...
        assert a[2] == 0 and b[2] == units                                   # ... the tall strips and the short ones (strip = pair + base)
        assert [s[:3] for s in segs[j]] == [s[:3] for s in segs[j + hg]]     # and the same stage segments
        for r0, r1, base in (a, b):
            for p in range(r0, r1):
                taken[p + base] += 1
    assert taken == [1] * (2 * units)                                        # every strip exactly once
    _check_segments(segs, per_stage, units // per_stage)
    if (units, per_stage, grid) == (768, 256, 512):
        assert all(r1 - r0 == 3 for r0, r1, _ in runs.values())
        assert [s[:3] for s in segs[85]] == [(255, 256, 0), (256, 258, 1)]   # workgroup pair 85 crosses into stage 1


# (quads, quads per stage, grid): configs[1] level 0 and level 1 on 512 workgroups; the GPU test's shape (3072 / 768 quads, and 2 stages);
# chunks that are no whole number of quads
QUADS = [(6144, 2048, 512), (1536, 512, 512), (3072, 1024, 512), (768, 256, 512), (2048, 1024, 512), (512, 256, 512), (1000, 500, 14),
         (999, 333, 200), (700, 350, 512 // 2), (12, 4, 6)]


@pytest.mark.parametrize('u', [1, 3, 4, 5, 6, 7])
@pytest.mark.parametrize('units,per_stage,grid', QUADS)
def test_attn_chunks(units, per_stage, grid, u):
    segs = _segments(ATTN, units, per_stage, grid, u)
    runs = _runs(segs)
    if u == 4:
        assert runs == {w: (w * units // grid, (w + 1) * units // grid, 0) for w in range(grid)}
        return
    hg = grid // 2
    taken = [0] * units
    for c in range(hg):
        c0, c1 = c * units // hg, (c + 1) * units // hg
        (a0, a1, ab), (b0, b1, bb) = runs[c], runs[c + hg]
        assert (a0, a1, b1) == (c0, b0, c1) and ab == bb == 0                # the two workgroups of a CU cover exactly its chunk, first then second
        assert a1 > a0 and b1 > b0
        assert abs((a1 - a0) - (c1 - c0) * u / 8) <= 1                       # the first one's share: the requested eighths to within a quad
        for q in range(c0, c1):
            taken[q] += 1
    assert taken == [1] * units
    _check_segments(segs, per_stage, units // per_stage)
    if (units, grid, u) == (6144, 512, 5):
        assert all(runs[c][1] - runs[c][0] == 15 and runs[c + hg][1] - runs[c + hg][0] == 9 for c in range(hg))
    if (units, grid, u) == (1536, 512, 5):
        assert all(runs[c][1] - runs[c][0] == 4 and runs[c + hg][1] - runs[c + hg][0] == 2 for c in range(hg))


def test_invalid_arguments():
    L = _lib()
    out = (ctypes.c_int32 * 40)()
    assert L.lg_debug_stage_runs(2, 12, 4, 4, 0, out, 8) == -1               # kind
    assert L.lg_debug_stage_runs(XR, 12, 5, 4, 0, out, 8) == -1              # no whole stages
    assert L.lg_debug_stage_runs(XR, 12, 4, 13, 0, out, 8) == -1             # more workgroups than units
    assert L.lg_debug_stage_runs(ATTN, 12, 4, 5, 5, out, 8) == -2            # an uneven split of an odd grid
    assert L.lg_debug_stage_runs(ATTN, 12, 4, 4, 8, out, 8) == -2
    assert L.lg_debug_stage_runs(XR, 12, 4, 4, 0, out, 2) == 6               # rows wanted: 4 runs, 2 of them cross a stage boundary
    assert L.lg_debug_stage_decision(3, 32, 32, 3, 2, 0, out) == -1


def _decision(kind, h, w, Bs, n, grid_cap=0):
    L = _lib()
    out = (ctypes.c_int32 * 8)()
    assert L.lg_debug_stage_decision(kind, h, w, Bs, n, grid_cap, out) == 0, L.lg_last_error()
    return list(out)


def test_launcher_decision():
    """C = 4, PAN 128 x 128, 32 samples per stage, 3 stages (configs[1]) takes the uneven form in all three kernels; the same shape under the
    test cap of 5 workgroups does not, nor do PAN 32 with B = 3 and a K = 2 module's single dead stage"""
    from lgteun_amd import _lib as lib_mod
    assert lib_mod.LG_ABI_VERSION == _lib().lg_abi_version() == 2           # additions only
    uneven, dS, units, per_stage, grid, SH, tiles_x, strips_y = _decision(0, 128, 128, 32, 3)
    assert (units, per_stage, grid, SH, tiles_x, strips_y) == (768, 256, 512, 64, 8, 2)
    assert uneven == 1 and dS == 16
    uneven, u, quads, per_stage, grid, nwin, _, _ = _decision(8, 128, 128, 32, 3)
    assert (quads, per_stage, grid, nwin) == (6144, 2048, 512, 24576) and (uneven, u) == (1, 5)
    uneven, u, quads, per_stage, grid, nwin, _, _ = _decision(16, 64, 64, 32, 3)
    assert (quads, per_stage, grid, nwin) == (1536, 512, 512, 6144) and (uneven, u) == (0, 4)     # left even: 4 : 2 measured slower (csrc/k_attn_m.hip)
    # the cap of the existing re-staging test: even strip runs / quad runs on 5 workgroups
    assert _decision(0, 128, 128, 32, 3, 5)[:5] == [0, 0, 1536, 512, 5]
    assert _decision(8, 128, 128, 32, 3, 5)[:5] == [0, 4, 6144, 2048, 5]
    assert _decision(16, 64, 64, 32, 3, 5)[:5] == [0, 4, 1536, 512, 5]
    # PAN 32, B = 3: 36 strips of 16 rows on 36 workgroups, 36 and 9 quads
    assert _decision(0, 32, 32, 3, 3)[:6] == [0, 0, 36, 12, 36, 16]
    assert _decision(8, 32, 32, 3, 3)[:5] == [0, 4, 36, 12, 36]
    assert _decision(8, 32, 32, 4, 3)[:5] == [0, 4, 48, 16, 48]
    # one stage per launch (K = 2): the one-stage launch's own rule; at this size it is not the measured one
    assert _decision(0, 32, 32, 3, 1)[:2] == [0, 0]
    assert _decision(8, 32, 32, 4, 1)[:2] == [0, 4]
    # a cap that does not bite changes nothing
    assert _decision(0, 128, 128, 32, 3, 512) == _decision(0, 128, 128, 32, 3)
    assert _decision(8, 128, 128, 32, 3, 600) == _decision(8, 128, 128, 32, 3)
    # FFN: a plane that is no whole number of strip pairs (72 rows: strips of 40 and 32) keeps the even strip runs
    assert _decision(0, 72, 128, 32, 3)[:2] == [0, 0] and _decision(0, 72, 128, 32, 3)[4] == 512
