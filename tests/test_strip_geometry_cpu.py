"""The launch geometry of the strip-walking kernels (csrc/kernels.h: strip_geometry), read from the host through lg_debug_stage_decision
(kind 0 = k_ffn_xr on 512 workgroups).  No device: the entry launches nothing.

The rule is restated here, not imported: 16-column strips; the strip height is the tallest multiple of 8 rows that still yields a strip per
resident workgroup, at least 16, taken from ONE stage's batch when the launch covers several; the grid is one workgroup per strip up to the
resident count, and (several stages only) up to the test cap."""
import ctypes

import pytest

WGS = 512
HS, WS, BS = range(8, 257, 8), range(16, 257, 16), (1, 2, 3, 4, 8, 16, 32, 48, 64)


def _rule(h, w, B, B_height, wgs, grid_cap):
    tiles_x = (w + 15) // 16
    SH = (h + 7) // 8 * 8
    while SH > 16 and B_height * tiles_x * ((h + SH - 1) // SH) < wgs:
        SH = (SH // 2 + 7) // 8 * 8
    strips_y = (h + SH - 1) // SH
    nstrips = B * tiles_x * strips_y
    grid = min(nstrips, wgs)
    if grid_cap > 0 and grid > grid_cap:
        grid = grid_cap
    return SH, tiles_x, strips_y, grid, nstrips


@pytest.mark.parametrize('n,grid_cap', [(1, 0), (3, 0), (3, 96)])
def test_strip_geometry_is_the_rule(n, grid_cap):
    from lgteun_amd import _lib as lib_mod
    L = lib_mod.lib()
    out = (ctypes.c_int32 * 8)()
    for h in HS:
        for w in WS:
            for Bs in BS:
                assert L.lg_debug_stage_decision(0, h, w, Bs, n, grid_cap, out) == 0, L.lg_last_error()
                uneven, _, units, _, grid, SH, tiles_x, strips_y = out
                nstrips = units * 2 if uneven else units       # an uneven launch reports strip PAIRS
                # one stage: its own batch sets the height and there is no cap; several: the batch of one stage, and the cap holds
                assert (SH, tiles_x, strips_y, grid, nstrips) == _rule(h, w, Bs * n, Bs, WGS, grid_cap if n > 1 else 0), (h, w, Bs)
