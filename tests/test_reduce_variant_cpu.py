"""The diagnostic switch of the parameter-gradient reduce launches (lg_config.variant LG_VAR_REDUCE_PER_BLOCK): the Python name, the
environment variable and the header agree, and a plan accepts the bit."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reduce_per_block_bit_matches_the_header_and_is_accepted():
    from lgteun_amd import _lib
    assert _lib.variant_from_env({'LG_REDUCE': 'per_block'}) == _lib.LG_VAR_REDUCE_PER_BLOCK == 1 << 17
    assert _lib.variant_from_env({'LG_REDUCE': 'merged'}) == 0
    hdr = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    a, b = re.search(r'#define LG_VAR_REDUCE_PER_BLOCK \((\d+)u << (\d+)\)', hdr).groups()
    assert int(a) << int(b) == _lib.LG_VAR_REDUCE_PER_BLOCK
    assert int(re.search(r'#define LG_VAR_ALL (0x[0-9a-f]+)u', hdr).group(1), 16) & _lib.LG_VAR_REDUCE_PER_BLOCK
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.lg_plan_create.restype = ctypes.c_int32
    n = 12 + 2 + 119 * 2
    offs = (ctypes.c_int64 * n)(*[4 * i for i in range(n)])
    out = ctypes.c_void_p()
    cfg = _lib.LgConfig(4, 2, 32, 32, 0, _lib.LG_VAR_REDUCE_PER_BLOCK)
    assert L.lg_plan_create(ctypes.byref(cfg), offs, n, ctypes.byref(out)) == 0
    L.lg_plan_destroy.argtypes = [ctypes.c_void_p]
    L.lg_plan_destroy(out)


def _disjoint(jobs):
    """jobs: (dst offset, dst2 offset or -1, rows, cols, row pitch) -> 0 or the library's error code"""
    from lgteun_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    n = len(jobs)
    ll, ii = ctypes.c_longlong * n, ctypes.c_int * n
    L.lg_debug_reduce_disjoint.restype = ctypes.c_int
    L.lg_debug_reduce_disjoint.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong),
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    rc = L.lg_debug_reduce_disjoint(n, ll(*[j[0] for j in jobs]), ll(*[j[1] for j in jobs]), ii(*[j[2] for j in jobs]),
                                    ii(*[j[3] for j in jobs]), ii(*[j[4] for j in jobs]))
    L.lg_last_error.restype = ctypes.c_char_p
    return rc, L.lg_last_error()


def test_merged_reduce_launch_refuses_jobs_that_share_a_destination_element():
    """the host-side check behind every new job table of a merged reduce launch (no GPU involved): disjoint and interleaved destinations
    pass, any shared element is an error instead of a launch"""
    ok = [
        [(0, -1, 1, 64, 64), (64, -1, 1, 64, 64)],                                  # neighbours
        [(k, -1, 4, 1, 9) for k in range(9)] + [(36, -1, 1, 4, 4)],                # the nine taps of a [4][3][3] depthwise weight, then its bias
        [(0, -1, 16, 16, 32), (16, -1, 16, 16, 32)],                                # the two halves of the fusion conv's weight (row pitch 2 E)
        [(0, 100, 4, 1, 1), (4, -1, 4, 1, 1), (104, -1, 1, 4, 4)],                  # a second destination next to other jobs
        [(0, -1, 48, 16, 16), (768, -1, 1, 48, 48)],
    ]
    for jobs in ok:
        assert _disjoint(jobs)[0] == 0, jobs
    bad = [
        [(0, -1, 1, 64, 64), (63, -1, 1, 64, 64)],                                  # one element shared by two rows
        [(0, -1, 1, 64, 64), (0, -1, 1, 32, 32)],                                   # same start, other shape (not a chain)
        [(k, -1, 4, 1, 9) for k in range(9)] + [(27, -1, 1, 4, 4)],                # a bias laid over the last channel's taps
        [(0, -1, 16, 17, 32), (16, -1, 16, 16, 32)],                                # column windows that meet
        [(0, -1, 16, 16, 32), (16, -1, 16, 16, 48)],                                # interleaved with another pitch: not provably disjoint
        [(0, 100, 4, 1, 1), (102, -1, 1, 4, 4)],                                    # a second destination under another job
    ]
    for jobs in bad:
        rc, msg = _disjoint(jobs)
        assert rc == -4 and b'same gradient elements' in msg, (jobs, rc, msg)
