"""Helper, not a test: what tests/test_gpu_abi_limits.py and tests/test_abi_limits_cpu.py share -- the probe arithmetic around element offset
2^31, input makers whose samples are all distinct, the memory gate, a peak-memory / time reporter, and one raw C-ABI call per classical
method with a workspace of the test's own that is freed with the call and synchronised behind it (the wrappers of lgteun_amd/classical.py,
mtf_glp.py and bdsd.py allocate theirs per call too, but return stats and outputs in their own shapes and do not synchronise).

Nothing here imports torch at module level, so the CPU file can use the arithmetic without it."""
import ctypes
import time

import numpy as np

TWO31, TWO32 = 1 << 31, 1 << 32
GIB = 1 << 30
LIMIT_BYTES = 16 * GIB                  # what one test may allocate
HEADROOM_BYTES = 2 * GIB                # free memory a test wants beyond its own need
FAKE = 1 << 32                          # a non-null, 4 KiB-aligned integer that is never dereferenced: validators reject the call first
POOL = 16                               # distinct host-made samples behind a large classical batch


# ------------------------------------------------------------------------------------------------------------------------
# probe arithmetic (no device)
# ------------------------------------------------------------------------------------------------------------------------
def boundary_unit(unit_elems, boundary=TWO31):
    """the unit (sample, item, plane, row ...) of `unit_elems` elements that holds element offset `boundary` of a contiguous tensor"""
    return boundary // unit_elems


def probe_units(n_units, unit_elems):
    """first unit, the unit below and the unit holding element offset 2^31, last unit -- sorted, without repeats.  The tensor must cross 2^31."""
    assert n_units * unit_elems > TWO31, (n_units, unit_elems, 'the tensor does not reach element 2^31')
    k = boundary_unit(unit_elems)
    assert 1 <= k < n_units
    return sorted({0, k - 1, k, n_units - 1})


def alias_partners(b, n_units, unit_sizes):
    """the units whose offset differs from unit b's by 2^31 or 2^32 elements in a tensor of the call: a 32-bit index that wrapped would land on
    one of them.  unit_sizes: elements per unit of every tensor of the call (inputs, outputs, workspace planes).  Where the distance is no
    whole number of units, the unit on either side is a partner."""
    out = set()
    for u in unit_sizes:
        for dist in (TWO31, TWO32):
            for d in {dist // u, -(-dist // u)}:
                for p in (b - d, b + d):
                    if 0 <= p < n_units and p != b:
                        out.add(p)
    return sorted(out)


def distinct_gains(n, seed=0):
    """n float32 gains in [0.5, 1], all different: a seeded permutation of an evenly spaced ladder (adjacent steps are 0.5 / n >= 7e-6 for
    n <= 65535, far above the spacing of float32 in that range)"""
    g = (0.5 + 0.5 * np.arange(n, dtype=np.float64) / max(n - 1, 1)).astype(np.float32)
    assert len(np.unique(g)) == n and g.min() >= 0.5 and g.max() <= 1.0
    return g[np.random.default_rng(seed).permutation(n)]


# ------------------------------------------------------------------------------------------------------------------------
# the network entries (tests/test_net_abi_cpu.py, tests/test_gpu_net_limits.py): the header's batch bound restated, plans made on the host
# ------------------------------------------------------------------------------------------------------------------------
F_FAITHFUL, F_SAVE, F_DROPOUT, F_BWD_LGT, F_BWD_DATA, F_CHAINED, F_DEFER_DEAD, F_STAGEWISE, F_LIVE_APART = 1, 2, 4, 8, 16, 32, 64, 128, 256
F_DEFINED = 0x1ff
F_UNDEFINED_BIT = 1 << 9
GRID_YZ_MAX, INT_MAX = 65535, TWO31 - 1


def net_stage_slots(C, K, H, W, train):
    """S of include/lgteun_hip.h: the stages whose samples one launch may see"""
    return K if (C == 4 and K >= 3 and H <= 128 and W <= 128 and train != 2) else 1


def net_max_batch(C, K, H, W, train):
    """include/lgteun_hip.h, "The network entries' argument contract": B_max = min(floor(65535 / C), floor((2^31 - 1) / (S 16 C H W)))"""
    return min(GRID_YZ_MAX // C, INT_MAX // (net_stage_slots(C, K, H, W, train) * 16 * C * H * W))


class NetPlan:
    """lg_plan_create on the host (no device): precision 0, the product routes, offsets of 4 i floats as tests/test_route_cpu.py uses them"""

    def __init__(self, C, K, H, W):
        from lgteun_amd import _lib
        self.lib, self.C, self.K, self.H, self.W = _lib.lib(), C, K, H, W
        n = 12 + K + 119 * K
        offs = (ctypes.c_int64 * n)(*[4 * i for i in range(n)])
        self.handle = ctypes.c_void_p()
        cfg = _lib.LgConfig(C, K, H, W, 0, 0)
        rc = self.lib.lg_plan_create(ctypes.byref(cfg), offs, n, ctypes.byref(self.handle))
        assert rc == 0, (rc, self.lib.lg_last_error())

    def bound(self, train):
        return net_max_batch(self.C, self.K, self.H, self.W, train)

    def ws(self, B, train):
        return int(self.lib.lg_workspace_bytes(self.handle, B, train))

    def parts(self, B, train):
        """(bytes of the forward carving, bytes of the backward's part behind it) from lg_debug_live_slot; their sum is lg_workspace_bytes"""
        out = (ctypes.c_size_t * 53)()
        assert self.lib.lg_debug_live_slot(self.handle, B, train, out) == 0, self.lib.lg_last_error()
        return int(out[0]), int(out[1])

    def describe(self):
        buf = ctypes.create_string_buffer(2048)
        assert self.lib.lg_plan_describe(self.handle, buf, len(buf)) == 0, self.lib.lg_last_error()
        return buf.value.decode()

    def __del__(self):
        if self.handle:
            self.lib.lg_plan_destroy(self.handle)


def scene_offset(elem, H, W):
    """element offset of a [planes, H, W] array -> (plane, row, column)"""
    plane, r = divmod(elem, H * W)
    return (plane,) + divmod(r, W)


# ------------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------------
def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def memory_gate(need_bytes):
    """skip (with the figures) only when the device shows less free memory than the test needs plus 2 GiB; a test never plans more than 16 GiB"""
    import pytest
    import torch
    assert need_bytes <= LIMIT_BYTES, f'the test plans {need_bytes / GIB:.2f} GiB, above the 16 GiB a test may allocate'
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < need_bytes + HEADROOM_BYTES:
        pytest.skip(f'needs {need_bytes / GIB:.2f} GiB + 2 GiB headroom, the device shows {free / GIB:.2f} GiB free of {total / GIB:.2f} GiB')


class Measured:
    """with Measured('case') as m: ... -- prints the case's wall time and peak allocated memory, asserts the 16 GiB limit, empties the cache"""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        import torch
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        self.base = torch.cuda.memory_allocated()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        import torch
        torch.cuda.synchronize()
        self.seconds = time.perf_counter() - self.t0
        self.peak = torch.cuda.max_memory_allocated() - self.base
        torch.cuda.empty_cache()
        print(f'[limits] {self.what}: {self.seconds:.2f} s, peak {self.peak / GIB:.2f} GiB allocated')
        if exc[0] is None:
            assert self.peak <= LIMIT_BYTES, (self.what, self.peak)
        return False


def fill_randint16(t, seed, chunk=1 << 28):
    """uniform 16-bit samples into the int16 tensor t (a uint16 array as the library reads it), chunk by chunk on the device"""
    import torch
    g = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    for o in range(0, flat.numel(), chunk):
        part = flat[o:o + chunk]
        part.copy_(torch.randint(-32768, 32768, (part.numel(),), generator=g, dtype=torch.int16, device=t.device))
    return t


def fill_uniform(t, lo, hi, seed, chunk=1 << 28):
    import torch
    g = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    for o in range(0, flat.numel(), chunk):
        flat[o:o + chunk].uniform_(lo, hi, generator=g)
    return t


def all_finite(t, chunk=1 << 28):
    """torch.isfinite(t).all() without a temporary of t's size"""
    import torch
    flat = t.view(-1)
    return all(bool(torch.isfinite(flat[o:o + chunk]).all()) for o in range(0, flat.numel(), chunk))


def u16(t):
    """a (small) int16 device tensor that holds uint16 bits -> numpy uint16 on the host"""
    return t.cpu().numpy().view(np.uint16)


def scaled32(a, divisor, n_div, post):
    """ba_scale in numpy's float32 arithmetic: n_div correctly rounded divisions, then one product unless post is 1"""
    x = a.astype(np.float32)
    for _ in range(n_div):
        x = x / np.float32(divisor)
    if post != 1.0:
        x = x * np.float32(post)
    assert x.dtype == np.float32
    return x


def same_bits(a, b):
    """two device tensors (or numpy arrays) hold the same bits"""
    import torch
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    v = {4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


# ------------------------------------------------------------------------------------------------------------------------
# classical batches: a pool of 16 host-made samples times distinct per-sample gains, applied on the device
# ------------------------------------------------------------------------------------------------------------------------
def classical_pool(C, h, w, smooth, seed):
    """ms [16, C, h, w], pan [16, 1, 4h, 4w] float32: the first 16 unsaturated classical_ref.make_scene samples, or bdsd_ref.make_scene's smooth fields (BDSD)"""
    import bdsd_ref
    import classical_ref
    make = bdsd_ref.make_scene if smooth else classical_ref.make_scene
    pairs, i = [], 0
    while len(pairs) < POOL:            # a sample with an element on the makers' clip values 0.02 / 0.98 is left out: at 16 x 16 PAN pixels the smooth
        ms, pan = make(C, h, w, seed * 1000 + i)      # fields of bdsd_ref.make_scene are often one constant, which BDSD answers with zero weights
        i += 1
        if min(ms.min(), pan.min()) > 0.02 and max(ms.max(), pan.max()) < 0.98:
            pairs.append((ms, pan))
        assert i < 20 * POOL, 'the maker keeps giving saturated samples'
    return np.stack([p[0] for p in pairs]), np.stack([p[1][None] for p in pairs])


def classical_batch(pool_ms, pool_pan, B, seed=0):
    """-> (ms [B, C, h, w], pan [B, 1, 4h, 4w], gains [B]) on the device: sample b is pool sample b % 16 times gain g_b, ms and pan alike"""
    import torch
    g = torch.from_numpy(distinct_gains(B, seed)).cuda()
    idx = torch.arange(B, device='cuda') % POOL
    ms = torch.from_numpy(np.array(pool_ms)).cuda()[idx]                 # copies: the cached pool is read-only
    ms.mul_(g.view(B, 1, 1, 1))
    pan = torch.from_numpy(np.array(pool_pan)).cuda()[idx]
    pan.mul_(g.view(B, 1, 1, 1))
    return ms, pan, g


CLASSICAL_METHODS = ('interp23', 'sfim', 'gsa', 'wavelet', 'glp', 'hpm', 'cbd', 'bdsd', 'bdsd32')
EQUAL_GAIN, GAIN_PAN = 0.3, 0.15          # mtf_glp_ref.EQUAL_GAIN / bdsd_ref.GAIN_PAN: one filter for every band


def stats_width(method, C, h, w):
    """fp64 values per sample in the call's stats array (0: the call has none)"""
    if method == 'gsa':
        return 2 * C + 1
    if method in ('glp', 'hpm', 'cbd'):
        return 2 * C
    if method == 'bdsd':
        return C * (C + 1)
    if method == 'bdsd32':
        return (4 * h // 32) * (4 * w // 32) * C * (C + 1)
    return 0


def classical_workspace_bytes(method, B, C, h, w):
    from lgteun_amd import _lib
    L = _lib.lib()
    if method in ('sfim', 'gsa'):
        return int(L.lg_classical_workspace_bytes(B, C, h, w, _lib.LG_CLASSICAL_GSA if method == 'gsa' else _lib.LG_CLASSICAL_SFIM))
    if method in ('glp', 'hpm', 'cbd'):
        return int(L.lg_mtfglp_workspace_bytes(B, C, h, w, 1, {'glp': 0, 'hpm': 1, 'cbd': 2}[method]))
    if method in ('bdsd', 'bdsd32'):
        return int(L.lg_bdsd_workspace_bytes(B, C, h, w, 32 if method == 'bdsd32' else 0))
    return 0


def classical_call(method, ms, pan):
    """one raw C-ABI call -> (out [B, C, 4h, 4w] float32, stats [B, n] float64 or None); the workspace lives for the call only"""
    import torch
    import mtf_glp_ref as mr
    from lgteun_amd import _lib
    L = _lib.lib()
    B, C, h, w = ms.shape
    out = torch.empty(B, C, 4 * h, 4 * w, dtype=torch.float32, device=ms.device)
    n = stats_width(method, C, h, w)
    stats = torch.empty(B, n, dtype=torch.float64, device=ms.device) if n else None
    need = classical_workspace_bytes(method, B, C, h, w)
    ws = torch.empty(need // 8, dtype=torch.float64, device=ms.device) if need else None
    if method == 'interp23':
        rc = L.lg_interp23_up4(ptr(ms), ptr(out), B, C, h, w, stream())
    elif method == 'wavelet':
        rc = L.lg_wavelet(ptr(ms), ptr(pan), ptr(out), B, C, h, w, stream())
    elif method == 'sfim':
        rc = L.lg_sfim(ptr(ms), ptr(pan), ptr(out), B, C, h, w, ptr(ws), need, stream())
    elif method == 'gsa':
        rc = L.lg_gsa(ptr(ms), ptr(pan), ptr(out), ptr(stats), B, C, h, w, ptr(ws), need, stream())
    elif method in ('glp', 'hpm', 'cbd'):
        taps = torch.from_numpy(mr.taps(EQUAL_GAIN)[None]).cuda()
        rc = L.lg_mtf_glp(ptr(ms), ptr(pan), ptr(out), ptr(stats), ptr(taps), 1, 41, {'glp': 0, 'hpm': 1, 'cbd': 2}[method], B, C, h, w, ptr(ws), need,
                          stream())
    else:
        taps_ms, taps_pan = torch.from_numpy(mr.taps(EQUAL_GAIN)[None]).cuda(), torch.from_numpy(mr.taps(GAIN_PAN)[None]).cuda()
        rc = L.lg_bdsd(ptr(ms), ptr(pan), ptr(out), ptr(stats), ptr(taps_ms), 1, ptr(taps_pan), 41, 32 if method == 'bdsd32' else 0, B, C, h, w, ptr(ws),
                       need, stream())
    _lib.check(rc, method)
    torch.cuda.synchronize()
    del ws
    return out, stats


def classical_restatement(method, ms, pan, dtype):
    """the float64 / float32 numpy restatement of one sample: ms [C, h, w], pan [4h, 4w] -> (out [C, 4h, 4w], stats as a flat array or None)"""
    import bdsd_ref as br
    import classical_ref as cr
    import mtf_glp_ref as mr
    import wavelet_ref as wr
    C = ms.shape[0]
    if method == 'interp23':
        return cr.interp23(ms, dtype), None
    if method == 'sfim':
        return cr.sfim(ms, pan, dtype), None
    if method == 'wavelet':
        return wr.wavelet(ms, pan, dtype), None
    if method == 'gsa':
        out, alpha, g = cr.gsa(ms, pan, dtype, return_stats=True)
        return out, np.concatenate([alpha, g])
    if method in ('glp', 'hpm', 'cbd'):
        out, a, g = mr.mtf_glp(ms, pan, method, [EQUAL_GAIN] * C, dtype=dtype, return_stats=True)
        return out, np.concatenate([a, g])
    out, gamma = br.bdsd(ms, pan, [EQUAL_GAIN] * C, 32 if method == 'bdsd32' else None, dtype=dtype, return_stats=True)
    return out, gamma.reshape(-1)
