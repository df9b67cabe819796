// The reductions and the host-side checks that the streaming loss / index kernels share (k_recloss.hip, k_qnr.hip, k_gradnorm.hip,
// k_iqa.hip).  The convention they implement: every sum is a per-workgroup fp64 partial in the caller's workspace followed by ONE pass in
// a fixed order, no floating-point atomics -- the same call gives the same bits every time.  Tests pin that, so it lives here once.
#pragma once
#include <initializer_list>
#include <utility>

#include "common.h"

#ifdef __HIPCC__
// butterfly sum over the 64 lanes: every lane ends with the same bits (each stage adds the same two values on both partners)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// sum over a 256-thread workgroup, in every thread: lane 0 of each wave writes red[wave], one barrier, the four waves meet pairwise.
// No leading barrier: a caller that reuses `red` puts its own in front.
template <typename T>
__device__ __forceinline__ T block_sum4(T v, T* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// sum_{j < n} part[j] by one 256-thread workgroup, in every thread: thread t adds j = t, t + 256, ... in ascending order (eight loads in
// flight at a time: one wave walking the 8,192 partials of 32 x 4 planes of 128 x 128 one load after the other took 30 us), then the
// butterfly inside a wave and the four waves in LDS -- one order, always
__device__ __forceinline__ double partials_sum(const double* __restrict__ part, long n, double* red) {
    double v = 0.0;
    long j = threadIdx.x;
    for (; j + 7 * 256 < n; j += 8 * 256) {
        double p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = part[j + u * 256];
        __builtin_amdgcn_sched_barrier(0);      // all eight loads are issued before the first add waits: left alone, the scheduler sinks adds between them
#pragma unroll
        for (int u = 0; u < 8; ++u) v += p[u];
    }
    for (; j < n; j += 256) v += part[j];
    return block_sum4(v, red);
}
#endif  // __HIPCC__

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// bytes of a workspace region that holds one slice of `per` bytes for each of B samples: every sample's share is reserved in whole 128-byte units
// (the kernels keep indexing with the slice's own size; the rest stays unused), so the region of two samples is whole 256-byte lines already and a
// workspace of B samples is never below B / 2 times the workspace of two -- ws_layout's rounding of a region's end no longer weighs more at a small
// batch than at a large one
inline size_t ws_region(size_t B, size_t per) { return B * ((per + 127) & ~(size_t)127); }

// n workspace regions of sz[i] bytes, each starting 256-byte aligned: their offsets -> off[i], the total is returned
inline size_t ws_layout(int n, const size_t* sz, size_t* off) {
    size_t bytes = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = bytes;
        bytes += align256(sz[i]);
    }
    return bytes;
}

// Argument checks of the loss entries.  false: the reason, naming the entry and the argument, is in lg_last_error.
inline bool check_shape(const char* who, int B, int C, int H, int W) {
    if (B < 1 || B > 65535) { lg_set_error("%s: B must be 1..65535 (got %d)", who, B); return false; }
    if (C != 4 && C != 8) { lg_set_error("%s: C must be 4 or 8 (got %d)", who, C); return false; }
    if (H > 65536 || W > 65536) { lg_set_error("%s: H and W must be <= 65536 (got %d x %d)", who, H, W); return false; }
    return true;
}
// the first of the named float tensors that is NULL or not 16-byte aligned
inline bool check_tensors(const char* who, std::initializer_list<std::pair<const char*, const void*>> ts) {
    for (const auto& t : ts) {
        if (!t.second) { lg_set_error("%s: %s is NULL", who, t.first); return false; }
        if ((uintptr_t)t.second & 15) { lg_set_error("%s: %s must be 16-byte aligned", who, t.first); return false; }
    }
    return true;
}
// what an entry that adds its share of a global-batch loss to loss_accum and writes or accumulates dout takes beside its tensors
inline bool check_loss_args(const char* who, const float* loss_accum, int B, int64_t B_global, float scale, int accumulate) {
    if (!loss_accum) { lg_set_error("%s: loss_accum is NULL", who); return false; }
    if ((uintptr_t)loss_accum & 3) { lg_set_error("%s: loss_accum must be 4-byte aligned", who); return false; }
    if (B_global < B) { lg_set_error("%s: B_global must be at least B (got %lld, B = %d)", who, (long long)B_global, B); return false; }
    if (!(scale == scale) || scale - scale != 0.f) { lg_set_error("%s: scale must be finite", who); return false; }
    if (accumulate != 0 && accumulate != 1) { lg_set_error("%s: accumulate must be 0 or 1 (got %d)", who, accumulate); return false; }
    return true;
}
// `sizer`: the C ABI function that returns `need`
inline bool check_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need, const char* sizer) {
    if (!workspace) { lg_set_error("%s: workspace is NULL", who); return false; }
    if ((uintptr_t)workspace & 7) { lg_set_error("%s: workspace must be 8-byte aligned", who); return false; }
    if (workspace_bytes < need) { lg_set_error("%s: workspace_bytes too small: %zu, need %zu (%s)", who, workspace_bytes, need, sizer); return false; }
    return true;
}
