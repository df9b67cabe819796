// What the kernels of the classical baselines share (k_classical.hip: SFIM, GSA, Wavelet, MTF-GLP, BDSD; k_cs.hip: IHS, Brovey, GS, PCA), each written once.
// Device: the 16 x 32 output tile and its origin (cl_tile), the upsampling of one band of a tile in LDS (cl_up_band) and of all C bands with the next band's
// loads in flight (cl_up_bands), the one rounding to fp32 (cl_clip), the sum of a column of per-workgroup partials (cl_partials_column), the sums of products of
// two LDS vectors with a wave per entry (cl_pair, cl_lane_dot, cl_pair_sums), and the Cholesky factor and solve in LDS (cl_cholesky, cl_chol_solve).  Every one
// of them fixes an order of additions that the outputs' bits depend on.  Host: the shape check (cl_shape), the tile count (cl_tiles), the argument checks every
// fused entry makes after its shape (cl_check_args) and a region of the workspace (cl_ws).  Everything is internal to the translation unit that includes it.
#pragma once
#include <cmath>

#include "abi.h"
#include "common.h"
#include "reduce.h"

namespace {

constexpr int CL_NT = 256;
constexpr int CL_TH = 16, CL_TW = 32, CL_PX = CL_TH * CL_TW;            // the output tile
constexpr int CL_L1R = CL_TH / 2 + 11, CL_L1C = CL_TW / 2 + 11;         // 19 x 27: level-1 rows / columns a tile depends on
constexpr int CL_MR = CL_TH / 4 + 16, CL_MC = CL_TW / 4 + 16;           // 20 x 24: ms rows / columns a tile depends on
constexpr int CL_LR = CL_TH / 4, CL_LC = CL_TW / 4, CL_LPX = CL_LR * CL_LC;      // the tile's own 4 x 8 low-resolution pixels
constexpr int CL_SCRATCH = CL_MR * CL_MC + CL_MR * CL_L1C + CL_L1R * CL_L1C + CL_L1R * CL_TW;      // doubles: M, R1, L1, R2
constexpr int CL_MLOADS = (CL_MR * CL_MC + CL_NT - 1) / CL_NT;           // ms samples a thread loads per band and tile
constexpr int CL_CUS = 256, CL_CU_LDS = 160 * 1024;                     // the MI355X: compute units, LDS bytes of one
constexpr int CL_MAX_C = LG_IQA_MAX_BANDS;
static_assert(CL_PX == 2 * CL_NT, "two adjacent pixels per thread in the apply pass");
static_assert(CL_PX % 64 == 0 && CL_LPX <= 64, "a wave sums a pair over the tile");

// the six half-band constants: the 23 taps are 1 at the centre, twice these at the offsets +-1, +-3, ..., +-11 and 0 at the even offsets
#define CL_HALF_BAND {0.305334091185, -0.072698593239, 0.021809577942, -0.005192756653, 0.000807762146, -0.000060081482}

#ifdef __HIPCC__
__device__ __forceinline__ int cl_mod(int i, int n) {
    i %= n;
    return i < 0 ? i + n : i;
}

// the 12 products of an interpolated sample: src[0], src[stride], ... are the inserted samples at offsets -11, -9, ..., 11 from it
__device__ __forceinline__ double cl_fir(const double* src, int stride) {
    constexpr double T[6] = {2 * 0.305334091185, -2 * 0.072698593239, 2 * 0.021809577942, -2 * 0.005192756653, 2 * 0.000807762146, -2 * 0.000060081482};
    double a = 0.0, b = 0.0;      // two chains of six: a thread has one or two samples per pass, so the chain's latency is the pass's
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        a = fma(T[5 - j], src[j * stride], a);
        b = fma(T[j], src[(j + 6) * stride], b);
    }
    return a + b;
}

// One axis of one level for `lines` lines of `nd` outputs: out[line * ol + d * os] from in[line * il + . * is].  By the tile geometry (origins
// of the three grids at tile 4 k, level-1 2 k - 5, ms k - 8) output d of either level is a copy of input 5 + d / 2 when d is even and the
// filter over inputs (d - 1) / 2 ... (d - 1) / 2 + 11 when d is odd.  Consecutive threads take consecutive addresses: along the line in the x passes, across
// the lines (LINE_FAST) in the y passes, whose lines are a row stride apart -- 32 doubles in level 2: one LDS bank for every lane otherwise.
template <bool LINE_FAST>
__device__ __forceinline__ void cl_axis(const double* in, int il, int is, double* out, int ol, int os, int lines, int nd) {
    const int n_odd = nd >> 1, n_even = nd - n_odd;
    for (int i = threadIdx.x; i < lines * n_odd; i += CL_NT) {
        const int line = LINE_FAST ? i % lines : i / n_odd, q = LINE_FAST ? i / lines : i - line * n_odd;
        out[line * ol + (2 * q + 1) * os] = cl_fir(in + line * il + q * is, is);
    }
    for (int i = threadIdx.x; i < lines * n_even; i += CL_NT) {
        const int line = LINE_FAST ? i % lines : i / n_even, q = LINE_FAST ? i / lines : i - line * n_even;
        out[line * ol + 2 * q * os] = in[line * il + (5 + q) * is];
    }
}

// the origin of output tile t, tiles_x tiles in a row:   const auto [Y0, X0] = cl_tile(t, tiles_x);
struct ClTile { int Y0, X0; };
__device__ __forceinline__ ClTile cl_tile(int t, int tiles_x) { return {(t / tiles_x) * CL_TH, (t % tiles_x) * CL_TW}; }

// the ms samples of one band the tile at o depends on, CL_MLOADS per thread, into registers: a caller issues them for the NEXT band (or tile)
// before it runs cl_up_band on the current one, so their latency passes under its four LDS passes
__device__ __forceinline__ void cl_ms_load(const float* __restrict__ ms, int h, int w, ClTile o, float (&v)[CL_MLOADS]) {
    const int my0 = o.Y0 / 4 - 8, mx0 = o.X0 / 4 - 8;
#pragma unroll
    for (int u = 0; u < CL_MLOADS; ++u) {
        const int i = threadIdx.x + u * CL_NT, r = i / CL_MC, c = i - r * CL_MC;
        v[u] = 0.f;
        if (i < CL_MR * CL_MC) v[u] = ms[(long)cl_mod(my0 + r, h) * w + cl_mod(mx0 + c, w)];
    }
}

// u of one band for a tile from its loaded ms samples -> U[16][32].  S: CL_SCRATCH doubles.  Ends WITHOUT a barrier: the caller puts one in front of
// its reads of U.  A following call may start at once: its first writes go to M, which was last read three barriers ago.  T: float (ms samples) or
// double (MTF-GLP's low-resolution plane q_k, which exists in registers only).
template <typename T>
__device__ __forceinline__ void cl_up_band(const T (&v)[CL_MLOADS], double* S, double* U) {
    double* M = S;
    double* R1 = M + CL_MR * CL_MC;
    double* L1 = R1 + CL_MR * CL_L1C;
    double* R2 = L1 + CL_L1R * CL_L1C;
#pragma unroll
    for (int u = 0; u < CL_MLOADS; ++u) {
        const int i = threadIdx.x + u * CL_NT;
        if (i < CL_MR * CL_MC) M[i] = (double)v[u];
    }
    __syncthreads();
    cl_axis<false>(M, CL_MC, 1, R1, CL_L1C, 1, CL_MR, CL_L1C);          // level 1 along x: 20 lines of 27
    __syncthreads();
    cl_axis<true>(R1, 1, CL_L1C, L1, 1, CL_L1C, CL_L1C, CL_L1R);       // level 1 along y: 27 lines of 19
    __syncthreads();
    cl_axis<false>(L1, CL_L1C, 1, R2, CL_TW, 1, CL_L1R, CL_TW);         // level 2 along x: 19 lines of 32
    __syncthreads();
    cl_axis<true>(R2, 1, CL_TW, U, 1, CL_TW, CL_TW, CL_TH);            // level 2 along y: 32 lines of 16
}

// v = vn: the samples loaded ahead become the current ones
template <typename T>
__device__ __forceinline__ void cl_next(T (&v)[CL_MLOADS], const T (&vn)[CL_MLOADS]) {
#pragma unroll
    for (int u = 0; u < CL_MLOADS; ++u) v[u] = vn[u];
}

// u of all C bands of the tile at (Y0, X0) -> U[C][16][32]; ms_b: the sample's bands, lp = h w apart.  Band k + 1's samples are loaded before band k's four LDS
// passes.  Ends WITHOUT a barrier, like cl_up_band.
__device__ __forceinline__ void cl_up_bands(const float* __restrict__ ms_b, long lp, int C, int h, int w, int Y0, int X0, double* S, double* U) {
    float v[CL_MLOADS], vn[CL_MLOADS] = {};
    cl_ms_load(ms_b, h, w, {Y0, X0}, v);
    for (int k = 0; k < C; ++k) {
        if (k + 1 < C) cl_ms_load(ms_b + (k + 1) * lp, h, w, {Y0, X0}, vn);
        cl_up_band(v, S, U + k * CL_PX);
        cl_next(v, vn);
    }
}

__device__ __forceinline__ float cl_clip(double o) { return (float)fmin(fmax(o, 0.0), 1.0); }      // the one rounding to fp32

// pe[0] + pe[stride] + ... + pe[(n - 1) stride] by one thread: the partials of n workgroups for one entry, one accumulator, ascending order.  (k_cs_finish is not
// a caller: it sums with a wave per entry and a butterfly, and its bits depend on that order.)
__device__ __forceinline__ double cl_partials_column(const double* __restrict__ pe, int n, long stride) {
    double s = 0.0;
    int j = 0;
    for (; j + 8 <= n; j += 8) {      // eight loads in flight, added in ascending order
        double q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = pe[(j + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += q[u];
    }
    for (; j < n; ++j) s += pe[j * stride];
    return s;
}

// entry e of a sum list: vectors a and b, of the high- (lo = 0) or the low-resolution table
__device__ __forceinline__ int cl_pair(int a, int b, int lo) { return a | (b << 8) | (lo << 16); }

// a lane's share of sum_i a[i] b[i] over N (a multiple of 64) elements of two LDS vectors: elements lane, lane + 64, ... in ascending order on ONE fma chain --
// the chain fixes the bits.  N at compile time: unrolled.
template <int N>
__device__ __forceinline__ double cl_lane_dot(const double* a, const double* b, int lane) {
    double v = 0.0;
#pragma unroll
    for (int u = 0; u < N / 64; ++u) v = fma(a[lane + 64 * u], b[lane + 64 * u], v);
    return v;
}
// the same over the first n elements, n at run time (the vectors hold zeros from n up to the next multiple of 64)
__device__ __forceinline__ double cl_lane_dot(const double* a, const double* b, int lane, int n) {
    double v = 0.0;
    for (int u = 0; u < n; u += 64) v = fma(a[lane + u], b[lane + u], v);
    return v;
}

// acc[e] += the sum over the wave of term(a, b, lo, lane) for every entry e < ns, (a, b, lo) = pairs[e] (cl_pair): wave j of the four owns the entries j, j + 4,
// ...; lane 0 adds.  The caller puts a barrier behind it before the vectors change.
template <typename F>
__device__ __forceinline__ void cl_pair_sums(const int* pairs, int ns, double* acc, F term) {
    const int lane = threadIdx.x & 63;
    for (int e = threadIdx.x >> 6; e < ns; e += CL_NT / 64) {
        const int pr = pairs[e];
        const double v = wave_sum(term(pr & 255, (pr >> 8) & 255, pr >> 16, lane));
        if (lane == 0) acc[e] += v;
    }
}

// The Cholesky factor L of a symmetric n x n matrix into the lower triangle of Lm (rows `pitch` apart), by ONE thread.  A(i, j): the matrix's entry, asked for
// i >= j, once, before L(i, j) is written (so A may read Lm itself).  bad_pivot(d, a_jj): the caller's rule for a column's pivot d before its root; true ends the
// factorisation with false returned.  The order of the subtractions inside a row fixes the bits.
template <typename M, typename P>
__device__ __forceinline__ bool cl_cholesky(double* Lm, int n, int pitch, M A, P bad_pivot) {
    for (int j = 0; j < n; ++j) {
        const double ajj = A(j, j);
        double d = ajj;
        for (int p = 0; p < j; ++p) d -= Lm[j * pitch + p] * Lm[j * pitch + p];
        if (bad_pivot(d, ajj)) return false;
        d = sqrt(d);
        Lm[j * pitch + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double s = A(i, j);
            for (int p = 0; p < j; ++p) s -= Lm[i * pitch + p] * Lm[j * pitch + p];
            Lm[i * pitch + j] = s / d;
        }
    }
    return true;
}

// x = (L L')^-1 rhs by one thread, forward then back; x may be rhs.  each(x_i): the caller's look at every component as the back substitution forms it (a pass
// of its own over x afterwards cost BDSD's one-wave solve 0.5 - 1 us)
template <typename E>
__device__ __forceinline__ void cl_chol_solve(const double* Lm, int n, int pitch, const double* rhs, double* x, E each) {
    for (int i = 0; i < n; ++i) {
        double s = rhs[i];
        for (int p = 0; p < i; ++p) s -= Lm[i * pitch + p] * x[p];
        x[i] = s / Lm[i * pitch + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = x[i];
        for (int p = i + 1; p < n; ++p) s -= Lm[p * pitch + i] * x[p];
        x[i] = s / Lm[i * pitch + i];
        each(x[i]);
    }
}
__device__ __forceinline__ void cl_chol_solve(const double* Lm, int n, int pitch, const double* rhs, double* x) {
    cl_chol_solve(Lm, n, pitch, rhs, x, [](double) {});
}
#endif  // __HIPCC__

// false: not a shape the calls take (the reason, naming the argument, is in lg_last_error)
inline bool cl_shape(const char* who, int B, int C, int h, int w) {
    if (B < 1 || B > 65535) { lg_set_error("%s: B must be 1..65535 (got %d)", who, B); return false; }
    if (C < 2 || C > CL_MAX_C) { lg_set_error("%s: C must be 2..%d (got %d)", who, CL_MAX_C, C); return false; }
    if (h < 4 || h > 4096) { lg_set_error("%s: h must be 4..4096 (got %d)", who, h); return false; }
    if (w < 4 || w > 4096) { lg_set_error("%s: w must be 4..4096 (got %d)", who, w); return false; }
    return true;
}

// the 16 x 32 output tiles of a sample: those in a row of tiles -> tiles_x, all of them returned
inline int cl_tiles(int h, int w, int& tiles_x) {
    tiles_x = (4 * w + CL_TW - 1) / CL_TW;
    return tiles_x * ((4 * h + CL_TH - 1) / CL_TH);
}

// the named fp64 arrays: all of them given (where `required`), then all of them 8-byte aligned
inline bool check_doubles(const char* who, std::initializer_list<std::pair<const char*, const void*>> ds, bool required) {
    if (required)
        for (const auto& d : ds)
            if (!d.second) { lg_set_error("%s: %s is NULL", who, d.first); return false; }
    for (const auto& d : ds)
        if ((uintptr_t)d.second & 7) { lg_set_error("%s: %s must be 8-byte aligned", who, d.first); return false; }
    return true;
}

// what every fused entry checks once its shape is known, in this order: the three float tensors, the fp64 arrays it cannot do without (`doubles`), stats (which
// may be NULL), the workspace (`sizer`: the C ABI function that returns `need`)
inline bool cl_check_args(const char* who, const float* ms, const float* pan, const float* out, std::initializer_list<std::pair<const char*, const void*>> doubles,
                          const double* stats, const void* workspace, size_t workspace_bytes, size_t need, const char* sizer) {
    return check_tensors(who, {{"ms", ms}, {"pan", pan}, {"out", out}}) && check_doubles(who, doubles, true) && check_doubles(who, {{"stats", stats}}, false) &&
           check_workspace(who, workspace, workspace_bytes, need, sizer);
}

// the workspace region at byte offset off (ws_layout)
inline double* cl_ws(void* workspace, size_t off) { return (double*)((char*)workspace + off); }

}  // namespace
