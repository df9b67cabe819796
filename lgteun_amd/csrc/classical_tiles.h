// What the kernels of the classical baselines share (k_classical.hip: SFIM, GSA, Wavelet, MTF-GLP, BDSD; k_cs.hip: IHS, Brovey, GS, PCA): the 16 x 32 output
// tile, the upsampling of one band of a tile in LDS (cl_up_band), the one rounding to fp32 (cl_clip) and the shape check of the entries.  Everything is
// internal to the translation unit that includes it.
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

// the ms samples of one band the tile at (Y0, X0) depends on, CL_MLOADS per thread, into registers: a caller issues them for the NEXT band (or tile)
// before it runs cl_up_band on the current one, so their latency passes under its four LDS passes
__device__ __forceinline__ void cl_ms_load(const float* __restrict__ ms, int h, int w, int Y0, int X0, float (&v)[CL_MLOADS]) {
    const int my0 = Y0 / 4 - 8, mx0 = X0 / 4 - 8;
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

__device__ __forceinline__ float cl_clip(double o) { return (float)fmin(fmax(o, 0.0), 1.0); }      // the one rounding to fp32
#endif  // __HIPCC__

// false: not a shape the calls take (the reason, naming the argument, is in lg_last_error)
inline bool cl_shape(const char* who, int B, int C, int h, int w) {
    if (B < 1 || B > 65535) { lg_set_error("%s: B must be 1..65535 (got %d)", who, B); return false; }
    if (C < 2 || C > CL_MAX_C) { lg_set_error("%s: C must be 2..%d (got %d)", who, CL_MAX_C, C); return false; }
    if (h < 4 || h > 4096) { lg_set_error("%s: h must be 4..4096 (got %d)", who, h); return false; }
    if (w < 4 || w > 4096) { lg_set_error("%s: w must be 4..4096 (got %d)", who, w); return false; }
    return true;
}

}  // namespace
