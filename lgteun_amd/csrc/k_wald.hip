// Wald-protocol degradation of a raw scene (lgteun_amd/wald.py): the once-per-scene low-pass and decimation by 4.
//
//   k_fir_decimate4<T, O>  a separable FIR with one row of fp64 taps per plane, evaluated at the decimated positions only: output (i, j) is
//                          the filtered plane at (4 i + phase, 4 j + phase), replicate border.  A block owns FIR_TO x FIR_TO outputs: it
//                          stages the row pass of the 4 (FIR_TO - 1) + n_taps input rows its column taps touch in LDS (FIR_TO columns of
//                          them: the decimated ones), then applies the column pass from LDS.  fp64 throughout, products and sums rounded
//                          one by one in ascending tap order (no contraction), so a value is a function of its own (2 r + 1)^2 samples and
//                          taps alone -- not of the tile it falls into, nor of the other planes of the call -- and a numpy loop in the same
//                          order gives the same fp64 bits.  One final rounding: to fp32, or to the input's integer type (half to even,
//                          saturated, NaN -> 0).
#include "abi.h"
#include "common.h"

#define FIR_TO 16                                   // outputs per tile edge
#define FIR_NT (FIR_TO * FIR_TO)
#define FIR_MAX_TAPS 63
#define FIR_SPAN (4 * (FIR_TO - 1) + FIR_MAX_TAPS)   // input rows under one tile's column taps

__device__ __forceinline__ int fir_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ __forceinline__ void fir_store(float* p, double v) { *p = (float)v; }
template <typename O>
__device__ __forceinline__ void fir_store(O* p, double v) {
    constexpr double top = (double)(O)~(O)0;
    double r = rint(v);                                       // round half to even
    r = r > 0.0 ? (r < top ? r : top) : 0.0;                  // NaN -> 0
    *p = (O)r;
}

template <typename T, typename O>
__global__ __launch_bounds__(FIR_NT) void k_fir_decimate4(const T* __restrict__ in, O* __restrict__ out, const double* __restrict__ taps, int H, int W,
                                                          int n_taps, int phase, int tiles_x, int tiles) {
#pragma clang fp contract(off)          // every product and every sum rounds on its own: the order of operations IS the result
    __shared__ double tp[FIR_MAX_TAPS];
    __shared__ double rowf[FIR_SPAN][FIR_TO + 1];
    const int ho = H >> 2, wo = W >> 2, r = n_taps >> 1;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int oy0 = ty * FIR_TO, ox0 = tx * FIR_TO;
    const T* __restrict__ p = in + (size_t)plane * H * W;
    if ((int)threadIdx.x < n_taps) tp[threadIdx.x] = taps[(size_t)plane * n_taps + threadIdx.x];
    __syncthreads();
    // row pass: slot s is input row 4 oy0 + phase - r + s (clamped into the plane), column j the tile's j-th decimated position
    const int rows = (oy0 + FIR_TO <= ho ? FIR_TO : ho - oy0), span = 4 * (rows - 1) + n_taps;
    const int y0 = 4 * oy0 + phase - r, x0 = 4 * ox0 + phase - r;
    for (int t = threadIdx.x; t < span * FIR_TO; t += FIR_NT) {
        const int s = t / FIR_TO, j = t - s * FIR_TO;
        if (ox0 + j >= wo) continue;
        const T* __restrict__ row = p + (size_t)fir_clamp(y0 + s, H) * W;
        const int xb = x0 + 4 * j;
        double acc = 0.0;
        for (int k = 0; k < n_taps; ++k) acc = acc + tp[k] * (double)row[fir_clamp(xb + k, W)];
        rowf[s][j] = acc;
    }
    __syncthreads();
    const int ly = threadIdx.x / FIR_TO, lx = threadIdx.x - ly * FIR_TO;
    if (ly >= rows || ox0 + lx >= wo) return;
    double acc = 0.0;
    for (int k = 0; k < n_taps; ++k) acc = acc + tp[k] * rowf[4 * ly + k][lx];
    fir_store(out + (size_t)plane * ho * wo + (size_t)(oy0 + ly) * wo + ox0 + lx, acc);
}

extern "C" int lg_fir_decimate4(const void* in, void* out, const double* taps, int64_t planes, int32_t H, int32_t W, int32_t n_taps, int32_t phase,
                                int32_t dtype, int32_t out_f32, void* stream) {
    const char* why = nullptr;
    if (!in || !out || !taps) why = "null pointer";
    else if (dtype < LG_DT_U8 || dtype > LG_DT_F32) why = "unknown sample type (LG_DT_U8 / LG_DT_U16 / LG_DT_F32)";
    else if (out_f32 != 0 && out_f32 != 1) why = "the output flag must be 0 (the input's integer type) or 1 (fp32)";
    else if (dtype == LG_DT_F32 && !out_f32) why = "float32 planes have a float32 output";
    else if (H < 8 || W < 8 || (H & 3) || (W & 3) || H > 65536 || W > 65536) why = "H and W must be multiples of 4 in 8 .. 65536";
    else if (n_taps < 1 || n_taps > FIR_MAX_TAPS || !(n_taps & 1)) why = "the tap count must be odd, in 1 .. 63";
    else if (phase < 0 || phase > 3) why = "the phase must be in 0 .. 3";
    else if ((uintptr_t)taps & 7) why = "the taps must be 8-byte aligned";
    else if (((uintptr_t)in & (dtype == LG_DT_U8 ? 0 : dtype == LG_DT_U16 ? 1 : 3)) || ((uintptr_t)out & (out_f32 ? 3 : dtype == LG_DT_U16 ? 1 : 0)))
        why = "planes must be aligned to their sample type";
    const int tiles_x = (W / 4 + FIR_TO - 1) / FIR_TO, tiles_y = (H / 4 + FIR_TO - 1) / FIR_TO;
    if (!why && (planes <= 0 || planes * tiles_x * tiles_y > 0x7fffffffll)) why = "planes must be positive and planes x tiles below 2^31";
    if (why) { lg_set_error("fir_decimate4: %s", why); return -1; }
    const int tiles = tiles_x * tiles_y;
    const unsigned grid = (unsigned)(planes * tiles);
    const hipStream_t s = (hipStream_t)stream;
#define FIR_GO(T, O) k_fir_decimate4<T, O><<<grid, FIR_NT, 0, s>>>((const T*)in, (O*)out, taps, H, W, n_taps, phase, tiles_x, tiles)
    if (dtype == LG_DT_U8) { if (out_f32) FIR_GO(uint8_t, float); else FIR_GO(uint8_t, uint8_t); }
    else if (dtype == LG_DT_U16) { if (out_f32) FIR_GO(uint16_t, float); else FIR_GO(uint16_t, uint16_t); }
    else FIR_GO(float, float);
#undef FIR_GO
    LG_CHECK_LAUNCH();
    return 0;
}
