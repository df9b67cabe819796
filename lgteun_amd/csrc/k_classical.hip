// The three classical (training-free) pan-sharpening baselines, whole batches on the device: SFIM and GSA with global regression, on top of the
// 23-tap half-band interpolator x4, and the two-level Haar substitution (Wavelet), which needs neither u nor a statistic (C ABI: lg_interp23_up4 /
// lg_sfim / lg_gsa / lg_wavelet, include/lgteun_hip.h; the definitions are in DESIGN.md 3.12, the fp64 numpy restatements the tests compare with
// are tests/classical_ref.py and tests/wavelet_ref.py).
//
//   cl_up_band       (classical_tiles.h, shared with k_cs.hip) the upsampling of ONE band for a 16 x 32 tile of the output, in LDS, all fp64: the 20 x 24 ms samples the tile depends on
//                    (cl_ms_load: loaded modulo h, w -- the circular boundary happens here and nowhere else -- into registers, one band
//                    ahead of their use), level 1 rows then columns (19 x 27 of the 2h x 2w plane: the tile's own 8 x 16 plus the halo of
//                    5 / 6 level 2 needs), level 2 rows then columns.  A level keeps the inserted samples (even / odd positions are copies)
//                    and fills the rest with 12 products per axis; the copy and the filter run as two loops, so no wave does both.  u is
//                    never stored in memory: every consumer recomputes its tile.
//   k_cl_interp      grid (tile, band, sample): the tile, rounded to fp32 once.
//   k_cl_moments     grid (gx, sample), gx = min(tiles, the workgroups resident at once); a workgroup walks the tiles gx apart: the C bands
//                    of the tile, PAN minus the sample's first PAN pixel (the pivot: a constant PAN has EXACTLY zero moments) and the mask of the pixels inside the image as C + 2 vectors
//                    in LDS, GSA also the C ms bands, the 2 x 2 centre mean of PAN and the mask at the tile's 4 x 8 low-resolution pixels.
//                    Every sum the method needs is the sum of a product of two of those vectors: a wave owns the pairs e = wave, wave + 4,
//                    ..., sums them over the tile and lane 0 adds to its slot in LDS -- one order, always (cl_pair_sums, classical_tiles.h, shared
//                    with k_bd_gram and k_cs_gram).  The workgroup writes its slots.
//   k_cl_finish      one workgroup per sample: the partials in ascending order (cl_partials_column), then one thread: SFIM's scales, or GSA's
//                    C x C Cholesky solve (cl_cholesky, cl_chol_solve) for alpha and the gains g = N / (N - 1) Sigma_u alpha / (alpha' Sigma_u alpha).
//                    A constant PAN gives scale 0; a non-positive pivot, alpha' Sigma_u alpha <= 0 or a gain that is not finite gives alpha = g = 0.
//   k_cl_apply       grid (tile, sample): the C bands of the tile again (cl_up_bands), then pointwise in fp64 with ONE rounding to fp32; SFIM stages
//                    PAN with a circular halo of 2 for the 5 x 5 box.  Two adjacent pixels per thread: 8-byte stores.
//   k_cl_wavelet     grid (tile, sample), the whole method in one launch: out_k = clip(pan - P + M_k) with P the 4 x 4 block mean of PAN and M_k the
//                    block mean of u_k, which is a separable 17-tap circular FIR on ms itself (cl_wavelet_taps).  A lane owns 4 x 4 blocks: 16-byte
//                    PAN loads, 16-byte stores, M_k from an ms halo tile in LDS (columns, then rows).  No u, no moments, no workspace.
//   k_mg_*           MTF-GLP with its three injection rules (lg_mtf_glp), on the same tiles: described where they stand, below k_cl_wavelet.
//   k_at_*           ATWT and AWLP, the a trous pair (lg_atrous; restated in tests/atrous_ref.py): described where they stand, below k_mg_apply.
//   k_hr_*           FS, HPM-R, HPM-H and BT-H, the regression-based and haze-corrected rules (lg_mtf_hr; restated in tests/mtf_hr_ref.py): described
//                    where they stand, below at_fuse.
//   k_bd_*           BDSD, global and block-wise (lg_bdsd; restated in tests/bdsd_ref.py): described where they stand, below k_mg_*.
// No atomics; a workgroup sees one sample and the grid of a sample depends on C, h and w only, so a sample has the same bits alone and inside
// any batch.  All indexing into tensors is 64-bit.
#include <cmath>

#include "abi.h"
#include "classical_tiles.h"
#include "common.h"
#include "reduce.h"

namespace {

constexpr int CL_BOX = 5, CL_BH = CL_TH + CL_BOX - 1, CL_BW = CL_TW + CL_BOX - 1;      // SFIM's staged PAN: 20 x 36
constexpr int CL_MAX_SUMS = (CL_MAX_C + 2) * (CL_MAX_C + 3);            // GSA: all pairs of C + 2 vectors, high and low resolution

__host__ __device__ inline int cl_moment_lds_doubles(int C) { return CL_SCRATCH + (C + 2) * (CL_PX + CL_LPX) + CL_MAX_SUMS; }
__host__ __device__ inline int cl_apply_lds_doubles(int C) { return CL_SCRATCH + C * CL_PX + CL_BH * CL_BW; }

__global__ __launch_bounds__(CL_NT) void k_cl_interp(const float* __restrict__ ms, float* __restrict__ out, int h, int w, int tiles_x) {
    extern __shared__ double cl_lds[];
    double* U = cl_lds + CL_SCRATCH;
    const int H4 = 4 * h, W4 = 4 * w;
    const auto [Y0, X0] = cl_tile(blockIdx.x, tiles_x);
    const long plane = (long)blockIdx.z * gridDim.y + blockIdx.y;
    float v[CL_MLOADS];
    cl_ms_load(ms + plane * ((long)h * w), h, w, {Y0, X0}, v);
    cl_up_band(v, cl_lds, U);
    __syncthreads();
    const int p = 2 * threadIdx.x, y = Y0 + p / CL_TW, x = X0 + p % CL_TW;
    if (y < H4 && x < W4)      // W4 is a multiple of 4 and x is even: both pixels or none
        *reinterpret_cast<float2*>(out + plane * ((long)H4 * W4) + (long)y * W4 + x) = make_float2((float)U[p], (float)U[p + 1]);
}

// part [B][gx][ns].  SFIM (ns = 2 C + 2): sum u_k, sum u_k^2 per band, then sum pc, sum pc^2 with pc = PAN - pivot.  GSA (ns = (C + 2)(C + 3)):
// all pairs a <= b of the vectors [mask, u_0 .. u_C-1, pc] in row-major order of the upper triangle, then the same of [mask, ms_0 .. ms_C-1, q]
// over the low-resolution pixels, q = the mean of pc over the 2 x 2 centre of the 4 x 4 block.
__global__ __launch_bounds__(CL_NT) void k_cl_moments(const float* __restrict__ ms, const float* __restrict__ pan, double* __restrict__ part, int C,
                                                      int h, int w, int tiles_x, int tiles, int gsa) {
    extern __shared__ double cl_lds[];
    __shared__ int pairs[CL_MAX_SUMS];
    const int n = C + 2, tid = threadIdx.x, gx = gridDim.x;
    double* Vhi = cl_lds + CL_SCRATCH;           // [n][512]: mask, u, pc
    double* Vlo = Vhi + n * CL_PX;               // [n][32]: mask, ms, q
    double* acc = Vlo + n * CL_LPX;              // [ns]
    const int ns = gsa ? n * (n + 1) : 2 * C + 2;
    const int H4 = 4 * h, W4 = 4 * w;
    const long b = blockIdx.y;
    const float* __restrict__ ms_b = ms + b * C * ((long)h * w);
    const float* __restrict__ pan_b = pan + b * ((long)H4 * W4);
    const double pv = (double)pan_b[0];
    if (tid == 0) {
        int e = 0;
        if (gsa) {
            for (int lo = 0; lo < 2; ++lo)
                for (int a = 0; a < n; ++a)
                    for (int c = a; c < n; ++c) pairs[e++] = cl_pair(a, c, lo);
        } else {
            for (int k = 0; k < C; ++k) {
                pairs[e++] = cl_pair(0, k + 1, 0);
                pairs[e++] = cl_pair(k + 1, k + 1, 0);
            }
            pairs[e++] = cl_pair(0, C + 1, 0);
            pairs[e++] = cl_pair(C + 1, C + 1, 0);
        }
    }
    for (int e = tid; e < ns; e += CL_NT) acc[e] = 0.0;
    // (the barriers inside cl_up_band order both before their first use)
    float v[CL_MLOADS], vn[CL_MLOADS] = {};
    cl_ms_load(ms_b, h, w, cl_tile(blockIdx.x, tiles_x), v);
    for (int t = blockIdx.x; t < tiles; t += gx) {
        const auto [Y0, X0] = cl_tile(t, tiles_x);
        for (int k = 0; k < C; ++k) {
            if (k + 1 < C)
                cl_ms_load(ms_b + (k + 1) * ((long)h * w), h, w, {Y0, X0}, vn);
            else if (t + gx < tiles)
                cl_ms_load(ms_b, h, w, cl_tile(t + gx, tiles_x), vn);
            cl_up_band(v, cl_lds, Vhi + (k + 1) * CL_PX);
            cl_next(v, vn);
            if (gsa && tid < CL_LPX) {
                const int gi = Y0 / 4 + tid / CL_LC, gj = X0 / 4 + tid % CL_LC;
                Vlo[(k + 1) * CL_LPX + tid] = (gi < h && gj < w) ? (double)ms_b[k * ((long)h * w) + (long)gi * w + gj] : 0.0;
            }
        }
        for (int p = tid; p < CL_PX; p += CL_NT) {
            const int y = Y0 + p / CL_TW, x = X0 + p % CL_TW;
            const bool in = y < H4 && x < W4;
            Vhi[p] = in ? 1.0 : 0.0;
            Vhi[(C + 1) * CL_PX + p] = in ? (double)pan_b[(long)y * W4 + x] - pv : 0.0;
        }
        __syncthreads();
        for (int i = tid; i < C * CL_PX; i += CL_NT) Vhi[CL_PX + i] *= Vhi[i % CL_PX];      // what a ragged tile holds outside the image counts as 0
        if (gsa && tid < CL_LPX) {
            const int i = tid / CL_LC, j = tid % CL_LC;
            const bool in = Y0 / 4 + i < h && X0 / 4 + j < w;
            const double* P = Vhi + (C + 1) * CL_PX + (4 * i + 1) * CL_TW + 4 * j + 1;
            Vlo[tid] = in ? 1.0 : 0.0;
            Vlo[(C + 1) * CL_LPX + tid] = in ? 0.25 * ((P[0] + P[1]) + (P[CL_TW] + P[CL_TW + 1])) : 0.0;
        }
        __syncthreads();
        cl_pair_sums(pairs, ns, acc, [&](int a, int c, int lo, int lane) {
            if (lo) return lane < CL_LPX ? Vlo[a * CL_LPX + lane] * Vlo[c * CL_LPX + lane] : 0.0;
            return cl_lane_dot<CL_PX>(Vhi + a * CL_PX, Vhi + c * CL_PX, lane);
        });
        __syncthreads();      // the next tile overwrites the vectors
    }
    for (int e = tid; e < ns; e += CL_NT) part[(b * gx + blockIdx.x) * ns + e] = acc[e];
}

// coef [B][3 C + 1]: mean of pc; mean u_k; SFIM's scale a_k or GSA's alpha_k; GSA's gain g_k (SFIM: unused).  stats: NULL or [B][2 C + 1].
__global__ __launch_bounds__(CL_NT) void k_cl_finish(const double* __restrict__ part, double* __restrict__ coef, double* __restrict__ stats, int C,
                                                     int gx, double N, double nl, int gsa) {
    __shared__ double sums[CL_MAX_SUMS];
    __shared__ double Lm[CL_MAX_C * CL_MAX_C], mu[CL_MAX_C], mm[CL_MAX_C], al[CL_MAX_C], v[CL_MAX_C];
    const int n = C + 2, np = n * (n + 1) / 2, ns = gsa ? 2 * np : 2 * C + 2;
    const long b = blockIdx.x;
    for (int e = threadIdx.x; e < ns; e += CL_NT) sums[e] = cl_partials_column(part + b * gx * ns + e, gx, ns);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* co = coef + b * (3 * C + 1);
    if (!gsa) {
        const double sp = sums[2 * C], var_p = (sums[2 * C + 1] - sp * sp / N) / (N - 1.0);
        co[0] = sp / N;
        for (int k = 0; k < C; ++k) {
            const double su = sums[2 * k], var_u = (sums[2 * k + 1] - su * su / N) / (N - 1.0);
            co[1 + k] = su / N;
            co[1 + C + k] = var_p > 0.0 ? sqrt(fmax(var_u, 0.0) / var_p) : 0.0;
            co[1 + 2 * C + k] = 0.0;
        }
        return;
    }
    auto at = [&](int lo, int a, int c) { return sums[lo * np + a * n - a * (a - 1) / 2 + (c - a)]; };      // a <= c
    const double mpc = at(0, 0, C + 1) / N, mq = at(1, 0, C + 1) / nl;
    for (int k = 0; k < C; ++k) {
        mu[k] = at(0, 0, k + 1) / N;
        mm[k] = at(1, 0, k + 1) / nl;
    }
    // Sigma_ms alpha = cov(ms, q) by Cholesky, the lower triangle in Lm
    for (int k = 0; k < C; ++k)
        for (int l = 0; l <= k; ++l) Lm[k * C + l] = at(1, l + 1, k + 1) / nl - mm[k] * mm[l];
    bool ok = cl_cholesky(Lm, C, C, [&](int i, int j) { return Lm[i * C + j]; }, [](double d, double) { return !(d > 0.0); });
    if (ok) {
        for (int i = 0; i < C; ++i) al[i] = at(1, i + 1, C + 1) / nl - mm[i] * mq;
        cl_chol_solve(Lm, C, C, al, al);
        double den = 0.0;
        for (int k = 0; k < C; ++k) {
            double s = 0.0;
            for (int l = 0; l < C; ++l) s += (at(0, (k < l ? k : l) + 1, (k < l ? l : k) + 1) / N - mu[k] * mu[l]) * al[l];
            v[k] = s;
            den += al[k] * s;
        }
        ok = den > 0.0;
        for (int k = 0; k < C && ok; ++k) {
            v[k] = N / (N - 1.0) * v[k] / den;
            ok = v[k] - v[k] == 0.0 && al[k] - al[k] == 0.0;
        }
    }
    co[0] = mpc;
    for (int k = 0; k < C; ++k) {
        co[1 + k] = mu[k];
        co[1 + C + k] = ok ? al[k] : 0.0;
        co[1 + 2 * C + k] = ok ? v[k] : 0.0;
    }
    if (stats) {
        double* st = stats + b * (2 * C + 1);
        for (int k = 0; k < C; ++k) {
            st[k] = ok ? al[k] : 0.0;
            st[C + 1 + k] = ok ? v[k] : 0.0;
        }
        st[C] = mq - mpc;      // the intercept: the mean of the low-resolution PAN (the other columns are centred)
    }
}

template <bool GSA>
__global__ __launch_bounds__(CL_NT) void k_cl_apply(const float* __restrict__ ms, const float* __restrict__ pan, float* __restrict__ out,
                                                    const double* __restrict__ coef, int C, int h, int w, int tiles_x) {
    extern __shared__ double cl_lds[];
    double* U = cl_lds + CL_SCRATCH;             // [C][512]
    double* PT = U + C * CL_PX;                  // SFIM: [20][36], staged pixel (r, c) = PAN pixel (Y0 - 2 + r, X0 - 2 + c) modulo the sides, minus the pivot
    const int tid = threadIdx.x, H4 = 4 * h, W4 = 4 * w;
    const auto [Y0, X0] = cl_tile(blockIdx.x, tiles_x);
    const long b = blockIdx.y, lp = (long)h * w;
    const float* __restrict__ pan_b = pan + b * ((long)H4 * W4);
    float* __restrict__ out_b = out + b * C * ((long)H4 * W4);
    const double* __restrict__ co = coef + b * (3 * C + 1);
    const double pv = (double)pan_b[0];
    cl_up_bands(ms + b * C * lp, lp, C, h, w, Y0, X0, cl_lds, U);
    if (!GSA)
        for (int i = tid; i < CL_BH * CL_BW; i += CL_NT) {
            const int r = i / CL_BW, c = i - r * CL_BW;
            PT[i] = (double)pan_b[(long)cl_mod(Y0 - CL_BOX / 2 + r, H4) * W4 + cl_mod(X0 - CL_BOX / 2 + c, W4)] - pv;
        }
    __syncthreads();
    const int p = 2 * tid, oy = p / CL_TW, ox = p % CL_TW, y = Y0 + oy, x = X0 + ox;
    if (y >= H4 || x >= W4) return;              // W4 is a multiple of 4 and x is even: both pixels or none
    const long o = (long)y * W4 + x;
    const double mpc = co[0];
    if (GSA) {
        const float2 pp = *reinterpret_cast<const float2*>(pan_b + o);
        double d0 = ((double)pp.x - pv) - mpc, d1 = ((double)pp.y - pv) - mpc;      // p~ - I0
        for (int k = 0; k < C; ++k) {
            const double a = co[1 + C + k], m = co[1 + k];
            d0 -= a * (U[k * CL_PX + p] - m);
            d1 -= a * (U[k * CL_PX + p + 1] - m);
        }
        for (int k = 0; k < C; ++k) {
            const double g = co[1 + 2 * C + k];
            *reinterpret_cast<float2*>(out_b + k * ((long)H4 * W4) + o) =
                make_float2(cl_clip(fma(g, d0, U[k * CL_PX + p])), cl_clip(fma(g, d1, U[k * CL_PX + p + 1])));
        }
    } else {
        const double* q = PT + oy * CL_BW + ox;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int dy = 0; dy < CL_BOX; ++dy) {
            double r[CL_BOX + 1];
#pragma unroll
            for (int dx = 0; dx < CL_BOX + 1; ++dx) r[dx] = q[dy * CL_BW + dx];
#pragma unroll
            for (int dx = 0; dx < CL_BOX; ++dx) {
                s0 += r[dx];
                s1 += r[dx + 1];
            }
        }
        const double c0 = q[2 * CL_BW + 2] - mpc, c1 = q[2 * CL_BW + 3] - mpc;
        const double b0 = s0 / (CL_BOX * CL_BOX) - mpc, b1 = s1 / (CL_BOX * CL_BOX) - mpc;
        for (int k = 0; k < C; ++k) {
            const double a = co[1 + C + k], m = co[1 + k];
            const double o0 = U[k * CL_PX + p] * fma(a, c0, m) / (fma(a, b0, m) + 1e-8);
            const double o1 = U[k * CL_PX + p + 1] * fma(a, c1, m) / (fma(a, b1, m) + 1e-8);
            *reinterpret_cast<float2*>(out_b + k * ((long)H4 * W4) + o) = make_float2(cl_clip(o0), cl_clip(o1));
        }
    }
}

// ---- Wavelet: the level-2 Haar approximation of PAN replaced by the band's.  With 4h x 4w sides both levels split evenly, the approximation is 1/4 of the
// sum of a 4 x 4 block and its synthesis alone is the block mean, so out_k(y, x) = clip(pan(y, x) - P(Y, X) + M_k(Y, X)), Y = y / 4, X = x / 4.
constexpr int CW_BY = 8, CW_BX = 64;                                    // the tile in 4 x 4 blocks: 32 x 256 output pixels
constexpr int CW_REACH = 8, CW_TAPS = 2 * CW_REACH + 1;                 // the FIR's offsets -8 .. 8
constexpr int CW_MR = CW_BY + 2 * CW_REACH, CW_MC = CW_BX + 2 * CW_REACH;      // 24 x 80: ms rows / columns a tile depends on
constexpr int CW_LROWS = CL_NT / CW_MC, CW_MLOADS = CW_MR / CW_LROWS;    // a thread loads column tid % 80 of rows tid / 80 + 3 u, u < 8 (240 of the 256 threads)
constexpr int CW_PER = CW_BY / (CL_NT / 64);                            // blocks of a lane: rows wave, wave + 4 of the tile, column lane
static_assert(CW_BX == 64 && CW_BY % (CL_NT / 64) == 0, "a wave spans the tile's columns: 64 lanes x 16 bytes are 1 KiB contiguous");
static_assert(CW_MR % CW_LROWS == 0 && CW_LROWS < 4, "the halo rows divide among the loads; a row index advanced by CW_LROWS wraps at most once (h >= 4)");

// M_k(i, j) = sum_a sum_b t[a] t[b] ms_k((i - a) mod h, (j - b) mod w): the response of "level 1 (zero insertion at the odd positions, the 23 taps), level 2
// (at the even positions, the 23 taps), mean of groups of 4" to a unit impulse, t[8 + a] for a = -8 .. 8.  An impulse at ms(0) is x1(1) = 1, so
// y1(n) = T(1 - n), u(m) = sum_n T(2 n - m) y1(n) and t_a = the mean of u(4 a .. 4 a + 3); T the 23 taps by offset, zero beyond +-11.  Asymmetric: ms(i)
// sits at u(4 i + 2), the block's centre at 4 i + 1.5.
struct ClWaveletTaps { double t[CW_TAPS]; };
__host__ __device__ constexpr ClWaveletTaps cl_wavelet_taps() {
    constexpr double HB[6] = {0.305334091185, -0.072698593239, 0.021809577942, -0.005192756653, 0.000807762146, -0.000060081482};
    double T[23] = {};
    T[11] = 1.0;
    for (int i = 0; i < 6; ++i) T[11 + 2 * i + 1] = T[11 - 2 * i - 1] = 2 * HB[i];
    ClWaveletTaps r = {};
    for (int a = -CW_REACH; a <= CW_REACH; ++a) {
        double s = 0.0;
        for (int m = 4 * a; m < 4 * a + 4; ++m) {
            double um = 0.0;
            for (int n = -10; n <= 12; ++n) {
                const int k = 2 * n - m;
                if (k >= -11 && k <= 11) um += T[11 + k] * T[11 + 1 - n];
            }
            s += um;
        }
        r.t[a + CW_REACH] = 0.25 * s;
    }
    return r;
}

// sum_a t_a src[(8 - a) stride]: src[0] is the sample at offset -8 (it takes tap t_8), src[16 stride] the one at offset +8 (tap t_-8); two chains, as in cl_fir
__device__ __forceinline__ double cw_fir(const double* src, int stride) {
    constexpr ClWaveletTaps W = cl_wavelet_taps();
    double a = 0.0, b = W.t[CW_REACH] * src[CW_REACH * stride];
#pragma unroll
    for (int u = 0; u < CW_REACH; ++u) {
        a = fma(W.t[CW_TAPS - 1 - u], src[u * stride], a);
        b = fma(W.t[CW_REACH - 1 - u], src[(CW_REACH + 1 + u) * stride], b);
    }
    return a + b;
}

// the 24 x 80 ms samples of one band a tile depends on, modulo (h, w): the only place the circular boundary appears.  (r, c): the thread's first halo
// row and its column, already modulo the sides
__device__ __forceinline__ void cw_ms_load(const float* __restrict__ ms, int h, int w, int r, int c, float (&v)[CW_MLOADS]) {
#pragma unroll
    for (int u = 0; u < CW_MLOADS; ++u) {
        v[u] = 0.f;
        if (threadIdx.x < CW_LROWS * CW_MC) v[u] = ms[(long)r * w + c];
        r += CW_LROWS;
        if (r >= h) r -= h;
    }
}

// Per band two LDS passes: the FIR along y on the halo tile (8 x 80 outputs), then along x straight into the register of the lane that owns the block.
// Columns first because the tile is wide: 17 (80 / 64 + 1) products per block and band, against 17 (24 / 8 + 1) rows first.  In both passes consecutive lanes
// read consecutive doubles.  V is double-buffered, so a band costs two barriers: band k + 1 writes M after barrier B of band k (M's last readers are in front
// of it) and the other V, and a wave that writes V[k & 1] again (band k + 2) has passed barrier A of band k + 1, which every wave reaches after its reads of band k.
__global__ __launch_bounds__(CL_NT, 4) void k_cl_wavelet(const float* __restrict__ ms, const float* __restrict__ pan, float* __restrict__ out, int C, int h, int w,
                                                      int tiles_x) {
    __shared__ double M[CW_MR * CW_MC];              // 15 KiB
    __shared__ double V[2][CW_BY * CW_MC];           // 2 x 5 KiB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H4 = 4 * h, W4 = 4 * w;
    const int i0 = (blockIdx.x / tiles_x) * CW_BY, j0 = (blockIdx.x % tiles_x) * CW_BX;
    const long b = blockIdx.y, plane = (long)H4 * W4;
    const float* __restrict__ ms_b = ms + b * C * ((long)h * w);
    const float* __restrict__ pan_b = pan + b * plane;
    float* __restrict__ out_b = out + b * C * plane;
    const int lr = tid / CW_MC, lc = tid - lr * CW_MC;      // halo row (of the first load) and column this thread loads
    const int mr = cl_mod(i0 - CW_REACH + lr, h), mc = cl_mod(j0 - CW_REACH + lc, w);
    float v[CW_MLOADS];
    cw_ms_load(ms_b, h, w, mr, mc, v);               // ahead of the PAN loads: the first M does not wait for them
    float4 p[CW_PER][4] = {};
    long o[CW_PER];
    bool in[CW_PER];
#pragma unroll
    for (int q = 0; q < CW_PER; ++q) {
        const int i = i0 + wave + q * (CL_NT / 64), j = j0 + lane;
        in[q] = i < h && j < w;
        o[q] = (long)(4 * i) * W4 + 4 * j;
        if (in[q]) {
#pragma unroll
            for (int dy = 0; dy < 4; ++dy) p[q][dy] = *reinterpret_cast<const float4*>(pan_b + o[q] + (long)dy * W4);
        }
    }
    double pm[CW_PER] = {};                           // the block mean of PAN
    for (int k = 0; k < C; ++k) {
#pragma unroll
        for (int u = 0; u < CW_MLOADS; ++u)
            if (tid < CW_LROWS * CW_MC) M[tid + u * (CW_LROWS * CW_MC)] = (double)v[u];
        if (k + 1 < C) cw_ms_load(ms_b + (k + 1) * ((long)h * w), h, w, mr, mc, v);      // the next band's, under this band's two passes
        __syncthreads();                             // A
        double* Vk = V[k & 1];
#pragma unroll 1
        for (int i = tid; i < CW_BY * CW_MC; i += CL_NT) {
            const int r = i / CW_MC, c = i - r * CW_MC;
            Vk[i] = cw_fir(M + r * CW_MC + c, CW_MC);          // ms rows i0 + r - 8 .. i0 + r + 8
        }
        __syncthreads();                             // B
        if (k == 0) {                                // here, not in front of the loop: the PAN loads have had the first band's passes to arrive
#pragma unroll
            for (int q = 0; q < CW_PER; ++q) {
                double s = 0.0;
#pragma unroll
                for (int dy = 0; dy < 4; ++dy) s += ((double)p[q][dy].x + (double)p[q][dy].y) + ((double)p[q][dy].z + (double)p[q][dy].w);
                pm[q] = 0.0625 * s;
            }
        }
#pragma unroll
        for (int q = 0; q < CW_PER; ++q) {
            const double d = cw_fir(Vk + (wave + q * (CL_NT / 64)) * CW_MC + lane, 1) - pm[q];      // M_k - P of the block
            if (in[q]) {
                float* dst = out_b + k * plane + o[q];
#pragma unroll
                for (int dy = 0; dy < 4; ++dy)
                    *reinterpret_cast<float4*>(dst + (long)dy * W4) = make_float4(cl_clip((double)p[q][dy].x + d), cl_clip((double)p[q][dy].y + d),
                                                                                  cl_clip((double)p[q][dy].z + d), cl_clip((double)p[q][dy].w + d));
            }
        }
    }
}

// ---- MTF-GLP: the generalised Laplacian pyramid with an MTF-matched Gaussian and three injection rules.  SFIM's moments and finish give
// mu, m_k and a_k; then
//   k_mg_lowpass   grid (tile, filter, sample): D_f(i, j) = the separable Gaussian of filter f on PAN minus the pivot at (4 i + 2, 4 j + 2), replicate border,
//                  evaluated at the decimated positions only -- rows into LDS, then columns (k_wald.hip's scheme), fp64 [B, F, h, w] in the workspace.
//   k_mg_moments   cbd only, grid (gx, sample) like k_cl_moments: per band the tiles of u_k (cl_up_band on ms) and of L_k (cl_up_band on q_k = a_k (D_k - mu) + m_k,
//                  the affine map applied where D is loaded, modulo the sides), both minus m_k; wave j sums vector j of {u, L, u L, L L} over the tile and
//                  lane 0 adds to its slot in LDS -- one order, always.  k_mg_finish: the partials in ascending order (cl_partials_column), then g_k per band.
//   k_mg_apply     grid (tile, sample): per band the tile of u, the tile of L, the thread's two PAN pixels, the rule, ONE rounding; the next band's ms and D
//                  samples are in flight under the current band's eight LDS passes.  The workgroup of tile 0 writes stats.
// Neither u nor L is ever stored in memory.  The two tile kernels carry a second stream of samples (q) beside ms and k_mg_moments loads across tiles, so
// they keep their own band loops, not cl_up_bands.
constexpr int MG_TO = 16, MG_MAX_TAPS = 63, MG_SPAN = 4 * (MG_TO - 1) + MG_MAX_TAPS;      // low-pass: outputs per tile edge, PAN rows under one tile's column taps
constexpr int MG_LDS = CL_SCRATCH + 2 * CL_PX;                           // doubles: the scratch of cl_up_band, the tile of u, the tile of L
constexpr int MG_PER_CU = 3, MG_RESIDENT = MG_PER_CU * CL_CUS;           // workgroups per sample of the second moments pass, at most
static_assert(MG_PER_CU * (MG_LDS + 4 * CL_MAX_C) * (int)sizeof(double) <= CL_CU_LDS, "three workgroups of the tile kernels per CU");
static_assert(CL_NT / 64 == 4 && MG_TO * MG_TO == CL_NT, "a wave per sum of the second moments pass; a thread per output of the low-pass tile");

__device__ __forceinline__ int mg_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__global__ __launch_bounds__(CL_NT) void k_mg_lowpass(const float* __restrict__ pan, const double* __restrict__ taps, double* __restrict__ dlow, int h, int w,
                                                      int n_taps, int tiles_x) {
    __shared__ double tp[MG_MAX_TAPS];
    __shared__ double rowf[MG_SPAN][MG_TO + 1];
    const int H4 = 4 * h, W4 = 4 * w, r = n_taps >> 1, tid = threadIdx.x;
    const int oy0 = (blockIdx.x / tiles_x) * MG_TO, ox0 = (blockIdx.x % tiles_x) * MG_TO;
    const long b = blockIdx.z, f = blockIdx.y;
    const float* __restrict__ pan_b = pan + b * ((long)H4 * W4);
    const double pv = (double)pan_b[0];
    if (tid < n_taps) tp[tid] = taps[f * n_taps + tid];
    __syncthreads();
    // row pass: slot s is PAN row 4 oy0 + 2 - r + s (clamped into the plane), column j the tile's j-th decimated position
    const int rows = oy0 + MG_TO <= h ? MG_TO : h - oy0, span = 4 * (rows - 1) + n_taps;
    const int y0 = 4 * oy0 + 2 - r, x0 = 4 * ox0 + 2 - r;
    for (int t = tid; t < span * MG_TO; t += CL_NT) {
        const int s = t / MG_TO, j = t - s * MG_TO;
        if (ox0 + j >= w) continue;
        const float* __restrict__ row = pan_b + (long)mg_clamp(y0 + s, H4) * W4;
        const int xb = x0 + 4 * j;
        double acc = 0.0;
        for (int k = 0; k < n_taps; ++k) acc = fma(tp[k], (double)row[mg_clamp(xb + k, W4)] - pv, acc);
        rowf[s][j] = acc;
    }
    __syncthreads();
    const int ly = tid / MG_TO, lx = tid - ly * MG_TO;
    if (ly >= rows || ox0 + lx >= w) return;
    double acc = 0.0;
    for (int k = 0; k < n_taps; ++k) acc = fma(tp[k], rowf[4 * ly + k][lx], acc);
    dlow[(b * gridDim.y + f) * ((long)h * w) + (long)(oy0 + ly) * w + ox0 + lx] = acc;
}

// the samples of q_k = a (D - mu) + m the tile at o depends on, where cl_ms_load takes those of ms: D is the filtered PAN minus the pivot, mpc = mu minus the pivot
__device__ __forceinline__ void mg_q_load(const double* __restrict__ dl, int h, int w, ClTile o, double a, double mpc, double m, double (&v)[CL_MLOADS]) {
    const int my0 = o.Y0 / 4 - 8, mx0 = o.X0 / 4 - 8;
#pragma unroll
    for (int u = 0; u < CL_MLOADS; ++u) {
        const int i = threadIdx.x + u * CL_NT, r = i / CL_MC, c = i - r * CL_MC;
        v[u] = 0.0;
        if (i < CL_MR * CL_MC) v[u] = fma(a, dl[(long)cl_mod(my0 + r, h) * w + cl_mod(mx0 + c, w)] - mpc, m);
    }
}

// part [B][gx][4 C]: per band the sums over the sample of u - m, L - m, (u - m)(L - m), (L - m)^2 (m = m_k: both vectors have a mean near zero, so the
// covariance and the variance lose nothing to cancellation)
__global__ __launch_bounds__(CL_NT) void k_mg_moments(const float* __restrict__ ms, const double* __restrict__ dlow, const double* __restrict__ coef,
                                                      double* __restrict__ part, int C, int F, int h, int w, int tiles_x, int tiles) {
    extern __shared__ double cl_lds[];
    double* U = cl_lds + CL_SCRATCH;
    double* Lt = U + CL_PX;
    double* acc = Lt + CL_PX;                    // [4 C]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, gx = gridDim.x;
    const int H4 = 4 * h, W4 = 4 * w;
    const long b = blockIdx.y, lp = (long)h * w;
    const float* __restrict__ ms_b = ms + b * C * lp;
    const double* __restrict__ dl_b = dlow + b * F * lp;
    const double* __restrict__ co = coef + b * (3 * C + 1);
    const double mpc = co[0];
    for (int e = tid; e < 4 * C; e += CL_NT) acc[e] = 0.0;      // (the barriers inside cl_up_band order this before the first use)
    float v[CL_MLOADS], vn[CL_MLOADS] = {};
    double q[CL_MLOADS], qn[CL_MLOADS] = {};
    cl_ms_load(ms_b, h, w, cl_tile(blockIdx.x, tiles_x), v);
    mg_q_load(dl_b, h, w, cl_tile(blockIdx.x, tiles_x), co[1 + C], mpc, co[1], q);
    for (int t = blockIdx.x; t < tiles; t += gx) {
        const auto [Y0, X0] = cl_tile(t, tiles_x);
        for (int k = 0; k < C; ++k) {
            const int kn = k + 1 < C ? k + 1 : 0, tn = k + 1 < C ? t : t + gx;
            if (tn < tiles) {
                cl_ms_load(ms_b + kn * lp, h, w, cl_tile(tn, tiles_x), vn);
                mg_q_load(dl_b + (F == 1 ? 0 : kn) * lp, h, w, cl_tile(tn, tiles_x), co[1 + C + kn], mpc, co[1 + kn], qn);
            }
            cl_up_band(v, cl_lds, U);
            cl_up_band(q, cl_lds, Lt);
            __syncthreads();
            const double m = co[1 + k];
            double s = 0.0;
#pragma unroll
            for (int u = 0; u < CL_PX / 64; ++u) {
                const int p = lane + 64 * u;
                const bool in = Y0 + p / CL_TW < H4 && X0 + p % CL_TW < W4;      // what a ragged tile holds outside the image counts as 0
                const double uc = U[p] - m, lc = Lt[p] - m;
                const double term = wave == 0 ? uc : wave == 1 ? lc : wave == 2 ? uc * lc : lc * lc;
                s += in ? term : 0.0;
            }
            s = wave_sum(s);
            if (lane == 0) acc[4 * k + wave] += s;
            cl_next(v, vn);
            cl_next(q, qn);
            // no barrier: the next cl_up_band writes U and Lt in its last pass, four barriers from here
        }
    }
    __syncthreads();
    for (int e = tid; e < 4 * C; e += CL_NT) part[(b * gx + blockIdx.x) * (4 * C) + e] = acc[e];
}

// g_k = cov(u_k, L_k) / var(L_k) into coef[b][1 + 2 C + k]; 0 for a band whose a_k is 0 (a constant PAN), whose variance is not positive or not finite, or
// whose gain is not finite
__global__ __launch_bounds__(CL_NT) void k_mg_finish(const double* __restrict__ part, double* __restrict__ coef, int C, int gx, double N) {
    __shared__ double sums[4 * CL_MAX_C];
    const long b = blockIdx.x;
    const int ns = 4 * C;
    for (int e = threadIdx.x; e < ns; e += CL_NT) sums[e] = cl_partials_column(part + b * gx * ns + e, gx, ns);
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= C) return;
    double* co = coef + b * (3 * C + 1);
    const double su = sums[4 * k], sl = sums[4 * k + 1], cov = sums[4 * k + 2] - su * sl / N, var = sums[4 * k + 3] - sl * sl / N;
    const double g = cov / var;
    const bool ok = co[1 + C + k] != 0.0 && var > 0.0 && var - var == 0.0 && g - g == 0.0;
    co[1 + 2 * C + k] = ok ? g : 0.0;
}

template <int MODE>
__global__ __launch_bounds__(CL_NT) void k_mg_apply(const float* __restrict__ ms, const float* __restrict__ pan, const double* __restrict__ dlow,
                                                    float* __restrict__ out, const double* __restrict__ coef, double* __restrict__ stats, int C, int F, int h,
                                                    int w, int tiles_x) {
    extern __shared__ double cl_lds[];
    double* U = cl_lds + CL_SCRATCH;
    double* Lt = U + CL_PX;
    const int tid = threadIdx.x, H4 = 4 * h, W4 = 4 * w;
    const auto [Y0, X0] = cl_tile(blockIdx.x, tiles_x);
    const long b = blockIdx.y, lp = (long)h * w, plane = (long)H4 * W4;
    const float* __restrict__ ms_b = ms + b * C * lp;
    const double* __restrict__ dl_b = dlow + b * F * lp;
    const float* __restrict__ pan_b = pan + b * plane;
    float* __restrict__ out_b = out + b * C * plane;
    const double* __restrict__ co = coef + b * (3 * C + 1);
    const double pv = (double)pan_b[0], mpc = co[0];
    if (stats && blockIdx.x == 0 && tid < C) {      // a_k, then g_k (1 where the rule has no gain)
        stats[b * (2 * C) + tid] = co[1 + C + tid];
        stats[b * (2 * C) + C + tid] = MODE == LG_MTFGLP_CBD ? co[1 + 2 * C + tid] : 1.0;
    }
    float v[CL_MLOADS], vn[CL_MLOADS] = {};
    double q[CL_MLOADS], qn[CL_MLOADS] = {};
    cl_ms_load(ms_b, h, w, {Y0, X0}, v);
    mg_q_load(dl_b, h, w, {Y0, X0}, co[1 + C], mpc, co[1], q);
    const int p = 2 * tid, y = Y0 + p / CL_TW, x = X0 + p % CL_TW;
    const bool in = y < H4 && x < W4;            // W4 is a multiple of 4 and x is even: both pixels or none
    const long o = (long)y * W4 + x;
    float2 pp = make_float2(0.f, 0.f);
    if (in) pp = *reinterpret_cast<const float2*>(pan_b + o);
    const double c0 = ((double)pp.x - pv) - mpc, c1 = ((double)pp.y - pv) - mpc;      // pan - mu
    for (int k = 0; k < C; ++k) {
        if (k + 1 < C) {
            cl_ms_load(ms_b + (k + 1) * lp, h, w, {Y0, X0}, vn);
            mg_q_load(dl_b + (F == 1 ? 0 : k + 1) * lp, h, w, {Y0, X0}, co[1 + C + k + 1], mpc, co[1 + k + 1], qn);
        }
        cl_up_band(v, cl_lds, U);
        cl_up_band(q, cl_lds, Lt);
        __syncthreads();
        if (in) {
            const double a = co[1 + C + k], m = co[1 + k];
            const double u0 = U[p], u1 = U[p + 1], l0 = Lt[p], l1 = Lt[p + 1], p0 = fma(a, c0, m), p1 = fma(a, c1, m);
            double o0, o1;
            if (MODE == LG_MTFGLP_HPM) {
                o0 = u0 * p0 / (l0 + 1e-8);
                o1 = u1 * p1 / (l1 + 1e-8);
            } else {
                const double g = MODE == LG_MTFGLP_CBD ? co[1 + 2 * C + k] : 1.0;
                o0 = fma(g, p0 - l0, u0);
                o1 = fma(g, p1 - l1, u1);
            }
            *reinterpret_cast<float2*>(out_b + k * plane + o) = make_float2(cl_clip(o0), cl_clip(o1));
        }
        cl_next(v, vn);
        cl_next(q, qn);
        // no barrier: the next cl_up_band writes U and Lt in its last pass, four barriers from here
    }
}

// ---- A trous: ATWT and AWLP, the detail of PAN against its two-level undecimated B3-spline low-pass (lg_atrous).  The cascade -- (1, 4, 6, 4, 1) / 16
// along rows and columns, then the same five taps 2 apart -- is ONE separable 13-tap circular filter (at_taps).  SFIM's moments and finish give mu, m_k and
// a_k = std(u_k) / std(pan); then
//   at_rows / at_cols2  the low-pass of a 16 x 32 tile, written once for both kernels: PAN minus the pivot with a circular halo of 6 (28 x 44) into LDS, the 13 row taps
//                  into a 28 x 32 plane, the 13 column taps straight into the registers of the thread that owns the two pixels.
//   k_at_lowvar    match = lowpass only, grid (gx2, sample), gx2 = min(tiles, 768); a workgroup walks the tiles gx2 apart and sums (P_L - mu)^2 over each in one order
//                  (butterfly inside a wave, the four waves pairwise): one partial per workgroup.  k_at_finish: SFIM's partials of u_k and these in ascending
//                  order (cl_partials_column), then a_k = std(u_k) / s_L over coef's a_k, and s_L into coef's first gain slot, which SFIM leaves unused.
//   k_at_apply     grid (tile, sample): the detail d = pan - P_L of the thread's two pixels into registers (the staged PAN lies in cl_up_band's scratch, which is free
//                  until the first band), for AWLP the tile of interp23 of the band mean of ms (interp23 is linear: that is the band mean of u, and the LDS does
//                  not grow with C), then per band the tile of u, the rule, ONE rounding; the next band's ms samples are in flight under the current band's
//                  passes.  The workgroup of tile 0 writes stats: a_k, then the reference deviation -- std(pan) from SFIM's partials, or s_L from coef.
// A PAN side is at least 16 and a ragged tile reaches up to 37 past the origin: an index may wrap more than once, which cl_mod (a true modulo) allows.
constexpr int AT_REACH = 6, AT_TAPS = 2 * AT_REACH + 1;
constexpr int AT_PH = CL_TH + 2 * AT_REACH, AT_PW = CL_TW + 2 * AT_REACH;      // the staged PAN: 28 x 44
constexpr int AT_STAGE = AT_PH * AT_PW + AT_PH * CL_TW;                  // doubles: the staged PAN, then the row-filtered plane [28][32]
constexpr int AT_RESIDENT = 768;                                         // workgroups per sample of k_at_lowvar, at most: three per CU
constexpr int AT_FINISH_NT = 64;
static_assert(AT_STAGE <= CL_SCRATCH, "k_at_apply stages PAN in the scratch of cl_up_band");
static_assert(AT_FINISH_NT >= 2 * CL_MAX_C + 1, "a thread per column of partials in k_at_finish");

__host__ __device__ inline int at_apply_lds_doubles(int rule) { return CL_SCRATCH + (rule == LG_ATROUS_AWLP ? 2 : 1) * CL_PX; }

// the 13 taps by offset -6 .. 6: tap a of level 1 meets tap c of level 2 at offset a + 2 c.  Every product and every sum is exact: (1, 4, 10, 20, 31, 40, 44, ...) / 256
struct AtTaps { double t[AT_TAPS]; };
__host__ __device__ constexpr AtTaps at_taps() {
    constexpr double B3[5] = {1.0 / 16, 4.0 / 16, 6.0 / 16, 4.0 / 16, 1.0 / 16};
    AtTaps r = {};
    for (int a = -2; a <= 2; ++a)
        for (int c = -2; c <= 2; ++c) r.t[AT_REACH + a + 2 * c] += B3[a + 2] * B3[c + 2];
    return r;
}

// PT[28][44]: staged pixel (r, c) = PAN pixel (Y0 - 6 + r, X0 - 6 + c) modulo the sides, minus the pivot; RW[28][32]: RW(r, c) = sum_j t_j PT(r, c + j), the row
// taps of tile column c.  Ends WITH a barrier.  (src[0] is the sample at offset -6; two chains, as in cl_fir)
__device__ __forceinline__ void at_rows(const float* __restrict__ pan_b, double pv, int H4, int W4, int Y0, int X0, double* PT, double* RW) {
    constexpr AtTaps T = at_taps();
    for (int i = threadIdx.x; i < AT_PH * AT_PW; i += CL_NT) {
        const int r = i / AT_PW, c = i - r * AT_PW;
        PT[i] = (double)pan_b[(long)cl_mod(Y0 - AT_REACH + r, H4) * W4 + cl_mod(X0 - AT_REACH + c, W4)] - pv;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < AT_PH * CL_TW; i += CL_NT) {
        const double* src = PT + (i / CL_TW) * AT_PW + i % CL_TW;
        double a = 0.0, b = T.t[AT_REACH] * src[AT_REACH];
#pragma unroll
        for (int u = 0; u < AT_REACH; ++u) {
            a = fma(T.t[u], src[u], a);
            b = fma(T.t[AT_REACH + 1 + u], src[AT_REACH + 1 + u], b);
        }
        RW[i] = a + b;
    }
    __syncthreads();
}

// P_L minus the pivot at the tile's pixels (oy, ox) and (oy, ox + 1): the 13 column taps on q = RW + oy * 32 + ox; the two pixels' samples are adjacent doubles
__device__ __forceinline__ void at_cols2(const double* q, double& l0, double& l1) {
    constexpr AtTaps T = at_taps();
    double a0 = 0.0, b0 = T.t[AT_REACH] * q[AT_REACH * CL_TW], a1 = 0.0, b1 = T.t[AT_REACH] * q[AT_REACH * CL_TW + 1];
#pragma unroll
    for (int u = 0; u < AT_REACH; ++u) {
        a0 = fma(T.t[u], q[u * CL_TW], a0);
        a1 = fma(T.t[u], q[u * CL_TW + 1], a1);
        b0 = fma(T.t[AT_REACH + 1 + u], q[(AT_REACH + 1 + u) * CL_TW], b0);
        b1 = fma(T.t[AT_REACH + 1 + u], q[(AT_REACH + 1 + u) * CL_TW + 1], b1);
    }
    l0 = a0 + b0;
    l1 = a1 + b1;
}

// part2 [B][gx2]: a workgroup's sum of (P_L - mu)^2 over its tiles
__global__ __launch_bounds__(CL_NT) void k_at_lowvar(const float* __restrict__ pan, const double* __restrict__ coef, double* __restrict__ part2, int C, int h,
                                                     int w, int tiles_x, int tiles) {
    __shared__ double S[AT_STAGE], red[CL_NT / 64];
    const int tid = threadIdx.x, gx = gridDim.x, H4 = 4 * h, W4 = 4 * w;
    const long b = blockIdx.y;
    const float* __restrict__ pan_b = pan + b * ((long)H4 * W4);
    const double pv = (double)pan_b[0], mpc = coef[b * (3 * C + 1)];
    const int p = 2 * tid, oy = p / CL_TW, ox = p % CL_TW;
    double acc = 0.0;
    for (int t = blockIdx.x; t < tiles; t += gx) {
        const auto [Y0, X0] = cl_tile(t, tiles_x);
        at_rows(pan_b, pv, H4, W4, Y0, X0, S, S + AT_PH * AT_PW);
        double l0, l1;
        at_cols2(S + AT_PH * AT_PW + oy * CL_TW + ox, l0, l1);
        const double e0 = l0 - mpc, e1 = l1 - mpc;
        const bool in = Y0 + oy < H4 && X0 + ox < W4;      // W4 is a multiple of 4 and ox is even: both pixels or none
        acc += block_sum4(in ? fma(e1, e1, e0 * e0) : 0.0, red);
        // no barrier: the next tile's at_rows writes the plane behind block_sum4's barrier, and red behind its own two
    }
    if (tid == 0) part2[b * gx + blockIdx.x] = acc;
}

// match = lowpass: a_k = std(u_k) / s_L into coef[b][1 + C + k], s_L into coef[b][1 + 2 C]; all of them 0 where s_L^2 is not > 0.  std(u_k) is k_cl_finish's,
// from the same partials in the same order.
__global__ __launch_bounds__(AT_FINISH_NT) void k_at_finish(const double* __restrict__ part, const double* __restrict__ part2, double* __restrict__ coef, int C,
                                                            int gx, int gx2, double N) {
    __shared__ double sums[2 * CL_MAX_C + 1];
    const long b = blockIdx.x;
    const int ns = 2 * C + 2, k = threadIdx.x;
    if (k < 2 * C) sums[k] = cl_partials_column(part + b * gx * ns + k, gx, ns);
    if (k == 2 * C) sums[k] = cl_partials_column(part2 + b * gx2, gx2, 1);
    __syncthreads();
    if (k >= C) return;
    double* co = coef + b * (3 * C + 1);
    const double var_l = sums[2 * C] / (N - 1.0);
    const double su = sums[2 * k], var_u = (sums[2 * k + 1] - su * su / N) / (N - 1.0);
    co[1 + C + k] = var_l > 0.0 ? sqrt(fmax(var_u, 0.0) / var_l) : 0.0;
    if (k == 0) co[1 + 2 * C] = var_l > 0.0 ? sqrt(var_l) : 0.0;
}

// part: SFIM's partials [B][gx][2 C + 2] (match = pan: the reference deviation is std(pan)) or NULL (match = lowpass: it is in coef).  stats: NULL or [B][C + 1].
template <int RULE>
__global__ __launch_bounds__(CL_NT) void k_at_apply(const float* __restrict__ ms, const float* __restrict__ pan, float* __restrict__ out,
                                                    const double* __restrict__ coef, const double* __restrict__ part, double* __restrict__ stats, int C, int h,
                                                    int w, int tiles_x, int gx, double N) {
    extern __shared__ double cl_lds[];
    __shared__ double pmom[2];
    double* U = cl_lds + CL_SCRATCH;
    double* Um = U + CL_PX;                      // AWLP: the tile of the band mean of u
    const int tid = threadIdx.x, H4 = 4 * h, W4 = 4 * w;
    const auto [Y0, X0] = cl_tile(blockIdx.x, tiles_x);
    const long b = blockIdx.y, lp = (long)h * w, plane = (long)H4 * W4;
    const float* __restrict__ ms_b = ms + b * C * lp;
    const float* __restrict__ pan_b = pan + b * plane;
    float* __restrict__ out_b = out + b * C * plane;
    const double* __restrict__ co = coef + b * (3 * C + 1);
    const double pv = (double)pan_b[0];
    if (stats && blockIdx.x == 0) {              // a_k, then the reference deviation
        if (tid < C) stats[b * (C + 1) + tid] = co[1 + C + tid];
        if (part) {
            const int ns = 2 * C + 2;
            if (tid < 2) pmom[tid] = cl_partials_column(part + b * gx * ns + 2 * C + tid, gx, ns);
            __syncthreads();
            const double var_p = (pmom[1] - pmom[0] * pmom[0] / N) / (N - 1.0);      // k_cl_finish's
            if (tid == 0) stats[b * (C + 1) + C] = var_p > 0.0 ? sqrt(var_p) : 0.0;
        } else if (tid == 0) {
            stats[b * (C + 1) + C] = co[1 + 2 * C];
        }
    }
    float v[CL_MLOADS], vn[CL_MLOADS] = {};
    cl_ms_load(ms_b, h, w, {Y0, X0}, v);         // the first band's, under the passes on PAN
    double mv[CL_MLOADS] = {};
    if (RULE == LG_ATROUS_AWLP) {                // the band mean of ms at the samples the tile depends on: four bands in flight, added in ascending order
        for (int k0 = 0; k0 < C; k0 += 4) {
            float t[4][CL_MLOADS];
#pragma unroll
            for (int j = 0; j < 4; ++j) cl_ms_load(ms_b + (k0 + j < C ? k0 + j : 0) * lp, h, w, {Y0, X0}, t[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int u = 0; u < CL_MLOADS; ++u) mv[u] += k0 + j < C ? (double)t[j][u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CL_MLOADS; ++u) mv[u] /= (double)C;
    }
    const int p = 2 * tid, oy = p / CL_TW, ox = p % CL_TW, y = Y0 + oy, x = X0 + ox;
    const bool in = y < H4 && x < W4;            // W4 is a multiple of 4 and x is even: both pixels or none
    const long o = (long)y * W4 + x;
    double d0, d1;                               // pan - P_L
    {
        double* PT = cl_lds;
        double* RW = PT + AT_PH * AT_PW;
        at_rows(pan_b, pv, H4, W4, Y0, X0, PT, RW);
        at_cols2(RW + oy * CL_TW + ox, d0, d1);
        d0 = PT[(oy + AT_REACH) * AT_PW + ox + AT_REACH] - d0;
        d1 = PT[(oy + AT_REACH) * AT_PW + ox + AT_REACH + 1] - d1;
        __syncthreads();                         // the scratch is cl_up_band's from here
    }
    if (RULE == LG_ATROUS_AWLP) cl_up_band(mv, cl_lds, Um);      // (the barriers inside the first band's cl_up_band order it before its use)
    for (int k = 0; k < C; ++k) {
        if (k + 1 < C) cl_ms_load(ms_b + (k + 1) * lp, h, w, {Y0, X0}, vn);
        cl_up_band(v, cl_lds, U);
        __syncthreads();
        if (in) {
            const double a = co[1 + C + k], u0 = U[p], u1 = U[p + 1];
            double g0 = a * d0, g1 = a * d1;
            if (RULE == LG_ATROUS_AWLP) {
                const double n0 = Um[p] + 1e-8, n1 = Um[p + 1] + 1e-8;
                g0 = n0 > 0.0 && n0 - n0 == 0.0 ? g0 * (u0 / n0) : 0.0;
                g1 = n1 > 0.0 && n1 - n1 == 0.0 ? g1 * (u1 / n1) : 0.0;
            }
            *reinterpret_cast<float2*>(out_b + k * plane + o) = make_float2(cl_clip(u0 + g0), cl_clip(u1 + g1));
        }
        cl_next(v, vn);
        // no barrier: the next cl_up_band writes U in its last pass, four barriers from here
    }
}

struct ClGeom {
    int tiles_x, tiles, gx, ns;
    size_t off[2], bytes;      // part, coef
};

// false: not a shape (cl_shape) or method the calls take: the geometry of the moments pass and the workspace of lg_sfim / lg_gsa
bool cl_geom(const char* who, int B, int C, int h, int w, int method, ClGeom& g) {
    if (!cl_shape(who, B, C, h, w)) return false;
    if (method != LG_CLASSICAL_SFIM && method != LG_CLASSICAL_GSA) { lg_set_error("%s: method must be LG_CLASSICAL_SFIM or LG_CLASSICAL_GSA (got %d)", who, method); return false; }
    g.tiles = cl_tiles(h, w, g.tiles_x);
    // the moments pass: at most as many workgroups per sample as are resident at once (768 at C = 4, 512 at C = 8, 256 at C = 16): a second,
    // partial round of workgroups would leave most of the chip idle for as long as the first took
    const int resident = CL_CUS * (CL_CU_LDS / (cl_moment_lds_doubles(C) * (int)sizeof(double) + CL_MAX_SUMS * (int)sizeof(int)));
    g.gx = g.tiles < resident ? g.tiles : resident;
    g.ns = method == LG_CLASSICAL_GSA ? (C + 2) * (C + 3) : 2 * C + 2;
    const size_t sz[2] = {ws_region(B, (size_t)g.gx * g.ns * sizeof(double)), ws_region(B, (size_t)(3 * C + 1) * sizeof(double))};
    g.bytes = ws_layout(2, sz, g.off);
    return true;
}

DeviceOnce cl_attr_once;
int cl_lds_attr(const char* who) {
    if (!cl_attr_once.need()) return 0;
    if (int rc = lds_attr_set(who, cl_moment_lds_doubles(CL_MAX_C) * (int)sizeof(double), k_cl_moments)) return rc;
    if (int rc = lds_attr_set(who, cl_apply_lds_doubles(CL_MAX_C) * (int)sizeof(double), k_cl_apply<false>, k_cl_apply<true>)) return rc;
    cl_attr_once.done();
    return 0;
}

int cl_fuse(const char* who, int method, const float* ms, const float* pan, float* out, double* stats, int B, int C, int h, int w, void* workspace,
            size_t workspace_bytes, hipStream_t s) {
    ClGeom g;
    if (!cl_geom(who, B, C, h, w, method, g)) return -1;
    if (!cl_check_args(who, ms, pan, out, {}, stats, workspace, workspace_bytes, g.bytes, "lg_classical_workspace_bytes")) return -1;
    if (int rc = cl_lds_attr(who)) return rc;
    const int gsa = method == LG_CLASSICAL_GSA;
    double *part = cl_ws(workspace, g.off[0]), *coef = cl_ws(workspace, g.off[1]);
    k_cl_moments<<<dim3(g.gx, B), CL_NT, cl_moment_lds_doubles(C) * sizeof(double), s>>>(ms, pan, part, C, h, w, g.tiles_x, g.tiles, gsa);
    LG_CHECK_LAUNCH();
    k_cl_finish<<<B, CL_NT, 0, s>>>(part, coef, stats, C, g.gx, 16.0 * h * w, (double)h * w, gsa);
    LG_CHECK_LAUNCH();
    const size_t lds = cl_apply_lds_doubles(C) * sizeof(double);
    if (gsa)
        k_cl_apply<true><<<dim3(g.tiles, B), CL_NT, lds, s>>>(ms, pan, out, coef, C, h, w, g.tiles_x);
    else
        k_cl_apply<false><<<dim3(g.tiles, B), CL_NT, lds, s>>>(ms, pan, out, coef, C, h, w, g.tiles_x);
    LG_CHECK_LAUNCH();
    return 0;
}

struct MgGeom {
    ClGeom cl;                 // SFIM's: the tiles and the first moments pass
    int gx2;                   // workgroups per sample of the second moments pass
    size_t off[4], bytes;      // part, coef, D, part2 (cbd)
};

// the two rules of the low-pass filters lg_mtf_glp and lg_bdsd take: one for all bands or one per band; an odd number of taps that fits the kernel's LDS
bool mg_filters_ok(const char* who, int C, int n_filters) {
    if (n_filters != 1 && n_filters != C) { lg_set_error("%s: n_filters must be 1 or C = %d (got %d)", who, C, n_filters); return false; }
    return true;
}
bool mg_taps_ok(const char* who, int n_taps) {
    if (n_taps < 1 || n_taps > MG_MAX_TAPS || !(n_taps & 1)) { lg_set_error("%s: n_taps must be odd, in 1..%d (got %d)", who, MG_MAX_TAPS, n_taps); return false; }
    return true;
}

bool mg_geom(const char* who, int B, int C, int h, int w, int n_filters, int mode, MgGeom& g) {
    if (!cl_geom(who, B, C, h, w, LG_CLASSICAL_SFIM, g.cl)) return false;
    if (!mg_filters_ok(who, C, n_filters)) return false;
    if (mode != LG_MTFGLP_GLP && mode != LG_MTFGLP_HPM && mode != LG_MTFGLP_CBD) {
        lg_set_error("%s: mode must be LG_MTFGLP_GLP, LG_MTFGLP_HPM or LG_MTFGLP_CBD (got %d)", who, mode);
        return false;
    }
    g.gx2 = g.cl.tiles < MG_RESIDENT ? g.cl.tiles : MG_RESIDENT;
    const size_t sz[4] = {ws_region(B, (size_t)g.cl.gx * g.cl.ns * sizeof(double)), ws_region(B, (size_t)(3 * C + 1) * sizeof(double)),
                          ws_region(B, (size_t)n_filters * h * w * sizeof(double)),
                          mode == LG_MTFGLP_CBD ? ws_region(B, (size_t)g.gx2 * 4 * C * sizeof(double)) : 0};
    g.bytes = ws_layout(4, sz, g.off);
    return true;
}

int mg_fuse(const char* who, const float* ms, const float* pan, float* out, double* stats, const double* taps, int n_filters, int n_taps, int mode, int B,
            int C, int h, int w, void* workspace, size_t workspace_bytes, hipStream_t s) {
    MgGeom g;
    if (!mg_geom(who, B, C, h, w, n_filters, mode, g)) return -1;
    if (!mg_taps_ok(who, n_taps)) return -1;
    if (!cl_check_args(who, ms, pan, out, {{"taps", taps}}, stats, workspace, workspace_bytes, g.bytes, "lg_mtfglp_workspace_bytes")) return -1;
    if (int rc = cl_lds_attr(who)) return rc;
    double *part = cl_ws(workspace, g.off[0]), *coef = cl_ws(workspace, g.off[1]), *dlow = cl_ws(workspace, g.off[2]), *part2 = cl_ws(workspace, g.off[3]);
    const int tiles_x = g.cl.tiles_x, tiles = g.cl.tiles;
    k_cl_moments<<<dim3(g.cl.gx, B), CL_NT, cl_moment_lds_doubles(C) * sizeof(double), s>>>(ms, pan, part, C, h, w, tiles_x, tiles, 0);
    LG_CHECK_LAUNCH();
    k_cl_finish<<<B, CL_NT, 0, s>>>(part, coef, nullptr, C, g.cl.gx, 16.0 * h * w, (double)h * w, 0);
    LG_CHECK_LAUNCH();
    const int lt_x = (w + MG_TO - 1) / MG_TO, lt = lt_x * ((h + MG_TO - 1) / MG_TO);
    k_mg_lowpass<<<dim3(lt, n_filters, B), CL_NT, 0, s>>>(pan, taps, dlow, h, w, n_taps, lt_x);
    LG_CHECK_LAUNCH();
    const size_t lds = MG_LDS * sizeof(double);
    if (mode == LG_MTFGLP_CBD) {
        k_mg_moments<<<dim3(g.gx2, B), CL_NT, lds + 4 * C * sizeof(double), s>>>(ms, dlow, coef, part2, C, n_filters, h, w, tiles_x, tiles);
        LG_CHECK_LAUNCH();
        k_mg_finish<<<B, CL_NT, 0, s>>>(part2, coef, C, g.gx2, 16.0 * h * w);
        LG_CHECK_LAUNCH();
        k_mg_apply<LG_MTFGLP_CBD><<<dim3(tiles, B), CL_NT, lds, s>>>(ms, pan, dlow, out, coef, stats, C, n_filters, h, w, tiles_x);
    } else if (mode == LG_MTFGLP_HPM) {
        k_mg_apply<LG_MTFGLP_HPM><<<dim3(tiles, B), CL_NT, lds, s>>>(ms, pan, dlow, out, coef, stats, C, n_filters, h, w, tiles_x);
    } else {
        k_mg_apply<LG_MTFGLP_GLP><<<dim3(tiles, B), CL_NT, lds, s>>>(ms, pan, dlow, out, coef, stats, C, n_filters, h, w, tiles_x);
    }
    LG_CHECK_LAUNCH();
    return 0;
}

struct AtGeom {
    ClGeom cl;                 // SFIM's: the tiles and the moments pass
    int gx2;                   // workgroups per sample of k_at_lowvar
    size_t off[3], bytes;      // part, coef, part2 (match = lowpass)
};

bool at_geom(const char* who, int B, int C, int h, int w, int match, AtGeom& g) {
    if (!cl_geom(who, B, C, h, w, LG_CLASSICAL_SFIM, g.cl)) return false;
    if (match != LG_ATROUS_MATCH_PAN && match != LG_ATROUS_MATCH_LOWPASS) {
        lg_set_error("%s: match must be LG_ATROUS_MATCH_PAN or LG_ATROUS_MATCH_LOWPASS (got %d)", who, match);
        return false;
    }
    g.gx2 = g.cl.tiles < AT_RESIDENT ? g.cl.tiles : AT_RESIDENT;
    const size_t sz[3] = {ws_region(B, (size_t)g.cl.gx * g.cl.ns * sizeof(double)), ws_region(B, (size_t)(3 * C + 1) * sizeof(double)),
                          match == LG_ATROUS_MATCH_LOWPASS ? ws_region(B, (size_t)g.gx2 * sizeof(double)) : 0};
    g.bytes = ws_layout(3, sz, g.off);
    return true;
}

int at_fuse(const char* who, const lg_atrous_args* a) {
    if (!a) { lg_set_error("%s: args is NULL", who); return -1; }
    if (a->struct_bytes != sizeof(lg_atrous_args)) {
        lg_set_error("%s: struct_bytes must be sizeof(lg_atrous_args) = %zu (got %u)", who, sizeof(lg_atrous_args), a->struct_bytes);
        return -1;
    }
    if (a->rule != LG_ATROUS_ATWT && a->rule != LG_ATROUS_AWLP) { lg_set_error("%s: rule must be LG_ATROUS_ATWT or LG_ATROUS_AWLP (got %d)", who, a->rule); return -1; }
    const int B = a->B, C = a->C, h = a->h, w = a->w;
    AtGeom g;
    if (!at_geom(who, B, C, h, w, a->match, g)) return -1;
    if (!cl_check_args(who, a->ms, a->pan, a->out, {}, a->stats, a->workspace, a->workspace_bytes, g.bytes, "lg_atrous_workspace_bytes")) return -1;
    if (int rc = cl_lds_attr(who)) return rc;
    hipStream_t s = (hipStream_t)a->stream;
    double *part = cl_ws(a->workspace, g.off[0]), *coef = cl_ws(a->workspace, g.off[1]), *part2 = cl_ws(a->workspace, g.off[2]);
    const int tiles_x = g.cl.tiles_x, tiles = g.cl.tiles;
    const double N = 16.0 * h * w;
    const bool lowpass = a->match == LG_ATROUS_MATCH_LOWPASS;
    k_cl_moments<<<dim3(g.cl.gx, B), CL_NT, cl_moment_lds_doubles(C) * sizeof(double), s>>>(a->ms, a->pan, part, C, h, w, tiles_x, tiles, 0);
    LG_CHECK_LAUNCH();
    k_cl_finish<<<B, CL_NT, 0, s>>>(part, coef, nullptr, C, g.cl.gx, N, (double)h * w, 0);
    LG_CHECK_LAUNCH();
    if (lowpass) {
        k_at_lowvar<<<dim3(g.gx2, B), CL_NT, 0, s>>>(a->pan, coef, part2, C, h, w, tiles_x, tiles);
        LG_CHECK_LAUNCH();
        k_at_finish<<<B, AT_FINISH_NT, 0, s>>>(part, part2, coef, C, g.cl.gx, g.gx2, N);
        LG_CHECK_LAUNCH();
    }
    const double* pmom = lowpass ? nullptr : part;
    const size_t lds = at_apply_lds_doubles(a->rule) * sizeof(double);
    if (a->rule == LG_ATROUS_AWLP)
        k_at_apply<LG_ATROUS_AWLP><<<dim3(tiles, B), CL_NT, lds, s>>>(a->ms, a->pan, a->out, coef, pmom, a->stats, C, h, w, tiles_x, g.cl.gx, N);
    else
        k_at_apply<LG_ATROUS_ATWT><<<dim3(tiles, B), CL_NT, lds, s>>>(a->ms, a->pan, a->out, coef, pmom, a->stats, C, h, w, tiles_x, g.cl.gx, N);
    LG_CHECK_LAUNCH();
    return 0;
}

// ---- MTF-HR: the regression-based and haze-corrected members of the MTF-GLP family -- FS, HPM-R, HPM-H, BT-H (lg_mtf_hr; restated in
// tests/mtf_hr_ref.py).  D_f is k_mg_lowpass's plane (the raw PAN minus the pivot under the MTF taps at the decimated positions); L_k = interp23(D_k) + pivot:
// there is no histogram matching in this family, and a constant PAN has L = pan exactly.
//   k_hr_moments   fs / hpm_r, grid (gx2, sample) like k_mg_moments: per band the tiles of u_k (cl_up_band on ms) and of L_k (cl_up_band on D_k), u minus
//                  m_k, L and PAN minus mu, zero outside the image, as vectors in LDS beside the mask; the seven sums both gains need are sums of products of two
//                  of them (cl_pair_sums).  k_hr_finish: the partials in ascending order, then thread k: g_k and b_k = m_k - g_k mean L_k.
//   k_hr_gram      hpm_h / bt_h, at the MS scale, grid (gpb, sample): a workgroup walks the sample's MS pixels in chunks of 256, gpb chunks apart: the mask, the C
//                  bands minus their first pixel and the F planes D_f as vectors in LDS; every sum of the regression is the sum of a product of two of them
//                  (cl_pair_sums).  The minimum of every band: a wave's by shuffles, the workgroup's over its four waves -- exact and free of any order.
//   k_hr_solve     one wave per sample: the partials in ascending order, the minimum of the minima, one thread's Cholesky of the centred Gram matrix of ms, then
//                  thread f solves for the slopes of D_f; H_P,f (hpm_h) or w_0 and H_I (bt_h) from the means.  A non-positive pivot or a slope that is not finite
//                  gives slopes 0.
//   k_hr_apply     grid (tile, sample), two adjacent pixels per thread, the PAN pair loaded ahead of the first band, ONE rounding, 8-byte stores.  fs / hpm_r /
//                  hpm_h: k_mg_apply's band loop (the tiles of u and L, the next band's samples in flight).  bt_h: the C tiles of u stay in LDS (cl_up_bands, as in
//                  k_cl_apply and k_bd_apply): sum_k w_k (u_k - H_k) needs every band before the first output, and one interpolation per band is cheaper than
//                  two sweeps.
// hc [B][2 C + 2] holds what the apply pass reads, in the layout of stats: fs g; hpm_r g, b; hpm_h H, H_P; bt_h H, w, w_0, H_I; unused slots 0.
constexpr int HR_SUMS = 7;                                               // per band: sum u, L, p, u p, L p, u L, L L (u, L, p centred)
constexpr int HR_CHUNK = CL_NT;                                          // MS pixels a Gram workgroup takes at a time: one per thread
constexpr int HR_GRAM_WGS = 128;                                         // Gram workgroups per sample, at most
constexpr int HR_SOLVE_NT = 64;
constexpr int HR_MAX_NS = (CL_MAX_C + 1) * (CL_MAX_C + 2) / 2 + CL_MAX_C * (CL_MAX_C + 1);
static_assert(HR_SOLVE_NT >= CL_MAX_C, "a thread per filtered plane solves");

__host__ __device__ inline bool hr_haze(int rule) { return rule == LG_MTFHR_HPM_H || rule == LG_MTFHR_BT_H; }
__host__ __device__ inline int hr_gram_ns(int C, int F) { return (C + 1) * (C + 2) / 2 + F * (C + 1); }
__host__ __device__ inline int hr_moments_lds_doubles(int C) { return CL_SCRATCH + 4 * CL_PX + HR_SUMS * C; }
__host__ __device__ inline int hr_gram_lds_doubles(int C, int F) { return (1 + C + F) * HR_CHUNK + hr_gram_ns(C, F) + 4 * C; }
__host__ __device__ inline int hr_apply_lds_doubles(int C, int rule) { return rule == LG_MTFHR_BT_H ? CL_SCRATCH + C * CL_PX : MG_LDS; }

// the samples of D (the filtered PAN minus the pivot) the tile at o depends on, where cl_ms_load takes those of ms: the tile holds L minus the pivot, which
// is exactly 0 for a constant PAN
__device__ __forceinline__ void hr_d_load(const double* __restrict__ dl, int h, int w, ClTile o, double (&v)[CL_MLOADS]) {
    const int my0 = o.Y0 / 4 - 8, mx0 = o.X0 / 4 - 8;
#pragma unroll
    for (int u = 0; u < CL_MLOADS; ++u) {
        const int i = threadIdx.x + u * CL_NT, r = i / CL_MC, c = i - r * CL_MC;
        v[u] = 0.0;
        if (i < CL_MR * CL_MC) v[u] = dl[(long)cl_mod(my0 + r, h) * w + cl_mod(mx0 + c, w)];
    }
}

// r = num / den, 1 (no injection) where the denominator is not > 0 or the ratio is not finite
__device__ __forceinline__ double hr_ratio(double num, double den) {
    const double r = num / den;
    return den > 0.0 && r - r == 0.0 ? r : 1.0;
}

// part [B][gx][7 C]: per band the sums over the sample of uc = u - m_k, lc = L - mu, pc = pan - mu, uc pc, lc pc, uc lc, lc lc
__global__ __launch_bounds__(CL_NT) void k_hr_moments(const float* __restrict__ ms, const float* __restrict__ pan, const double* __restrict__ dlow,
                                                      const double* __restrict__ coef, double* __restrict__ part, int C, int F, int h, int w, int tiles_x,
                                                      int tiles) {
    extern __shared__ double cl_lds[];
    __shared__ int pairs[HR_SUMS];
    double* V = cl_lds + CL_SCRATCH;             // [4][512]: uc, lc, pc, mask
    double* acc = V + 4 * CL_PX;                 // [7 C]
    const int tid = threadIdx.x, gx = gridDim.x;
    const int H4 = 4 * h, W4 = 4 * w;
    const long b = blockIdx.y, lp = (long)h * w;
    const float* __restrict__ ms_b = ms + b * C * lp;
    const float* __restrict__ pan_b = pan + b * ((long)H4 * W4);
    const double* __restrict__ dl_b = dlow + b * F * lp;
    const double* __restrict__ co = coef + b * (3 * C + 1);
    const double pv = (double)pan_b[0], mpc = co[0];
    if (tid == 0) {
        pairs[0] = cl_pair(3, 0, 0);
        pairs[1] = cl_pair(3, 1, 0);
        pairs[2] = cl_pair(3, 2, 0);
        pairs[3] = cl_pair(0, 2, 0);
        pairs[4] = cl_pair(1, 2, 0);
        pairs[5] = cl_pair(0, 1, 0);
        pairs[6] = cl_pair(1, 1, 0);
    }
    for (int e = tid; e < HR_SUMS * C; e += CL_NT) acc[e] = 0.0;      // (the barriers inside cl_up_band order both before their first use)
    float v[CL_MLOADS], vn[CL_MLOADS] = {};
    double q[CL_MLOADS], qn[CL_MLOADS] = {};
    cl_ms_load(ms_b, h, w, cl_tile(blockIdx.x, tiles_x), v);
    hr_d_load(dl_b, h, w, cl_tile(blockIdx.x, tiles_x), q);
    for (int t = blockIdx.x; t < tiles; t += gx) {
        const auto [Y0, X0] = cl_tile(t, tiles_x);
        float pn[CL_PX / CL_NT];
#pragma unroll
        for (int u = 0; u < CL_PX / CL_NT; ++u) {
            const int p = tid + u * CL_NT, y = Y0 + p / CL_TW, x = X0 + p % CL_TW;
            pn[u] = y < H4 && x < W4 ? pan_b[(long)y * W4 + x] : 0.f;
        }
        for (int k = 0; k < C; ++k) {
            const int kn = k + 1 < C ? k + 1 : 0, tn = k + 1 < C ? t : t + gx;
            if (tn < tiles) {
                cl_ms_load(ms_b + kn * lp, h, w, cl_tile(tn, tiles_x), vn);
                hr_d_load(dl_b + (F == 1 ? 0 : kn) * lp, h, w, cl_tile(tn, tiles_x), qn);
            }
            cl_up_band(v, cl_lds, V);
            cl_up_band(q, cl_lds, V + CL_PX);
            __syncthreads();
            const double m = co[1 + k];
#pragma unroll
            for (int u = 0; u < CL_PX / CL_NT; ++u) {
                const int p = tid + u * CL_NT;
                const bool in = Y0 + p / CL_TW < H4 && X0 + p % CL_TW < W4;      // what a ragged tile holds outside the image counts as 0
                V[p] = in ? V[p] - m : 0.0;
                V[CL_PX + p] = in ? V[CL_PX + p] - mpc : 0.0;      // (L - pivot) - (mu - pivot)
                if (k == 0) {      // the tile's own: the last reads of the tile before lie eight barriers back
                    V[2 * CL_PX + p] = in ? ((double)pn[u] - pv) - mpc : 0.0;
                    V[3 * CL_PX + p] = in ? 1.0 : 0.0;
                }
            }
            __syncthreads();
            cl_pair_sums(pairs, HR_SUMS, acc + HR_SUMS * k, [&](int a, int c, int, int lane) { return cl_lane_dot<CL_PX>(V + a * CL_PX, V + c * CL_PX, lane); });
            cl_next(v, vn);
            cl_next(q, qn);
            // no barrier: the next cl_up_band writes the tiles of u and L in its last pass, four barriers from here
        }
    }
    __syncthreads();
    for (int e = tid; e < HR_SUMS * C; e += CL_NT) part[(b * gx + blockIdx.x) * (HR_SUMS * C) + e] = acc[e];
}

// hc (and stats, unless NULL) [B][2 C + 2]: g_k, then b_k (hpm_r; 0 for fs), then two zeros.  g_k = 0 where the denominator is not > 0 or not finite or the gain
// is not finite
__global__ __launch_bounds__(CL_NT) void k_hr_finish(const double* __restrict__ part, const float* __restrict__ pan, const double* __restrict__ coef,
                                                     double* __restrict__ hc, double* __restrict__ stats, int C, int gx, double N, int rule) {
    __shared__ double sums[HR_SUMS * CL_MAX_C];
    const long b = blockIdx.x;
    const int ns = HR_SUMS * C, k = threadIdx.x;
    for (int e = threadIdx.x; e < ns; e += CL_NT) sums[e] = cl_partials_column(part + b * gx * ns + e, gx, ns);
    __syncthreads();
    if (k >= C + 2) return;
    double g = 0.0, bk = 0.0;
    if (k < C) {
        const double* co = coef + b * (3 * C + 1);
        const double* s = sums + HR_SUMS * k;
        const double su = s[0], sl = s[1], sp = s[2];
        const double num = rule == LG_MTFHR_FS ? s[3] - su * sp / N : s[5] - su * sl / N;
        const double den = rule == LG_MTFHR_FS ? s[4] - sl * sp / N : s[6] - sl * sl / N;
        g = num / den;
        if (!(den > 0.0 && den - den == 0.0 && g - g == 0.0)) g = 0.0;
        const double mean_l = ((double)pan[b * (long)N] + co[0]) + sl / N;
        if (rule == LG_MTFHR_HPM_R) bk = co[1 + k] - g * mean_l;
    }
    double* o = hc + b * (2 * C + 2);
    double* st = stats ? stats + b * (2 * C + 2) : nullptr;
    if (k < C) {
        o[k] = g;
        o[C + k] = bk;
        if (st) st[k] = g, st[C + k] = bk;
    } else {
        o[C + k] = 0.0;
        if (st) st[C + k] = 0.0;
    }
}

// part [B][gpb][ns + C], ns = hr_gram_ns(C, F): with the vectors [mask, ms_0 - ms_0(0) .. , D_0 ..] the upper triangle over the first C + 1 in row-major order,
// then per plane f the C + 1 sums against D_f (the mask first); then the C minima of the raw bands
__global__ __launch_bounds__(CL_NT) void k_hr_gram(const float* __restrict__ ms, const double* __restrict__ dlow, double* __restrict__ part, int C, int F,
                                                   int h, int w) {
    extern __shared__ double cl_lds[];
    __shared__ int pairs[HR_MAX_NS];
    const int n = C + 1, nv = n + F, ns = hr_gram_ns(C, F), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, gpb = gridDim.x;
    double* V = cl_lds;                          // [nv][256]
    double* acc = V + nv * HR_CHUNK;             // [ns]
    double* mins = acc + ns;                     // [C][4]
    const long b = blockIdx.y, lp = (long)h * w;
    const float* __restrict__ ms_b = ms + b * C * lp;
    const double* __restrict__ dl_b = dlow + b * F * lp;
    if (tid == 0) {
        int e = 0;
        for (int a = 0; a < n; ++a)
            for (int c = a; c < n; ++c) pairs[e++] = cl_pair(a, c, 0);
        for (int f = 0; f < F; ++f)
            for (int j = 0; j < n; ++j) pairs[e++] = cl_pair(j, n + f, 0);
    }
    for (int e = tid; e < ns; e += CL_NT) acc[e] = 0.0;
    for (int e = tid; e < 4 * C; e += CL_NT) mins[e] = INFINITY;
    __syncthreads();
    for (long c0 = (long)blockIdx.x * HR_CHUNK; c0 < lp; c0 += (long)gpb * HR_CHUNK) {
        const long o = c0 + tid;
        const int live = lp - c0 < HR_CHUNK ? (int)(lp - c0) : HR_CHUNK;
        const bool in = o < lp;
        V[tid] = in ? 1.0 : 0.0;
        for (int k = 0; k < C; ++k) {
            const float x = in ? ms_b[k * lp + o] : INFINITY;
            V[(1 + k) * HR_CHUNK + tid] = in ? (double)x - (double)ms_b[k * lp] : 0.0;
            float mn = x;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mn = fminf(mn, __shfl_xor(mn, off));
            if (lane == 0) mins[4 * k + wave] = fmin(mins[4 * k + wave], (double)mn);
        }
        for (int f = 0; f < F; ++f) V[(n + f) * HR_CHUNK + tid] = in ? dl_b[f * lp + o] : 0.0;
        __syncthreads();
        cl_pair_sums(pairs, ns, acc, [&](int a, int c, int, int ln) { return cl_lane_dot(V + a * HR_CHUNK, V + c * HR_CHUNK, ln, live); });
        __syncthreads();      // the next chunk overwrites the vectors
    }
    double* pb = part + (b * gpb + blockIdx.x) * (ns + C);
    for (int e = tid; e < ns; e += CL_NT) pb[e] = acc[e];
    for (int k = tid; k < C; k += CL_NT) pb[ns + k] = fmin(fmin(mins[4 * k], mins[4 * k + 1]), fmin(mins[4 * k + 2], mins[4 * k + 3]));
}

// hc (and stats, unless NULL) [B][2 C + 2].  hpm_h: H_k, then H_P,k (F = 1: one value for every band), two zeros.  bt_h: H_k, the slopes w_k, w_0, H_I.
__global__ __launch_bounds__(HR_SOLVE_NT) void k_hr_solve(const double* __restrict__ part, const float* __restrict__ ms, const float* __restrict__ pan,
                                                          double* __restrict__ hc, double* __restrict__ stats, int C, int F, int gpb, long lp, int rule) {
    __shared__ double sums[HR_MAX_NS];
    __shared__ double Lm[CL_MAX_C * CL_MAX_C], sl[CL_MAX_C * CL_MAX_C], H[CL_MAX_C], mm[CL_MAX_C], hp[CL_MAX_C], w0[CL_MAX_C];
    __shared__ int bad_pivot;
    const int n = C + 1, ng = n * (n + 1) / 2, ns = hr_gram_ns(C, F), stride = ns + C, tid = threadIdx.x;
    const long b = blockIdx.x;
    const double nl = (double)lp;
    const double* pb = part + b * gpb * stride;
    for (int e = tid; e < ns; e += HR_SOLVE_NT) sums[e] = cl_partials_column(pb + e, gpb, stride);
    if (tid < C) {
        double m = INFINITY;
        for (int j = 0; j < gpb; ++j) m = fmin(m, pb[(long)j * stride + ns + tid]);
        H[tid] = m;
    }
    if (tid == 0) bad_pivot = 0;
    __syncthreads();
    auto S = [&](int a, int c) { return sums[a * n - a * (a - 1) / 2 + (c - a)]; };      // a <= c, both among the mask and the bands
    if (tid < C) mm[tid] = (double)ms[(b * C + tid) * lp] + S(0, 1 + tid) / nl;
    if (tid == 0) {
        // the centred Gram matrix of ms, the lower triangle in Lm
        for (int k = 0; k < C; ++k)
            for (int l = 0; l <= k; ++l) Lm[k * C + l] = S(1 + l, 1 + k) - S(0, 1 + k) * S(0, 1 + l) / nl;
        if (!cl_cholesky(Lm, C, C, [&](int i, int j) { return Lm[i * C + j]; }, [](double d, double) { return !(d > 0.0); })) bad_pivot = 1;
    }
    __syncthreads();
    if (tid < F) {
        const double* r = sums + ng + tid * n;   // sum D_f, then sum (ms_j - pivot_j) D_f
        double* x = sl + tid * C;
        bool ok = !bad_pivot;
        if (ok) {
            for (int i = 0; i < C; ++i) x[i] = r[1 + i] - S(0, 1 + i) * r[0] / nl;
            cl_chol_solve(Lm, C, C, x, x, [&](double xi) { ok = ok && xi - xi == 0.0; });
        }
        if (!ok)
            for (int i = 0; i < C; ++i) x[i] = 0.0;
        const double mean_d = (double)pan[b * 16 * lp] + r[0] / nl;
        double a = mean_d, c = mean_d;
        for (int j = 0; j < C; ++j) {
            a = fma(x[j], H[j] - mm[j], a);
            c = fma(-x[j], mm[j], c);
        }
        hp[tid] = a;
        w0[tid] = c;
    }
    __syncthreads();
    double* o = hc + b * (2 * C + 2);
    double* st = stats ? stats + b * (2 * C + 2) : nullptr;
    for (int i = tid; i < 2 * C + 2; i += HR_SOLVE_NT) {
        double v;
        if (i < C) {
            v = H[i];
        } else if (rule == LG_MTFHR_HPM_H) {
            v = i < 2 * C ? hp[F == 1 ? 0 : i - C] : 0.0;
        } else if (i < 2 * C) {
            v = sl[i - C];
        } else if (i == 2 * C) {
            v = w0[0];
        } else {
            v = w0[0];
            for (int k = 0; k < C; ++k) v = fma(sl[k], H[k], v);
        }
        o[i] = v;
        if (st) st[i] = v;
    }
}

template <int RULE>
__global__ __launch_bounds__(CL_NT) void k_hr_apply(const float* __restrict__ ms, const float* __restrict__ pan, const double* __restrict__ dlow,
                                                    float* __restrict__ out, const double* __restrict__ hc, int C, int F, int h, int w, int tiles_x) {
    extern __shared__ double cl_lds[];
    double* U = cl_lds + CL_SCRATCH;
    const int tid = threadIdx.x, H4 = 4 * h, W4 = 4 * w;
    const auto [Y0, X0] = cl_tile(blockIdx.x, tiles_x);
    const long b = blockIdx.y, lp = (long)h * w, plane = (long)H4 * W4;
    const float* __restrict__ ms_b = ms + b * C * lp;
    const float* __restrict__ pan_b = pan + b * plane;
    float* __restrict__ out_b = out + b * C * plane;
    const double* __restrict__ co = hc + b * (2 * C + 2);
    const int p = 2 * tid, y = Y0 + p / CL_TW, x = X0 + p % CL_TW;
    const bool in = y < H4 && x < W4;            // W4 is a multiple of 4 and x is even: both pixels or none
    const long o = (long)y * W4 + x;
    float2 pp = make_float2(0.f, 0.f);
    if (in) pp = *reinterpret_cast<const float2*>(pan_b + o);
    const double p0 = (double)pp.x, p1 = (double)pp.y;
    if constexpr (RULE == LG_MTFHR_BT_H) {
        cl_up_bands(ms_b, lp, C, h, w, Y0, X0, cl_lds, U);
        __syncthreads();
        if (!in) return;
        double s0 = 0.0, s1 = 0.0;                // I - H_I = sum_k w_k (u_k - H_k)
        for (int k = 0; k < C; ++k) {
            const double wk = co[C + k], H = co[k];
            s0 = fma(wk, U[k * CL_PX + p] - H, s0);
            s1 = fma(wk, U[k * CL_PX + p + 1] - H, s1);
        }
        const double hi = co[2 * C + 1], r0 = hr_ratio(p0 - hi, s0), r1 = hr_ratio(p1 - hi, s1);
        for (int k = 0; k < C; ++k) {
            const double H = co[k];
            *reinterpret_cast<float2*>(out_b + k * plane + o) =
                make_float2(cl_clip(fma(U[k * CL_PX + p] - H, r0, H)), cl_clip(fma(U[k * CL_PX + p + 1] - H, r1, H)));
        }
    } else {
        double* Lt = U + CL_PX;
        const double* __restrict__ dl_b = dlow + b * F * lp;
        const double pv = (double)pan_b[0];
        float v[CL_MLOADS], vn[CL_MLOADS] = {};
        double q[CL_MLOADS], qn[CL_MLOADS] = {};
        cl_ms_load(ms_b, h, w, {Y0, X0}, v);
        hr_d_load(dl_b, h, w, {Y0, X0}, q);
        for (int k = 0; k < C; ++k) {
            if (k + 1 < C) {
                cl_ms_load(ms_b + (k + 1) * lp, h, w, {Y0, X0}, vn);
                hr_d_load(dl_b + (F == 1 ? 0 : k + 1) * lp, h, w, {Y0, X0}, qn);
            }
            cl_up_band(v, cl_lds, U);
            cl_up_band(q, cl_lds, Lt);
            __syncthreads();
            if (in) {
                const double c0 = co[k], c1 = co[C + k];      // fs: g; hpm_r: g, b; hpm_h: H, H_P
                const double u0 = U[p], u1 = U[p + 1], l0 = Lt[p] + pv, l1 = Lt[p + 1] + pv;
                double o0, o1;
                if (RULE == LG_MTFHR_FS) {
                    o0 = fma(c0, p0 - l0, u0);
                    o1 = fma(c0, p1 - l1, u1);
                } else if (RULE == LG_MTFHR_HPM_R) {
                    o0 = u0 * hr_ratio(fma(c0, p0, c1), fma(c0, l0, c1));
                    o1 = u1 * hr_ratio(fma(c0, p1, c1), fma(c0, l1, c1));
                } else {
                    o0 = fma(u0 - c0, hr_ratio(p0 - c1, l0 - c1), c0);
                    o1 = fma(u1 - c0, hr_ratio(p1 - c1, l1 - c1), c0);
                }
                *reinterpret_cast<float2*>(out_b + k * plane + o) = make_float2(cl_clip(o0), cl_clip(o1));
            }
            cl_next(v, vn);
            cl_next(q, qn);
            // no barrier: the next cl_up_band writes U and Lt in its last pass, four barriers from here
        }
    }
}

struct HrGeom {
    ClGeom cl;                 // SFIM's: the tiles and the first moments pass (fs, hpm_r)
    int gx2;                   // workgroups per sample of k_hr_moments (fs, hpm_r) or of k_hr_gram (hpm_h, bt_h)
    size_t off[5], bytes;      // part, coef (fs, hpm_r), D, part2, hc
};

bool hr_geom(const char* who, int B, int C, int h, int w, int n_filters, int rule, HrGeom& g) {
    if (rule != LG_MTFHR_FS && rule != LG_MTFHR_HPM_R && rule != LG_MTFHR_HPM_H && rule != LG_MTFHR_BT_H) {
        lg_set_error("%s: rule must be LG_MTFHR_FS, LG_MTFHR_HPM_R, LG_MTFHR_HPM_H or LG_MTFHR_BT_H (got %d)", who, rule);
        return false;
    }
    if (!cl_geom(who, B, C, h, w, LG_CLASSICAL_SFIM, g.cl)) return false;
    if (!mg_filters_ok(who, C, n_filters)) return false;
    if (rule == LG_MTFHR_BT_H && n_filters != 1) { lg_set_error("%s: n_filters must be 1 for LG_MTFHR_BT_H (got %d)", who, n_filters); return false; }
    const bool haze = hr_haze(rule);
    if (haze) {
        const long chunks = ((long)h * w + HR_CHUNK - 1) / HR_CHUNK;
        g.gx2 = chunks < HR_GRAM_WGS ? (int)chunks : HR_GRAM_WGS;
    } else {
        g.gx2 = g.cl.tiles < MG_RESIDENT ? g.cl.tiles : MG_RESIDENT;
    }
    const size_t per2 = haze ? (size_t)g.gx2 * (hr_gram_ns(C, n_filters) + C) : (size_t)g.gx2 * HR_SUMS * C;
    const size_t sz[5] = {haze ? 0 : ws_region(B, (size_t)g.cl.gx * g.cl.ns * sizeof(double)), haze ? 0 : ws_region(B, (size_t)(3 * C + 1) * sizeof(double)),
                          ws_region(B, (size_t)n_filters * h * w * sizeof(double)), ws_region(B, per2 * sizeof(double)),
                          ws_region(B, (size_t)(2 * C + 2) * sizeof(double))};
    g.bytes = ws_layout(5, sz, g.off);
    return true;
}

DeviceOnce hr_attr_once;
int hr_lds_attr(const char* who) {
    if (!hr_attr_once.need()) return 0;
    if (int rc = lds_attr_set(who, hr_moments_lds_doubles(CL_MAX_C) * (int)sizeof(double), k_hr_moments)) return rc;
    if (int rc = lds_attr_set(who, hr_gram_lds_doubles(CL_MAX_C, CL_MAX_C) * (int)sizeof(double), k_hr_gram)) return rc;
    if (int rc = lds_attr_set(who, hr_apply_lds_doubles(CL_MAX_C, LG_MTFHR_BT_H) * (int)sizeof(double), k_hr_apply<LG_MTFHR_BT_H>)) return rc;
    hr_attr_once.done();
    return 0;
}

int hr_fuse(const char* who, const lg_mtf_hr_args* a) {
    if (!a) { lg_set_error("%s: args is NULL", who); return -1; }
    if (a->struct_bytes != sizeof(lg_mtf_hr_args)) {
        lg_set_error("%s: struct_bytes must be sizeof(lg_mtf_hr_args) = %zu (got %u)", who, sizeof(lg_mtf_hr_args), a->struct_bytes);
        return -1;
    }
    const int B = a->B, C = a->C, h = a->h, w = a->w, F = a->n_filters, rule = a->rule;
    HrGeom g;
    if (!hr_geom(who, B, C, h, w, F, rule, g)) return -1;
    if (!mg_taps_ok(who, a->n_taps)) return -1;
    if (!cl_check_args(who, a->ms, a->pan, a->out, {{"taps", a->taps}}, a->stats, a->workspace, a->workspace_bytes, g.bytes, "lg_mtf_hr_workspace_bytes"))
        return -1;
    if (int rc = cl_lds_attr(who)) return rc;
    if (int rc = hr_lds_attr(who)) return rc;
    hipStream_t s = (hipStream_t)a->stream;
    double *part = cl_ws(a->workspace, g.off[0]), *coef = cl_ws(a->workspace, g.off[1]), *dlow = cl_ws(a->workspace, g.off[2]);
    double *part2 = cl_ws(a->workspace, g.off[3]), *hc = cl_ws(a->workspace, g.off[4]);
    const int tiles_x = g.cl.tiles_x, tiles = g.cl.tiles;
    const double N = 16.0 * h * w;
    const int lt_x = (w + MG_TO - 1) / MG_TO, lt = lt_x * ((h + MG_TO - 1) / MG_TO);
    const size_t lds = hr_apply_lds_doubles(C, rule) * sizeof(double);
    if (hr_haze(rule)) {
        k_mg_lowpass<<<dim3(lt, F, B), CL_NT, 0, s>>>(a->pan, a->taps, dlow, h, w, a->n_taps, lt_x);
        LG_CHECK_LAUNCH();
        k_hr_gram<<<dim3(g.gx2, B), CL_NT, hr_gram_lds_doubles(C, F) * sizeof(double), s>>>(a->ms, dlow, part2, C, F, h, w);
        LG_CHECK_LAUNCH();
        k_hr_solve<<<B, HR_SOLVE_NT, 0, s>>>(part2, a->ms, a->pan, hc, a->stats, C, F, g.gx2, (long)h * w, rule);
        LG_CHECK_LAUNCH();
        if (rule == LG_MTFHR_BT_H)
            k_hr_apply<LG_MTFHR_BT_H><<<dim3(tiles, B), CL_NT, lds, s>>>(a->ms, a->pan, dlow, a->out, hc, C, F, h, w, tiles_x);
        else
            k_hr_apply<LG_MTFHR_HPM_H><<<dim3(tiles, B), CL_NT, lds, s>>>(a->ms, a->pan, dlow, a->out, hc, C, F, h, w, tiles_x);
    } else {
        k_cl_moments<<<dim3(g.cl.gx, B), CL_NT, cl_moment_lds_doubles(C) * sizeof(double), s>>>(a->ms, a->pan, part, C, h, w, tiles_x, tiles, 0);
        LG_CHECK_LAUNCH();
        k_cl_finish<<<B, CL_NT, 0, s>>>(part, coef, nullptr, C, g.cl.gx, N, (double)h * w, 0);
        LG_CHECK_LAUNCH();
        k_mg_lowpass<<<dim3(lt, F, B), CL_NT, 0, s>>>(a->pan, a->taps, dlow, h, w, a->n_taps, lt_x);
        LG_CHECK_LAUNCH();
        k_hr_moments<<<dim3(g.gx2, B), CL_NT, hr_moments_lds_doubles(C) * sizeof(double), s>>>(a->ms, a->pan, dlow, coef, part2, C, F, h, w, tiles_x, tiles);
        LG_CHECK_LAUNCH();
        k_hr_finish<<<B, CL_NT, 0, s>>>(part2, a->pan, coef, hc, a->stats, C, g.gx2, N, rule);
        LG_CHECK_LAUNCH();
        if (rule == LG_MTFHR_FS)
            k_hr_apply<LG_MTFHR_FS><<<dim3(tiles, B), CL_NT, lds, s>>>(a->ms, a->pan, dlow, a->out, hc, C, F, h, w, tiles_x);
        else
            k_hr_apply<LG_MTFHR_HPM_R><<<dim3(tiles, B), CL_NT, lds, s>>>(a->ms, a->pan, dlow, a->out, hc, C, F, h, w, tiles_x);
    }
    LG_CHECK_LAUNCH();
    return 0;
}

// ---- BDSD: the band-dependent spatial detail method, global or per block of block x block PAN pixels.  Per block and band the weights gamma
// are the least-squares fit of ms_k - A_k on x = [A_1 .. A_C, D] at the MS scale (A_k: the band low-passed on its own grid, D: the raw PAN low-passed at the
// decimated positions, k_mg_lowpass's plane plus the pivot); out_k = clip(u_k + sum_j gamma_kj u_j + gamma_kC pan).
//   k_bd_lowpass_ms  grid (tile, band, sample): A_k on 16 x 16 tiles of the MS grid, replicate border -- rows into LDS, then columns; fp64 [B, C, h, w].  It is
//                    k_mg_lowpass on the band's own grid without the pivot, and stays a kernel of its own: as two instances of one template the pair cost a
//                    call of lg_bdsd 0.5 us at PAN 128 x 128 (HISTORY.md).
//   k_bd_gram        grid (block x workgroup of the block, sample): a workgroup walks the block's pixels (row-major inside the block) in chunks of 256, gpb
//                    chunks apart: the 2 C + 1 vectors [x, y] of the chunk in LDS, zero past the block's end; every entry of G = sum x x' (upper triangle) and
//                    of r_k = sum x y_k is the sum of a product of two of them, summed over the chunk in k_cl_moments's order (cl_pair_sums).  The workgroup
//                    writes its slots.
//   k_bd_solve       one wave per block: the partials in ascending order (cl_partials_column), one thread's Cholesky of G (cl_cholesky), then thread k solves
//                    for gamma_k (cl_chol_solve).  A pivot at or below 1e-12 G_jj or not finite, or a weight that is not finite, gives the block gamma = 0: its
//                    output is clip(u) bit for bit.
//   k_bd_apply       grid (tile, sample), k_cl_apply's structure: the C bands of the tile (cl_up_bands) and the weights of the tile's block in LDS (block edges
//                    are multiples of 32: a tile lies in one block), two adjacent pixels per thread, ONE rounding, 8-byte stores.
// Neither u nor A is stored at PAN size.  The geometry of a sample depends on C, h, w and block only.
constexpr int BD_CHUNK = CL_NT;                                          // MS pixels of a block a Gram workgroup takes at a time: one per thread
constexpr int BD_MAX_N = CL_MAX_C + 1;                                   // regressors, at most
constexpr int BD_MAX_NS = BD_MAX_N * (BD_MAX_N + 1) / 2 + CL_MAX_C * BD_MAX_N;      // entries of G and of the C right-hand sides
constexpr int BD_GRAM_WGS = 128;                                         // Gram workgroups per sample, at most, where blocks are larger than a chunk
constexpr int BD_SOLVE_NT = 64;
constexpr double BD_PIVOT_TOL = 1e-12;
static_assert(BD_SOLVE_NT >= CL_MAX_C, "a thread per band solves");

__host__ __device__ inline int bd_ns(int C) { return (C + 1) * (C + 2) / 2 + C * (C + 1); }
__host__ __device__ inline int bd_gram_lds_doubles(int C) { return (2 * C + 1) * BD_CHUNK + bd_ns(C); }
__host__ __device__ inline int bd_apply_lds_doubles(int C) { return CL_SCRATCH + C * CL_PX + C * (C + 1); }

__global__ __launch_bounds__(CL_NT) void k_bd_lowpass_ms(const float* __restrict__ ms, const double* __restrict__ taps, double* __restrict__ alow, int F, int h,
                                                         int w, int n_taps, int tiles_x) {
    __shared__ double tp[MG_MAX_TAPS];
    __shared__ double rowf[MG_TO + MG_MAX_TAPS - 1][MG_TO + 1];
    const int r = n_taps >> 1, tid = threadIdx.x;
    const int oy0 = (blockIdx.x / tiles_x) * MG_TO, ox0 = (blockIdx.x % tiles_x) * MG_TO;
    const long plane = (long)blockIdx.z * gridDim.y + blockIdx.y;
    const float* __restrict__ ms_k = ms + plane * ((long)h * w);
    if (tid < n_taps) tp[tid] = taps[(F == 1 ? 0 : blockIdx.y) * n_taps + tid];
    __syncthreads();
    // row pass: slot s is ms row oy0 - r + s (clamped into the plane), column j the tile's j-th column
    const int rows = oy0 + MG_TO <= h ? MG_TO : h - oy0, span = rows + n_taps - 1;
    for (int t = tid; t < span * MG_TO; t += CL_NT) {
        const int s = t / MG_TO, j = t - s * MG_TO;
        if (ox0 + j >= w) continue;
        const float* __restrict__ row = ms_k + (long)mg_clamp(oy0 - r + s, h) * w;
        const int xb = ox0 + j - r;
        double acc = 0.0;
        for (int k = 0; k < n_taps; ++k) acc = fma(tp[k], (double)row[mg_clamp(xb + k, w)], acc);
        rowf[s][j] = acc;
    }
    __syncthreads();
    const int ly = tid / MG_TO, lx = tid - ly * MG_TO;
    if (ly >= rows || ox0 + lx >= w) return;
    double acc = 0.0;
    for (int k = 0; k < n_taps; ++k) acc = fma(tp[k], rowf[ly + k][lx], acc);
    alow[plane * ((long)h * w) + (long)(oy0 + ly) * w + ox0 + lx] = acc;
}

// part [B][nblocks][gpb][ns]: the upper triangle of G in row-major order (a <= c < C + 1), then r_k[j] at (C + 1)(C + 2) / 2 + k (C + 1) + j.  A block is bh x bw
// MS pixels (the whole sample in the global form), nbx blocks in a row of blocks.
__global__ __launch_bounds__(CL_NT) void k_bd_gram(const float* __restrict__ ms, const float* __restrict__ pan, const double* __restrict__ alow,
                                                   const double* __restrict__ dlow, double* __restrict__ part, int C, int h, int w, int bh, int bw, int nbx,
                                                   int gpb) {
    extern __shared__ double cl_lds[];
    __shared__ int pairs[BD_MAX_NS];
    const int n = C + 1, nv = 2 * C + 1, ns = bd_ns(C), tid = threadIdx.x;
    double* V = cl_lds;                          // [nv][256]: A_0 .. A_C-1, D, y_0 .. y_C-1
    double* acc = V + nv * BD_CHUNK;             // [ns]
    const int blk = blockIdx.x / gpb, g = blockIdx.x - blk * gpb;
    const int i0 = (blk / nbx) * bh, j0 = (blk % nbx) * bw, npx = bh * bw;
    const long b = blockIdx.y, lp = (long)h * w;
    const float* __restrict__ ms_b = ms + b * C * lp;
    const double* __restrict__ al_b = alow + b * C * lp;
    const double* __restrict__ dl_b = dlow + b * lp;
    const double pv = (double)pan[b * 16 * lp];  // k_mg_lowpass filters PAN minus the sample's first pixel; the taps sum to 1
    if (tid == 0) {
        int e = 0;
        for (int a = 0; a < n; ++a)
            for (int c = a; c < n; ++c) pairs[e++] = cl_pair(a, c, 0);
        for (int k = 0; k < C; ++k)
            for (int j = 0; j < n; ++j) pairs[e++] = cl_pair(j, n + k, 0);
    }
    for (int e = tid; e < ns; e += CL_NT) acc[e] = 0.0;
    for (int c0 = g * BD_CHUNK; c0 < npx; c0 += gpb * BD_CHUNK) {
        const int q = c0 + tid, live = npx - c0 < BD_CHUNK ? npx - c0 : BD_CHUNK;
        if (q < npx) {
            const int ii = q / bw, jj = q - ii * bw;
            const long o = (long)(i0 + ii) * w + j0 + jj;
            for (int k = 0; k < C; ++k) {
                const double a = al_b[k * lp + o];
                V[k * BD_CHUNK + tid] = a;
                V[(n + k) * BD_CHUNK + tid] = (double)ms_b[k * lp + o] - a;
            }
            V[C * BD_CHUNK + tid] = dl_b[o] + pv;
        } else {
            for (int v = 0; v < nv; ++v) V[v * BD_CHUNK + tid] = 0.0;
        }
        __syncthreads();
        cl_pair_sums(pairs, ns, acc, [&](int a, int c, int, int lane) { return cl_lane_dot(V + a * BD_CHUNK, V + c * BD_CHUNK, lane, live); });
        __syncthreads();      // the next chunk overwrites the vectors
    }
    for (int e = tid; e < ns; e += CL_NT) part[(b * gridDim.x + blockIdx.x) * ns + e] = acc[e];
}

// gamma [B][nblocks][C][C + 1] (stats: NULL or the same layout): per block G gamma_k = r_k by Cholesky, the lower triangle in Lm
__global__ __launch_bounds__(BD_SOLVE_NT) void k_bd_solve(const double* __restrict__ part, double* __restrict__ gamma, double* __restrict__ stats, int C,
                                                          int gpb) {
    __shared__ double sums[BD_MAX_NS];
    __shared__ double Lm[BD_MAX_N * BD_MAX_N], gam[CL_MAX_C * BD_MAX_N];
    __shared__ int bad_pivot, bad_weight;
    const int n = C + 1, ng = n * (n + 1) / 2, ns = bd_ns(C), tid = threadIdx.x;
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    for (int e = tid; e < ns; e += BD_SOLVE_NT) sums[e] = cl_partials_column(part + blk * gpb * ns + e, gpb, ns);
    if (tid == 0) bad_pivot = bad_weight = 0;
    __syncthreads();
    auto G = [&](int i, int j) { return sums[j * n - j * (j - 1) / 2 + (i - j)]; };      // i >= j: the upper triangle, row-major, holds (j, i)
    if (tid == 0 && !cl_cholesky(Lm, n, n, G, [](double d, double gjj) { return !(d > BD_PIVOT_TOL * gjj) || d - d != 0.0; })) bad_pivot = 1;
    __syncthreads();
    if (!bad_pivot && tid < C) {
        double* x = gam + tid * n;
        bool ok = true;
        cl_chol_solve(Lm, n, n, sums + ng + tid * n, x, [&](double xi) { ok = ok && xi - xi == 0.0; });
        if (!ok) bad_weight = 1;
    }
    __syncthreads();
    const bool ok = !bad_pivot && !bad_weight;
    for (int i = tid; i < C * n; i += BD_SOLVE_NT) {
        const double v = ok ? gam[i] : 0.0;
        gamma[blk * (C * n) + i] = v;
        if (stats) stats[blk * (C * n) + i] = v;
    }
}

__global__ __launch_bounds__(CL_NT) void k_bd_apply(const float* __restrict__ ms, const float* __restrict__ pan, const double* __restrict__ gamma,
                                                    float* __restrict__ out, int C, int h, int w, int tiles_x, int block, int nbx, int nblocks) {
    extern __shared__ double cl_lds[];
    double* U = cl_lds + CL_SCRATCH;             // [C][512]
    double* Gm = U + C * CL_PX;                  // [C][C + 1]: the weights of the tile's block
    const int tid = threadIdx.x, H4 = 4 * h, W4 = 4 * w, n = C + 1;
    const auto [Y0, X0] = cl_tile(blockIdx.x, tiles_x);
    const long b = blockIdx.y, lp = (long)h * w, plane = (long)H4 * W4;
    const float* __restrict__ pan_b = pan + b * plane;
    float* __restrict__ out_b = out + b * C * plane;
    const int blk = block ? (Y0 / block) * nbx + X0 / block : 0;
    const double* __restrict__ gm = gamma + (b * nblocks + blk) * (C * n);
    for (int i = tid; i < C * n; i += CL_NT) Gm[i] = gm[i];      // (the barriers inside cl_up_band order this before its use)
    const int p = 2 * tid, y = Y0 + p / CL_TW, x = X0 + p % CL_TW;
    const bool in = y < H4 && x < W4;            // W4 is a multiple of 4 and x is even: both pixels or none
    const long o = (long)y * W4 + x;
    float2 pp = make_float2(0.f, 0.f);
    if (in) pp = *reinterpret_cast<const float2*>(pan_b + o);
    cl_up_bands(ms + b * C * lp, lp, C, h, w, Y0, X0, cl_lds, U);
    __syncthreads();
    if (!in) return;
    const double p0 = (double)pp.x, p1 = (double)pp.y;
    for (int k = 0; k < C; ++k) {
        const double* g = Gm + k * n;
        double s0 = g[C] * p0, s1 = g[C] * p1;
        for (int j = 0; j < C; ++j) {
            s0 = fma(g[j], U[j * CL_PX + p], s0);
            s1 = fma(g[j], U[j * CL_PX + p + 1], s1);
        }
        *reinterpret_cast<float2*>(out_b + k * plane + o) = make_float2(cl_clip(U[k * CL_PX + p] + s0), cl_clip(U[k * CL_PX + p + 1] + s1));
    }
}

struct BdGeom {
    int tiles_x, tiles, bh, bw, nbx, nblocks, gpb;
    size_t off[4], bytes;      // D, A, part, gamma
};

// false: not a shape or a block the call takes (the reason, naming the argument, is in lg_last_error)
bool bd_geom(const char* who, int B, int C, int h, int w, int block, BdGeom& g) {
    if (!cl_shape(who, B, C, h, w)) return false;
    if (block == 0) {
        if ((long)h * w < 2 * (C + 1)) { lg_set_error("%s: the global form needs h * w >= 2 (C + 1) = %d (got %d x %d)", who, 2 * (C + 1), h, w); return false; }
        g.bh = h;
        g.bw = w;
    } else {
        if (block < 32 || block % 32) { lg_set_error("%s: block must be 0 (global) or a multiple of 32 (got %d)", who, block); return false; }
        if ((4 * h) % block || (4 * w) % block) { lg_set_error("%s: block must divide 4 h = %d and 4 w = %d (got %d)", who, 4 * h, 4 * w, block); return false; }
        g.bh = g.bw = block / 4;
    }
    g.tiles = cl_tiles(h, w, g.tiles_x);
    g.nbx = w / g.bw;
    g.nblocks = g.nbx * (h / g.bh);
    const int chunks = (g.bh * g.bw + BD_CHUNK - 1) / BD_CHUNK, cap = BD_GRAM_WGS / g.nblocks > 1 ? BD_GRAM_WGS / g.nblocks : 1;
    g.gpb = chunks < cap ? chunks : cap;
    const size_t lp = (size_t)h * w * sizeof(double), nb = (size_t)B * g.nblocks * sizeof(double);
    const size_t sz[4] = {B * lp, (size_t)B * C * lp, nb * g.gpb * bd_ns(C), nb * C * (C + 1)};
    g.bytes = ws_layout(4, sz, g.off);
    return true;
}

DeviceOnce bd_attr_once;
int bd_lds_attr(const char* who) {
    if (!bd_attr_once.need()) return 0;
    if (int rc = lds_attr_set(who, bd_gram_lds_doubles(CL_MAX_C) * (int)sizeof(double), k_bd_gram)) return rc;
    if (int rc = lds_attr_set(who, bd_apply_lds_doubles(CL_MAX_C) * (int)sizeof(double), k_bd_apply)) return rc;
    bd_attr_once.done();
    return 0;
}

int bd_fuse(const char* who, const float* ms, const float* pan, float* out, double* stats, const double* taps_ms, int n_filters, const double* taps_pan,
            int n_taps, int block, int B, int C, int h, int w, void* workspace, size_t workspace_bytes, hipStream_t s) {
    BdGeom g;
    if (!bd_geom(who, B, C, h, w, block, g)) return -1;
    if (!mg_filters_ok(who, C, n_filters) || !mg_taps_ok(who, n_taps)) return -1;
    if (!cl_check_args(who, ms, pan, out, {{"taps_ms", taps_ms}, {"taps_pan", taps_pan}}, stats, workspace, workspace_bytes, g.bytes, "lg_bdsd_workspace_bytes"))
        return -1;
    if (int rc = bd_lds_attr(who)) return rc;
    double *dlow = cl_ws(workspace, g.off[0]), *alow = cl_ws(workspace, g.off[1]), *part = cl_ws(workspace, g.off[2]), *gamma = cl_ws(workspace, g.off[3]);
    const int lt_x = (w + MG_TO - 1) / MG_TO, lt = lt_x * ((h + MG_TO - 1) / MG_TO);
    k_mg_lowpass<<<dim3(lt, 1, B), CL_NT, 0, s>>>(pan, taps_pan, dlow, h, w, n_taps, lt_x);
    LG_CHECK_LAUNCH();
    k_bd_lowpass_ms<<<dim3(lt, C, B), CL_NT, 0, s>>>(ms, taps_ms, alow, n_filters, h, w, n_taps, lt_x);
    LG_CHECK_LAUNCH();
    k_bd_gram<<<dim3(g.nblocks * g.gpb, B), CL_NT, bd_gram_lds_doubles(C) * sizeof(double), s>>>(ms, pan, alow, dlow, part, C, h, w, g.bh, g.bw, g.nbx, g.gpb);
    LG_CHECK_LAUNCH();
    k_bd_solve<<<dim3(g.nblocks, B), BD_SOLVE_NT, 0, s>>>(part, gamma, stats, C, g.gpb);
    LG_CHECK_LAUNCH();
    k_bd_apply<<<dim3(g.tiles, B), CL_NT, bd_apply_lds_doubles(C) * sizeof(double), s>>>(ms, pan, gamma, out, C, h, w, g.tiles_x, block, g.nbx, g.nblocks);
    LG_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t lg_bdsd_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t block) {
    BdGeom g;
    return bd_geom("bdsd_workspace_bytes", B, C, h, w, block, g) ? g.bytes : 0;
}

extern "C" int lg_bdsd(const float* ms, const float* pan, float* out, double* stats, const double* taps_ms, int32_t n_filters, const double* taps_pan,
                       int32_t n_taps, int32_t block, int32_t B, int32_t C, int32_t h, int32_t w, void* workspace, size_t workspace_bytes, void* stream) {
    return bd_fuse("bdsd", ms, pan, out, stats, taps_ms, n_filters, taps_pan, n_taps, block, B, C, h, w, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t lg_mtfglp_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t n_filters, int32_t mode) {
    MgGeom g;
    return mg_geom("mtfglp_workspace_bytes", B, C, h, w, n_filters, mode, g) ? g.bytes : 0;
}

extern "C" int lg_mtf_glp(const float* ms, const float* pan, float* out, double* stats, const double* taps, int32_t n_filters, int32_t n_taps, int32_t mode,
                          int32_t B, int32_t C, int32_t h, int32_t w, void* workspace, size_t workspace_bytes, void* stream) {
    return mg_fuse("mtf_glp", ms, pan, out, stats, taps, n_filters, n_taps, mode, B, C, h, w, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t lg_atrous_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t match) {
    AtGeom g;
    return at_geom("atrous_workspace_bytes", B, C, h, w, match, g) ? g.bytes : 0;
}

extern "C" int lg_atrous(const lg_atrous_args* args) { return at_fuse("atrous", args); }

extern "C" size_t lg_mtf_hr_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t n_filters, int32_t rule) {
    HrGeom g;
    return hr_geom("mtf_hr_workspace_bytes", B, C, h, w, n_filters, rule, g) ? g.bytes : 0;
}

extern "C" int lg_mtf_hr(const lg_mtf_hr_args* args) { return hr_fuse("mtf_hr", args); }

extern "C" int lg_atrous_taps(double* out13) {
    if (!out13) { lg_set_error("atrous_taps: out13 is NULL"); return -1; }
    constexpr AtTaps T = at_taps();
    for (int a = 0; a < AT_TAPS; ++a) out13[a] = T.t[a];
    return 0;
}

extern "C" size_t lg_classical_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t method) {
    ClGeom g;
    return cl_geom("classical_workspace_bytes", B, C, h, w, method, g) ? g.bytes : 0;
}

extern "C" int lg_interp23_up4(const float* ms, float* out, int32_t B, int32_t C, int32_t h, int32_t w, void* stream) {
    static const char* who = "interp23_up4";
    ClGeom g;
    if (!cl_geom(who, B, C, h, w, LG_CLASSICAL_SFIM, g)) return -1;
    if (!check_tensors(who, {{"ms", ms}, {"out", out}})) return -1;
    k_cl_interp<<<dim3(g.tiles, C, B), CL_NT, (CL_SCRATCH + CL_PX) * sizeof(double), (hipStream_t)stream>>>(ms, out, h, w, g.tiles_x);
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_sfim(const float* ms, const float* pan, float* out, int32_t B, int32_t C, int32_t h, int32_t w, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return cl_fuse("sfim", LG_CLASSICAL_SFIM, ms, pan, out, nullptr, B, C, h, w, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lg_gsa(const float* ms, const float* pan, float* out, double* stats, int32_t B, int32_t C, int32_t h, int32_t w, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return cl_fuse("gsa", LG_CLASSICAL_GSA, ms, pan, out, stats, B, C, h, w, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lg_wavelet(const float* ms, const float* pan, float* out, int32_t B, int32_t C, int32_t h, int32_t w, void* stream) {
    static const char* who = "wavelet";
    if (!cl_shape(who, B, C, h, w)) return -1;
    if (!check_tensors(who, {{"ms", ms}, {"pan", pan}, {"out", out}})) return -1;
    const int tiles_x = (w + CW_BX - 1) / CW_BX, tiles = tiles_x * ((h + CW_BY - 1) / CW_BY);
    k_cl_wavelet<<<dim3(tiles, B), CL_NT, 0, (hipStream_t)stream>>>(ms, pan, out, C, h, w, tiles_x);
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_wavelet_taps(double* out17) {
    if (!out17) { lg_set_error("wavelet_taps: out17 is NULL"); return -1; }
    constexpr ClWaveletTaps W = cl_wavelet_taps();
    for (int a = 0; a < CW_TAPS; ++a) out17[a] = W.t[a];
    return 0;
}
