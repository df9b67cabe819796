// The component-substitution baselines, whole batches on the device: generalised IHS, Brovey, Gram-Schmidt and PCA (C ABI: lg_cs, include/lgteun_hip.h; the
// definitions are DESIGN.md 3.15, the fp64 numpy restatement the tests compare with is tests/cs_ref.py).  Each method is fixed by the means and the second
// moments of u = interp23(ms) and PAN, C intensity weights w and C gains g.  interp23 is linear and circular, u(y, x) = sum_ij t(y - 4 i - 2) t(x - 4 j - 2)
// ms(i, j) with the 67 taps t of its impulse response, so every moment is formed at the MS scale and u is computed once, in the apply pass:
//   sum_x u_k(x) pan'(x)  = sum_i ms_k(i) q(i),     q(i, j) = sum_yx t(y - 4 i - 2) t(x - 4 j - 2) pan'(y, x)      (the adjoint of interp23 on PAN)
//   sum_x u_k(x) u_l(x)   = sum_i ms_k(i) v_l(i),   v_l = R * ms_l, R(d) = sum_m t(m) t(m - 4 d), d = -16 .. 16      (the Gram operator of interp23)
//   mean u_k              = (sum t)^2 / 16 . mean ms_k
// PAN enters minus its first pixel and every band minus its first sample (ms_k = ms'_k + c_k): a constant PAN or band has EXACTLY zero moments.  The
// pivot of a band comes back in closed form: interp23 of the constant 1 is e(y, x) = p(y mod 4) p(x mod 4), p the sums of the four polyphase parts of t,
// so sum u_k pan' = sum ms'_k q + c_k sum q, and in the centred second moments of u the terms in c_k carry the factor sum R - (sum t)^2 / 4 = 4 var(p)
// ~ 1e-19, below the rounding of fp64: they are left out.
//
//   k_cs_adjoint   grid (tile, sample), 16 x 16 outputs of q per tile: the 127 x 127 PAN pixels under them, minus the pivot, in chunks of 32 rows in LDS (fp64,
//                  row stride 129: the lanes of the row pass run down a column and hit distinct banks); the 67 taps along x at the 16 decimated
//                  positions of every row, then along y; a thread forms four outputs in one pass over the samples they share (cs_fir4).  PAN is read once (plus the halo); the workgroup also sums pan' and pan'^2 over its own 64 x 64
//                  pixels and q over its outputs: three partials per tile.
//   k_cs_gram      grid (gx, sample), gx = min(tiles, 512); a workgroup walks the 16 x 16 tiles of the MS grid gx apart: per band the 48 x 48 samples of ms'
//                  around the tile (modulo h, w), the 33 taps of R along x, then along y -> v_l; then every sum the method needs is the sum of a product of
//                  two of the vectors {ms'_k} x {v_l (l >= k), q, 1} over the tile, summed in k_cl_moments's order (cl_pair_sums, classical_tiles.h).  The
//                  workgroup writes its slots.
//   k_cs_finish    one workgroup per sample: the partials in a fixed order (a wave per sum), then one thread: the centred moments, the method's w (PCA:
//                  a cyclic Jacobi eigen-solve of Sigma in fp64 by the whole workgroup, at most 30 sweeps, until the off-diagonal squares fall below 1e-32 of the
//                  diagonal's), then
//                  a, g and the degenerate flag into coef and, on request, stats.
//   k_cs_apply     grid (tile, sample), k_cl_apply's structure: the C bands of the 16 x 32 output tile by cl_up_bands, I accumulated over the bands, the additive
//                  or the multiplicative rule in fp64 with ONE rounding to fp32; two adjacent pixels per thread: 8-byte stores.
// No atomics; a workgroup sees one sample and the grid of a sample depends on C, h and w only, so a sample has the same bits alone and inside any batch.
// All indexing into tensors is 64-bit.  Nothing is allocated, nothing synchronises.
#include <cmath>

#include "abi.h"
#include "classical_tiles.h"
#include "common.h"
#include "reduce.h"

namespace {

constexpr int CS_TREACH = 33, CS_T = 2 * CS_TREACH + 1;                 // t: offsets -33 .. 33
constexpr int CS_RREACH = 16, CS_R = 2 * CS_RREACH + 1;                 // R: offsets -16 .. 16
constexpr int CS_AT = 16;                                                // adjoint pass: outputs per tile edge
constexpr int CS_ASPAN = 4 * (CS_AT - 1) + CS_T;                        // 127: PAN rows / columns under one tile's outputs
constexpr int CS_ACH = 32, CS_ANCH = (CS_ASPAN + CS_ACH - 1) / CS_ACH;  // rows of a staged chunk, chunks
constexpr int CS_APW = CS_ASPAN + 2;                                     // 129: row stride of the staged chunk, odd
constexpr int CS_ALW = 128;                                              // threads along a staged row: the span rounded up to a power of two
static_assert(CS_ALW >= CS_ASPAN && CL_NT % CS_ALW == 0 && CL_NT / CS_ALW <= 16, "a thread per staged column; the row advance is below the smallest side (16 PAN pixels)");
constexpr int CS_GT = 16, CS_GH = CS_GT + 2 * CS_RREACH, CS_GW = CS_GH + 1;      // Gram pass: the tile, its halo tile 48 x 48, row stride 49
constexpr int CS_GPX = CS_GT * CS_GT;
constexpr int CS_GLR = CL_NT / CS_GH;                                    // 5: halo rows staged per pass (240 of the 256 threads)
static_assert(CS_GLR < 8, "a row index advanced by CS_GLR wraps at most twice (h >= 4)");
constexpr int CS_GRAM_WGS = 512;                                         // Gram workgroups per sample, at most: two per compute unit
constexpr int CS_MAX_NS = CL_MAX_C * (CL_MAX_C + 1) / 2 + 2 * CL_MAX_C;  // entries: ms'_k v_l (k <= l), ms'_k q, ms'_k
constexpr int CS_SWEEPS = 30;
constexpr int CS_COEF = 4;                                               // coef [B][4 + 3 C]: mean of pan', a, m_I, degenerate; m_k; w_k; g_k
static_assert(CS_GPX == CL_NT && CS_AT * CS_AT == CL_NT, "a thread per output of the adjoint tile and per pixel of the Gram tile");
static_assert(CS_ANCH * CS_ACH >= CS_ASPAN, "the chunks cover the span");

__host__ __device__ inline int cs_ns(int C) { return C * (C + 1) / 2 + 2 * C; }
__host__ __device__ inline int cs_gram_lds_doubles(int C) { return CS_GH * CS_GW + CS_GH * (CS_GT + 1) + (2 * C + 1) * CS_GPX + CS_MAX_NS; }
__host__ __device__ inline int cs_apply_lds_doubles(int C) { return CL_SCRATCH + C * CL_PX; }

// t(d) = sum_n T(d - 2 n) T(n) with T the 23 taps by offset (level 1 inserts ms(i) at 2 i + 1 of the 2h grid, level 2 its result at the even positions of the
// 4h grid: ms(i) sits at u(4 i + 2)); R(d) = sum_m t(m) t(m - 4 d); st = sum t
struct CsTaps { double t[CS_T], r[CS_R], st; };
__host__ __device__ constexpr CsTaps cs_taps() {
    constexpr double HB[6] = CL_HALF_BAND;
    double T[23] = {};
    T[11] = 1.0;
    for (int i = 0; i < 6; ++i) T[11 + 2 * i + 1] = T[11 - 2 * i - 1] = 2 * HB[i];
    CsTaps c = {};
    for (int d = -CS_TREACH; d <= CS_TREACH; ++d) {
        double s = 0.0;
        for (int n = -11; n <= 11; ++n) {
            const int k = d - 2 * n;
            if (k >= -11 && k <= 11) s += T[11 + k] * T[11 + n];
        }
        c.t[d + CS_TREACH] = s;
    }
    for (int d = -CS_RREACH; d <= CS_RREACH; ++d) {
        double s = 0.0;
        for (int m = -CS_TREACH; m <= CS_TREACH; ++m) {
            const int k = m - 4 * d;
            if (k >= -CS_TREACH && k <= CS_TREACH) s += c.t[m + CS_TREACH] * c.t[k + CS_TREACH];
        }
        c.r[d + CS_RREACH] = s;
    }
    for (int i = 0; i < CS_T; ++i) c.st += c.t[i];
    return c;
}

// Four outputs STEP samples apart in one pass over the samples they share: out[o] = sum_k taps[k] src[(o STEP + k) stride].  Fully unrolled, so the taps are
// literals: a sample is read from LDS once for up to four products, and no tap is read from memory at all.  RT: the 33 taps of R, else the 67 of t.
template <bool RT, int STEP>
__device__ __forceinline__ void cs_fir4(const double* src, int stride, double (&out)[4]) {
    constexpr CsTaps K = cs_taps();
    constexpr int N = RT ? CS_R : CS_T;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int m = 0; m < N + 3 * STEP; ++m) {
        const double x = src[m * stride];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = m - o * STEP;
            if (k >= 0 && k < N) acc[o] = fma(RT ? K.r[k] : K.t[k], x, acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = acc[o];
}
static_assert(CS_AT % 4 == 0 && CS_GT % 4 == 0 && 4 * (CS_AT / 4) * (CS_AT / 4) <= CL_NT, "outputs in groups of four");

// part [B][3][tiles]: the sums over the tile of pan' and pan'^2 (its own pixels) and of q (its outputs).  qlow [B][h][w].  Three workgroups per compute unit by
// LDS: the registers are held to that.
__global__ __launch_bounds__(CL_NT, 3) void k_cs_adjoint(const float* __restrict__ pan, double* __restrict__ qlow, double* __restrict__ part, int h, int w,
                                                      int tiles_x, int tiles) {
    __shared__ double P[CS_ACH][CS_APW];                     // 32.25 KiB
    __shared__ double rowf[CS_ANCH * CS_ACH][CS_AT + 1];     // 17 KiB: slot s is PAN row 4 i0 - 31 + s, column j the tile's j-th decimated position
    __shared__ double red[4];
    const int tid = threadIdx.x, H4 = 4 * h, W4 = 4 * w;
    const int i0 = (blockIdx.x / tiles_x) * CS_AT, j0 = (blockIdx.x % tiles_x) * CS_AT;
    const long b = blockIdx.y;
    const float* __restrict__ pan_b = pan + b * ((long)H4 * W4);
    const double pv = (double)pan_b[0];
    const int rows = i0 + CS_AT <= h ? CS_AT : h - i0, cols = j0 + CS_AT <= w ? CS_AT : w - j0;
    const int span_y = 4 * (rows - 1) + CS_T, span_x = 4 * (cols - 1) + CS_T;
    const int y0 = 4 * i0 + 2 - CS_TREACH, x0 = 4 * j0 + 2 - CS_TREACH;
    // a thread stages one column of the chunk, every second row: its column modulo the side is formed once, its row advances by two
    const int c = tid & (CS_ALW - 1), r0 = tid / CS_ALW, xx = x0 + c, xm = cl_mod(xx, W4);
    const bool cin = c < span_x, ownx = xx >= 4 * j0 && xx < 4 * (j0 + cols);
    double s1 = 0.0, s2 = 0.0;
    for (int sb = 0; sb < span_y; sb += CS_ACH) {
        const int nrow = span_y - sb < CS_ACH ? span_y - sb : CS_ACH;
        int ym = cl_mod(y0 + sb + r0, H4);
#pragma unroll 4
        for (int r = r0; r < nrow; r += CL_NT / CS_ALW) {
            if (cin) {
                const int yy = y0 + sb + r;
                const double v = (double)pan_b[(long)ym * W4 + xm] - pv;
                P[r][c] = v;
                if (ownx && yy >= 4 * i0 && yy < 4 * (i0 + rows)) {      // the tile's own pixels: every PAN pixel is in one tile
                    s1 += v;
                    s2 = fma(v, v, s2);
                }
            }
            ym += CL_NT / CS_ALW;
            if (ym >= H4) ym -= H4;
        }
        __syncthreads();
        for (int i = tid; i < nrow * (CS_AT / 4); i += CL_NT) {
            const int r = i % nrow, jg = i / nrow;      // down the column: consecutive lanes are a row stride apart
            if (4 * jg >= cols) continue;               // (a group that reaches past the tile's columns reads staged slots nobody wrote: those outputs are never used)
            double o[4];
            cs_fir4<false, 4>(&P[r][16 * jg], 1, o);
#pragma unroll
            for (int u = 0; u < 4; ++u) rowf[sb + r][4 * jg + u] = o[u];
        }
        __syncthreads();
    }
    double q = 0.0;                               // the sum of the thread's outputs
    if (tid < CS_AT * CS_AT / 4) {               // a thread per column and group of four rows
        const int lyg = tid / CS_AT, lx = tid - lyg * CS_AT;
        if (4 * lyg < rows && lx < cols) {
            double o[4];
            cs_fir4<false, 4>(&rowf[16 * lyg][lx], CS_AT + 1, o);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (4 * lyg + u < rows) {
                    qlow[(b * h + i0 + 4 * lyg + u) * w + j0 + lx] = o[u];
                    q += o[u];
                }
        }
    }
    s1 = block_sum4(s1, red);
    __syncthreads();
    s2 = block_sum4(s2, red);
    __syncthreads();
    q = block_sum4(q, red);
    if (tid == 0) {
        part[(b * 3 + 0) * tiles + blockIdx.x] = s1;
        part[(b * 3 + 1) * tiles + blockIdx.x] = s2;
        part[(b * 3 + 2) * tiles + blockIdx.x] = q;
    }
}

// part [B][ns][gx]: entry (k, l >= k) in row-major order of the upper triangle = sum ms'_k v_l, then sum ms'_k q (C), then sum ms'_k (C)
__global__ __launch_bounds__(CL_NT) void k_cs_gram(const float* __restrict__ ms, const double* __restrict__ qlow, double* __restrict__ part, int C, int h, int w,
                                                   int tiles_x, int tiles) {
    extern __shared__ double cs_lds[];
    __shared__ int pairs[CS_MAX_NS];
    double* M = cs_lds;                          // [48][49]: ms'_l around the tile
    double* rf = M + CS_GH * CS_GW;              // [48][17]: R along x
    double* X = rf + CS_GH * (CS_GT + 1);        // [C][256]: ms'_k, 0 outside the image
    double* Y = X + C * CS_GPX;                  // [C + 1][256]: v_l, then q
    double* acc = Y + (C + 1) * CS_GPX;          // [ns]
    const int tid = threadIdx.x, gx = gridDim.x, ns = cs_ns(C);
    const long b = blockIdx.y, lp = (long)h * w;
    const float* __restrict__ ms_b = ms + b * C * lp;
    const double* __restrict__ q_b = qlow + b * lp;
    if (tid == 0) {
        int e = 0;
        for (int k = 0; k < C; ++k)
            for (int l = k; l < C; ++l) pairs[e++] = cl_pair(k, l, 0);
        for (int k = 0; k < C; ++k) pairs[e++] = cl_pair(k, C, 0);
        for (int k = 0; k < C; ++k) pairs[e++] = cl_pair(k, 255, 0);      // 255: the plain sum of ms'_k
    }
    for (int e = tid; e < ns; e += CL_NT) acc[e] = 0.0;
    // (the barriers of the first band order both before their first use)
    const int ly = tid / CS_GT, lx = tid - ly * CS_GT;
    const int lr = tid / CS_GH, lc = tid - lr * CS_GH;      // the halo row (of the first load) and column this thread stages
    for (int t = blockIdx.x; t < tiles; t += gx) {
        const int i0 = (t / tiles_x) * CS_GT, j0 = (t % tiles_x) * CS_GT;
        const bool in = i0 + ly < h && j0 + lx < w;
        const int rm0 = cl_mod(i0 - CS_RREACH + lr, h), cm = cl_mod(j0 - CS_RREACH + lc, w);
        for (int l = 0; l < C; ++l) {
            const float* __restrict__ ms_l = ms_b + l * lp;
            const double c = (double)ms_l[0];
            if (tid < CS_GLR * CS_GH) {          // a thread stages one column, every fifth row: modulo the sides without a division per sample
                int rm = rm0;
#pragma unroll
                for (int u = 0; u < (CS_GH + CS_GLR - 1) / CS_GLR; ++u) {
                    const int r = lr + u * CS_GLR;
                    if (r < CS_GH) M[r * CS_GW + lc] = (double)ms_l[(long)rm * w + cm] - c;
                    rm += CS_GLR;
                    if (rm >= h) rm -= h;
                    if (rm >= h) rm -= h;
                }
            }
            __syncthreads();
            if (tid < CS_GH * (CS_GT / 4)) {
                const int r = tid % CS_GH, jg = tid / CS_GH;      // down the column, as in the adjoint pass
                double o[4];
                cs_fir4<true, 1>(M + r * CS_GW + 4 * jg, 1, o);
#pragma unroll
                for (int u = 0; u < 4; ++u) rf[r * (CS_GT + 1) + 4 * jg + u] = o[u];
            }
            __syncthreads();
            if (tid < CS_GPX / 4) {                              // a thread per column and group of four rows
                const int lyg = tid / CS_GT, cx = tid - lyg * CS_GT;
                double o[4];
                cs_fir4<true, 1>(rf + 4 * lyg * (CS_GT + 1) + cx, CS_GT + 1, o);
#pragma unroll
                for (int u = 0; u < 4; ++u) Y[l * CS_GPX + (4 * lyg + u) * CS_GT + cx] = o[u];
            }
            X[l * CS_GPX + tid] = in ? M[(ly + CS_RREACH) * CS_GW + lx + CS_RREACH] : 0.0;
            __syncthreads();      // the next band overwrites M and rf
        }
        Y[C * CS_GPX + tid] = in ? q_b[(long)(i0 + ly) * w + j0 + lx] : 0.0;
        __syncthreads();
        cl_pair_sums(pairs, ns, acc, [&](int k, int l, int, int lane) {
            if (l != 255) return cl_lane_dot<CS_GPX>(X + k * CS_GPX, Y + l * CS_GPX, lane);
            double v = 0.0;
#pragma unroll
            for (int u = 0; u < CS_GPX / 64; ++u) v += X[k * CS_GPX + lane + 64 * u];
            return v;
        });
        __syncthreads();      // the next tile overwrites the vectors
    }
    for (int e = tid; e < ns; e += CL_NT) part[(b * ns + e) * gx + blockIdx.x] = acc[e];
}

struct CsWeights { double w[CL_MAX_C]; };

// coef [B][4 + 3 C]; stats: NULL or [B][2 C + 2] = w, g, a, m_I
__global__ __launch_bounds__(CL_NT) void k_cs_finish(const float* __restrict__ ms, const double* __restrict__ part1, const double* __restrict__ part2,
                                                     double* __restrict__ coef, double* __restrict__ stats, CsWeights wt, int mode, int C, int h, int w, int tiles,
                                                     int gx) {
    __shared__ double sums[CS_MAX_NS + 3];
    __shared__ double Sg[CL_MAX_C * CL_MAX_C], A[CL_MAX_C * CL_MAX_C], V[CL_MAX_C * CL_MAX_C], mk[CL_MAX_C], sk[CL_MAX_C], wv[CL_MAX_C], gv[CL_MAX_C], rk[CL_MAX_C], sw[CL_MAX_C];
    __shared__ double pm[2];                     // mean of pan', var(pan)
    const int ns = cs_ns(C), tid = threadIdx.x, lane = tid & 63;
    const long b = blockIdx.x;
    // a wave per sum: lane j adds the partials j, j + 64, ... in ascending order (eight loads in flight), then the butterfly -- one order, always
    for (int e = tid >> 6; e < ns + 3; e += CL_NT / 64) {
        const double* __restrict__ src = e < 3 ? part1 + (b * 3 + e) * tiles : part2 + (b * ns + e - 3) * gx;
        const int np = e < 3 ? tiles : gx;
        double v = 0.0;
        int j = lane;
        for (; j + 7 * 64 < np; j += 8 * 64) {
            double p[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) p[u] = src[j + u * 64];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; ++u) v += p[u];
        }
        for (; j < np; j += 64) v += src[j];
        v = wave_sum(v);
        if (lane == 0) sums[e] = v;
    }
    __syncthreads();
    constexpr double ST = cs_taps().st;
    const double n = (double)h * w, N = 16.0 * n, st2 = ST * ST, k16 = st2 / 16.0;
    if (tid == 0) {
        const double sp = sums[0], spp = sums[1], sq = sums[2];
        const double* G = sums + 3;              // upper triangle
        const double* XQ = G + C * (C + 1) / 2;
        const double* XS = XQ + C;
        pm[0] = sp / N;
        pm[1] = (spp - sp * sp / N) / (N - 1.0);
        for (int k = 0; k < C; ++k) {
            const double c = (double)ms[(b * C + k) * ((long)h * w)];
            sk[k] = XS[k];
            mk[k] = k16 * (sk[k] / n + c);
            rk[k] = (XQ[k] - k16 * (sk[k] / n) * sp + c * (sq - k16 * sp)) / (N - 1.0);
        }
        for (int k = 0, e = 0; k < C; ++k)
            for (int l = k; l < C; ++l, ++e) Sg[k * C + l] = Sg[l * C + k] = (G[e] - st2 * k16 * sk[k] * sk[l] / n) / (N - 1.0);
    }
    __syncthreads();
    if (mode == LG_CS_PCA) {
        // cyclic Jacobi on a copy of Sigma, the whole workgroup in step: every thread reads the pivot and forms the rotation, thread k < C turns row and column k of
        // A, thread 64 + k row k of V; two barriers per rotation.  The control flow depends on LDS values every thread reads alike.
        for (int i = tid; i < C * C; i += CL_NT) {
            A[i] = Sg[i];
            V[i] = i / C == i % C ? 1.0 : 0.0;
        }
        __syncthreads();
        for (int sweep = 0; sweep < CS_SWEEPS; ++sweep) {
            double off = 0.0, dg = 0.0;
            for (int p = 0; p < C; ++p) {
                dg = fma(A[p * C + p], A[p * C + p], dg);
                for (int q = p + 1; q < C; ++q) off = fma(A[p * C + q], A[p * C + q], off);
            }
            if (!(off > 1e-32 * dg)) break;      // converged, or not a number
            for (int p = 0; p < C - 1; ++p)
                for (int q = p + 1; q < C; ++q) {
                    const double apq = A[p * C + q], app = A[p * C + p], aqq = A[q * C + q];
                    if (apq == 0.0) continue;
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
                    const double cs = 1.0 / sqrt(fma(tt, tt, 1.0)), sn = tt * cs;
                    __syncthreads();             // every thread has read the pivot
                    if (tid < C) {
                        const int k = tid;
                        if (k == p) {
                            A[p * C + p] = app - tt * apq;
                            A[p * C + q] = A[q * C + p] = 0.0;
                        } else if (k == q) {
                            A[q * C + q] = aqq + tt * apq;
                        } else {
                            const double akp = A[k * C + p], akq = A[k * C + q];
                            A[k * C + p] = A[p * C + k] = cs * akp - sn * akq;
                            A[k * C + q] = A[q * C + k] = sn * akp + cs * akq;
                        }
                    } else if (tid >= 64 && tid < 64 + C) {
                        const int k = tid - 64;
                        const double vkp = V[k * C + p], vkq = V[k * C + q];
                        V[k * C + p] = cs * vkp - sn * vkq;
                        V[k * C + q] = sn * vkp + cs * vkq;
                    }
                    __syncthreads();
                }
        }
    }
    if (tid != 0) return;
    const double mpc = pm[0], vp = pm[1];
    double lam = 1.0;
    if (mode == LG_CS_PCA) {
        int jm = 0;
        for (int j = 1; j < C; ++j)
            if (A[j * C + j] > A[jm * C + jm]) jm = j;
        lam = A[jm * C + jm];
        double d = 0.0, sum = 0.0;
        for (int k = 0; k < C; ++k) {
            wv[k] = V[k * C + jm];
            d = fma(wv[k], rk[k], d);
            sum += wv[k];
        }
        if (d < 0.0 || (d == 0.0 && sum < 0.0))      // the sign rule: w'r >= 0, then sum w >= 0
            for (int k = 0; k < C; ++k) wv[k] = -wv[k];
    } else {
        for (int k = 0; k < C; ++k) wv[k] = wt.w[k];
    }
    double vi = 0.0, mi = 0.0;
    for (int k = 0; k < C; ++k) {
        double s = 0.0;
        for (int l = 0; l < C; ++l) s = fma(Sg[k * C + l], wv[l], s);
        sw[k] = s;                               // (Sigma w)_k
        vi = fma(wv[k], s, vi);
        mi = fma(wv[k], mk[k], mi);
    }
    const double a = sqrt(vi / vp);
    const bool ok = vp > 0.0 && vi > 0.0 && a - a == 0.0 && lam > 0.0;
    for (int k = 0; k < C; ++k) gv[k] = !ok ? 0.0 : mode == LG_CS_GS ? sw[k] / vi : mode == LG_CS_PCA ? wv[k] : 1.0;
    double* co = coef + b * (CS_COEF + 3 * C);
    co[0] = mpc;
    co[1] = ok ? a : 0.0;
    co[2] = mi;
    co[3] = ok ? 0.0 : 1.0;
    for (int k = 0; k < C; ++k) {
        co[CS_COEF + k] = mk[k];
        co[CS_COEF + C + k] = wv[k];
        co[CS_COEF + 2 * C + k] = gv[k];
    }
    if (stats) {
        double* st = stats + b * (2 * C + 2);
        for (int k = 0; k < C; ++k) {
            st[k] = wv[k];
            st[C + k] = gv[k];
        }
        st[2 * C] = ok ? a : 0.0;
        st[2 * C + 1] = mi;
    }
}

template <bool BROVEY>
__global__ __launch_bounds__(CL_NT) void k_cs_apply(const float* __restrict__ ms, const float* __restrict__ pan, float* __restrict__ out,
                                                    const double* __restrict__ coef, int C, int h, int w, int tiles_x) {
    extern __shared__ double cs_lds[];
    double* U = cs_lds + CL_SCRATCH;             // [C][512]
    const int tid = threadIdx.x, H4 = 4 * h, W4 = 4 * w;
    const auto [Y0, X0] = cl_tile(blockIdx.x, tiles_x);
    const long b = blockIdx.y, lp = (long)h * w, plane = (long)H4 * W4;
    const float* __restrict__ pan_b = pan + b * plane;
    float* __restrict__ out_b = out + b * C * plane;
    const double* __restrict__ co = coef + b * (CS_COEF + 3 * C);
    const double pv = (double)pan_b[0];
    cl_up_bands(ms + b * C * lp, lp, C, h, w, Y0, X0, cs_lds, U);
    __syncthreads();
    const int p = 2 * tid, y = Y0 + p / CL_TW, x = X0 + p % CL_TW;
    if (y >= H4 || x >= W4) return;              // W4 is a multiple of 4 and x is even: both pixels or none
    const long o = (long)y * W4 + x;
    const double mpc = co[0], a = co[1], mi = co[2];
    const bool deg = co[3] != 0.0;
    const float2 pp = *reinterpret_cast<const float2*>(pan_b + o);
    const double P0 = a * (((double)pp.x - pv) - mpc), P1 = a * (((double)pp.y - pv) - mpc);      // PAN matched to the intensity, minus m_I
    double I0 = 0.0, I1 = 0.0;                   // I
    for (int k = 0; k < C; ++k) {
        const double wk = co[CS_COEF + C + k], m = co[CS_COEF + k];
        I0 = fma(wk, U[k * CL_PX + p] - m, I0);
        I1 = fma(wk, U[k * CL_PX + p + 1] - m, I1);
    }
    if (BROVEY) {
        const double r0 = (P0 + mi) / (I0 + mi + 0x1p-52), r1 = (P1 + mi) / (I1 + mi + 0x1p-52);
        for (int k = 0; k < C; ++k) {
            const double u0 = U[k * CL_PX + p], u1 = U[k * CL_PX + p + 1];
            *reinterpret_cast<float2*>(out_b + k * plane + o) = make_float2(cl_clip(deg ? u0 : u0 * r0), cl_clip(deg ? u1 : u1 * r1));
        }
    } else {
        const double d0 = P0 - I0, d1 = P1 - I1;
        for (int k = 0; k < C; ++k) {
            const double g = co[CS_COEF + 2 * C + k], u0 = U[k * CL_PX + p], u1 = U[k * CL_PX + p + 1];
            *reinterpret_cast<float2*>(out_b + k * plane + o) = make_float2(cl_clip(deg ? u0 : fma(g, d0, u0)), cl_clip(deg ? u1 : fma(g, d1, u1)));
        }
    }
}

struct CsGeom {
    int at_x, at, gx, ns, tiles_x, tiles;      // the 16 x 16 tiles of the MS grid (adjoint and Gram), Gram workgroups, entries; the 16 x 32 output tiles
    size_t off[4], bytes;                       // q, part1, part2, coef
};

bool cs_geom(const char* who, int B, int C, int h, int w, CsGeom& g) {
    if (!cl_shape(who, B, C, h, w)) return false;
    g.at_x = (w + CS_AT - 1) / CS_AT;
    g.at = g.at_x * ((h + CS_AT - 1) / CS_AT);
    g.gx = g.at < CS_GRAM_WGS ? g.at : CS_GRAM_WGS;
    g.ns = cs_ns(C);
    g.tiles = cl_tiles(h, w, g.tiles_x);
    const size_t sz[4] = {(size_t)B * h * w * sizeof(double), ws_region(B, (size_t)3 * g.at * sizeof(double)),
                          ws_region(B, (size_t)g.ns * g.gx * sizeof(double)), ws_region(B, (size_t)(CS_COEF + 3 * C) * sizeof(double))};
    g.bytes = ws_layout(4, sz, g.off);
    return true;
}

DeviceOnce cs_attr_once;
int cs_lds_attr(const char* who) {
    if (!cs_attr_once.need()) return 0;
    if (int rc = lds_attr_set(who, cs_gram_lds_doubles(CL_MAX_C) * (int)sizeof(double), k_cs_gram)) return rc;
    if (int rc = lds_attr_set(who, cs_apply_lds_doubles(CL_MAX_C) * (int)sizeof(double), k_cs_apply<false>, k_cs_apply<true>)) return rc;
    cs_attr_once.done();
    return 0;
}

}  // namespace

extern "C" size_t lg_cs_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w) {
    CsGeom g;
    return cs_geom("cs_workspace_bytes", B, C, h, w, g) ? g.bytes : 0;
}

extern "C" int lg_cs(const float* ms, const float* pan, float* out, double* stats, const double* weights, int32_t mode, int32_t B, int32_t C, int32_t h,
                     int32_t w, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "cs";
    CsGeom g;
    if (!cs_geom(who, B, C, h, w, g)) return -1;
    if (mode != LG_CS_IHS && mode != LG_CS_BROVEY && mode != LG_CS_GS && mode != LG_CS_PCA) {
        lg_set_error("%s: mode must be LG_CS_IHS, LG_CS_BROVEY, LG_CS_GS or LG_CS_PCA (got %d)", who, mode);
        return -1;
    }
    if (weights && mode == LG_CS_PCA) { lg_set_error("%s: weights must be NULL for LG_CS_PCA: its weights are the first principal axis", who); return -1; }
    CsWeights wt = {};
    for (int k = 0; k < C; ++k) {
        wt.w[k] = weights ? weights[k] : 1.0 / C;
        if (wt.w[k] - wt.w[k] != 0.0) { lg_set_error("%s: weights[%d] must be finite", who, k); return -1; }
    }
    if (!cl_check_args(who, ms, pan, out, {}, stats, workspace, workspace_bytes, g.bytes, "lg_cs_workspace_bytes")) return -1;
    if (int rc = cs_lds_attr(who)) return rc;
    hipStream_t s = (hipStream_t)stream;
    double *qlow = cl_ws(workspace, g.off[0]), *part1 = cl_ws(workspace, g.off[1]), *part2 = cl_ws(workspace, g.off[2]), *coef = cl_ws(workspace, g.off[3]);
    k_cs_adjoint<<<dim3(g.at, B), CL_NT, 0, s>>>(pan, qlow, part1, h, w, g.at_x, g.at);
    LG_CHECK_LAUNCH();
    k_cs_gram<<<dim3(g.gx, B), CL_NT, cs_gram_lds_doubles(C) * sizeof(double), s>>>(ms, qlow, part2, C, h, w, g.at_x, g.at);
    LG_CHECK_LAUNCH();
    k_cs_finish<<<B, CL_NT, 0, s>>>(ms, part1, part2, coef, stats, wt, mode, C, h, w, g.at, g.gx);
    LG_CHECK_LAUNCH();
    const size_t lds = cs_apply_lds_doubles(C) * sizeof(double);
    if (mode == LG_CS_BROVEY)
        k_cs_apply<true><<<dim3(g.tiles, B), CL_NT, lds, s>>>(ms, pan, out, coef, C, h, w, g.tiles_x);
    else
        k_cs_apply<false><<<dim3(g.tiles, B), CL_NT, lds, s>>>(ms, pan, out, coef, C, h, w, g.tiles_x);
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_cs_taps(double* t67, double* r33) {
    if (!t67) { lg_set_error("cs_taps: t67 is NULL"); return -1; }
    if (!r33) { lg_set_error("cs_taps: r33 is NULL"); return -1; }
    constexpr CsTaps K = cs_taps();
    for (int i = 0; i < CS_T; ++i) t67[i] = K.t[i];
    for (int i = 0; i < CS_R; ++i) r33[i] = K.r[i];
    return 0;
}
