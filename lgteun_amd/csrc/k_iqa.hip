// Evaluation indices of lgteun_amd/metrics.py on the device, in fp64 (C ABI: lg_iqa_ref / lg_iqa_no_ref, include/lgteun_hip.h).
//
// Reduced resolution (metrics.ref_evaluate: PSNR, SSIM, Q, SAM, ERGAS), per image of the batch:
//   k_iqa_pix        pixel pass: a thread owns pixels across the band loop -- SAM angle sum, then per band the squared error and target sums
//   k_iqa_win<...>   window pass per (tile, band): the Gaussian (SSIM) or box (Q) local moments of one image pair from an LDS tile with halo,
//                    direct separable sums (vertical, then horizontal, like metrics._inside_windows), the index map summed over the tile's
//                    fully covered windows
//   k_iqa_fin_ref    one wave per image: fixed-order sums of the partials, the five indices
// Full resolution (metrics.no_ref_evaluate: D_lambda, D_s, QNR):
//   k_iqa_mtf_rows / k_iqa_mtf_cols   PAN_lr = metrics.mtf_degrade(pan), evaluated at the decimated samples only
//   k_iqa_win<Q>     Q maps of the band pairs l < r and of the band-to-PAN pairs, at PAN resolution and at MS resolution
//   k_iqa_fin_noref  one wave per image
// Every sum is a per-workgroup partial in the caller's workspace followed by a fixed-order pass; no atomics (the wave butterfly and the
// workspace layout are reduce.h's; the workgroup and per-image sums keep their own order, below).  Two calls give the same bits,
// and no reduction mixes images: row b of a batch is the row of image b scored alone.
#include <float.h>
#include <math.h>

#include "abi.h"
#include "common.h"
#include "reduce.h"

// Inputs are scaled in fp32 and each product is rounded on its own before it is widened (the rounding of data_denormalize on the host
// path); a product contracted into an fma with the following subtraction would round differently.  Nothing in this file is contracted,
// so the fp64 arithmetic is also the host's, operation for operation, up to the order of the sums.
#pragma clang fp contract(off)

namespace {

constexpr int IQA_NT = 256;                // threads per workgroup of the pixel, window and MTF passes
constexpr int IQA_TX = 32, IQA_TY = 8;     // window positions per tile of the window pass: one per thread
constexpr int IQA_PIX_BLOCKS = 64;         // at most this many workgroups per image in the pixel pass
constexpr int IQA_MTF_HALF = LG_IQA_MTF_TAPS / 2;
constexpr double IQA_TINY = DBL_EPSILON;   // metrics._TINY
constexpr double IQA_Q_FLAT = 1e-8;        // metrics._q_band: a factor whose denominator is <= this counts as 1
constexpr double IQA_PSNR_FLOOR = 1e-10;   // metrics.psnr: an mse <= this is reported as +inf

enum { IQA_SSIM = 0, IQA_Q = 1 };

struct Taps {
    double w[LG_IQA_MTF_TAPS];   // the longest filter; the window passes use the first n
};

// the pair of planes a window-pass workgroup scores
struct WinPlanes {
    const float* a;     // [B][C][H][W]: pred (reduced resolution, no-reference at PAN resolution) or ms (no-reference at MS resolution)
    const float* b;     // reduced resolution: gt [B][C][H][W]
    const float* p32;   // no-reference at PAN resolution: pan [B][H][W], scaled like `a`
    const double* p64;  // no-reference at MS resolution: PAN_lr [B][H][W], already scaled
};

__device__ __forceinline__ double ld_scaled(const float* __restrict__ p, long i, float s) { return (double)__fmul_rn(p[i], s); }

// sum over the workgroup, valid in thread 0; every thread calls it (red: IQA_NT / 64 doubles of LDS, reused call after call)
// not reduce.h's block_sum4: this one is reuse-safe and meets the waves left to right; another association would move the indices' last bits
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < IQA_NT / 64; ++i) t += red[i];
    return t;
}

// sum_{j < n} p[j * stride] in a fixed order for one wave: lane l takes j = l, l + 64, ...
__device__ __forceinline__ double lanes_sum(const double* __restrict__ p, int n, long stride) {
    double v = 0.0;
    for (int j = threadIdx.x; j < n; j += 64) v += p[(long)j * stride];
    return wave_sum(v);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// reduced resolution: pixel pass.  part[b][blk][1 + 2C] = { sum of angles, squared error per band, target sum per band }
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IQA_NT) void k_iqa_pix(const float* __restrict__ pred, const float* __restrict__ gt, int C, int HW, float s,
                                                   double* __restrict__ part) {
    __shared__ double red[IQA_NT / 64];
    const int b = blockIdx.y, nblk = gridDim.x, step = nblk * IQA_NT, i0 = blockIdx.x * IQA_NT + threadIdx.x;
    const float* x = pred + (long)b * C * HW;
    const float* y = gt + (long)b * C * HW;
    double* out = part + ((long)b * nblk + blockIdx.x) * (1 + 2 * C);
    double sam = 0.0;
    for (int i = i0; i < HW; i += step) {
        double dot = 0.0, nx = 0.0, ny = 0.0;
        for (int c = 0; c < C; ++c) {
            const double a = ld_scaled(x, (long)c * HW + i, s), g = ld_scaled(y, (long)c * HW + i, s);
            dot += a * g;
            nx += a * a;
            ny += g * g;
        }
        double cs = dot / (sqrt(nx) * sqrt(ny) + IQA_TINY);
        cs = cs < 0.0 ? 0.0 : (cs > 1.0 ? 1.0 : cs);   // np.clip (a NaN stays NaN)
        sam += acos(cs);
    }
    double t = block_sum(sam, red);
    if (threadIdx.x == 0) out[0] = t;
    for (int c = 0; c < C; ++c) {
        double se = 0.0, sg = 0.0;
        for (int i = i0; i < HW; i += step) {
            const double a = ld_scaled(x, (long)c * HW + i, s), g = ld_scaled(y, (long)c * HW + i, s), d = a - g;
            se += d * d;
            sg += g;
        }
        t = block_sum(se, red);
        if (threadIdx.x == 0) out[1 + c] = t;
        t = block_sum(sg, red);
        if (threadIdx.x == 0) out[1 + C + c] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// window pass: grid (tile, pair, image).  part[b][pair][tile] = sum of the SSIM / Q map over the tile's fully covered windows.
// fam 0: pair c = (a_c, b_c).  fam 1: pairs (a_l, a_r), l < r, in the order of metrics.d_lambda, then (a_l, PAN) for l = 0 .. C-1.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int MODE, int NMAX>
__global__ __launch_bounds__(IQA_NT) void k_iqa_win(WinPlanes pl, int fam, int C, int H, int W, int n, float s, Taps taps, int tiles_x,
                                                   double* __restrict__ part) {
    constexpr int SW = IQA_TX + NMAX - 1, SH = IQA_TY + NMAX - 1;
    __shared__ double X[SH * SW], Y[SH * SW];
    __shared__ double V[5][IQA_TY * SW];
    __shared__ double T[NMAX];
    __shared__ double red[IQA_NT / 64];
    const int tile = blockIdx.x, p = blockIdx.y, b = blockIdx.z;
    const int r0 = (tile / tiles_x) * IQA_TY, c0 = (tile % tiles_x) * IQA_TX;
    const long HW = (long)H * W;
    const float* xa;
    const float* ya = nullptr;
    const double* yd = nullptr;
    if (fam == 0) {
        xa = pl.a + ((long)b * C + p) * HW;
        ya = pl.b + ((long)b * C + p) * HW;
    } else if (p < C * (C - 1) / 2) {
        int l = 0, q = p;
        while (q >= C - 1 - l) { q -= C - 1 - l; ++l; }
        xa = pl.a + ((long)b * C + l) * HW;
        ya = pl.a + ((long)b * C + l + 1 + q) * HW;
    } else {
        xa = pl.a + ((long)b * C + p - C * (C - 1) / 2) * HW;
        if (pl.p64) yd = pl.p64 + b * HW;
        else ya = pl.p32 + b * HW;
    }
    if (threadIdx.x < n) T[threadIdx.x] = taps.w[threadIdx.x];
    // the tile's input with its halo; what lies outside the image feeds only windows that are not fully inside it
    const int sw = IQA_TX + n - 1, sh = IQA_TY + n - 1;
    for (int i = threadIdx.x; i < sh * sw; i += IQA_NT) {
        const int r = i / sw, c = i - r * sw, gr = r0 + r, gc = c0 + c;
        double vx = 0.0, vy = 0.0;
        if (gr < H && gc < W) {
            const long o = (long)gr * W + gc;
            vx = ld_scaled(xa, o, s);
            vy = yd ? yd[o] : ld_scaled(ya, o, s);
        }
        X[r * SW + c] = vx;
        Y[r * SW + c] = vy;
    }
    __syncthreads();
    // vertical window sums of x, y, x^2, y^2, xy (the squares and the cross product before the weighting, like the host)
    for (int i = threadIdx.x; i < IQA_TY * sw; i += IQA_NT) {
        const int r = i / sw, c = i - r * sw;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
        for (int k = 0; k < n; ++k) {
            const double x = X[(r + k) * SW + c], y = Y[(r + k) * SW + c], w = T[k];
            m0 += w * x;
            m1 += w * y;
            m2 += w * (x * x);
            m3 += w * (y * y);
            m4 += w * (x * y);
        }
        const int o = r * SW + c;
        V[0][o] = m0;
        V[1][o] = m1;
        V[2][o] = m2;
        V[3][o] = m3;
        V[4][o] = m4;
    }
    __syncthreads();
    // horizontal sums and the index at this thread's window position
    const int r = threadIdx.x / IQA_TX, c = threadIdx.x % IQA_TX;
    double val = 0.0;
    if (r0 + r <= H - n && c0 + c <= W - n) {
        double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
        for (int k = 0; k < n; ++k) {
            const int o = r * SW + c + k;
            const double w = T[k];
            mx += w * V[0][o];
            my += w * V[1][o];
            exx += w * V[2][o];
            eyy += w * V[3][o];
            exy += w * V[4][o];
        }
        const double vx = exx - mx * mx, vy = eyy - my * my, cxy = exy - mx * my;
        if (MODE == IQA_SSIM) {
            const double c1 = (0.01 * LG_IQA_PEAK) * (0.01 * LG_IQA_PEAK), c2 = (0.03 * LG_IQA_PEAK) * (0.03 * LG_IQA_PEAK);
            const double luminance = (2.0 * mx * my + c1) / (mx * mx + my * my + c1);
            const double structure = (2.0 * cxy + c2) / (vx + vy + c2);
            val = luminance * structure;
        } else {
            const double energy = mx * mx + my * my, spread = vx + vy;
            const double luminance = energy > IQA_Q_FLAT ? 2.0 * mx * my / energy : 1.0;
            const double structure = spread > IQA_Q_FLAT ? 2.0 * cxy / spread : 1.0;
            val = luminance * structure;
        }
    }
    const double t = block_sum(val, red);
    if (threadIdx.x == 0) part[((long)b * gridDim.y + p) * gridDim.x + tile] = t;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// PAN_lr = mtf_degrade(pan): the separable low-pass with replicated edges at the decimated samples only.
// rows[b][i][c] = sum_k w_k pan[4 i + k - 20][c - 20] (c < W + 40, indices clamped), then plr[b][i][j] = sum_l w_l rows[b][i][4 j + l].
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IQA_NT) void k_iqa_mtf_rows(const float* __restrict__ pan, int H, int W, float s, Taps taps,
                                                        double* __restrict__ rows) {
    __shared__ double T[LG_IQA_MTF_TAPS];
    if (threadIdx.x < LG_IQA_MTF_TAPS) T[threadIdx.x] = taps.w[threadIdx.x];
    __syncthreads();
    const int Wp = W + 2 * IQA_MTF_HALF, h = H / LG_IQA_RATIO, i = blockIdx.y, b = blockIdx.z;
    const int c = blockIdx.x * IQA_NT + threadIdx.x;
    if (c >= Wp) return;
    const float* p = pan + (long)b * H * W;
    const int col = clampi(c - IQA_MTF_HALF, 0, W - 1);
    double acc = 0.0;
    for (int k = 0; k < LG_IQA_MTF_TAPS; ++k)
        acc += T[k] * ld_scaled(p, (long)clampi(LG_IQA_RATIO * i + k - IQA_MTF_HALF, 0, H - 1) * W + col, s);
    rows[((long)b * h + i) * Wp + c] = acc;
}

__global__ __launch_bounds__(IQA_NT) void k_iqa_mtf_cols(const double* __restrict__ rows, int H, int W, Taps taps, double* __restrict__ plr) {
    __shared__ double T[LG_IQA_MTF_TAPS];
    if (threadIdx.x < LG_IQA_MTF_TAPS) T[threadIdx.x] = taps.w[threadIdx.x];
    __syncthreads();
    const int Wp = W + 2 * IQA_MTF_HALF, h = H / LG_IQA_RATIO, w = W / LG_IQA_RATIO, i = blockIdx.y, b = blockIdx.z;
    const int j = blockIdx.x * IQA_NT + threadIdx.x;
    if (j >= w) return;
    const double* r = rows + ((long)b * h + i) * Wp + LG_IQA_RATIO * j;
    double acc = 0.0;
    for (int l = 0; l < LG_IQA_MTF_TAPS; ++l) acc += T[l] * r[l];
    plr[((long)b * h + i) * w + j] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// finishing passes: one wave per image
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_iqa_fin_ref(const double* __restrict__ pix, int npix, const double* __restrict__ ssim, int nts,
                                                   double cnt_s, const double* __restrict__ q, int ntq, double cnt_q, int C, int HW,
                                                   double* __restrict__ out) {
    const int b = blockIdx.x, K = 1 + 2 * C;
    const double* pb = pix + (long)b * npix * K;
    const double n = (double)HW;
    const double sam = lanes_sum(pb, npix, K) / n;
    double sse = 0.0, erg = 0.0, ss = 0.0, qq = 0.0;
    for (int c = 0; c < C; ++c) {
        const double e = lanes_sum(pb + 1 + c, npix, K), g = lanes_sum(pb + 1 + C + c, npix, K), mean = g / n;
        sse += e;
        erg += (e / n) / (mean * mean + IQA_TINY);
        ss += lanes_sum(ssim + ((long)b * C + c) * nts, nts, 1) / cnt_s;
        qq += lanes_sum(q + ((long)b * C + c) * ntq, ntq, 1) / cnt_q;
    }
    if (threadIdx.x == 0) {
        const double mse = sse / ((double)C * n);
        double* o = out + (long)b * 5;
        o[0] = mse <= IQA_PSNR_FLOOR ? __builtin_huge_val() : 20.0 * log10(LG_IQA_PEAK / (sqrt(mse) + IQA_TINY));
        o[1] = ss / C;
        o[2] = qq / C;
        o[3] = sam;
        o[4] = 100.0 / LG_IQA_RATIO * sqrt(erg / C);
    }
}

__global__ __launch_bounds__(64) void k_iqa_fin_noref(const double* __restrict__ qf, int ntf, double cnt_f, const double* __restrict__ qm,
                                                     int ntm, double cnt_m, int C, double* __restrict__ out) {
    const int b = blockIdx.x, np = C * (C + 1) / 2, nbp = C * (C - 1) / 2;
    double dl = 0.0, ds = 0.0;
    for (int p = 0; p < np; ++p) {
        const double qfp = lanes_sum(qf + ((long)b * np + p) * ntf, ntf, 1) / cnt_f;
        const double qmp = lanes_sum(qm + ((long)b * np + p) * ntm, ntm, 1) / cnt_m;
        if (p < nbp) dl += fabs(qfp - qmp);
        else ds += fabs(qfp - qmp);
    }
    if (threadIdx.x == 0) {
        dl /= nbp;
        ds /= C;
        double* o = out + (long)b * 3;
        o[0] = dl;
        o[1] = ds;
        o[2] = (1.0 - dl) * (1.0 - ds);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: taps, geometry, workspace layout, validation
// ---------------------------------------------------------------------------------------------------------------------------------
Taps gaussian_taps(int n, double sigma) {   // metrics.gaussian_taps
    Taps t{};
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const double x = (k - 0.5 * (n - 1)) / sigma;
        t.w[k] = exp(-0.5 * (x * x));
        sum += t.w[k];
    }
    for (int k = 0; k < n; ++k) t.w[k] /= sum;
    return t;
}
Taps box_taps(int n) {   // np.full(block, 1.0 / block)
    Taps t{};
    for (int k = 0; k < n; ++k) t.w[k] = 1.0 / n;
    return t;
}
double bessel_i0(double x) {   // metrics._bessel_i0: the power series, 24 terms
    double term = 1.0, total = 1.0;
    for (int k = 1; k < 25; ++k) {
        term = term * (0.5 * x / k) * (0.5 * x / k);
        total = total + term;
    }
    return total;
}
// metrics.mtf_taps(MTF_GAIN_PAN, ERGAS_RATIO): the row sums of the window-method filter (metrics.mtf_window_filter, operation for operation
// up to the order of the sums).  Computed on the first call; a function-local static is initialised once, whatever thread asks first.
Taps mtf_taps_compute() {
    constexpr int N = LG_IQA_MTF_TAPS, HALF = N / 2;
    static_assert(N % 2 == 1 && N >= 3, "the window method is written for an odd number of taps");
    const double alpha = sqrt(((N - 1) * (0.5 / LG_IQA_RATIO)) * ((N - 1) * (0.5 / LG_IQA_RATIO)) / (-2.0 * log(LG_IQA_MTF_GAIN)));
    double resp[N], g[N], kaiser[HALF + 1], t[N];
    for (int k = 0; k < N; ++k) {
        const double q = (k - HALF) / alpha;
        resp[k] = exp(-0.5 * (q * q));
        t[k] = (double)(k - HALF) / (N - 1.0);
    }
    for (int m = 0; m < N; ++m) {     // the centred inverse DFT of the (even, real) response
        double s = 0.0;
        for (int k = 0; k < N; ++k) s += resp[k] * cos(2.0 * M_PI * (k - HALF) * (m - HALF) / N);
        g[m] = s / N;
    }
    const double i0_beta = bessel_i0(0.5);
    for (int j = 0; j <= HALF; ++j) kaiser[j] = bessel_i0(0.5 * sqrt(1.0 - ((double)j / HALF) * ((double)j / HALF))) / i0_beta;
    double rows[N], total = 0.0;
    for (int i = 0; i < N; ++i) {
        rows[i] = 0.0;
        for (int j = 0; j < N; ++j) {
            const double radius = sqrt(t[i] * t[i] + t[j] * t[j]);
            double win = 0.0;
            if (!(radius > t[N - 1])) {   // the radial Kaiser window, read between its samples; zero beyond the radius 1/2
                const double x = radius * (N - 1.0);
                int lo = (int)x;
                if (lo > HALF - 1) lo = HALF - 1;
                win = kaiser[lo] + (x - lo) * (kaiser[lo + 1] - kaiser[lo]);
            }
            rows[i] += (g[i] * g[j]) * win;
        }
        total += rows[i];
    }
    Taps out{};
    for (int i = 0; i < N; ++i) out.w[i] = rows[i] / total;
    return out;
}
const Taps& mtf_taps() {
    static const Taps taps = mtf_taps_compute();
    return taps;
}

struct WinGrid {
    int tiles_x, tiles;
    double windows;   // fully covered window positions: the denominator of the map's mean
};
WinGrid win_grid(int H, int W, int n) {
    const int ho = H - n + 1, wo = W - n + 1, tx = (wo + IQA_TX - 1) / IQA_TX;
    return {tx, tx * ((ho + IQA_TY - 1) / IQA_TY), (double)ho * wo};
}

struct IqaGeom {
    int npix, bsm;       // reduced resolution: pixel-pass workgroups per image; no-reference: the Q window at MS resolution
    WinGrid g0, g1;      // reduced resolution: SSIM and Q tiles; no-reference: PAN-resolution and MS-resolution tiles
    size_t off[4];       // workspace regions: reduced resolution pix | ssim | q; no-reference rows | PAN_lr | qf | qm
    size_t bytes;
};

// false: not a shape the indices are defined for (the reason is in lg_last_error)
bool iqa_geom(int B, int C, int H, int W, int no_ref, IqaGeom& g) {
    if (B < 1 || B > 65535) { lg_set_error("iqa: B must be 1..65535 (got %d)", B); return false; }
    if (C < 2 || C > LG_IQA_MAX_BANDS) { lg_set_error("iqa: C must be 2..%d (SAM and D_lambda need bands; got %d)", LG_IQA_MAX_BANDS, C); return false; }
    if (H < LG_IQA_SSIM_TAPS || W < LG_IQA_SSIM_TAPS) { lg_set_error("iqa: H and W must be >= %d (an SSIM window; got %d x %d)", LG_IQA_SSIM_TAPS, H, W); return false; }
    if (H > 8192 || W > 8192) { lg_set_error("iqa: H and W must be <= 8192 (got %d x %d)", H, W); return false; }
    const size_t d = sizeof(double);
    size_t sz[4] = {0, 0, 0, 0};
    if (!no_ref) {
        const int blocks = (H * W + IQA_NT - 1) / IQA_NT;
        g.npix = blocks < IQA_PIX_BLOCKS ? blocks : IQA_PIX_BLOCKS;
        g.bsm = 0;
        g.g0 = win_grid(H, W, LG_IQA_SSIM_TAPS);
        g.g1 = win_grid(H, W, LG_IQA_Q_BLOCK);
        sz[0] = (size_t)B * g.npix * (1 + 2 * C) * d;
        sz[1] = (size_t)B * C * g.g0.tiles * d;
        sz[2] = (size_t)B * C * g.g1.tiles * d;
    } else {
        if (H < LG_IQA_QNR_BLOCK || W < LG_IQA_QNR_BLOCK || H % LG_IQA_RATIO || W % LG_IQA_RATIO) {
            lg_set_error("iqa: the no-reference indices need H and W >= %d and multiples of %d (got %d x %d)", LG_IQA_QNR_BLOCK, LG_IQA_RATIO, H, W);
            return false;
        }
        const int h = H / LG_IQA_RATIO, w = W / LG_IQA_RATIO, np = C * (C + 1) / 2;
        g.npix = 0;
        g.bsm = h < w ? h : w;
        if (g.bsm > LG_IQA_QNR_BLOCK) g.bsm = LG_IQA_QNR_BLOCK;   // min(block, min(shape)) of metrics.d_lambda / d_s
        g.g0 = win_grid(H, W, LG_IQA_QNR_BLOCK);
        g.g1 = win_grid(h, w, g.bsm);
        sz[0] = (size_t)B * h * (W + 2 * IQA_MTF_HALF) * d;
        sz[1] = (size_t)B * h * w * d;
        sz[2] = (size_t)B * np * g.g0.tiles * d;
        sz[3] = (size_t)B * np * g.g1.tiles * d;
    }
    g.bytes = ws_layout(4, sz, g.off);
    return true;
}

bool iqa_check_buffers(bool ptrs_ok, float scale, void* workspace, size_t workspace_bytes, const IqaGeom& g) {
    if (!ptrs_ok || !workspace) { lg_set_error("iqa: null pointer"); return false; }
    if (!isfinite(scale)) { lg_set_error("iqa: scale must be finite"); return false; }
    if ((uintptr_t)workspace & 7) { lg_set_error("iqa: workspace must be 8-byte aligned"); return false; }
    if (workspace_bytes < g.bytes) { lg_set_error("iqa: workspace too small: %zu bytes, need %zu", workspace_bytes, g.bytes); return false; }
    return true;
}

}  // namespace

extern "C" size_t lg_iqa_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t no_ref) {
    IqaGeom g;
    return iqa_geom(B, C, H, W, no_ref, g) ? g.bytes : 0;
}

extern "C" int lg_iqa_mtf_taps(double* out41) {
    if (!out41) { lg_set_error("iqa_mtf_taps: out41 is NULL"); return -1; }
    const Taps& t = mtf_taps();
    for (int k = 0; k < LG_IQA_MTF_TAPS; ++k) out41[k] = t.w[k];
    return 0;
}

extern "C" int lg_iqa_ref(const float* pred, const float* gt, double* out, int32_t B, int32_t C, int32_t H, int32_t W, float scale,
                          void* workspace, size_t workspace_bytes, void* stream) {
    IqaGeom g;
    if (!iqa_geom(B, C, H, W, 0, g) || !iqa_check_buffers(pred && gt && out, scale, workspace, workspace_bytes, g)) return -1;
    const hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double *pix = (double*)(ws + g.off[0]), *ssim = (double*)(ws + g.off[1]), *q = (double*)(ws + g.off[2]);
    const WinPlanes pl{pred, gt, nullptr, nullptr};
    k_iqa_pix<<<dim3(g.npix, B), IQA_NT, 0, s>>>(pred, gt, C, H * W, scale, pix);
    LG_CHECK_LAUNCH();
    k_iqa_win<IQA_SSIM, LG_IQA_SSIM_TAPS><<<dim3(g.g0.tiles, C, B), IQA_NT, 0, s>>>(
        pl, 0, C, H, W, LG_IQA_SSIM_TAPS, scale, gaussian_taps(LG_IQA_SSIM_TAPS, LG_IQA_SSIM_SIGMA), g.g0.tiles_x, ssim);
    LG_CHECK_LAUNCH();
    static_assert(LG_IQA_Q_BLOCK <= LG_IQA_SSIM_TAPS, "the Q pass runs in the SSIM pass's tile geometry");
    k_iqa_win<IQA_Q, LG_IQA_SSIM_TAPS><<<dim3(g.g1.tiles, C, B), IQA_NT, 0, s>>>(
        pl, 0, C, H, W, LG_IQA_Q_BLOCK, scale, box_taps(LG_IQA_Q_BLOCK), g.g1.tiles_x, q);
    LG_CHECK_LAUNCH();
    k_iqa_fin_ref<<<B, 64, 0, s>>>(pix, g.npix, ssim, g.g0.tiles, g.g0.windows, q, g.g1.tiles, g.g1.windows, C, H * W, out);
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_iqa_no_ref(const float* pred, const float* pan, const float* ms, double* out, int32_t B, int32_t C, int32_t H, int32_t W,
                             float scale, void* workspace, size_t workspace_bytes, void* stream) {
    IqaGeom g;
    if (!iqa_geom(B, C, H, W, 1, g) || !iqa_check_buffers(pred && pan && ms && out, scale, workspace, workspace_bytes, g)) return -1;
    const hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double *rows = (double*)(ws + g.off[0]), *plr = (double*)(ws + g.off[1]), *qf = (double*)(ws + g.off[2]), *qm = (double*)(ws + g.off[3]);
    const int h = H / LG_IQA_RATIO, w = W / LG_IQA_RATIO, np = C * (C + 1) / 2;
    const Taps tm = mtf_taps();
    k_iqa_mtf_rows<<<dim3((W + 2 * IQA_MTF_HALF + IQA_NT - 1) / IQA_NT, h, B), IQA_NT, 0, s>>>(pan, H, W, scale, tm, rows);
    LG_CHECK_LAUNCH();
    k_iqa_mtf_cols<<<dim3((w + IQA_NT - 1) / IQA_NT, h, B), IQA_NT, 0, s>>>(rows, H, W, tm, plr);
    LG_CHECK_LAUNCH();
    k_iqa_win<IQA_Q, LG_IQA_QNR_BLOCK><<<dim3(g.g0.tiles, np, B), IQA_NT, 0, s>>>(
        WinPlanes{pred, nullptr, pan, nullptr}, 1, C, H, W, LG_IQA_QNR_BLOCK, scale, box_taps(LG_IQA_QNR_BLOCK), g.g0.tiles_x, qf);
    LG_CHECK_LAUNCH();
    k_iqa_win<IQA_Q, LG_IQA_QNR_BLOCK><<<dim3(g.g1.tiles, np, B), IQA_NT, 0, s>>>(
        WinPlanes{ms, nullptr, nullptr, plr}, 1, C, h, w, g.bsm, scale, box_taps(g.bsm), g.g1.tiles_x, qm);
    LG_CHECK_LAUNCH();
    k_iqa_fin_noref<<<B, 64, 0, s>>>(qf, g.g0.tiles, g.g0.windows, qm, g.g1.tiles, g.g1.windows, C, out);
    LG_CHECK_LAUNCH();
    return 0;
}
