// The extended evaluation indices of lgteun_amd/metrics.py on the device, in fp64 (C ABI: lg_iqa_ref_ext / lg_iqa_q2n, include/lgteun_hip.h;
// definitions: DESIGN.md 3.8.1).  Per image of the batch:
//   k_iqa_q2n<N>     Q2n, N = 2, 4, 8 components: one workgroup per 32 x 32 block.  A thread owns 4 pixels x N bands of both images in
//                    registers; the per-band mean and deviation (two passes), the normalised tiles, the hypercomplex product per pixel and
//                    the 3 N + 2 block sums; thread 0 forms the block's value
//   k_iqa_scc        SCC: Sobel magnitudes of both images at a 32 x 8 tile of interior pixels of one band, the three sums per workgroup
//   k_iqa_cc         CC: one workgroup per band: min, max and mean, then the centred moments (two passes), Pearson's r or NaN
//   k_iqa_fin_ext    one wave per image: fixed-order sums of the partials, the indices
// As in k_iqa.hip every sum is a per-workgroup partial in the caller's workspace followed by a fixed-order pass, no atomics; the partition
// depends on the shape only and no reduction mixes images.  Q2n's block sums are ONE tree, the one metrics._block_sum restates on the
// host: pixel p of a block belongs to thread p % 256, which adds its four as (v0 + v1) + (v2 + v3); the lanes of a wave halve (32, 16, ...,
// 1); the four waves meet as (w0 + w1) + (w2 + w3).  A tree of halvings adds equal values exactly, so a flat block takes the host's branch.
#include <float.h>
#include <math.h>

#include "abi.h"
#include "common.h"
#include "reduce.h"

// as in k_iqa.hip: the fp32 scaling is rounded on its own and nothing is contracted, so the fp64 arithmetic is the host's operation for operation
#pragma clang fp contract(off)

namespace {

constexpr int EXT_NT = 256;                 // threads per workgroup of every pass but the finish
constexpr int Q2N_BS = 32;                  // metrics.Q2N_BLOCK
constexpr int Q2N_PIX = Q2N_BS * Q2N_BS;    // pixels per block: 4 per thread
constexpr int SCC_TX = 32, SCC_TY = 8;      // interior pixels per tile of the SCC pass: one per thread
static_assert(Q2N_PIX == 4 * EXT_NT, "a thread owns four pixels of a block");

// k_iqa.hip's two helpers (its namespace is private to that file)
__device__ __forceinline__ double ld_scaled(const float* __restrict__ p, long i, float s) { return (double)__fmul_rn(p[i], s); }
__device__ __forceinline__ double lanes_sum(const double* __restrict__ p, int n, long stride) {
    double v = 0.0;
    for (int j = threadIdx.x; j < n; j += 64) v += p[(long)j * stride];
    return wave_sum(v);
}

__device__ __forceinline__ double sum4(double v0, double v1, double v2, double v3) { return (v0 + v1) + (v2 + v3); }

// K sums over the workgroup at once, in every thread: the tree of the file comment (red: 4 K doubles of LDS, reused call after call)
template <int K>
__device__ __forceinline__ void block_tree(double (&v)[K], double* red) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
}

// metrics.hmul, fully unrolled: x * y = ( a*c - conj(d)*b , conj(a)*conj(d) + c*conj(b) ) on the halves x = (a, b), y = (c, d)
template <int N>
struct HMul {
    static __device__ __forceinline__ void conj(const double* a, double* o) {
        o[0] = a[0];
#pragma unroll
        for (int i = 1; i < N; ++i) o[i] = -a[i];
    }
    static __device__ __forceinline__ void mul(const double* x, const double* y, double* o) {
        constexpr int h = N / 2;
        double ca[h], cb[h], cd[h], t1[h], t2[h];
        HMul<h>::conj(x, ca);
        HMul<h>::conj(x + h, cb);
        HMul<h>::conj(y + h, cd);
        HMul<h>::mul(x, y, t1);
        HMul<h>::mul(cd, x + h, t2);
#pragma unroll
        for (int i = 0; i < h; ++i) o[i] = t1[i] - t2[i];
        HMul<h>::mul(ca, cd, t1);
        HMul<h>::mul(y, cb, t2);
#pragma unroll
        for (int i = 0; i < h; ++i) o[h + i] = t1[i] + t2[i];
    }
};
template <>
struct HMul<1> {
    static __device__ __forceinline__ void conj(const double* a, double* o) { o[0] = a[0]; }
    static __device__ __forceinline__ void mul(const double* x, const double* y, double* o) { o[0] = x[0] * y[0]; }
};

// index into a side of length L of coordinate i of the side extended to a multiple of 32: the lines L-1, L-2, ... follow the last one.
// i < L + 31 and L >= 32, so the mirrored index lies in 1 .. L-1
__device__ __forceinline__ int mirror(int i, int L) { return i < L ? i : 2 * L - 1 - i; }

// ---------------------------------------------------------------------------------------------------------------------------------
// Q2n: grid (block, image).  vals[b][block] = the block's value (metrics._q2n_block)
// ---------------------------------------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(EXT_NT) void k_iqa_q2n(const float* __restrict__ gt, const float* __restrict__ fused, int C, int H, int W, float s,
                                                   int blocks_x, double* __restrict__ vals) {
    constexpr int K3 = 3 * N + 2;
    __shared__ double red[4 * K3];
    const int blk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int r0 = (blk / blocks_x) * Q2N_BS, c0 = (blk % blocks_x) * Q2N_BS;
    const long HW = (long)H * W;
    const float* g = gt + (long)b * C * HW;
    const float* f = fused + (long)b * C * HW;
    const double n = (double)Q2N_PIX, k = n / (n - 1.0);
    double x[4][N], z[4][N];   // pixel p = j * 256 + t of the block, row-major: row j * 8 + t / 32, column t % 32
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long o = (long)mirror(r0 + j * 8 + (t >> 5), H) * W + mirror(c0 + (t & 31), W);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            x[j][i] = i < C ? ld_scaled(g, i * HW + o, s) : 0.0;   // bands C .. N-1 are zero planes in both images
            z[j][i] = i < C ? ld_scaled(f, i * HW + o, s) : 0.0;
        }
    }
    // a = mean(x), c = sqrt(sum (x - a)^2 / (n - 1)) from the rounded mean; both images through the ground truth's map
    double a[N], c[N];
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = sum4(x[0][i], x[1][i], x[2][i], x[3][i]);
    block_tree<N>(a, red);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        a[i] = a[i] / n;
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j][i] = x[j][i] - a[i];
        c[i] = sum4(x[0][i] * x[0][i], x[1][i] * x[1][i], x[2][i] * x[2][i], x[3][i] * x[3][i]);
    }
    block_tree<N>(c, red);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double ci = sqrt(c[i] / (n - 1.0));
        if (ci == 0.0) ci = 1.0;             // a flat band keeps its scale
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[j][i] = x[j][i] / ci + 1.0;
            const double y = (z[j][i] - a[i]) / ci + 1.0;
            z[j][i] = i ? -y : y;
        }
    }
    // the block sums: m1 (N), m2 (N), P1, P2, u (N)
    double v[K3], sq1[4], sq2[4], pr[4][N];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sq1[j] = 0.0;
        sq2[j] = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            sq1[j] = sq1[j] + x[j][i] * x[j][i];
            sq2[j] = sq2[j] + z[j][i] * z[j][i];
        }
        HMul<N>::mul(x[j], z[j], pr[j]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        v[i] = sum4(x[0][i], x[1][i], x[2][i], x[3][i]);
        v[N + i] = sum4(z[0][i], z[1][i], z[2][i], z[3][i]);
        v[2 * N + 2 + i] = sum4(pr[0][i], pr[1][i], pr[2][i], pr[3][i]);
    }
    v[2 * N] = sum4(sq1[0], sq1[1], sq1[2], sq1[3]);
    v[2 * N + 1] = sum4(sq2[0], sq2[1], sq2[2], sq2[3]);
    block_tree<K3>(v, red);
    if (t != 0) return;
    double m1[N], m2[N], mm[N], M1 = 0.0, M2 = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        m1[i] = v[i] / n;
        m2[i] = v[N + i] / n;
        M1 = M1 + m1[i] * m1[i];
        M2 = M2 + m2[i] * m2[i];
    }
    const double P1 = v[2 * N] / n, P2 = v[2 * N + 1] / n;
    const double t3 = k * P1 + k * P2 - k * (M1 + M2);
    const double bias = 2.0 * sqrt(M1) * sqrt(M2) / (M1 + M2);
    double val;
    if (t3 == 0.0) {
        val = fabs(bias);
    } else {
        HMul<N>::mul(m1, m2, mm);
        const double cbm = 2.0 / t3;
        double ss = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double q = (k * (v[2 * N + 2 + i] / n) - k * mm[i]) * bias * cbm;
            ss = ss + q * q;
        }
        val = sqrt(ss);
    }
    vals[(long)b * gridDim.x + blk] = val;
}

// sum over the workgroup, valid in thread 0; every thread calls it (red: EXT_NT / 64 doubles of LDS, reused call after call)
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < EXT_NT / 64; ++i) t += red[i];
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// SCC: grid (tile, band, image).  part[b][band][tile][3] = sum FG, sum F^2, sum G^2 over the tile's interior pixels
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sobel_magnitude(const float* __restrict__ p, int W, float s) {   // p: the top-left neighbour
    const double x00 = ld_scaled(p, 0, s), x01 = ld_scaled(p, 1, s), x02 = ld_scaled(p, 2, s);
    const double x10 = ld_scaled(p, W, s), x12 = ld_scaled(p, W + 2, s);
    const double x20 = ld_scaled(p, 2 * W, s), x21 = ld_scaled(p, 2 * W + 1, s), x22 = ld_scaled(p, 2 * W + 2, s);
    const double gx = (x02 - x00) + 2.0 * (x12 - x10) + (x22 - x20);
    const double gy = (x20 - x00) + 2.0 * (x21 - x01) + (x22 - x02);
    return sqrt(gx * gx + gy * gy);
}

__global__ __launch_bounds__(EXT_NT) void k_iqa_scc(const float* __restrict__ gt, const float* __restrict__ fused, int H, int W, float s,
                                                   int tiles_x, double* __restrict__ part) {
    __shared__ double red[EXT_NT / 64];
    const int tile = blockIdx.x, band = blockIdx.y, b = blockIdx.z, C = gridDim.y;
    const int r = (tile / tiles_x) * SCC_TY + threadIdx.x / SCC_TX, c = (tile % tiles_x) * SCC_TX + threadIdx.x % SCC_TX;
    double fg = 0.0, ff = 0.0, gg = 0.0;
    if (r < H - 2 && c < W - 2) {            // interior pixel (r + 1, c + 1): its 3 x 3 neighbourhood is rows r .. r + 2, columns c .. c + 2
        const long o = ((long)b * C + band) * H * W + (long)r * W + c;
        const double F = sobel_magnitude(fused + o, W, s), G = sobel_magnitude(gt + o, W, s);
        fg = F * G;
        ff = F * F;
        gg = G * G;
    }
    double* out = part + (((long)b * C + band) * gridDim.x + tile) * 3;
    double t = block_sum(fg, red);
    if (threadIdx.x == 0) out[0] = t;
    t = block_sum(ff, red);
    if (threadIdx.x == 0) out[1] = t;
    t = block_sum(gg, red);
    if (threadIdx.x == 0) out[2] = t;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// CC: grid (band, image).  r[b][band] = Pearson's r of the band, NaN if the band is constant in either image
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(EXT_NT) void k_iqa_cc(const float* __restrict__ gt, const float* __restrict__ fused, int HW, float s,
                                                  double* __restrict__ r) {
    __shared__ double red[EXT_NT / 64];
    __shared__ double bc[6];   // mean x, mean y, min x, -max x, min y, -max y
    const int band = blockIdx.x, b = blockIdx.y, C = gridDim.x;
    const float* x = gt + ((long)b * C + band) * HW;
    const float* y = fused + ((long)b * C + band) * HW;
    double sx = 0.0, sy = 0.0, lox = DBL_MAX, hix = -DBL_MAX, loy = DBL_MAX, hiy = -DBL_MAX;
    for (int i = threadIdx.x; i < HW; i += EXT_NT) {
        const double u = ld_scaled(x, i, s), w = ld_scaled(y, i, s);
        sx += u;
        sy += w;
        lox = fmin(lox, u);
        hix = fmax(hix, u);
        loy = fmin(loy, w);
        hiy = fmax(hiy, w);
    }
    // minima and maxima over the workgroup as sums are: the wave, then the four waves by thread 0 (a maximum is minus the minimum of the negated values)
    double t = block_sum(sx, red);
    if (threadIdx.x == 0) bc[0] = t / HW;
    t = block_sum(sy, red);
    if (threadIdx.x == 0) bc[1] = t / HW;
    const double ext[4] = {lox, -hix, loy, -hiy};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double m = wave_min(ext[e]);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) bc[2 + e] = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    }
    __syncthreads();
    const double mx = bc[0], my = bc[1];
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int i = threadIdx.x; i < HW; i += EXT_NT) {
        const double u = ld_scaled(x, i, s) - mx, w = ld_scaled(y, i, s) - my;
        sxx += u * u;
        syy += w * w;
        sxy += u * w;
    }
    const double txx = block_sum(sxx, red), tyy = block_sum(syy, red), txy = block_sum(sxy, red);
    if (threadIdx.x == 0) {
        const bool flat = bc[2] == -bc[3] || bc[4] == -bc[5];      // min == max
        double v = txy / (sqrt(txx) * sqrt(tyy));
        v = v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v);                 // np.corrcoef clips to [-1, 1]
        r[(long)b * C + band] = flat ? (double)NAN : v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// finishing pass: one wave per image.  out[b * ostride] = Q2n; with scc / cc given, out[b * ostride + 1] = SCC and [+ 2] = CC
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_iqa_fin_ext(const double* __restrict__ vals, int nblk, const double* __restrict__ scc, int nscc,
                                                   const double* __restrict__ cc, int C, int ostride, double* __restrict__ out) {
    const int b = blockIdx.x;
    const double q = lanes_sum(vals + (long)b * nblk, nblk, 1) / nblk;
    double fg = 0.0, ff = 0.0, gg = 0.0;
    if (scc) {
        const double* p = scc + (long)b * nscc * 3;
        fg = lanes_sum(p, nscc, 3);
        ff = lanes_sum(p + 1, nscc, 3);
        gg = lanes_sum(p + 2, nscc, 3);
    }
    if (threadIdx.x != 0) return;
    double* o = out + (long)b * ostride;
    o[0] = q;
    if (!scc) return;
    o[1] = (ff == 0.0 || gg == 0.0) ? (ff == gg ? 1.0 : 0.0) : fg / sqrt(ff * gg);
    double r = 0.0;
    for (int c = 0; c < C; ++c) r += cc[(long)b * C + c];
    o[2] = r / C;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: geometry, workspace layout, validation
// ---------------------------------------------------------------------------------------------------------------------------------
struct ExtGeom {
    int blocks_x, nblk;       // Q2n blocks of the extended image
    int tiles_x, ntile;       // SCC tiles of the interior
    size_t off[3], bytes;     // workspace regions: block values | SCC partials | CC per band
};

// false: not a shape the indices are defined for (the reason is in lg_last_error)
bool ext_geom(const char* who, int B, int C, int H, int W, ExtGeom& g) {
    if (B < 1 || B > 65535) { lg_set_error("%s: B must be 1..65535 (got %d)", who, B); return false; }
    if (C < 2 || C > LG_IQA_Q2N_MAX_BANDS) { lg_set_error("%s: C must be 2..%d (Q2n has at most 8 components; got %d)", who, LG_IQA_Q2N_MAX_BANDS, C); return false; }
    if (H < LG_IQA_Q2N_BLOCK || W < LG_IQA_Q2N_BLOCK) { lg_set_error("%s: H and W must be >= %d (one Q2n block; got %d x %d)", who, LG_IQA_Q2N_BLOCK, H, W); return false; }
    if (H > 8192 || W > 8192) { lg_set_error("%s: H and W must be <= 8192 (got %d x %d)", who, H, W); return false; }
    g.blocks_x = (W + Q2N_BS - 1) / Q2N_BS;
    g.nblk = g.blocks_x * ((H + Q2N_BS - 1) / Q2N_BS);
    g.tiles_x = (W - 2 + SCC_TX - 1) / SCC_TX;
    g.ntile = g.tiles_x * ((H - 2 + SCC_TY - 1) / SCC_TY);
    const size_t d = sizeof(double);
    const size_t sz[3] = {ws_region(B, (size_t)g.nblk * d), ws_region(B, (size_t)C * g.ntile * 3 * d), ws_region(B, (size_t)C * d)};
    g.bytes = ws_layout(3, sz, g.off);
    return true;
}

bool ext_check_buffers(const char* who, bool ptrs_ok, float scale, void* workspace, size_t workspace_bytes, const ExtGeom& g) {
    if (!ptrs_ok || !workspace) { lg_set_error("%s: null pointer", who); return false; }
    if (!isfinite(scale)) { lg_set_error("%s: scale must be finite", who); return false; }
    if ((uintptr_t)workspace & 7) { lg_set_error("%s: workspace must be 8-byte aligned", who); return false; }
    if (workspace_bytes < g.bytes) { lg_set_error("%s: workspace too small: %zu bytes, need %zu", who, workspace_bytes, g.bytes); return false; }
    return true;
}

int launch_q2n(const float* gt, const float* fused, int B, int C, int H, int W, float scale, const ExtGeom& g, double* vals, hipStream_t s) {
    const dim3 grid(g.nblk, B);
    if (C <= 2) k_iqa_q2n<2><<<grid, EXT_NT, 0, s>>>(gt, fused, C, H, W, scale, g.blocks_x, vals);
    else if (C <= 4) k_iqa_q2n<4><<<grid, EXT_NT, 0, s>>>(gt, fused, C, H, W, scale, g.blocks_x, vals);
    else k_iqa_q2n<8><<<grid, EXT_NT, 0, s>>>(gt, fused, C, H, W, scale, g.blocks_x, vals);
    LG_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t lg_iqa_ext_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    ExtGeom g;
    return ext_geom("lg_iqa_ext_workspace_bytes", B, C, H, W, g) ? g.bytes : 0;
}

extern "C" int lg_iqa_ref_ext(const float* pred, const float* gt, double* out, int32_t B, int32_t C, int32_t H, int32_t W, float scale,
                              void* workspace, size_t workspace_bytes, void* stream) {
    ExtGeom g;
    if (!ext_geom("lg_iqa_ref_ext", B, C, H, W, g) || !ext_check_buffers("lg_iqa_ref_ext", pred && gt && out, scale, workspace, workspace_bytes, g))
        return -1;
    const hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double *vals = (double*)(ws + g.off[0]), *scc = (double*)(ws + g.off[1]), *cc = (double*)(ws + g.off[2]);
    if (launch_q2n(gt, pred, B, C, H, W, scale, g, vals, s)) return -1;
    k_iqa_scc<<<dim3(g.ntile, C, B), EXT_NT, 0, s>>>(gt, pred, H, W, scale, g.tiles_x, scc);
    LG_CHECK_LAUNCH();
    k_iqa_cc<<<dim3(C, B), EXT_NT, 0, s>>>(gt, pred, H * W, scale, cc);
    LG_CHECK_LAUNCH();
    k_iqa_fin_ext<<<B, 64, 0, s>>>(vals, g.nblk, scc, C * g.ntile, cc, C, 3, out);
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_iqa_q2n(const float* gt, const float* fused, double* out, int32_t B, int32_t C, int32_t H, int32_t W, float scale,
                          void* workspace, size_t workspace_bytes, void* stream) {
    ExtGeom g;
    if (!ext_geom("lg_iqa_q2n", B, C, H, W, g) || !ext_check_buffers("lg_iqa_q2n", gt && fused && out, scale, workspace, workspace_bytes, g)) return -1;
    const hipStream_t s = (hipStream_t)stream;
    double* vals = (double*)((char*)workspace + g.off[0]);
    if (launch_q2n(gt, fused, B, C, H, W, scale, g, vals, s)) return -1;
    k_iqa_fin_ext<<<B, 64, 0, s>>>(vals, g.nblk, nullptr, 0, nullptr, C, 1, out);
    LG_CHECK_LAUNCH();
    return 0;
}
