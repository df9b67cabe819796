// The no-reference training loss 1 - QNR and its gradient (C ABI: lg_qnr_stats / lg_qnr_grad, include/lgteun_hip.h; the reference's
// QNRLoss, models/base/losses.py:141-153, over D_lambda_torch / D_s_torch / QIndex_torch, models/base/metrics.py:336-397): Wang-Bovik Q
// over the WHOLE image of every sample, Alparone's D_lambda / D_s with p = q = 1, the batch entering through batch means of Q taken before
// the absolute value.
//
//   k_qnr_moments<C>  grid (gf + gm, B): the first gf workgroups of a sample stream out [b] and pan [b] (float4 loads, C + 1 of them in
//                     flight per lane), the last gm walk ms [b] and pan_l [b].  A lane keeps the M = C + C (C + 1) / 2 + C + 2 sums
//                     { x_i | x_i x_j, i <= j | x_i p | p, p p } in fp64 (the product of two fp32 values is exact there); the lanes of a
//                     wave meet by shuffles (reduce.h wave_sum), the four waves in an LDS slab of M columns -- one barrier for all M, where
//                     block_sum4 would take M -- and the workgroup writes ONE row of M partials.  gf and gm depend on
//                     H and W only, so a sample's Q values have the same bits in any batch.
//   k_qnr_finish<C>   one wave per sample: the partials in ascending workgroup order, Q of the P = C (C - 1) / 2 + C pairs on both sides
//                     and dQ / d(E[a], E[b], E[aa], E[bb], E[ab]) of the fused-side pairs -> workspace (and the caller's q)
//   k_qnr_table       table[p] = sum_n (Q_n,fused[p] - Q_n,ms[p]), n ascending
//   k_qnr_grad<C>     grid (gf, B): every workgroup derives D_lambda, D_s and the signs from the P table values (after the caller's
//                     all-reduce, if any) and its sample's alpha_i, beta_ij, gamma_i from the stored derivatives, then streams the
//                     sample: dout[i] = fl32(scale * (alpha_i + sum_j beta_ij x_j + gamma_i pan)), evaluated in fp64 and rounded once.
// No floating-point atomics: the same call gives the same bits every time (the convention that reduce.h implements).
#include "abi.h"
#include "common.h"
#include "reduce.h"

namespace {

constexpr int QNR_NT = 256;
constexpr int QNR_MAX_GF = 64;      // workgroups per sample on the fused side: ceil(H W / 1024), at most this
constexpr int QNR_MAX_GM = 8;       // ... and on the MS side: ceil(h w / 1024), at most this
constexpr double QNR_EPS = 1e-8;    // QIndex_torch's eps

template <int C>
struct QnrDims {
    static constexpr int PL = C * (C - 1) / 2;       // band pairs i < j, row-major
    static constexpr int NP = PL + C;                // ... then the C band-to-PAN pairs: the table
    static constexpr int NXX = C * (C + 1) / 2;      // products x_i x_j, i <= j, row-major
    static constexpr int M = C + NXX + C + 2;        // moments of one side
    static constexpr int XX0 = C, XP0 = C + NXX, SP = C + NXX + C, SPP = C + NXX + C + 1;
};
__host__ __device__ constexpr int qnr_np(int C) { return C * (C - 1) / 2 + C; }
__host__ __device__ constexpr int qnr_m(int C) { return C + C * (C + 1) / 2 + C + 2; }
__device__ __forceinline__ constexpr int qnr_xx(int C, int i, int j) { return i * C - i * (i - 1) / 2 + (j - i); }      // i <= j
__device__ __forceinline__ constexpr int qnr_pair(int C, int i, int j) { return i * C - i * (i + 1) / 2 + (j - i - 1); }  // i < j

template <int C>
__device__ __forceinline__ void qnr_accum(double (&acc)[QnrDims<C>::M], const float (&x)[C], float p) {
    double xd[C];
    const double pd = (double)p;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        xd[i] = (double)x[i];
        acc[i] += xd[i];
    }
    int k = C;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
        for (int j = i; j < C; ++j) acc[k++] += xd[i] * xd[j];
#pragma unroll
    for (int i = 0; i < C; ++i) acc[k++] += xd[i] * pd;
    acc[k++] += pd;
    acc[k] += pd * pd;
}

// part_f [B][gf][M], part_m [B][gm][M]
template <int C>
__global__ __launch_bounds__(QNR_NT) void k_qnr_moments(const float* __restrict__ out, const float* __restrict__ pan,
                                                        const float* __restrict__ ms, const float* __restrict__ pan_l, long HW, long hw,
                                                        int gf, int gm, double* __restrict__ part_f, double* __restrict__ part_m) {
    constexpr int M = QnrDims<C>::M;
    __shared__ double sm[QNR_NT / 64][M];
    const long b = blockIdx.y;
    double acc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m] = 0.0;
    double* dst;
    if ((int)blockIdx.x < gf) {
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(out + b * C * HW);
        const float4* __restrict__ p4 = reinterpret_cast<const float4*>(pan + b * HW);
        const long nv = HW >> 2, stride = (long)gf * QNR_NT;
        for (long v = (long)blockIdx.x * QNR_NT + threadIdx.x; v < nv; v += stride) {
            float4 a[C];
#pragma unroll
            for (int i = 0; i < C; ++i) a[i] = x4[i * nv + v];
            const float4 p = p4[v];
            float x[C];
#pragma unroll
            for (int i = 0; i < C; ++i) x[i] = a[i].x;
            qnr_accum<C>(acc, x, p.x);
#pragma unroll
            for (int i = 0; i < C; ++i) x[i] = a[i].y;
            qnr_accum<C>(acc, x, p.y);
#pragma unroll
            for (int i = 0; i < C; ++i) x[i] = a[i].z;
            qnr_accum<C>(acc, x, p.z);
#pragma unroll
            for (int i = 0; i < C; ++i) x[i] = a[i].w;
            qnr_accum<C>(acc, x, p.w);
        }
        dst = part_f + (b * gf + blockIdx.x) * M;
    } else {
        // MS side: h w need not be a multiple of 4, so a sample's planes need not be 16-byte aligned -- scalar loads
        const int g = (int)blockIdx.x - gf;
        const float* __restrict__ xs = ms + b * C * hw;
        const float* __restrict__ ps = pan_l + b * hw;
        const long stride = (long)gm * QNR_NT;
        for (long v = (long)g * QNR_NT + threadIdx.x; v < hw; v += stride) {
            float x[C];
#pragma unroll
            for (int i = 0; i < C; ++i) x[i] = xs[i * hw + v];
            qnr_accum<C>(acc, x, ps[v]);
        }
        dst = part_m + (b * gm + g) * M;
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const double t = wave_sum(acc[m]);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][m] = t;
    }
    __syncthreads();
    if (threadIdx.x < M) dst[threadIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

// the five means of pair p of one side, from that side's M means
template <int C>
__device__ __forceinline__ void qnr_pair_means(const double* mom, int p, double& ea, double& eb, double& eaa, double& ebb, double& eab) {
    using D = QnrDims<C>;
    if (p < D::PL) {
        int i = 0, q = p;
        while (q >= C - 1 - i) { q -= C - 1 - i; ++i; }
        const int j = i + 1 + q;
        ea = mom[i];
        eb = mom[j];
        eaa = mom[D::XX0 + qnr_xx(C, i, i)];
        ebb = mom[D::XX0 + qnr_xx(C, j, j)];
        eab = mom[D::XX0 + qnr_xx(C, i, j)];
    } else {
        const int i = p - D::PL;
        ea = mom[i];
        eb = mom[D::SP];
        eaa = mom[D::XX0 + qnr_xx(C, i, i)];
        ebb = mom[D::SPP];
        eab = mom[D::XP0 + i];
    }
}

// qd [B][7][NP]: Q fused, Q ms, then dQ_fused / d(E[a], E[b], E[aa], E[bb], E[ab])
template <int C>
__global__ __launch_bounds__(64) void k_qnr_finish(const double* __restrict__ part_f, const double* __restrict__ part_m, int gf, int gm,
                                                   double n_f, double n_m, double* __restrict__ qd, double* __restrict__ q_out) {
    using D = QnrDims<C>;
    static_assert(D::M <= 64 && D::NP <= 64, "one wave finishes a sample");
    __shared__ double mf[D::M], mm[D::M];
    const long b = blockIdx.x;
    const int t = threadIdx.x;
    if (t < D::M) {
        double s = 0.0;
        for (int g = 0; g < gf; ++g) s += part_f[(b * gf + g) * D::M + t];
        mf[t] = s / n_f;
        s = 0.0;
        for (int g = 0; g < gm; ++g) s += part_m[(b * gm + g) * D::M + t];
        mm[t] = s / n_m;
    }
    __syncthreads();
    if (t >= D::NP) return;
    double* o = qd + b * 7 * D::NP + t;
    double ea, eb, eaa, ebb, eab;
    {
        qnr_pair_means<C>(mm, t, ea, eb, eaa, ebb, eab);
        const double cov = eab - ea * eb, V = (eaa - ea * ea) + (ebb - eb * eb), E2 = ea * ea + eb * eb;
        const double Q = 4.0 * cov * ea * eb / (V * E2 + QNR_EPS);
        o[D::NP] = Q;
        if (q_out) q_out[(b * 2 + 1) * D::NP + t] = Q;
    }
    qnr_pair_means<C>(mf, t, ea, eb, eaa, ebb, eab);
    const double cov = eab - ea * eb, V = (eaa - ea * ea) + (ebb - eb * eb), E2 = ea * ea + eb * eb;
    const double den = V * E2 + QNR_EPS;
    const double Q = 4.0 * cov * ea * eb / den;
    o[0] = Q;
    if (q_out) q_out[(b * 2) * D::NP + t] = Q;
    // Q = N / den with N = 4 cov E[a] E[b]: dQ = (dN - Q d(den)) / den
    o[2 * D::NP] = (4.0 * eb * (cov - ea * eb) - Q * 2.0 * ea * (V - E2)) / den;
    o[3 * D::NP] = (4.0 * ea * (cov - ea * eb) - Q * 2.0 * eb * (V - E2)) / den;
    o[4 * D::NP] = -Q * E2 / den;
    o[5 * D::NP] = -Q * E2 / den;
    o[6 * D::NP] = 4.0 * ea * eb / den;
}

__global__ __launch_bounds__(64) void k_qnr_table(const double* __restrict__ qd, int B, int np, double* __restrict__ table) {
    const int t = threadIdx.x;
    if (t >= np) return;
    double s = 0.0;
    for (long n = 0; n < B; ++n) s += qd[n * 7 * np + t] - qd[n * 7 * np + np + t];
    table[t] = s;
}

template <int C>
__global__ __launch_bounds__(QNR_NT) void k_qnr_grad(const float* __restrict__ out, const float* __restrict__ pan,
                                                     const double* __restrict__ table, const double* __restrict__ qd,
                                                     float* __restrict__ dout, float* loss_accum, double* __restrict__ indices, int B,
                                                     double b_global, long HW, int gf, double scale, int accumulate) {
    using D = QnrDims<C>;
    __shared__ double sd[D::NP];             // table / B_global, then the weight of Q_n[p] in the loss
    __shared__ double coef[C][C + 2];        // alpha_i | beta_i0 .. beta_i,C-1 | gamma_i
    const long b = blockIdx.y;
    const int t = threadIdx.x;
    if (t < D::NP) sd[t] = table[t] / b_global;
    __syncthreads();
    double dl = 0.0, ds = 0.0;
    for (int p = 0; p < D::PL; ++p) dl += fabs(sd[p]);
    for (int p = D::PL; p < D::NP; ++p) ds += fabs(sd[p]);
    dl /= (double)D::PL;
    ds /= (double)C;
    const double loss = 1.0 - (1.0 - dl) * (1.0 - ds);
    __syncthreads();
    if (t < D::NP) {
        const double d = sd[t];
        const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);      // torch.abs differentiates to sign(0) = 0
        sd[t] = sg * (t < D::PL ? (1.0 - ds) / ((double)D::PL * b_global) : (1.0 - dl) / ((double)C * b_global));
    }
    __syncthreads();
    if (t < C) {
        const int i = t;
        const double* dq = qd + b * 7 * D::NP + 2 * D::NP;      // [5][NP]
        double alpha = 0.0, bii = 0.0;
        for (int j = 0; j < C; ++j) {
            if (j == i) continue;
            const int p = i < j ? qnr_pair(C, i, j) : qnr_pair(C, j, i);
            const double w = sd[p];
            alpha += w * dq[(i < j ? 0 : 1) * D::NP + p];
            bii += w * dq[(i < j ? 2 : 3) * D::NP + p];
            coef[i][1 + j] = w * dq[4 * D::NP + p] / (double)HW;
        }
        const int p = D::PL + i;
        const double w = sd[p];
        alpha += w * dq[p];
        bii += w * dq[2 * D::NP + p];
        coef[i][0] = alpha / (double)HW;
        coef[i][1 + i] = 2.0 * bii / (double)HW;
        coef[i][C + 1] = w * dq[4 * D::NP + p] / (double)HW;
    }
    __syncthreads();
    double k[C][C + 2];
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
        for (int j = 0; j < C + 2; ++j) k[i][j] = coef[i][j];
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(out + b * C * HW);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(pan + b * HW);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dout + b * C * HW);
    const long nv = HW >> 2, stride = (long)gf * QNR_NT;
    for (long v = (long)blockIdx.x * QNR_NT + t; v < nv; v += stride) {
        float4 a[C];
#pragma unroll
        for (int i = 0; i < C; ++i) a[i] = x4[i * nv + v];
        const float4 p = p4[v];
        const float pv[4] = {p.x, p.y, p.z, p.w};
        float r[C][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double x[C];
#pragma unroll
            for (int j = 0; j < C; ++j) x[j] = (double)(c == 0 ? a[j].x : (c == 1 ? a[j].y : (c == 2 ? a[j].z : a[j].w)));
            const double pd = (double)pv[c];
#pragma unroll
            for (int i = 0; i < C; ++i) {
                double g = k[i][0];
#pragma unroll
                for (int j = 0; j < C; ++j) g += k[i][1 + j] * x[j];
                g += k[i][C + 1] * pd;
                r[i][c] = (float)(scale * g);      // the one rounding to fp32
            }
        }
#pragma unroll
        for (int i = 0; i < C; ++i) {
            float4 o = make_float4(r[i][0], r[i][1], r[i][2], r[i][3]);
            if (accumulate) {
                const float4 old = d4[i * nv + v];
                o = make_float4(old.x + o.x, old.y + o.y, old.z + o.z, old.w + o.w);
            }
            d4[i * nv + v] = o;
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
        loss_accum[0] += (float)(loss * (double)B / b_global);      // this rank's share of the global batch; a plain read-add-write
        if (indices) {
            indices[0] = dl;
            indices[1] = ds;
            indices[2] = loss;
        }
    }
}

struct QnrGeom {
    int gf, gm, np, m;
    long HW, hw;
    size_t off[3];      // part_f | part_m | qd
    size_t bytes;
};

// false: not a shape the calls take (the reason, naming the argument, is in lg_last_error)
bool qnr_geom(const char* who, int B, int C, int H, int W, QnrGeom& g) {
    if (!check_shape(who, B, C, H, W)) return false;
    if (H < 8 || W < 8 || H % 4 || W % 4) { lg_set_error("%s: H and W must be multiples of 4 and at least 8 (got %d x %d)", who, H, W); return false; }
    g.HW = (long)H * W;
    g.hw = g.HW / 16;
    const long f = (g.HW + 1023) / 1024, m = (g.hw + 1023) / 1024;
    g.gf = (int)(f < QNR_MAX_GF ? f : QNR_MAX_GF);
    g.gm = (int)(m < QNR_MAX_GM ? m : QNR_MAX_GM);
    g.np = qnr_np(C);
    g.m = qnr_m(C);
    const size_t sz[3] = {ws_region(B, (size_t)g.gf * g.m * sizeof(double)), ws_region(B, (size_t)g.gm * g.m * sizeof(double)),
                          ws_region(B, (size_t)7 * g.np * sizeof(double))};
    g.bytes = ws_layout(3, sz, g.off);
    return true;
}

}  // namespace

extern "C" size_t lg_qnr_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    QnrGeom g;
    return qnr_geom("qnr_workspace_bytes", B, C, H, W, g) ? g.bytes : 0;
}

extern "C" int lg_qnr_stats(const float* out, const float* pan, const float* ms, const float* pan_l, double* q, double* table, int32_t B,
                            int32_t C, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "qnr_stats";
    QnrGeom g;
    if (!qnr_geom(who, B, C, H, W, g)) return -1;
    if (!check_tensors(who, {{"out", out}, {"pan", pan}, {"ms", ms}, {"pan_l", pan_l}})) return -1;
    if (!table) { lg_set_error("%s: table is NULL", who); return -1; }
    if (((uintptr_t)table | (uintptr_t)q) & 7) { lg_set_error("%s: q and table must be 8-byte aligned", who); return -1; }
    if (!check_workspace(who, workspace, workspace_bytes, g.bytes, "lg_qnr_workspace_bytes")) return -1;
    char* ws = (char*)workspace;
    double *pf = (double*)(ws + g.off[0]), *pm = (double*)(ws + g.off[1]), *qd = (double*)(ws + g.off[2]);
    const dim3 grid(g.gf + g.gm, B);
    const hipStream_t s = (hipStream_t)stream;
    if (C == 4) {
        k_qnr_moments<4><<<grid, QNR_NT, 0, s>>>(out, pan, ms, pan_l, g.HW, g.hw, g.gf, g.gm, pf, pm);
        LG_CHECK_LAUNCH();
        k_qnr_finish<4><<<B, 64, 0, s>>>(pf, pm, g.gf, g.gm, (double)g.HW, (double)g.hw, qd, q);
    } else {
        k_qnr_moments<8><<<grid, QNR_NT, 0, s>>>(out, pan, ms, pan_l, g.HW, g.hw, g.gf, g.gm, pf, pm);
        LG_CHECK_LAUNCH();
        k_qnr_finish<8><<<B, 64, 0, s>>>(pf, pm, g.gf, g.gm, (double)g.HW, (double)g.hw, qd, q);
    }
    LG_CHECK_LAUNCH();
    k_qnr_table<<<1, 64, 0, s>>>(qd, B, g.np, table);
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_qnr_grad(const float* out, const float* pan, const double* table, float* dout, float* loss_accum, double* indices, int32_t B,
                           int64_t B_global, int32_t C, int32_t H, int32_t W, float scale, int32_t accumulate, const void* workspace,
                           size_t workspace_bytes, void* stream) {
    static const char* who = "qnr_grad";
    QnrGeom g;
    if (!qnr_geom(who, B, C, H, W, g)) return -1;
    if (!check_tensors(who, {{"out", out}, {"pan", pan}, {"dout", dout}})) return -1;
    if (!table) { lg_set_error("%s: table is NULL", who); return -1; }
    if (((uintptr_t)table | (uintptr_t)indices) & 7) { lg_set_error("%s: table and indices must be 8-byte aligned", who); return -1; }
    if (!check_loss_args(who, loss_accum, B, B_global, scale, accumulate)) return -1;
    if (!check_workspace(who, workspace, workspace_bytes, g.bytes, "lg_qnr_workspace_bytes")) return -1;
    const double* qd = (const double*)((const char*)workspace + g.off[2]);
    const dim3 grid(g.gf, B);
    const hipStream_t s = (hipStream_t)stream;
    if (C == 4)
        k_qnr_grad<4><<<grid, QNR_NT, 0, s>>>(out, pan, table, qd, dout, loss_accum, indices, B, (double)B_global, g.HW, g.gf, (double)scale, accumulate);
    else
        k_qnr_grad<8><<<grid, QNR_NT, 0, s>>>(out, pan, table, qd, dout, loss_accum, indices, B, (double)B_global, g.HW, g.gf, (double)scale, accumulate);
    LG_CHECK_LAUNCH();
    return 0;
}
