// The training losses against a target and their gradients: l1 / l2 over a flat range, the spectral (SAM) and the structural (1 - SSIM)
// loss per sample (C ABI: lg_l1_loss / lg_l2_loss / lg_sam_loss / lg_ssim_loss, include/lgteun_hip.h; SAM and SSIM are those of
// lgteun_amd/metrics.py `sam` and `_ssim_band`, restated with their gradients in lgteun_amd/losses.py SAMLoss / SSIMLoss).
//
//   k_sam_loss<C>     grid (gx, B): one streaming pass over a sample, float4 loads along W with the C band planes of out and gt of a pixel
//                     quad in flight together.  Per pixel in fp64: o^ = o / |o|, g^ = g / |g|, c = <o^, g^>, u = g^ - c o^, s = |u|,
//                     theta = atan2(s, c), d theta / d o = -u / (s |o|) -- acos is never differentiated.  A pixel with c <= 0 or a zero
//                     vector counts pi / 2 and has no gradient; one with s < 1e-6 counts its theta and has no gradient.  dout is rounded to
//                     fp32 once.  The workgroup writes ONE fp64 partial of its angles.
//   k_ssim_loss       grid (tile, band, image), 16 x 16 pixels of dout per workgroup, all arithmetic in fp64, the maps in LDS: the x and y tile with a
//                     10-pixel halo (36 x 36), the column pass of the five moment maps (26 x 36), the row pass and, pointwise, S and
//                     dS / d(m1, m2, m3) at the 26 x 26 window positions whose windows touch the tile (zero where a window is not fully
//                     inside the image), the transposed row pass (26 x 16) and the transposed column pass, which ends in
//                     dout = fl32(k (T(d1) + 2 x T(d2) + y T(d3))).  The workgroup writes ONE fp64 partial: the sum of S over the windows
//                     whose top-left pixel lies in its tile.  The staged tile stays fp32 (it is fp32 data); 64,032 bytes of LDS: two
//                     workgroups per CU.
//   k_recloss_finish  one workgroup: the partials in a fixed order (reduce.h partials_sum), one float read-add-write into loss_accum.
//   k_l1 / k_l2       at the end of the file, with their own comments: one streaming body (rl_stream_diff), two element functors.
// SAM and SSIM use no atomics (reduce.h): the same call gives the same bits.  A workgroup sees one sample only and the grid of a sample
// depends on H and W only, so a sample's dout has the same bits alone and inside any batch.  k_l1 / k_l2 end in atomics, as their comments say.
#include <cmath>

#include "abi.h"
#include "common.h"
#include "reduce.h"
#include "net_args.h"

namespace {

constexpr int RL_NT = 256;                       // block_sum4 and partials_sum (reduce.h) are written for this
constexpr int SAM_MAX_GX = 64;                    // workgroups per sample of the SAM pass: ceil(H W / 1024), at most this
constexpr double SAM_MIN_S = 1e-6;                // below this |u| is rounding noise: the direction of the gradient is undefined
constexpr double RL_HALF_PI = 1.57079632679489661923;

constexpr int SS_N = 11;                          // taps of the window (metrics.SSIM_TAPS)
constexpr int SS_T = 16;                          // dout pixels per tile side
constexpr int SS_IN = SS_T + 2 * (SS_N - 1);      // 36: staged rows / columns
constexpr int SS_WN = SS_T + SS_N - 1;            // 26: window positions per side whose windows touch the tile
constexpr int SS_STAGE = (SS_IN * SS_IN + RL_NT - 1) / RL_NT;      // staged pixels per thread
constexpr int SS_LDS_DOUBLES = 5 * SS_WN * SS_IN + 3 * SS_WN * SS_WN;
constexpr int SS_LDS_BYTES = SS_LDS_DOUBLES * (int)sizeof(double) + 2 * SS_IN * SS_IN * (int)sizeof(float);
static_assert(SS_T * SS_T == RL_NT, "one dout pixel per thread in the last pass");
static_assert(3 * SS_WN * SS_T <= 5 * SS_WN * SS_IN, "the transposed row pass reuses the column pass's maps");
static_assert(2 * (SS_LDS_BYTES + 64) <= 160 * 1024, "two workgroups per CU");

struct SsimTaps {
    double w[SS_N];
};

__device__ __forceinline__ float rl_lane(const float4& v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

// part [B][gx]; k = scale / (B_global H W)
template <int C>
__global__ __launch_bounds__(RL_NT) void k_sam_loss(const float* __restrict__ out, const float* __restrict__ gt, float* __restrict__ dout,
                                                    double* __restrict__ part, long HW, int gx, double k, int accumulate) {
    __shared__ double red[RL_NT / 64];
    const long b = blockIdx.y;
    const float4* __restrict__ o4 = reinterpret_cast<const float4*>(out + b * C * HW);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(gt + b * C * HW);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dout + b * C * HW);
    const long nv = HW >> 2, stride = (long)gx * RL_NT;
    double acc = 0.0;
    for (long v = (long)blockIdx.x * RL_NT + threadIdx.x; v < nv; v += stride) {
        float4 o[C], g[C];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            o[i] = o4[i * nv + v];
            g[i] = g4[i * nv + v];
        }
        float r[C][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double od[C], gd[C], no2 = 0.0, ng2 = 0.0;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                od[i] = (double)rl_lane(o[i], c);
                gd[i] = (double)rl_lane(g[i], c);
                no2 += od[i] * od[i];
                ng2 += gd[i] * gd[i];
                r[i][c] = 0.f;
            }
            double theta = RL_HALF_PI;
            if (no2 > 0.0 && ng2 > 0.0) {
                const double no = sqrt(no2), ino = 1.0 / no, ing = 1.0 / sqrt(ng2);
                double cs = 0.0;
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    od[i] *= ino;
                    gd[i] *= ing;
                    cs += od[i] * gd[i];
                }
                if (cs > 0.0) {
                    double s2 = 0.0;
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        gd[i] -= cs * od[i];      // u
                        s2 += gd[i] * gd[i];
                    }
                    const double s = sqrt(s2);
                    theta = atan2(s, cs);
                    if (s >= SAM_MIN_S) {
                        const double f = -k / (s * no);
#pragma unroll
                        for (int i = 0; i < C; ++i) r[i][c] = (float)(f * gd[i]);      // the one rounding to fp32
                    }
                }
            }
            acc += theta;
        }
#pragma unroll
        for (int i = 0; i < C; ++i) {
            float4 w = make_float4(r[i][0], r[i][1], r[i][2], r[i][3]);
            if (accumulate) {
                const float4 old = d4[i * nv + v];
                w = make_float4(old.x + w.x, old.y + w.y, old.z + w.z, old.w + w.w);
            }
            d4[i * nv + v] = w;
        }
    }
    const double t = block_sum4(acc, red);
    if (threadIdx.x == 0) part[b * gx + blockIdx.x] = t;
}

// part [B][C][tiles]; k = -scale / (B_global C windows per plane)
__global__ __launch_bounds__(RL_NT) void k_ssim_loss(const float* __restrict__ out, const float* __restrict__ gt, float* __restrict__ dout,
                                                     double* __restrict__ part, int C, int H, int W, int tiles_x, SsimTaps taps, double c1,
                                                     double c2, double k, int accumulate) {
    extern __shared__ double ss_lds[];
    __shared__ double red[RL_NT / 64];
    double* V = ss_lds;                       // [5][26][36] column sums of x, y, xx, yy, xy; later E [3][26][16]
    double* D = V + 5 * SS_WN * SS_IN;        // [3][26][26] dS / d(m1, m2, m3), window (wi, wj) = image window (r0 - 10 + wi, c0 - 10 + wj)
    double* E = V;
    float* X = reinterpret_cast<float*>(D + 3 * SS_WN * SS_WN);      // [36][36], staged pixel (i, j) = image pixel (r0 - 10 + i, c0 - 10 + j)
    float* Y = X + SS_IN * SS_IN;
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int r0 = (tile / tiles_x) * SS_T, c0 = (tile % tiles_x) * SS_T;
    const long plane = ((long)blockIdx.z * C + blockIdx.y) * ((long)H * W);
    const float* __restrict__ x = out + plane;
    const float* __restrict__ y = gt + plane;
    // what lies outside the image feeds only windows that are not fully inside it: any finite value does
    // every load of the thread is issued before the first store waits for one
    float sx[SS_STAGE], sy[SS_STAGE];
#pragma unroll
    for (int u = 0; u < SS_STAGE; ++u) {
        const int i = tid + u * RL_NT, r = i / SS_IN, c = i - r * SS_IN, gr = r0 - (SS_N - 1) + r, gc = c0 - (SS_N - 1) + c;
        sx[u] = sy[u] = 0.f;
        if (i < SS_IN * SS_IN && gr >= 0 && gr < H && gc >= 0 && gc < W) {
            const long o = (long)gr * W + gc;
            sx[u] = x[o];
            sy[u] = y[o];
        }
    }
#pragma unroll
    for (int u = 0; u < SS_STAGE; ++u) {
        const int i = tid + u * RL_NT;
        if (i < SS_IN * SS_IN) {
            X[i] = sx[u];
            Y[i] = sy[u];
        }
    }
    __syncthreads();
    // column pass: window row wi covers the staged rows wi .. wi + 10
    for (int i = tid; i < SS_WN * SS_IN; i += RL_NT) {
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int t = 0; t < SS_N; ++t) {
            const double a = (double)X[i + t * SS_IN], b = (double)Y[i + t * SS_IN], w = taps.w[t];
            m0 += w * a;
            m1 += w * b;
            m2 += w * (a * a);
            m3 += w * (b * b);
            m4 += w * (a * b);
        }
        V[i] = m0;
        V[SS_WN * SS_IN + i] = m1;
        V[2 * SS_WN * SS_IN + i] = m2;
        V[3 * SS_WN * SS_IN + i] = m3;
        V[4 * SS_WN * SS_IN + i] = m4;
    }
    __syncthreads();
    // row pass, then S and its derivatives at the window positions
    double ssum = 0.0;
    for (int i = tid; i < SS_WN * SS_WN; i += RL_NT) {
        const int wi = i / SS_WN, wj = i - wi * SS_WN, gi = r0 - (SS_N - 1) + wi, gj = c0 - (SS_N - 1) + wj;
        double d1 = 0.0, d2 = 0.0, d3 = 0.0;
        if (gi >= 0 && gi <= H - SS_N && gj >= 0 && gj <= W - SS_N) {
            const double* v = V + wi * SS_IN + wj;
            double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
            for (int t = 0; t < SS_N; ++t) {
                const double w = taps.w[t];
                mx += w * v[t];
                my += w * v[SS_WN * SS_IN + t];
                exx += w * v[2 * SS_WN * SS_IN + t];
                eyy += w * v[3 * SS_WN * SS_IN + t];
                exy += w * v[4 * SS_WN * SS_IN + t];
            }
            const double A1 = 2.0 * mx * my + c1, B1 = mx * mx + my * my + c1;
            const double A2 = 2.0 * (exy - mx * my) + c2, B2 = (exx - mx * mx) + (eyy - my * my) + c2;
            // one division: 1 / B1 = B2 ib and 1 / B2 = B1 ib.  None by A2: it can be <= 0
            const double ib = 1.0 / (B1 * B2), S = A1 * A2 * ib;
            d3 = 2.0 * A1 * ib;
            d2 = -S * (B1 * ib);
            d1 = 2.0 * my * (A2 - A1) * ib + 2.0 * mx * S * ((B1 - B2) * ib);
            if (wi >= SS_N - 1 && wj >= SS_N - 1) ssum += S;      // the window's top-left pixel lies in this tile
        }
        D[i] = d1;
        D[SS_WN * SS_WN + i] = d2;
        D[2 * SS_WN * SS_WN + i] = d3;
    }
    __syncthreads();
    // transposed row pass: pixel column c of the tile collects the windows wj = c + 10 - t
    for (int i = tid; i < SS_WN * SS_T; i += RL_NT) {
        const int wi = i / SS_T, c = i - wi * SS_T;
        const double* d = D + wi * SS_WN + c + (SS_N - 1);
        double e1 = 0.0, e2 = 0.0, e3 = 0.0;
#pragma unroll
        for (int t = 0; t < SS_N; ++t) {
            const double w = taps.w[t];
            e1 += w * d[-t];
            e2 += w * d[SS_WN * SS_WN - t];
            e3 += w * d[2 * SS_WN * SS_WN - t];
        }
        E[i] = e1;
        E[SS_WN * SS_T + i] = e2;
        E[2 * SS_WN * SS_T + i] = e3;
    }
    __syncthreads();
    // transposed column pass: pixel row r collects the window rows wi = r + 10 - t
    {
        const int r = tid / SS_T, c = tid - r * SS_T, gr = r0 + r, gc = c0 + c;
        if (gr < H && gc < W) {
            const double* e = E + (r + SS_N - 1) * SS_T + c;
            double t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
            for (int t = 0; t < SS_N; ++t) {
                const double w = taps.w[t];
                t1 += w * e[-t * SS_T];
                t2 += w * e[SS_WN * SS_T - t * SS_T];
                t3 += w * e[2 * SS_WN * SS_T - t * SS_T];
            }
            const int o = (r + SS_N - 1) * SS_IN + c + SS_N - 1;
            const float g = (float)(k * (t1 + 2.0 * (double)X[o] * t2 + (double)Y[o] * t3));      // the one rounding to fp32
            float* dst = dout + plane + (long)gr * W + gc;
            *dst = accumulate ? *dst + g : g;
        }
    }
    const double t = block_sum4(ssum, red);
    if (tid == 0) part[((long)blockIdx.z * C + blockIdx.y) * gridDim.x + tile] = t;
}

// loss_accum[0] += (float)((offset + sum_j part[j]) * mul), one workgroup, the partials in the fixed order of partials_sum
__global__ __launch_bounds__(RL_NT) void k_recloss_finish(const double* __restrict__ part, long n, double offset, double mul, float* loss_accum) {
    __shared__ double red[RL_NT / 64];
    const double v = partials_sum(part, n, red);
    if (threadIdx.x == 0) loss_accum[0] += (float)((offset + v) * mul);
}

struct RlGeom {
    long HW;
    int gx;                     // SAM: workgroups per sample
    int tiles_x, tiles;         // SSIM: tiles per plane; 0 when a side is below the window
    size_t sam_bytes, ssim_bytes;
};

// false: not a shape the calls take (the reason, naming the argument, is in lg_last_error)
bool rl_geom(const char* who, int B, int C, int H, int W, RlGeom& g) {
    if (!check_shape(who, B, C, H, W)) return false;
    if (H < 1 || W < 4 || W % 4) { lg_set_error("%s: W must be a multiple of 4 and H at least 1 (got %d x %d)", who, H, W); return false; }
    g.HW = (long)H * W;
    const long f = (g.HW + 1023) / 1024;
    g.gx = (int)(f < SAM_MAX_GX ? f : SAM_MAX_GX);
    g.sam_bytes = align256((size_t)B * g.gx * sizeof(double));
    g.tiles_x = g.tiles = 0;
    g.ssim_bytes = 0;
    if (H >= SS_N && W >= SS_N) {
        g.tiles_x = (W + SS_T - 1) / SS_T;
        g.tiles = g.tiles_x * ((H + SS_T - 1) / SS_T);
        g.ssim_bytes = align256((size_t)B * C * g.tiles * sizeof(double));
    }
    return true;
}

bool rl_check_args(const char* who, const float* out, const float* gt, const float* dout, const float* loss_accum, int B, int64_t B_global,
                   float scale, int accumulate, const void* workspace, size_t workspace_bytes, size_t need) {
    return check_tensors(who, {{"out", out}, {"gt", gt}, {"dout", dout}}) && check_loss_args(who, loss_accum, B, B_global, scale, accumulate) &&
           check_workspace(who, workspace, workspace_bytes, need, "lg_recloss_workspace_bytes");
}

// The streaming body of k_l1 / k_l2 over a flat range of n floats: dout[i] = one(out[i] - gt[i]).  16-byte accesses, four of them in flight
// per thread, then the float4 tail and the scalar tail.  `one` also gathers the thread's share of the loss.
template <class F>
__device__ __forceinline__ void rl_stream_diff(const float* __restrict__ out, const float* __restrict__ gt, float* __restrict__ dout, long n, F one) {
    const long n4 = n >> 2, stride = (long)gridDim.x * 256L;
    const float4* __restrict__ o4 = reinterpret_cast<const float4*>(out);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(gt);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dout);
    long i = blockIdx.x * 256L + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = o4[i + u * stride]; b[u] = g4[i + u * stride]; }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            d4[i + u * stride] = make_float4(one(a[u].x - b[u].x), one(a[u].y - b[u].y), one(a[u].z - b[u].z), one(a[u].w - b[u].w));
    }
    for (; i < n4; i += stride) {
        const float4 a = o4[i], b = g4[i];
        d4[i] = make_float4(one(a.x - b.x), one(a.y - b.y), one(a.z - b.z), one(a.w - b.w));
    }
    for (long j = 4 * n4 + blockIdx.x * 256L + threadIdx.x; j < n; j += stride) dout[j] = one(out[j] - gt[j]);
}

// what lg_l1_loss / lg_l2_loss check; the grid of k_l1 / k_l2, 0 when an argument is not taken
int rl_flat_grid(const char* who, const float* out, const float* gt, const float* dout, const float* loss_accum, int64_t n_local, int64_t n_global) {
    // at most 256 workgroups, every index in long (k_l1, k_l2): no bound on n_local beyond int64
    NetArgs v(who);
    v.f32(out, "out").f32(gt, "gt").f32(dout, "dout").ptr(loss_accum, "loss_accum").aligned(loss_accum, "loss_accum", 4);
    if (!v.rc && n_local <= 0) v.fail(-1, "n_local must be positive (got %lld)", (long long)n_local);
    if (!v.rc && n_global <= 0) v.fail(-1, "n_global must be positive (got %lld)", (long long)n_global);
    if (v.rc) return 0;
    const int64_t grid = (n_local / 4 + 255) / 256;
    return (int)(grid > 256 ? 256 : (grid < 1 ? 1 : grid));
}

}  // namespace

// L1 loss (mean) forward + backward -- models/base/losses.py:19-40, unlg_former.py:99-104
// At most 256 workgroups: every workgroup ends in one float atomic on the loss scalar, and those serialise in L2 (the 1024-workgroup
// scalar-load form spent its 21 us there and in load latency).  The four waves meet left to right, here and in k_l2: block_sum4's pairwise
// meet would move the last bit of the loss.
__global__ __launch_bounds__(256) void k_l1(const float* __restrict__ out, const float* __restrict__ gt, float* __restrict__ dout,
                                            float* loss_accum, long n, float inv_n, float gscale) {
    float part = 0.f;
    rl_stream_diff(out, gt, dout, n, [&](float d) { part += fabsf(d); return d > 0.f ? gscale : (d < 0.f ? -gscale : 0.f); });
    part = wave_sum(part);
    __shared__ float sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss_accum, (sm[0] + sm[1] + sm[2] + sm[3]) * inv_n);
}

extern "C" int lg_l1_loss(const float* out, const float* gt, float* dout, float* loss_accum, int64_t n_local, int64_t n_global, float scale,
                          void* stream) {
    const int grid = rl_flat_grid("l1_loss", out, gt, dout, loss_accum, n_local, n_global);
    if (!grid) return -1;
    k_l1<<<grid, 256, 0, (hipStream_t)stream>>>(out, gt, dout, loss_accum, n_local, 1.0f / (float)n_global, scale / (float)n_global);
    LG_CHECK_LAUNCH();
    return 0;
}

// L2 loss (nn.MSELoss, mean) forward + backward -- models/base/losses.py:19-40 with type 'l2'
// k_l1's access pattern and reduction shape.  The squares are summed in fp64 and the workgroups meet in an fp64 slot of the library
// (one per launch in flight, handed out round-robin), so loss_accum takes ONE float add per launch, by the workgroup that arrives
// last: up to 256 float atomics on the scalar would each round at the loss's magnitude, in an order that changes from run to run.
// dout = (fl(2 / n) d) scale, rounded after each product: the bits of torch's own MSE backward (norm * (input - target) * grad_output).
#define LG_L2_SLOTS 64
struct l2_slot { double acc; unsigned int arrived; unsigned int pad; };
__device__ l2_slot g_l2_slots[LG_L2_SLOTS];

__global__ __launch_bounds__(256) void k_l2(const float* __restrict__ out, const float* __restrict__ gt, float* __restrict__ dout,
                                            float* loss_accum, long n, double inv_n, float norm, float scale, int slot_id) {
    l2_slot* slot = &g_l2_slots[slot_id];
    double part = 0.0;
    rl_stream_diff(out, gt, dout, n, [&](float d) { part += (double)d * (double)d; return (norm * d) * scale; });
    part = wave_sum(part);
    __shared__ double sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&slot->acc, sm[0] + sm[1] + sm[2] + sm[3]);
        __threadfence();
        if (atomicAdd(&slot->arrived, 1u) == gridDim.x - 1) {       // every workgroup's sum is in: hand the slot back empty
            __threadfence();
            const double total = __longlong_as_double((long long)atomicExch((unsigned long long*)&slot->acc, 0ull));
            atomicExch(&slot->arrived, 0u);
            atomicAdd(loss_accum, (float)(total * inv_n));
        }
    }
}

extern "C" int lg_l2_loss(const float* out, const float* gt, float* dout, float* loss_accum, int64_t n_local, int64_t n_global, float scale,
                          void* stream) {
    const int grid = rl_flat_grid("l2_loss", out, gt, dout, loss_accum, n_local, n_global);
    if (!grid) return -1;
    static std::atomic<unsigned> next_slot{0};
    k_l2<<<grid, 256, 0, (hipStream_t)stream>>>(out, gt, dout, loss_accum, n_local, 1.0 / (double)n_global, (float)(2.0 / (double)n_global), scale,
                                                (int)(next_slot.fetch_add(1) % LG_L2_SLOTS));
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t lg_recloss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    RlGeom g;
    if (!rl_geom("recloss_workspace_bytes", B, C, H, W, g)) return 0;
    return g.sam_bytes > g.ssim_bytes ? g.sam_bytes : g.ssim_bytes;
}

extern "C" int lg_sam_loss(const float* out, const float* gt, float* dout, float* loss_accum, int32_t B, int64_t B_global, int32_t C, int32_t H,
                           int32_t W, float scale, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "sam_loss";
    RlGeom g;
    if (!rl_geom(who, B, C, H, W, g)) return -1;
    if (!rl_check_args(who, out, gt, dout, loss_accum, B, B_global, scale, accumulate, workspace, workspace_bytes, g.sam_bytes)) return -1;
    double* part = (double*)workspace;
    const double n_global = (double)B_global * (double)g.HW;
    const dim3 grid(g.gx, B);
    const hipStream_t s = (hipStream_t)stream;
    if (C == 4)
        k_sam_loss<4><<<grid, RL_NT, 0, s>>>(out, gt, dout, part, g.HW, g.gx, (double)scale / n_global, accumulate);
    else
        k_sam_loss<8><<<grid, RL_NT, 0, s>>>(out, gt, dout, part, g.HW, g.gx, (double)scale / n_global, accumulate);
    LG_CHECK_LAUNCH();
    k_recloss_finish<<<1, RL_NT, 0, s>>>(part, (long)B * g.gx, 0.0, 1.0 / n_global, loss_accum);
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_ssim_loss(const float* out, const float* gt, float* dout, float* loss_accum, int32_t B, int64_t B_global, int32_t C, int32_t H,
                            int32_t W, float scale, float data_range, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "ssim_loss";
    RlGeom g;
    if (!rl_geom(who, B, C, H, W, g)) return -1;
    if (!g.tiles) { lg_set_error("%s: H and W must be at least %d, one window (got %d x %d)", who, SS_N, H, W); return -1; }
    if (!(data_range > 0.f) || data_range - data_range != 0.f) { lg_set_error("%s: data_range must be positive and finite", who); return -1; }
    if (!rl_check_args(who, out, gt, dout, loss_accum, B, B_global, scale, accumulate, workspace, workspace_bytes, g.ssim_bytes)) return -1;
    static DeviceOnce attr_once;
    if (int rc = lds_attr_once(attr_once, who, SS_LDS_BYTES, k_ssim_loss)) return rc;
    SsimTaps taps;      // metrics.gaussian_taps: 11 samples of a centred Gaussian of sigma 1.5, normalised to sum 1
    double sum = 0.0;
    for (int t = 0; t < SS_N; ++t) {
        const double d = ((double)t - 0.5 * (SS_N - 1)) / 1.5;
        taps.w[t] = std::exp(-0.5 * d * d);
        sum += taps.w[t];
    }
    for (int t = 0; t < SS_N; ++t) taps.w[t] /= sum;
    const double R = (double)data_range, c1 = (0.01 * R) * (0.01 * R), c2 = (0.03 * R) * (0.03 * R);
    const double win_local = (double)B * C * (double)(H - SS_N + 1) * (double)(W - SS_N + 1);
    const double win_global = win_local / (double)B * (double)B_global;
    double* part = (double*)workspace;
    const hipStream_t s = (hipStream_t)stream;
    k_ssim_loss<<<dim3(g.tiles, C, B), RL_NT, SS_LDS_BYTES, s>>>(out, gt, dout, part, C, H, W, g.tiles_x, taps, c1, c2,
                                                                 -(double)scale / win_global, accumulate);
    LG_CHECK_LAUNCH();
    // this rank's share of 1 - mean S: (windows of this rank - sum S) / windows of all ranks
    k_recloss_finish<<<1, RL_NT, 0, s>>>(part, (long)B * C * g.tiles, -win_local, -1.0 / win_global, loss_accum);
    LG_CHECK_LAUNCH();
    return 0;
}
