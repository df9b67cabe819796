// Weight-gradient GEMMs of the 1x1 convs for gfx950:  dW[n][k] = sum_p Y[p][n] * X[p][k],  db[n] = sum_p Y[p][n]
// (autograd of bmu.point_conv, reference models/common/basic_module_unformer_v2.py:13-14).
// The reduction runs over PIXELS (up to B*H*W = 524 288 at bs=32), the output is tiny (16..256 squared), so the
// pixel axis is the MFMA K dimension: v_mfma_f32_16x16x4_f32 with lane (r,g) feeding A[i=r][k=g] = Y[p+g][n0+r] and
// B[k=g][j=r] = X[p+g][k0+r] -- both operands are read in their natural [pixel][channel] layout, 64-byte segments,
// no transposes.  Every wave owns a 64x64 block of dW over a slice of the pixels; the 4 waves of a workgroup are summed in
// LDS and the workgroup's partial goes to a slab that a second kernel sums in a fixed slice order.
#include "kernels.h"
#include "bwd_kernels.h"
#include "hstore.h"
#include <string.h>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));


// Block shape: NT x KT tiles of 16 (compile time, so the pixel loop is branch-free and software-pipelined: the operands of
// the next 16 pixels are in flight while the MFMAs of the current 16 issue).  VEC (64x64 blocks only): lane (r,g) loads ONE
// float4 of Y and ONE of X per 4-pixel step, Y[p+g][n0 + 4r .. 4r+3] / X[p+g][k0 + 4r ..]; element t of the float4 feeds MFMA
// tile t, so tile t owns the strided channel set {4r + t}: a 64-channel row is one fully coalesced 256-byte segment per 16
// lanes and 2 loads feed 16 MFMAs.  Output acc[i][j][v] (MFMA row 4g+v, col r) is then dW[n0 + 4(4g+v) + i][k0 + 4r + j].
// Non-VEC: scalar loads in the natural tile order (tile t = channels 16t .. 16t+15), columns >= n_valid / k_valid read as 0.
// 4-pixel MFMA steps per batch: narrow blocks have few MFMAs per pixel, so they keep more pixels in flight
constexpr int WGRAD_VEC_U = 4;     // the VEC blocks' steps per batch
constexpr int WGRAD_WGS = 512;     // workgroups of a launch (wgrad_splits): two waves per SIMD
__host__ __device__ constexpr int wgrad_batch(int nt, int kt, bool vec) { return vec ? WGRAD_VEC_U : (nt + kt <= 2 ? 16 : (nt + kt <= 4 ? 8 : 4)); }

// XGELU: the stored X is a pre-activation and the conv input is gelu(X) (feed_forward's second and third 1x1 convs when the forward
// saved h1 / h3 instead of gelu(h1) / gelu(h3)): evaluated on the operand registers, under the loads of the next batch
template <int NT, int KT, bool VEC, bool YBF, bool XBF, bool XGELU = false>
__global__ __launch_bounds__(256) void k_wgrad_t(WgradArgs a, int k_blocks, long px_per_wave, float* slab, float* bslab) {
    constexpr int U = wgrad_batch(NT, KT, VEC);
    constexpr int NB = 16 * NT, KB = 16 * KT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int nb = blockIdx.y / k_blocks, kb = blockIdx.y - nb * k_blocks;
    const int n0 = nb * NB, k0 = kb * KB;
    const long slice = (long)blockIdx.x * 4 + wave;
    // batches of 4 U pixels dealt round-robin to the waves of the grid: at any moment the whole grid reads ONE contiguous window of the
    // operands (all HBM channels), instead of 2 048 streams that all sit at the same offset of their own 64 KiB-aligned chunk (against one
    // contiguous range of px_per_wave pixels per wave, an argument no longer read: the 16-wide blocks run 35 -> 31.5 us interleaved, the 64 x 64 ones the same)
    const long p_stride = (long)gridDim.x * 4 * (4 * U);
    const long p_begin = slice * (4 * U);
    const long p_end = a.P;
    f32x4 acc[NT][KT];
    float bsum[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        bsum[i] = 0.f;
#pragma unroll
        for (int j = 0; j < KT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // column offsets / masks of this lane (non-VEC)
    int ycol[NT], xcol[KT];
    bool yok[NT], xok[KT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { const int c = n0 + t * 16 + r; yok[t] = c < a.n_valid; ycol[t] = yok[t] ? c : 0; }
#pragma unroll
    for (int t = 0; t < KT; ++t) { const int c = k0 + t * 16 + r; xok[t] = c < a.k_valid; xcol[t] = xok[t] ? c : 0; }
    // masks are applied by multiplication (operands are finite tensors): a select would let the compiler sink the loads into
    // branches with a full wait each, which is what made the first version of this kernel pure load latency
    float ym[NT], xm[KT];
#pragma unroll
    for (int t = 0; t < NT; ++t) ym[t] = yok[t] ? 1.f : 0.f;
#pragma unroll
    for (int t = 0; t < KT; ++t) xm[t] = xok[t] ? 1.f : 0.f;
    auto fetch = [&](long p, float (&y)[U][NT], float (&x)[U][KT]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = p + 4 * u + g;
            const long rc = row < p_end ? row : p_begin;   // a row that exists; masked in `consume`
            if (VEC) {
                const float4 yv = HS<YBF>::ld4(a.Y, rc * a.ldy + n0 + 4 * r);
                const float4 xv = HS<XBF>::ld4(a.X, rc * a.ldx + k0 + 4 * r);
                const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int t = 0; t < NT; ++t) y[u][t] = yy[t & 3];
#pragma unroll
                for (int t = 0; t < KT; ++t) x[u][t] = xx[t & 3];
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) y[u][t] = HS<YBF>::ld1(a.Y, rc * a.ldy + ycol[t]);
#pragma unroll
                for (int t = 0; t < KT; ++t) x[u][t] = HS<XBF>::ld1(a.X, rc * a.ldx + xcol[t]);
            }
        }
    };
    if (p_begin < p_end) {
        float yc[U][NT], xc[U][KT];
        fetch(p_begin, yc, xc);
#pragma unroll 1
        for (long p = p_begin; p < p_end; p += p_stride) {
            float yn[U][NT], xn[U][KT];
            fetch(p + p_stride, yn, xn);   // next batch in flight under this batch's MFMAs (past the slice end: cached, unused)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float rm = (p + 4 * u + g) < p_end ? 1.f : 0.f;
                float yv[NT], xv[KT];
#pragma unroll
                for (int i = 0; i < NT; ++i) { yv[i] = yc[u][i] * (VEC ? rm : rm * ym[i]); bsum[i] += yv[i]; }
                if constexpr (XGELU && KT % 2 == 0) {   // gelu on operand PAIRS (packed fp32, the forward's own gelu2_f): half the vector instructions
#pragma unroll
                    for (int j = 0; j < KT; j += 2) {
                        const lg_v2f gp = gelu2_f((lg_v2f){xc[u][j], xc[u][j + 1]});
                        xv[j] = VEC ? gp.x : gp.x * xm[j];
                        xv[j + 1] = VEC ? gp.y : gp.y * xm[j + 1];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < KT; ++j) {
                        const float xg = XGELU ? gelu_f(xc[u][j]) : xc[u][j];
                        xv[j] = VEC ? xg : xg * xm[j];
                    }
                }
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < KT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[i], xv[j], acc[i][j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int i = 0; i < NT; ++i) yc[u][i] = yn[u][i];
#pragma unroll
                for (int j = 0; j < KT; ++j) xc[u][j] = xn[u][j];
            }
        }
    }
    // the 4 waves of the workgroup hold partials of the same block: summed in LDS in a fixed order (no float atomics ->
    // bitwise reproducible), one slab slice per workgroup
    __shared__ float red[NB * KB + NB];
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < KT; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int idx = VEC ? (4 * (4 * g + v) + i) * KB + 4 * r + j : (i * 16 + 4 * g + v) * KB + j * 16 + r;
                        red[idx] = (w == 0 ? 0.f : red[idx]) + acc[i][j][v];
                    }
            // bias: lanes with equal r hold the same channels for different pixels
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                float sv = bsum[i];
                sv += __shfl_xor(sv, 16);
                sv += __shfl_xor(sv, 32);
                const int idx = NB * KB + (VEC ? 4 * r + i : i * 16 + r);
                if (g == 0) red[idx] = (w == 0 ? 0.f : red[idx]) + sv;
            }
        }
        __syncthreads();
    }
    float* my = slab + (long)blockIdx.x * ((long)a.N * a.K);
    for (int i = threadIdx.x; i < NB * KB; i += 256) {
        const int rr = i / KB, cc = i - rr * KB;
        my[(long)(n0 + rr) * a.K + k0 + cc] = red[i];
    }
    if (a.db && kb == 0 && threadIdx.x < NB) bslab[(long)blockIdx.x * a.N + n0 + threadIdx.x] = red[NB * KB + threadIdx.x];
}

// dst[row*ld + col] += sum_s slab[s][row*cols + col]   for row < rows_valid, col < cols_valid
// block = 64 consecutive outputs x 4 slice phases (fixed summation order: bitwise reproducible)
// block = 64 consecutive outputs x 4 slice phases (fixed summation order: bitwise reproducible)
__global__ __launch_bounds__(256) void k_reduce_slab(const float* __restrict__ slab, long nslices, int rows, int cols, float* dst,
                                                     int ld, int rows_valid, int cols_valid, const float* __restrict__ slab2, int n2,
                                                     float* dst2, int n2_valid) {
    // 16 outputs x 16 slice phases per workgroup: every thread has 8 independent loads in flight (the old 64 x 4 shape walked 128
    // slices per thread and was pure load latency, ~12 us per call); fixed summation order -> deterministic.
    __shared__ float part[16][17];
    // job 0 (blockIdx.y == 0): the [rows][cols] slab; job 1: an optional [n2] vector slab (bias) in the same launch
    if (blockIdx.y == 1) { slab = slab2; rows = 1; cols = n2; dst = dst2; ld = n2; rows_valid = 1; cols_valid = n2_valid; }
    const long n = (long)rows * cols;
    const int o = threadIdx.x & 15, ph = threadIdx.x >> 4;
    const long i = blockIdx.x * 16L + o;
    float sv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) sv[u] = 0.f;
    if (i < n) {
        long k = ph;
        for (; k + 16 * 7 < nslices; k += 16 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) sv[u] += slab[(k + 16 * u) * n + i];
        }
        for (; k < nslices; k += 16) sv[0] += slab[k * n + i];
    }
    part[ph][o] = ((sv[0] + sv[1]) + (sv[2] + sv[3])) + ((sv[4] + sv[5]) + (sv[6] + sv[7]));
    __syncthreads();
    if (ph == 0 && i < n) {
        const int row = (int)(i / cols), col = (int)(i - (long)row * cols);
        if (row < rows_valid && col < cols_valid) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += part[q][o];
            dst[(long)row * ld + col] += t;
        }
    }
}

// round 6: jobs whose rows are whole, 16-byte aligned quads (every large one: pos_emb, the FFN weight slabs) move FOUR outputs per thread -- a
// 16-lane group reads 256 contiguous bytes of a slice instead of 64, a quarter of the workgroups.  Same order of additions per output.
__host__ __device__ inline bool reduce_job_v4(const ReduceJob& jb) {
    return ((jb.cols | jb.row_stride | jb.ld) & 3) == 0 && (jb.slice_stride & 3) == 0 && jb.rows_valid == jb.rows && jb.cols_valid == jb.cols &&
           ((reinterpret_cast<uintptr_t>(jb.slab) | reinterpret_cast<uintptr_t>(jb.dst) | reinterpret_cast<uintptr_t>(jb.dst2)) & 15) == 0;
}
__host__ __device__ inline long reduce_job_wgs(const ReduceJob& jb, bool v4) {
    const long n = (long)jb.rows * jb.cols;
    return v4 ? ((n >> 2) + 15) / 16 : (n + 15) / 16;
}
// one job, the outputs of workgroup `wg` of it (wg < reduce_job_wgs): 16 outputs (V4: 16 quads of outputs) x 16 slice phases, the shape of
// k_reduce_slab.  The order of additions of an output is the same in both forms.
// (slabs and destinations are global memory; said explicitly, because an entry rebuilt from scalar registers has lost that and would read through flat loads)
typedef __attribute__((address_space(1))) const float* rq_gsrc;
typedef __attribute__((address_space(1))) float* rq_gdst;
typedef __attribute__((address_space(1))) const f32x4* rq_gsrc4;
typedef __attribute__((address_space(1))) f32x4* rq_gdst4;
__device__ __forceinline__ float4 rq_ld4(rq_gsrc p) { const f32x4 v = *(rq_gsrc4)p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void rq_add4(rq_gdst p, const float4& t) {   // *p += t
    const rq_gdst4 d = (rq_gdst4)p;
    const f32x4 v = *d;
    *d = (f32x4){v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w};
}
template <bool V4>
__device__ __forceinline__ void reduce_job_wg(const ReduceJob& jb, long wg, float4 (*part)[17]) {
    const long n = (long)jb.rows * jb.cols;
    const int o = threadIdx.x & 15, ph = threadIdx.x >> 4;
    if (V4) {
        const long n4 = n >> 2;
        const long i4 = wg * 16L + o;
        const long i = i4 << 2;
        const int row = (int)(i / jb.cols), col = (int)(i - (long)row * jb.cols);
        float4 sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) sv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i4 < n4) {
            const rq_gsrc src = (rq_gsrc)jb.slab + (long)row * jb.row_stride + col;
            const long ss = jb.slice_stride, ns = jb.nslices;
            long k = ph;
            for (; k + 16 * 7 < ns; k += 16 * 8) {
                float4 ld[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) ld[u] = rq_ld4(src + (k + 16 * u) * ss);
#pragma unroll
                for (int u = 0; u < 8; ++u) { sv[u].x += ld[u].x; sv[u].y += ld[u].y; sv[u].z += ld[u].z; sv[u].w += ld[u].w; }
            }
            for (; k < ns; k += 16) {
                const float4 l = rq_ld4(src + k * ss);
                sv[0].x += l.x; sv[0].y += l.y; sv[0].z += l.z; sv[0].w += l.w;
            }
        }
        auto add4 = [](const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
        part[ph][o] = add4(add4(add4(sv[0], sv[1]), add4(sv[2], sv[3])), add4(add4(sv[4], sv[5]), add4(sv[6], sv[7])));
        __syncthreads();
        if (ph == 0 && i4 < n4) {
            float4 ts = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < 16; ++q) ts = add4(ts, part[q][o]);
            rq_add4((rq_gdst)jb.dst + (long)row * jb.ld + col, ts);
            if (jb.dst2) rq_add4((rq_gdst)jb.dst2 + (long)row * jb.ld + col, ts);
        }
        return;
    }
    const long i = wg * 16L + o;
    const int row = (int)(i / jb.cols), col = (int)(i - (long)row * jb.cols);
    float sv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) sv[u] = 0.f;
    if (i < n) {
        const rq_gsrc src = (rq_gsrc)jb.slab + (long)row * jb.row_stride + col;
        const long ss = jb.slice_stride, ns = jb.nslices;
        long k = ph;
        for (; k + 16 * 7 < ns; k += 16 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) sv[u] += src[(k + 16 * u) * ss];
        }
        for (; k < ns; k += 16) sv[0] += src[k * ss];
    }
    float* parts = reinterpret_cast<float*>(part);
    parts[ph * 17 + o] = ((sv[0] + sv[1]) + (sv[2] + sv[3])) + ((sv[4] + sv[5]) + (sv[6] + sv[7]));
    __syncthreads();
    if (ph == 0 && i < n && row < jb.rows_valid && col < jb.cols_valid) {
        float tsum = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) tsum += parts[q * 17 + o];
        ((rq_gdst)jb.dst)[(long)row * jb.ld + col] += tsum;
        if (jb.dst2) ((rq_gdst)jb.dst2)[(long)row * jb.ld + col] += tsum;
    }
}

// one chain of jobs (the same destination: bwd_kernels.h), link after link in the SAME threads -- an output's value goes through the additions
// dst += total(link 0), dst += total(link 1), ... exactly as one launch per link would have done them
// (a table entry is the same for every lane: read once and kept in scalar registers, so the slab / destination addresses are scalar base + lane
// offset as they are when the table is a kernel argument -- loads behind a barrier are not turned into scalar loads by the compiler itself)
__device__ __forceinline__ ReduceJob reduce_job_uniform(const ReduceJob* p) {
    constexpr int NW = sizeof(ReduceJob) / 4;
    const int* q = reinterpret_cast<const int*>(p);
    int w[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = __builtin_amdgcn_readfirstlane(q[k]);
    ReduceJob j;
    __builtin_memcpy(&j, w, sizeof(ReduceJob));
    return j;
}
__device__ __forceinline__ void reduce_chain_wg(const ReduceJob* jb, const ReduceJob* tab, long wg, float4 (*part)[17]) {
    ReduceJob j = reduce_job_uniform(jb);
    const bool v4 = j.v4 == 1;   // (the head's: flush() clears it when a link of the chain cannot run in that form)
    for (;;) {
        if (v4) reduce_job_wg<true>(j, wg, part);
        else reduce_job_wg<false>(j, wg, part);
        if (j.next < 0) break;
        j = reduce_job_uniform(tab + j.next);
        __syncthreads();   // `part` is read by the phase-0 threads of the link just done
    }
}
// per_block form and the direct single-job launches: table as a kernel argument, blockIdx.y = job
__global__ __launch_bounds__(256) void k_reduce_jobs_tab(ReduceJobTable t) {
    __shared__ float4 part[16][17];
    const ReduceJob& jb = t.j[blockIdx.y];
    const bool v4 = reduce_job_v4(jb);
    if ((long)blockIdx.x >= reduce_job_wgs(jb, v4)) return;
    if (v4) reduce_job_wg<true>(jb, blockIdx.x, part);
    else reduce_job_wg<false>(jb, blockIdx.x, part);
}
// merged form: every job of a backward pass in one flat grid; workgroup -> job through the prefix sums of the per-job workgroup counts
// (<= 512 entries: two loads per thread and a count, no search chain)
__global__ __launch_bounds__(256) void k_reduce_jobs(const ReduceImage* __restrict__ img) {
    __shared__ float4 part[16][17];
    __shared__ int s_cnt;
    const int nh = img->nheads;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int c = 0;
    for (int k = threadIdx.x; k < nh; k += 256) c += img->wg_start[k] <= (int)blockIdx.x ? 1 : 0;
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    const int job = __builtin_amdgcn_readfirstlane(s_cnt) - 1;   // wg_start[0] = 0: job >= 0
    const int wg0 = __builtin_amdgcn_readfirstlane(img->wg_start[job]);
    reduce_chain_wg(img->j + job, img->j, (long)((int)blockIdx.x - wg0), part);
}

static thread_local ReduceQueue* tl_rq = nullptr;
static std::atomic<long long> g_rq_stats[LG_RQ_NSTATS];   // process-wide (bwd_kernels.h: reduce_queue_stats)
void reduce_queue_stats(long long out[LG_RQ_NSTATS], int reset) {
    for (int k = 0; k < LG_RQ_NSTATS; ++k) out[k] = reset ? g_rq_stats[k].exchange(0) : g_rq_stats[k].load();
}
// debug export (tests/test_gpu_reduce_merge.py): the LG_RQ_NSTATS = 6 counters since the last reset
extern "C" __attribute__((visibility("default"))) int lg_debug_reduce_stats(long long* out6, int reset) {
    if (!out6) return -1;
    reduce_queue_stats(out6, reset);
    return 0;
}
void reduce_queue_begin(ReduceQueue* q) { tl_rq = q; }
int reduce_queue_end() {
    ReduceQueue* q = tl_rq;
    tl_rq = nullptr;
    return q ? q->flush() : 0;
}

// ---- merged form: the device-side tables ----
// The image of a launch depends on the plan, the batch size, the flags and the workspace / gradient pointers only, so a training loop builds
// the same two images (LGT part, data part) every step.  Uploaded images are kept per device and found again by content: a hit costs one
// memcmp on the host and nothing on the stream.  A miss takes the least recently filled slot; the device is drained first (a launch that
// still reads the slot, on whatever stream, has finished; the slot's host copy is no longer the source of a pending transfer).
// The content includes the workspace and gradient-buffer POINTERS: a caller whose gradient buffer moves from step to step misses twice per
// backward (counter [2] of reduce_queue_stats).  The 16 images of a device (630 KB) are allocated at the first launch there and live as long
// as the library.
namespace {
constexpr int RQ_SLOTS = 16;
struct RqSlot { std::vector<char> host; uint64_t hash = 0; };
struct RqCache {
    ReduceImage* dev = nullptr;   // RQ_SLOTS images
    RqSlot slot[RQ_SLOTS];
    int next_victim = 0;
};
std::mutex g_rq_mu;
RqCache* g_rq_cache[64];
size_t image_bytes(const ReduceImage& im) { return offsetof(ReduceImage, j) + (size_t)im.njobs * sizeof(ReduceJob); }
uint64_t fnv1a(const char* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    const uint64_t* q = reinterpret_cast<const uint64_t*>(p);
    for (size_t k = 0; k < n / 8; ++k) { h ^= q[k]; h *= 1099511628211ull; }
    return h;   // (image_bytes is a multiple of 8)
}
// No two heads of one launch may touch the same destination element: their workgroups run concurrently.  Extents are sorted; where two
// overlap as intervals they may still interleave (the 3 x 3 taps of a depthwise weight are nine jobs of stride 9, the two halves of the
// fusion conv's weight two jobs of row pitch 2E): same pitch and disjoint column windows.  Anything else is an error.
struct RqExtent { uintptr_t lo, hi; long ld; long cols; int job; };
bool extents_clash(const RqExtent& a, const RqExtent& b) {
    const long ld = a.ld ? a.ld : b.ld;
    if (!ld) return true;                              // two single rows whose intervals overlap
    if ((a.ld && a.ld != ld) || (b.ld && b.ld != ld)) return true;
    if (a.cols > ld || b.cols > ld) return true;
    const long d = (long)(((b.lo - a.lo) / sizeof(float)) % (uintptr_t)ld);   // b's first column in a's rows (b.lo >= a.lo)
    return !(d >= a.cols && d + b.cols <= ld);
}
int check_disjoint(const ReduceImage& im) {
    std::vector<RqExtent> ex;
    ex.reserve(2 * (size_t)im.nheads);
    for (int k = 0; k < im.nheads; ++k) {
        const ReduceJob& j = im.j[k];
        if (j.rows_valid <= 0 || j.cols_valid <= 0) continue;
        float* dsts[2] = {j.dst, j.dst2};
        for (float* d : dsts) {
            if (!d) continue;
            RqExtent e;
            e.lo = reinterpret_cast<uintptr_t>(d);
            e.hi = reinterpret_cast<uintptr_t>(d + (long)(j.rows_valid - 1) * j.ld + j.cols_valid);
            e.ld = j.rows_valid > 1 ? j.ld : 0;   // a single row fits any pitch
            e.cols = j.cols_valid;
            e.job = k;
            ex.push_back(e);
        }
    }
    std::sort(ex.begin(), ex.end(), [](const RqExtent& a, const RqExtent& b) { return a.lo < b.lo; });
    for (size_t a = 0; a < ex.size(); ++a)
        for (size_t b = a + 1; b < ex.size() && ex[b].lo < ex[a].hi; ++b)
            if (extents_clash(ex[a], ex[b])) {
                lg_set_error("reduce queue: jobs %d and %d of one launch add into the same gradient elements", ex[a].job, ex[b].job);
                return -4;
            }
    return 0;
}
// launches k_reduce_jobs on the device copy of `im` (uploaded on `s` first if it is not there yet).  The launch is queued UNDER the lock: a miss of
// another host thread may then take any slot -- it drains the device first, and the launch that reads the slot is already in its stream
int launch_image(const ReduceImage& im, hipStream_t s) {
    const size_t bytes = image_bytes(im);
    const char* src = reinterpret_cast<const char*>(&im);
    const uint64_t h = fnv1a(src, bytes);
    std::lock_guard<std::mutex> lock(g_rq_mu);
    RqCache*& c = g_rq_cache[DeviceOnce::dev()];
    if (!c) {
        RqCache* nc = new RqCache;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&nc->dev), sizeof(ReduceImage) * RQ_SLOTS);
        if (e != hipSuccess) { delete nc; lg_set_error("reduce queue: hipMalloc(job tables): %s", hipGetErrorString(e)); return (int)e; }
        c = nc;
    }
    for (int k = 0; k < RQ_SLOTS; ++k) {
        const RqSlot& sl = c->slot[k];
        if (sl.hash == h && sl.host.size() == bytes && memcmp(sl.host.data(), src, bytes) == 0) {
            k_reduce_jobs<<<(unsigned)im.total_wgs, 256, 0, s>>>(c->dev + k);
            LG_CHECK_LAUNCH();
            return 0;
        }
    }
    int rc = check_disjoint(im);
    if (rc) return rc;
    const int k = c->next_victim;
    c->next_victim = (k + 1) % RQ_SLOTS;
    RqSlot& sl = c->slot[k];
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { lg_set_error("reduce queue: hipDeviceSynchronize: %s", hipGetErrorString(e)); return (int)e; }
    sl.host.clear();   // (invalid until the transfer is queued)
    sl.hash = 0;
    e = hipMemcpyAsync(c->dev + k, src, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // `im` is the caller's staging buffer
    if (e != hipSuccess) { lg_set_error("reduce queue: upload of a job table: %s", hipGetErrorString(e)); return (int)e; }
    sl.host.assign(src, src + bytes);
    sl.hash = h;
    g_rq_stats[2]++;
    k_reduce_jobs<<<(unsigned)im.total_wgs, 256, 0, s>>>(c->dev + k);
    LG_CHECK_LAUNCH();
    return 0;
}
}  // namespace

// debug export (tests/test_reduce_variant_cpu.py; host only): the destination check of a merged launch on n made-up jobs -- job k adds into
// rows_valid[k] x cols_valid[k] elements of row pitch ld[k] that start dst_off[k] floats into one buffer (dst2_off[k] >= 0: a second destination).
// 0 = no two jobs share an element, -4 (error set) otherwise
extern "C" __attribute__((visibility("default"))) int lg_debug_reduce_disjoint(int n, const long long* dst_off, const long long* dst2_off,
                                                                                const int* rows_valid, const int* cols_valid, const int* ld) {
    if (n < 0 || n > LG_RQ_MAX_JOBS || !dst_off || !dst2_off || !rows_valid || !cols_valid || !ld) return -1;
    static thread_local ReduceImage im;
    float* const base = reinterpret_cast<float*>((uintptr_t)1 << 32);   // never dereferenced
    for (int k = 0; k < n; ++k) {
        ReduceJob& j = im.j[k];
        j = ReduceJob();
        j.slab = nullptr; j.dst = base + dst_off[k]; j.dst2 = dst2_off[k] >= 0 ? base + dst2_off[k] : nullptr;
        j.rows = j.rows_valid = rows_valid[k]; j.cols = j.cols_valid = cols_valid[k]; j.ld = ld[k];
    }
    im.nheads = im.njobs = n;
    return check_disjoint(im);
}

int ReduceQueue::flush() {
    off = 0;
    if (n == 0) return 0;
    const int nj = n;
    n = 0;
    g_rq_stats[0]++;
    if (per_block) {
        static thread_local ReduceJobTable tab;   // (nj <= LG_MAX_REDUCE_JOBS: push() drains the queue there)
        long nmax = 0;
        for (int k = 0; k < nj; ++k) {
            tab.j[k] = jobs[k];
            const long m = (long)jobs[k].rows * jobs[k].cols;
            if (m > nmax) nmax = m;
        }
        tab.n = nj;
        dim3 grid((unsigned)((nmax + 15) / 16), (unsigned)nj);
        k_reduce_jobs_tab<<<grid, 256, 0, stream>>>(tab);
        LG_CHECK_LAUNCH();
        return 0;
    }
    // chains: a job whose destination an earlier job of the table already has joins that job's chain (same output shape; anything else is
    // left to check_disjoint).  Heads keep their order and come first in the image, then the other links.
    static thread_local ReduceImage im;
    static thread_local int head_of[LG_RQ_MAX_JOBS], tail_of[LG_RQ_MAX_JOBS], slot_of[LG_RQ_MAX_JOBS], heads[LG_RQ_MAX_JOBS], prev_of[LG_RQ_MAX_JOBS];
    static thread_local int by_dst[4 * LG_RQ_MAX_JOBS];   // open-addressing table of the heads, keyed by destination: the search is linear in the jobs
    const auto t0 = std::chrono::steady_clock::now();
    memset(by_dst, 0xff, sizeof(by_dst));
    int nheads = 0;
    for (int i = 0; i < nj; ++i) {
        const ReduceJob& a = jobs[i];
        int h = -1;
        unsigned p = (unsigned)((reinterpret_cast<uintptr_t>(a.dst) >> 2) * 0x9E3779B97F4A7C15ull >> 40) % (4 * LG_RQ_MAX_JOBS);
        for (; by_dst[p] >= 0; p = (p + 1) % (4 * LG_RQ_MAX_JOBS)) {
            const ReduceJob& b = jobs[by_dst[p]];
            if (b.dst == a.dst && b.dst2 == a.dst2 && b.rows == a.rows && b.cols == a.cols && b.ld == a.ld && b.rows_valid == a.rows_valid &&
                b.cols_valid == a.cols_valid) {
                h = by_dst[p];
                break;
            }
        }
        if (h < 0) { by_dst[p] = i; heads[nheads++] = i; head_of[i] = i; tail_of[i] = i; prev_of[i] = -1; }
        else { head_of[i] = h; prev_of[i] = tail_of[h]; tail_of[h] = i; }
    }
    int pos = 0;
    for (int k = 0; k < nheads; ++k) slot_of[heads[k]] = pos++;
    for (int i = 0; i < nj; ++i) if (head_of[i] != i) slot_of[i] = pos++;
    memset(&im, 0, offsetof(ReduceImage, j));
    for (int i = 0; i < nj; ++i) {
        ReduceJob& d = im.j[slot_of[i]];
        d = jobs[i];
        d.next = -1;
        d.v4 = reduce_job_v4(jobs[i]) ? 1 : 0;
    }
    for (int i = 0; i < nj; ++i) {
        if (prev_of[i] >= 0) im.j[slot_of[prev_of[i]]].next = slot_of[i];
        if (!im.j[slot_of[i]].v4) im.j[slot_of[head_of[i]]].v4 = 0;   // a chain runs in the form all of its links can
    }
    long total = 0;
    for (int k = 0; k < nheads; ++k) {
        im.wg_start[k] = (int)total;
        total += reduce_job_wgs(im.j[k], im.j[k].v4 == 1);
    }
    if (total <= 0 || total > 0x3fffffffL) { lg_set_error("reduce queue: %ld workgroups in one launch", total); return -4; }
    im.nheads = nheads; im.njobs = nj; im.total_wgs = (int)total;
    const int rc = launch_image(im, stream);
    if (g_rq_stats[3].load() < nj) g_rq_stats[3] = nj;
    if (g_rq_stats[5].load() < nheads) g_rq_stats[5] = nheads;
    g_rq_stats[4] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}
int ReduceQueue::push(const ReduceJob& j) {
    if (n == (per_block ? LG_MAX_REDUCE_JOBS : LG_RQ_MAX_JOBS)) {
        // the slabs already handed out stay valid: only the table is drained (off is restored)
        const size_t keep = off;
        g_rq_stats[1]++;
        int rc = flush();
        off = keep;
        if (rc) return rc;
    }
    jobs[n++] = j;
    return 0;
}
float* ReduceQueue::take(size_t nfloats) {
    nfloats = (nfloats + 63) & ~(size_t)63;
    if (nfloats > cap) { lg_set_error("reduce queue: slab of %zu floats exceeds the arena (%zu)", nfloats, cap); return nullptr; }
    if (off + nfloats > cap) {
        g_rq_stats[1]++;
        if (flush()) return nullptr;
    }
    float* p = arena + off;
    off += nfloats;
    return p;
}

static int launch_reduce_slab2(const float* slab, long nslices, int rows, int cols, float* dst, int ld, int rows_valid, int cols_valid,
                               const float* slab2, int n2, float* dst2, int n2_valid, hipStream_t s) {
    if (tl_rq) {
        ReduceJob j;
        j.slab = slab; j.dst = dst; j.dst2 = nullptr; j.nslices = nslices; j.slice_stride = (long)rows * cols;
        j.rows = rows; j.cols = cols; j.row_stride = cols; j.ld = ld; j.rows_valid = rows_valid; j.cols_valid = cols_valid;
        int rc = tl_rq->push(j);
        if (rc || !slab2) return rc;
        j.slab = slab2; j.dst = dst2; j.slice_stride = n2; j.rows = 1; j.cols = n2; j.row_stride = n2; j.ld = n2; j.rows_valid = 1;
        j.cols_valid = n2_valid;
        return tl_rq->push(j);
    }
    long n = (long)rows * cols;
    dim3 grid((unsigned)((n + 15) / 16), slab2 ? 2 : 1);
    k_reduce_slab<<<grid, 256, 0, s>>>(slab, nslices, rows, cols, dst, ld, rows_valid, cols_valid, slab2, n2, dst2, n2_valid);
    LG_CHECK_LAUNCH();
    return 0;
}
int launch_reduce_job(const ReduceJob& j, hipStream_t s) {
    if (tl_rq) return tl_rq->push(j);
    static thread_local ReduceJobTable t;
    t.j[0] = j;
    t.n = 1;
    const long n = (long)j.rows * j.cols;
    k_reduce_jobs_tab<<<dim3((unsigned)((n + 15) / 16), 1), 256, 0, s>>>(t);
    LG_CHECK_LAUNCH();
    return 0;
}
// per-channel partial rows (k_dw_bwd / k_dstep_top_bwd) as queue jobs; false when no queue is active
bool reduce_chan_enqueue(const float* part, const ChanReduce& m, int* rc) {
    if (!tl_rq) return false;
    *rc = 0;
    for (int k = 0; k < m.NK && !*rc; ++k) {
        ReduceJob j;
        j.slab = part + k; j.dst = m.dst[k]; j.dst2 = m.dst2[k]; j.cols = 1; j.cols_valid = 1;
        if ((m.allc_mask >> k) & 1u) {
            j.nslices = (long)m.nslices * m.C; j.slice_stride = m.NK; j.rows = 1; j.row_stride = 0; j.ld = 1; j.rows_valid = 1;
        } else {
            j.nslices = m.nslices; j.slice_stride = (long)m.C * m.NK; j.rows = m.C; j.row_stride = m.NK; j.ld = m.stride[k]; j.rows_valid = m.C;
        }
        *rc = tl_rq->push(j);
    }
    return true;
}
// [nslices][rows*cols] matrix slab + [nslices][rows] bias slab -> dW[rows][ld] , db[rows] (+=)
int launch_reduce_slab_wb(const float* wslab, const float* bslab, long nslices, int rows, int cols, float* dW, int ld, float* db, hipStream_t s) {
    return launch_reduce_slab2(wslab, nslices, rows, cols, dW, ld, rows, cols, bslab, rows, db, rows, s);
}
// two [nslices][n] vector slabs -> dst_a[n], dst_b[n] (+=) in one launch
int launch_reduce_slab_pair(const float* slab_a, const float* slab_b, long nslices, int n, float* dst_a, float* dst_b, hipStream_t s) {
    return launch_reduce_slab2(slab_a, nslices, 1, n, dst_a, n, 1, n, slab_b, n, dst_b, n, s);
}
int launch_reduce_slab(const float* slab, long nslices, int rows, int cols, float* dst, int ld, int rows_valid, int cols_valid,
                       hipStream_t s) {
    return launch_reduce_slab2(slab, nslices, rows, cols, dst, ld, rows_valid, cols_valid, nullptr, 0, nullptr, 0, s);
}

static int tiles_per_block(int n16) {   // largest of 4,3,2,1 dividing the tile count
    for (int t = 4; t > 1; --t) if (n16 % t == 0) return t;
    return 1;
}
static long wgrad_splits(int N, int K) {
    const int blocks = (N / 16 / tiles_per_block(N / 16)) * (K / 16 / tiles_per_block(K / 16));
    long splits = WGRAD_WGS / blocks;
    return splits < 1 ? 1 : splits;
}
size_t wgrad_slab_floats(int N, int K, long P) {
    // sized for the launch geometry below (upper bound)
    (void)P;
    return (size_t)wgrad_splits(N, K) * ((size_t)N * K + N);
}

template <int NT, int KT, bool VEC>
static void wgrad_dispatch_bf(const WgradArgs& a, dim3 grid, int k_blocks, long px, float* slab, float* bslab, hipStream_t s) {
    if constexpr (KT == 4) {
        if (a.xgelu) { k_wgrad_t<NT, KT, VEC, false, false, true><<<grid, 256, 0, s>>>(a, k_blocks, px, slab, bslab); return; }
    }
    if (a.ybf && a.xbf) k_wgrad_t<NT, KT, VEC, true, true><<<grid, 256, 0, s>>>(a, k_blocks, px, slab, bslab);
    else if (a.ybf) k_wgrad_t<NT, KT, VEC, true, false><<<grid, 256, 0, s>>>(a, k_blocks, px, slab, bslab);
    else if (a.xbf) k_wgrad_t<NT, KT, VEC, false, true><<<grid, 256, 0, s>>>(a, k_blocks, px, slab, bslab);
    else k_wgrad_t<NT, KT, VEC, false, false><<<grid, 256, 0, s>>>(a, k_blocks, px, slab, bslab);
}
template <int NT>
static void wgrad_dispatch_kt(int KT, const WgradArgs& a, dim3 grid, int k_blocks, long px, float* slab, float* bslab, hipStream_t s) {
    switch (KT) {
        case 1: wgrad_dispatch_bf<NT, 1, false>(a, grid, k_blocks, px, slab, bslab, s); break;
        case 2: wgrad_dispatch_bf<NT, 2, false>(a, grid, k_blocks, px, slab, bslab, s); break;
        case 3: wgrad_dispatch_bf<NT, 3, false>(a, grid, k_blocks, px, slab, bslab, s); break;
        default: wgrad_dispatch_bf<NT, 4, false>(a, grid, k_blocks, px, slab, bslab, s); break;
    }
}

int launch_wgrad(const WgradArgs& a, float* slab, hipStream_t s) {
    ProfScope prof__(LG_K_WGRAD, s);
    if ((a.N & 15) || (a.K & 15) || a.N <= 0 || a.K <= 0 || a.P <= 0) { lg_set_error("wgrad: N,K must be positive multiples of 16"); return -2; }
    if (a.n_valid > a.N || a.k_valid > a.K || a.n_valid > a.ldy || a.k_valid > a.ldx) { lg_set_error("wgrad: valid extents exceed the operands"); return -2; }
    const int NT = tiles_per_block(a.N / 16), KT = tiles_per_block(a.K / 16);
    if (a.xgelu && (KT != 4 || a.ybf || a.xbf)) { lg_set_error("wgrad: gelu(X) operands need fp32 storage and K a multiple of 64"); return -2; }
    const int n_blocks = a.N / (16 * NT), k_blocks = a.K / (16 * KT);
    const int blocks = n_blocks * k_blocks;
    long splits = wgrad_splits(a.N, a.K);
    long nslices = splits * 4;
    long px = (a.P + nslices - 1) / nslices;
    const bool vec = NT == 4 && KT == 4 && a.n_valid == a.N && a.k_valid == a.K && (a.ldy & 3) == 0 && (a.ldx & 3) == 0;
    const long batch = 4L * wgrad_batch(NT, KT, vec);
    px = (px + batch - 1) / batch * batch;   // whole batches
    // shrink the slice count if the tensor is small
    nslices = (a.P + px - 1) / px;
    splits = (nslices + 3) / 4;
    float* bslab = slab + splits * (long)a.N * a.K;
    dim3 grid((unsigned)splits, (unsigned)blocks);
    if (vec) wgrad_dispatch_bf<4, 4, true>(a, grid, k_blocks, px, slab, bslab, s);
    else switch (NT) {
        case 1: wgrad_dispatch_kt<1>(KT, a, grid, k_blocks, px, slab, bslab, s); break;
        case 2: wgrad_dispatch_kt<2>(KT, a, grid, k_blocks, px, slab, bslab, s); break;
        case 3: wgrad_dispatch_kt<3>(KT, a, grid, k_blocks, px, slab, bslab, s); break;
        default: wgrad_dispatch_kt<4>(KT, a, grid, k_blocks, px, slab, bslab, s); break;
    }
    LG_CHECK_LAUNCH();
    return launch_reduce_slab2(slab, splits, a.N, a.K, a.dW, a.ldw, a.n_valid, a.k_valid, a.db ? bslab : nullptr, a.N, a.db, a.n_valid, s);
}
