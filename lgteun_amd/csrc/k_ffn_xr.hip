// k_ffn_xr: the fused feed_forward half-block (reference models/common/LGT.py:91-109 + pre_norm / residual :45-61) at e = 16 as a
// REGISTER CHAIN (round 6) -- the local mixer's lane map (k_attn_m.hip) applied to the FFN:
//
//   y = x + W3 gelu( dw3x3( W2 gelu( W1 LN(x) + b1 ) + b2 ) ) + b3
//
// k_ffn_xs (k_ffn_x.hip, rounds 2 - 5) splits the hidden CHANNELS over the four waves of a workgroup: every wave needs all 64 channels
// of gelu(h1) for its 16 rows of GEMM2, so LN(x) and gelu(h1) cross LDS as operand pieces and a 48-pixel chunk costs three workgroup
// barriers -- eleven per 8-row step; the counters showed 52 % vector-active, 10 % matrix-busy and ~40 % of the SIMD's cycles in neither
// pipe at two waves per SIMD.  Here a wave owns PIXELS, not channels:
//
//   lane l = (g = l >> 4, c = l & 15): pixel c of a 16-pixel block; of that pixel the lane holds channels 4 g .. 4 g + 3 of x and, after a
//   product with the weights on the A side, rows 4 g + v of every 16-row output tile: channels 16 mt + 4 g + v of h1 / h2.
//
// That is at once (a) the coalesced 16-byte access for x, the residual and y, (b) the B operand of GEMM1 (k-slots 4 g + j = the lane's
// four channels), (c) the C layout of GEMM1 -- and the lane's sixteen h1 values, in the order (tile, v), ARE k-slots of GEMM2 as long as
// the weight fragments agree on which channel a slot means (they are built for it) -- (d) the C layout of GEMM2: float4 stores of h2
// into the halo ring, and (e) in the spatial phase the same map again: dw3x3 from the ring, gelu, GEMM3, residual, the next block's
// LayerNorm.  LN(x), gelu(h1) and gelu(h3) never touch LDS; a step has TWO workgroup barriers (ring rows complete / ring rows free);
// the weight fragments are staged once per workgroup as [fragment][lane] 16-byte units (a conflict-free ds_read_b128 per use).
//
// Work split of an 8-row step of a 16-column strip: the 8 x 18 halo pixels are nine 16-pixel blocks -- wave w takes blocks 2 w and
// 2 w + 1 together (two independent chains in one instruction stream: one block's GEMMs run under the other's GELU), the ninth goes to
// the waves in turn; then wave w takes tile rows 2 w, 2 w + 1 of the spatial phase (their 3 x 3 windows share two ring rows).
// Arithmetic: f16 pairs with the proven operand scales of k_ffn_prep.hip, exactly as k_ffn_xs<., 2> (split_bf16.h NP = 2).
// LDS 79.0 KB (two workgroups per CU): ring [10][18][68] fp32 | 28 weight fragments | depthwise taps [64][9] | biases.
#include "kernels.h"

#include "hstore.h"
#include "split_bf16.h"

// In-kernel phase stamps (diagnostic build only, -DLG_STAMPS: tools/mkvariant.sh + tools/xr_stamps.py): branch-free, every wave of every workgroup stores
// s_memtime at the phase boundaries of every step; no stamp executes in the product build.
#ifdef LG_STAMPS
__device__ unsigned long long g_xr_stamps[512 * 4 * 10 * 8];   // [workgroup][wave][step of the strip][stamp]
#define XSTAMP_AT(si_, i) do { unsigned long long t__; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)); \
                       g_xr_stamps[(((blockIdx.x & 511) * 4 + wave) * 10 + (si_)) * 8 + (i)] = t__; } while (0)
#define XSTAMP(i) do { unsigned long long t__; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)); \
                       g_xr_stamps[(((blockIdx.x & 511) * 4 + wave) * 10 + (stamp_si < 9 ? stamp_si : 9)) * 8 + (i)] = t__; } while (0)
extern "C" __attribute__((visibility("default"))) int lg_debug_xr_stamps(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_xr_stamps), sizeof(g_xr_stamps));
}
#else
#define XSTAMP_AT(si_, i) do { } while (0)
#define XSTAMP(i) do { } while (0)
#endif

namespace xr {

constexpr int E = 16, N1 = 64, TX = 16, HX = 18, TY = 8, RING = 10, LDR = 68;
constexpr int NF1 = 8, NF2 = 16, NF3 = 4, NFRAG = NF1 + NF2 + NF3;
constexpr int GRID = 512;          // resident workgroups (two per CU)
// Two workgroups share a CU and the SIMD arbiter issues the OLDER wave first: the workgroup dispatched first runs as if it were alone, the other gets what is
// left (profiles/r06_ffn_xr_fairness.txt; strip_geo below).  Tried: priority turns by the clock (step 5.299 -> 5.286 ms), the uneven split does better, DESIGN 3.7.
constexpr int UNEVEN = 16;         // rows (per 64-row strip) moved from the second workgroup of a CU to the first; 0: even strips
constexpr int MULTI_UNEVEN = 16;   // the same in the multi-stage instances, whose workgroups walk runs of strip pairs (kernels.h: stage_run_pairs); 0: even strip runs
                                   // (k_ffn_xr<0,2,true> over 3 x 32 pairs, us per launch on one box: even 212.3, 8 rows 208.7, 16 rows 200.9, 24 rows 203.7)
// the tables FIRST: a ds_read's immediate offset has 16 bits, and behind the 48 KB ring every fragment / tap row / bias vector needed a base
// register of its own (the first build: 28 + 16 + .. hoisted addresses, 206 spilled registers)
constexpr size_t OFF_W = 0;
constexpr size_t OFF_TAPS = OFF_W + (size_t)NFRAG * 64 * 16;
constexpr size_t OFF_PAR = OFF_TAPS + (size_t)N1 * 9 * 4;
constexpr int P_B1 = 0, P_B2 = 64, P_DWB = 128, P_B3 = 192, P_N1G = 208, P_N1B = 224, P_FLOATS = 240;
constexpr size_t OFF_RING = OFF_PAR + (size_t)P_FLOATS * 4;
constexpr size_t LDS_BYTES = OFF_RING + (size_t)RING * HX * LDR * 4;
static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
static_assert(OFF_RING % 16 == 0 && OFF_TAPS % 16 == 0 && OFF_PAR % 16 == 0, "16-byte aligned LDS regions");

// the saved tensors leave by plain stores (tried: streaming stores, whose 64-byte pieces only the L2 merges into lines: WRITE_SIZE 421 MB against 310 MB of data, slower)
// __builtin_amdgcn_sched_barrier(0) between the sections of a block: without these fences the scheduler interleaves every section of a step and spills (206 registers)
template <int N>
struct IC { static constexpr int value = N; };

// NP = 2: f16 pairs (the default arithmetic); NP = 1 (precision = 'bf16'): ONE round-to-nearest bf16 piece per operand, plain bf16 MFMAs, the tanh-form
// GELU and bf16 storage of the saved tensors, as the NP = 1 instances of k_ffn_xs
template <int NP>
__device__ __forceinline__ void pairN(float a, float b, uint32_t& hi, uint32_t& lo) {
    if (NP == 2) pair2(a, b, hi, lo);
    else {
        typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
        const bf16x2_t v = {(__bf16)a, (__bf16)b};      // v_cvt_pk_bf16_f32 (RNE)
        hi = __builtin_bit_cast(uint32_t, v);
        lo = 0u;
    }
}
// GEMM1 (K = 16): pairs: A = {w_lo | w_hi}, {w_hi | 0} against B = {x_hi | x_lo}, {x_hi | 0}; bf16: the second product alone
template <int NP>
__device__ __forceinline__ f32x4_t mfma_g1(u32x4_t wa, u32x4_t wb, u32x4_t xb1, u32x4_t xb2, f32x4_t acc) {
    if (NP == 2) {
        acc = mfma_h(wa, xb1, acc);
        return mfma_h(wb, xb2, acc);
    }
    return mfma_b(wb, xb2, acc);
}
template <int NP>
__device__ __forceinline__ lg_v2f geluN(lg_v2f x, const GeluK& k) {
    if constexpr (NP == 2) return gelu2_k(x, k);
    else return gelu2_t<true>(x);
}

}  // namespace xr

// SAVE: 0 nothing; 3 the pre-activations h2 and h3 (the backward re-computes h1 from x: k_ffn1_bwd_xs) -- the two modes of the default path
// MULTI: the launch covers the samples of several stages (kernels.h: StageSel); false: the segment loop below is ONE straight pass and the kernel the
// one-stage kernel it always was.
template <int SAVE, int NP, bool MULTI = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_ffn_xr(Ffn1Args a1_, Ffn2Args a2_, int tiles_x, int strips_y, int nstrips,
                                                                                       int SH, int dS) {
    using namespace xr;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* ring = reinterpret_cast<float*>(smem_raw + OFF_RING);             // [RING * HX][LDR] h2
    u32x4_t* sW = reinterpret_cast<u32x4_t*>(smem_raw + OFF_W);              // [NFRAG][64]
    float* sTaps = reinterpret_cast<float*>(smem_raw + OFF_TAPS);            // [16 quads][9 taps][4 channels of the quad]
    float* sPar = reinterpret_cast<float*>(smem_raw + OFF_PAR);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c_ = lane & 15, c = c_;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);   // provably wave-uniform: branches on it are scalar branches
    const int h = a2_.h, w = a2_.w;
    // The workgroup's strips.  One stage in the launch: strips blockIdx.x, + gridDim.x, ... and ONE pass of the segment loop below.  Several stages
    // (kernels.h: StageSel; strips ascend with the sample, so a stage is a contiguous range of them): a contiguous run of strips, cut into one segment
    // per stage -- at a stage boundary the tables are staged again, behind a barrier, from that stage's weights (at 3 x 32 pairs two workgroups of 512).
    const StageSel sg = a1_.sg;
    constexpr bool multi = MULTI;
    // dS != 0 (launcher: the 512 resident workgroups): the units of the run are strip PAIRS, and the two workgroups of a CU walk the same run of them -- the
    // first the tall strips, the second the short ones, at strip index pair + nstrips / 2.  The run is kept in strip indices (unit + base): the short strips of
    // stage st are then [(n + st) per_stage, (n + st + 1) per_stage), and no base stays live across the kernel
    const bool pairs = multi && dS != 0;
    const int per_stage = multi ? (sg.Bs * tiles_x * strips_y) >> (pairs ? 1 : 0) : nstrips;
    const StageRun rn = stage_run_halves(nstrips >> (pairs ? 1 : 0), (int)gridDim.x >> (pairs ? 1 : 0), (int)blockIdx.x);   // = stage_run_pairs : stage_run_even   (grid x strips < 2^31: both are
    const int run0 = multi ? __builtin_amdgcn_readfirstlane(rn.run0 + rn.base) : (int)blockIdx.x;                                                             //  below 2^15 x 2^16)
    const int run1 = multi ? __builtin_amdgcn_readfirstlane(rn.run1 + rn.base) : nstrips;
    const int rstep = multi ? 1 : (int)gridDim.x;
    int seg0 = run0;
    do {
    const int sq = multi ? __builtin_amdgcn_readfirstlane(seg0 / per_stage) : 0;   // (division runs on the vector pipe: kernels.h, stage_of)
    const int st = sq >= sg.n ? sq - sg.n : sq;                                    // (short strips: see above)
    const int seg1 = multi ? stage_seg_end(sq, run1, per_stage) : run1;
    Ffn1Args a1 = a1_;
    Ffn2Args a2 = a2_;
    {
        const long po = st * sg.pstride;
        a1.ln2g += po; a1.ln2b += po; a1.w1 += po; a1.b1 += po; a1.w2 += po; a1.b2 += po;
        a2.dww += po; a2.dwb += po; a2.w3 += po; a2.b3 += po;
        if (a2.g) { a2.n1g += po; a2.n1b += po; }
        if (NP == 2) a1.scales += st * sg.fs_stride;
    }
    if (seg0 != run0) __syncthreads();   // every wave is done with the previous stage's tables
    // operand scales (k_ffn_prep.hip; k_ffn_x.hip has the derivation): S1 h1, S2 h2, S3 (...) in the accumulators
    constexpr bool BF = NP == 1;
    float sx = 1.f, sa1 = 1.f, sa3 = 1.f, sw1 = 1.f, sw2 = 1.f, sw3 = 1.f;
    if (NP == 2) { sx = uniform_f(a1.scales[0]); sa1 = uniform_f(a1.scales[1]); sa3 = uniform_f(a1.scales[2]); sw1 = uniform_f(a1.scales[3]); sw2 = uniform_f(a1.scales[4]); sw3 = uniform_f(a1.scales[5]); }
    const float S1 = sx * sw1, S2 = sa1 * sw2, S3 = sa3 * sw3;
    const float inv2 = 1.0f / S2, inv3 = 1.0f / S3;   // (powers of two: exact)
    const GeluK gk1 = gelu_k(0.70710678118654752440f / S1, 0.5f * sa1 / S1), gk3 = gelu_k(0.70710678118654752440f, 0.5f * sa3);   // S1 h1 -> s_a1 gelu(h1); h3 -> s_a3 gelu(h3)

    // strip -> (column strip, sample, rows [Y0, Yend)).  dS != 0 (launcher: exactly two strips per CU, one per workgroup): the rows of two vertically adjacent
    // strips are split UNEVENLY, SH + dS to the strip of a workgroup of the first half of the grid and SH - dS to its neighbour's in the second half.  The
    // dispatcher places workgroups 0 .. 255 one per CU before the second 256, and the SIMD arbiter issues the OLDER wave first: the first workgroup of a CU runs as
    // if it were alone (13.1 k cycles per step), the second gets what is left (24 k per step) and used to finish 40 % later, alone on a half-empty CU
    // (profiles/r06_ffn_xr_fairness.txt: lifetimes 105 k / 148 k cycles, all of 0 .. 255 in the first group).  With 10 : 6 steps both are done at ~135 k.
    auto strip_geo = [&](int strip, int& tx_i, long& b, int& Y0, int& Yend) {
        if (dS) {
            const int half = nstrips >> 1, shortone = strip >= half ? 1 : 0;
            int p_ = strip - (shortone ? half : 0);
            tx_i = p_ % tiles_x;
            p_ /= tiles_x;
            const int hy2 = strips_y >> 1, ky = p_ % hy2;
            b = p_ / hy2;
            Y0 = ky * 2 * SH + (shortone ? SH + dS : 0);
            Yend = min(Y0 + (shortone ? SH - dS : SH + dS), h);
        } else {
            int t_ = strip;
            tx_i = t_ % tiles_x;
            t_ /= tiles_x;
            const int sy = t_ % strips_y;
            b = t_ / strips_y;
            Y0 = sy * SH;
            Yend = min(Y0 + SH, h);
        }
    };
    XSTAMP_AT(9, 0);
    // the prologue's x vector of this workgroup's FIRST strip: requested now, its HBM round trip runs under the table staging
    float4 xp_first;
    {
        int tx_i, Y0f, Yendf;
        long b;
        strip_geo(seg0, tx_i, b, Y0f, Yendf);
        const int m = 16 * (wave < 3 ? wave : 0) + c, hy = m / HX, hx = m - hy * HX;
        const int y = clampi(Y0f - 1 + hy, 0, h - 1), x = clampi(tx_i * TX + hx - 1, 0, w - 1);
        xp_first = *reinterpret_cast<const float4*>(a1.x + ((b * h + y) * (long)w + x) * E + 4 * g);
    }
    // ---- once per (persistent) workgroup: weight fragments, taps, biases
    float4 lng, lnb;
    {
        int t = threadIdx.x;
        if (MULTI) asm volatile("" : "+v"(t));   // (the staging addresses are formed again per segment: hoisted out of the segment loop they would hold ~30 registers for the whole kernel)
        const int ln = t >> 2, i = t & 3, lg = ln >> 4, lr = ln & 15;
        // every value is requested before the first store
        // taps, biases, LayerNorm affines: requested with the weights, from clamped indices (as a `for (k = t; ...; k += 256)` loop and two `if (t < n)`
        // blocks this was five further dependent round trips: 5 k of a launch's ~ 160 k cycles went to the staging)
        constexpr int NTP = (N1 * 9 + 255) / 256;
        float tp[NTP];
#pragma unroll
        for (int j = 0; j < NTP; ++j) {
            const int k = min(t + 256 * j, N1 * 9 - 1);
            tp[j] = a2.dww[(4 * (k / 36) + (k & 3)) * 9 + (k % 36) / 4];   // [quad][tap][u] <- dww[4 quad + u][tap]
        }
        const int tn = t < N1 ? t : N1 - 1, te = t < E ? t : E - 1;
        const float pb1 = a1.b1[tn], pb2 = a1.b2[tn], pdwb = a2.dwb[tn], pb3 = a2.b3[te];
        const float* const ng = a2.g ? a2.n1g : a2.b3;   // no planar half: any valid address, value unused
        const float* const nb_ = a2.g ? a2.n1b : a2.b3;
        const float png = ng[te], pnb = nb_[te];
        lng = *reinterpret_cast<const float4*>(a1.ln2g + 4 * g);
        lnb = *reinterpret_cast<const float4*>(a1.ln2b + 4 * g);
        float2 v1[4], v2[8], v3[2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) v1[mt] = *reinterpret_cast<const float2*>(a1.w1 + (size_t)(16 * mt + lr) * E + 4 * lg + 2 * (i & 1));
#pragma unroll
        for (int f = 0; f < 8; ++f) {   // f = mt2 * 2 + s: k-slots of dword i = channels 16 (2 s + (i >> 1)) + 4 lg + 2 (i & 1) + {0, 1}
            const int mt2 = f >> 1, s = f & 1;
            v2[f] = *reinterpret_cast<const float2*>(a1.w2 + (size_t)(16 * mt2 + lr) * N1 + 16 * (2 * s + (i >> 1)) + 4 * lg + 2 * (i & 1));
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) v3[s] = *reinterpret_cast<const float2*>(a2.w3 + (size_t)lr * N1 + 16 * (2 * s + (i >> 1)) + 4 * lg + 2 * (i & 1));
        __builtin_amdgcn_sched_barrier(0);   // every request above this line, every conversion and store below it
        uint32_t* d32 = reinterpret_cast<uint32_t*>(sW);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {   // GEMM1 (K = 16): two piece products share one 32-deep instruction: A = {w_lo | w_hi}, {w_hi | 0} against B = {x_hi | x_lo}, {x_hi | 0}
            uint32_t hi, lo;
            pairN<NP>(v1[mt].x * sw1, v1[mt].y * sw1, hi, lo);
            d32[(2 * mt) * 256 + t] = i < 2 ? lo : hi;
            d32[(2 * mt + 1) * 256 + t] = i < 2 ? hi : 0u;
        }
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            uint32_t hi, lo;
            pairN<NP>(v2[f].x * sw2, v2[f].y * sw2, hi, lo);
            d32[(NF1 + 2 * f) * 256 + t] = hi;
            d32[(NF1 + 2 * f + 1) * 256 + t] = lo;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            uint32_t hi, lo;
            pairN<NP>(v3[s].x * sw3, v3[s].y * sw3, hi, lo);
            d32[(NF1 + NF2 + 2 * s) * 256 + t] = hi;
            d32[(NF1 + NF2 + 2 * s + 1) * 256 + t] = lo;
        }
#pragma unroll
        for (int j = 0; j < NTP; ++j) asm volatile("" : "+v"(tp[j]));   // (or the load of the last, partial trip sinks into its store's `if`, with a wait of its own)
#pragma unroll
        for (int j = 0; j < NTP; ++j)
            if (t + 256 * j < N1 * 9) sTaps[t + 256 * j] = tp[j];
        if (t < N1) { sPar[P_B1 + t] = pb1 * S1; sPar[P_B2 + t] = pb2 * S2; sPar[P_DWB + t] = pdwb; }
        if (t < E) {
            sPar[P_B3 + t] = pb3 * S3;
            sPar[P_N1G + t] = a2.g ? png : 0.f;
            sPar[P_N1B + t] = a2.g ? pnb : 0.f;
        }
    }
    // LayerNorm affine of the lane's four channels, with the operand scale folded in
    lng = make_float4(lng.x * sx, lng.y * sx, lng.z * sx, lng.w * sx);
    lnb = make_float4(lnb.x * sx, lnb.y * sx, lnb.z * sx, lnb.w * sx);
    __syncthreads();
    XSTAMP_AT(9, 1);

#pragma unroll 1
    for (int strip = seg0; strip < seg1; strip += rstep) {
        int tx_i, Y0, Yend;
        long b;
        strip_geo(strip, tx_i, b, Y0, Yend);
        const int x0 = tx_i * TX;

        // x vector of the lane's pixel of halo block blk of the row block starting at ya: unconditional, from a clamped (always valid) address
        auto xload = [&](int ya, int blk) -> float4 {
            const int m = 16 * blk + c;
            const int hy = m / HX, hx = m - hy * HX;
            const int y = clampi(ya + hy, 0, h - 1), x = clampi(x0 + hx - 1, 0, w - 1);
            return *reinterpret_cast<const float4*>(a1.x + ((b * h + y) * (long)w + x) * E + 4 * g);
        };

        // h2 of NB halo blocks (blk0, blk0 + 1, ..) of halo rows [ya, ..) -> ring.  LN -> GEMM1 -> GELU -> GEMM2, all in registers.
        // PART 0: the whole block.  The NINTH block of a step is split between two waves along the hidden channels (a whole block on one wave
        // held the other three at the barrier for 22 % of a step): PART 1 = h1 tiles 0, 1 = k-step 0 of GEMM2, with the bias, stored to the ring;
        // PART 2 = tiles 2, 3 = k-step 1, kept in registers (`part`) and ADDED to the ring behind the barrier by ninth_add() -- on the wave that owns
        // the step's last two tile rows, the only reader of those ring pixels before the next barrier.
        // Every LDS operand is requested a section ahead of its use (a section = the code between two scheduling fences): the weight fragments of
        // GEMM1 in front of the LayerNorm arithmetic, those of GEMM2's first tile in front of the GELUs, each further tile's behind the previous
        // tile's MFMAs, whose results leave one tile later.
        struct Geo { float mk; int rp; bool inner; uint32_t prow; };   // prow: element index into the saved h2 (32 bits: the launcher checks the tensor's size)
        auto halo = [&](auto nbc, auto partc, int ya, int npx, int blk0, const float4* xin, f32x4_t* part, Geo* geo_out) {
            constexpr int NB = decltype(nbc)::value, PART = decltype(partc)::value;
            constexpr int MT0 = PART == 2 ? 2 : 0, NMT = PART == 0 ? 4 : 2;      // h1 tiles [MT0, MT0 + NMT)
            constexpr int S0 = PART == 2 ? 1 : 0, NS = PART == 0 ? 2 : 1;        // k-steps of GEMM2
            int c = c_;
            asm volatile("" : "+v"(c));    // the block geometry (row / column of the lane's halo pixel) is re-derived per call: as loop invariants of the
                                            // step loop its ~30 values per lane were hoisted and spilled
            const int ring0 = ((ya - Y0 + 1) % RING) * HX;
            // GEMM1's fragments and biases: in flight under the LayerNorm
            u32x4_t wa[NMT], wb[NMT];
            float4 b1v[NMT];
#pragma unroll
            for (int i = 0; i < NMT; ++i) {
                wa[i] = sW[(2 * (MT0 + i)) * 64 + lane];
                wb[i] = sW[(2 * (MT0 + i) + 1) * 64 + lane];
                b1v[i] = *reinterpret_cast<const float4*>(sPar + P_B1 + 16 * (MT0 + i) + 4 * g);
            }
            u32x4_t xb1[NB], xb2[NB];
            Geo geo[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int m = 16 * (blk0 + nb) + c;
                const int hy = m / HX, hx = m - hy * HX;
                const int y = ya + hy, x = x0 + hx - 1;
                const bool in = m < npx && y >= 0 && y < h && x >= 0 && x < w;
                geo[nb].mk = in ? inv2 : 0.0f;            // dep_conv zero-pads h2; the mask also takes S2 out of the accumulator
                int r_ = ring0 + m;
                r_ = r_ >= RING * HX ? r_ - RING * HX : r_;
                geo[nb].rp = m < npx ? r_ : -1;
                geo[nb].inner = SAVE && m < npx && hx >= 1 && hx <= TX && x < w && y >= Y0 && y < Yend;
                geo[nb].prow = (uint32_t)(((b * h + y) * (long)w + x) * N1 + 4 * g);
                const float4 xv = xin[nb];
                const float s = xg_sum((xv.x + xv.y) + (xv.z + xv.w));
                const float mu = s * (1.0f / E);
                const float d0 = xv.x - mu, d1 = xv.y - mu, d2 = xv.z - mu, d3 = xv.w - mu;
                const float vs = xg_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
                const float rstd = __builtin_amdgcn_rsqf(vs * (1.0f / E) + LG_EPS);
                uint32_t h01, l01, h23, l23;
                pairN<NP>(d0 * rstd * lng.x + lnb.x, d1 * rstd * lng.y + lnb.y, h01, l01);
                pairN<NP>(d2 * rstd * lng.z + lnb.z, d3 * rstd * lng.w + lnb.w, h23, l23);
                xb1[nb] = (u32x4_t){h01, h23, l01, l23};
                xb2[nb] = (u32x4_t){h01, h23, 0u, 0u};
            }
            __builtin_amdgcn_sched_barrier(0);
            // ---- GEMM1: every tile's MFMAs are issued before the first GELU reads a result
            f32x4_t a1c[NB][NMT];
#pragma unroll
            for (int i = 0; i < NMT; ++i)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    f32x4_t acc = {b1v[i].x, b1v[i].y, b1v[i].z, b1v[i].w};
                    a1c[nb][i] = mfma_g1<NP>(wa[i], wb[i], xb1[nb], xb2[nb], acc);
                }
            // GEMM2's first tile: fragments and bias requested now, in flight under the GELUs
            u32x4_t wh[NS], wl[NS];
            float4 b2v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int s = 0; s < NS; ++s) { wh[s] = sW[(NF1 + 2 * (S0 + s)) * 64 + lane]; wl[s] = sW[(NF1 + 2 * (S0 + s) + 1) * 64 + lane]; }
            if (PART != 2) b2v = *reinterpret_cast<const float4*>(sPar + P_B2 + 4 * g);
            __builtin_amdgcn_sched_barrier(0);
            // ---- GELU -> f16 pairs of s_a1 gelu(h1): hi / lo [tile][channel pair]
            uint32_t ghi[NB][NMT][2], glo[NB][NMT][2];
#pragma unroll
            for (int i = 0; i < NMT; ++i) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const lg_v2f a01 = geluN<NP>((lg_v2f){a1c[nb][i][0], a1c[nb][i][1]}, gk1);
                    const lg_v2f a23 = geluN<NP>((lg_v2f){a1c[nb][i][2], a1c[nb][i][3]}, gk1);
                    pairN<NP>(a01.x, a01.y, ghi[nb][i][0], glo[nb][i][0]);
                    pairN<NP>(a23.x, a23.y, ghi[nb][i][1], glo[nb][i][1]);
                    asm volatile("" : "+v"(ghi[nb][i][0]), "+v"(glo[nb][i][0]), "+v"(ghi[nb][i][1]), "+v"(glo[nb][i][1]));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- GEMM2 (K = 64: two 32-deep steps, k-slot j of step s = channel 16 (2 s + (j >> 2)) + 4 g + (j & 3)) -> ring (+ save)
            // h2 = (b2 + k-step 0) mk + (k-step 1) mk, the two k-steps in accumulators of their own and joined by ONE fma: the form in which a
            // split ninth block (k-step 0 stored, k-step 1 added behind the barrier) gives bit for bit what a whole block gives -- which pixels fall
            // into a ninth block depends on the strip partition, i.e. on the batch size, and a pixel's value must not
            auto leave = [&](int mt2, const f32x4_t (&k0)[NB], const f32x4_t (&k1)[NB]) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    if (PART == 2) { part[mt2] = k1[nb]; continue; }
                    const float mk = geo[nb].mk;
                    float4 hh = make_float4(k0[nb][0] * mk, k0[nb][1] * mk, k0[nb][2] * mk, k0[nb][3] * mk);
                    if (PART == 0) hh = make_float4(__builtin_fmaf(k1[nb][0], mk, hh.x), __builtin_fmaf(k1[nb][1], mk, hh.y), __builtin_fmaf(k1[nb][2], mk, hh.z), __builtin_fmaf(k1[nb][3], mk, hh.w));
                    if (SAVE && PART == 0 && geo[nb].inner) HS<BF>::st4(a1.h2, geo[nb].prow + 16 * mt2, hh);
                    if (geo[nb].rp >= 0) *reinterpret_cast<float4*>(ring + geo[nb].rp * LDR + 16 * mt2 + 4 * g) = hh;
                }
            };
            f32x4_t accp0[NB], accp1[NB];
#pragma unroll
            for (int mt2 = 0; mt2 < 4; ++mt2) {
                f32x4_t acc0[NB], acc1[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) { acc0[nb] = (f32x4_t){b2v.x, b2v.y, b2v.z, b2v.w}; acc1[nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        const u32x4_t bh = {ghi[nb][2 * s][0], ghi[nb][2 * s][1], ghi[nb][2 * s + 1][0], ghi[nb][2 * s + 1][1]};
                        const u32x4_t bl = {glo[nb][2 * s][0], glo[nb][2 * s][1], glo[nb][2 * s + 1][0], glo[nb][2 * s + 1][1]};
                        f32x4_t& acc = (S0 + s) == 0 ? acc0[nb] : acc1[nb];
                        acc = mfma3<NP>(wh[s], wl[s], bh, bl, acc);
                    }
                if (mt2 < 3) {   // the next tile's operands: requested behind this tile's MFMAs
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        wh[s] = sW[(NF1 + 2 * (2 * (mt2 + 1) + S0 + s)) * 64 + lane];
                        wl[s] = sW[(NF1 + 2 * (2 * (mt2 + 1) + S0 + s) + 1) * 64 + lane];
                    }
                    if (PART != 2) b2v = *reinterpret_cast<const float4*>(sPar + P_B2 + 16 * (mt2 + 1) + 4 * g);
                }
                if (mt2 > 0) leave(mt2 - 1, accp0, accp1);   // the previous tile's results leave while this tile's MFMAs run
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) { accp0[nb] = acc0[nb]; accp1[nb] = acc1[nb]; }
                __builtin_amdgcn_sched_barrier(0);
            }
            leave(3, accp0, accp1);
            if (PART == 2) *geo_out = geo[0];
        };
        // Two whole blocks as ONE software pipeline (the step's main work): block A's GEMM2 tile j (6 MFMAs) is issued in the section that holds block
        // B's GELU of tile j -- matrix and vector work side by side in one instruction stream, whatever the SIMD's other wave is doing (two
        // co-resident workgroups start in lockstep: with both waves of a SIMD in their GELUs, then both in their GEMM2s, steps took 17.4 k ticks
        // against 13.0 k once the workgroups had drifted apart).
        auto halo_pair = [&](int ya, int blk0, const float4* xin) {
            int c = c_;
            asm volatile("" : "+v"(c));
            const int ring0 = ((ya - Y0 + 1) % RING) * HX;
            u32x4_t wa[4], wb[4];
            float4 b1v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                wa[i] = sW[(2 * i) * 64 + lane];
                wb[i] = sW[(2 * i + 1) * 64 + lane];
                b1v[i] = *reinterpret_cast<const float4*>(sPar + P_B1 + 16 * i + 4 * g);
            }
            u32x4_t xb1[2], xb2[2];
            Geo geo[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int m = 16 * (blk0 + nb) + c;
                const int hy = m / HX, hx = m - hy * HX;
                const int y = ya + hy, x = x0 + hx - 1;
                const bool in = y >= 0 && y < h && x >= 0 && x < w;
                geo[nb].mk = in ? inv2 : 0.0f;
                int r_ = ring0 + m;
                r_ = r_ >= RING * HX ? r_ - RING * HX : r_;
                geo[nb].rp = r_;
                geo[nb].inner = SAVE && hx >= 1 && hx <= TX && x < w && y >= Y0 && y < Yend;
                geo[nb].prow = (uint32_t)(((b * h + y) * (long)w + x) * N1 + 4 * g);
                const float4 xv = xin[nb];
                const float s = xg_sum((xv.x + xv.y) + (xv.z + xv.w));
                const float mu = s * (1.0f / E);
                const float d0 = xv.x - mu, d1 = xv.y - mu, d2 = xv.z - mu, d3 = xv.w - mu;
                const float vs = xg_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
                const float rstd = __builtin_amdgcn_rsqf(vs * (1.0f / E) + LG_EPS);
                uint32_t h01, l01, h23, l23;
                pairN<NP>(d0 * rstd * lng.x + lnb.x, d1 * rstd * lng.y + lnb.y, h01, l01);
                pairN<NP>(d2 * rstd * lng.z + lnb.z, d3 * rstd * lng.w + lnb.w, h23, l23);
                xb1[nb] = (u32x4_t){h01, h23, l01, l23};
                xb2[nb] = (u32x4_t){h01, h23, 0u, 0u};
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x4_t a1c[2][4];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    f32x4_t acc = {b1v[i].x, b1v[i].y, b1v[i].z, b1v[i].w};
                    a1c[nb][i] = mfma_g1<NP>(wa[i], wb[i], xb1[nb], xb2[nb], acc);
                }
            u32x4_t wh[2], wl[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) { wh[s] = sW[(NF1 + 2 * s) * 64 + lane]; wl[s] = sW[(NF1 + 2 * s + 1) * 64 + lane]; }
            float4 b2v = *reinterpret_cast<const float4*>(sPar + P_B2 + 4 * g);
            __builtin_amdgcn_sched_barrier(0);
            uint32_t ghi[2][4][2], glo[2][4][2];
            auto gelu_tile = [&](int nb, int i) {
                const lg_v2f a01 = geluN<NP>((lg_v2f){a1c[nb][i][0], a1c[nb][i][1]}, gk1);
                const lg_v2f a23 = geluN<NP>((lg_v2f){a1c[nb][i][2], a1c[nb][i][3]}, gk1);
                pairN<NP>(a01.x, a01.y, ghi[nb][i][0], glo[nb][i][0]);
                pairN<NP>(a23.x, a23.y, ghi[nb][i][1], glo[nb][i][1]);
                asm volatile("" : "+v"(ghi[nb][i][0]), "+v"(glo[nb][i][0]), "+v"(ghi[nb][i][1]), "+v"(glo[nb][i][1]));
            };
            struct Acc2 { f32x4_t k0, k1; };     // the two k-steps in accumulators of their own (see `halo`: bitwise the split ninth block's arithmetic)
            auto gemm2_tile = [&](int nb) -> Acc2 {
                Acc2 r;
                r.k0 = (f32x4_t){b2v.x, b2v.y, b2v.z, b2v.w};
                r.k1 = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const u32x4_t bh = {ghi[nb][2 * s][0], ghi[nb][2 * s][1], ghi[nb][2 * s + 1][0], ghi[nb][2 * s + 1][1]};
                    const u32x4_t bl = {glo[nb][2 * s][0], glo[nb][2 * s][1], glo[nb][2 * s + 1][0], glo[nb][2 * s + 1][1]};
                    f32x4_t& acc = s == 0 ? r.k0 : r.k1;
                    acc = mfma3<NP>(wh[s], wl[s], bh, bl, acc);
                }
                return r;
            };
            auto next_w2 = [&](int mt2) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    wh[s] = sW[(NF1 + 2 * (2 * mt2 + s)) * 64 + lane];
                    wl[s] = sW[(NF1 + 2 * (2 * mt2 + s) + 1) * 64 + lane];
                }
                b2v = *reinterpret_cast<const float4*>(sPar + P_B2 + 16 * mt2 + 4 * g);
            };
            auto leave = [&](int nb, int mt2, const Acc2& acc) {
                const float mk = geo[nb].mk;
                const float4 hh = make_float4(__builtin_fmaf(acc.k1[0], mk, acc.k0[0] * mk), __builtin_fmaf(acc.k1[1], mk, acc.k0[1] * mk),
                                              __builtin_fmaf(acc.k1[2], mk, acc.k0[2] * mk), __builtin_fmaf(acc.k1[3], mk, acc.k0[3] * mk));
                if (SAVE && geo[nb].inner) HS<BF>::st4(a1.h2, geo[nb].prow + 16 * mt2, hh);
                *reinterpret_cast<float4*>(ring + geo[nb].rp * LDR + 16 * mt2 + 4 * g) = hh;
            };
#pragma unroll
            for (int i = 0; i < 4; ++i) { gelu_tile(0, i); __builtin_amdgcn_sched_barrier(0); }
            Acc2 accp;
#pragma unroll
            for (int j = 0; j < 4; ++j) {        // block A's GEMM2 tile j beside block B's GELU of tile j
                const Acc2 acc = gemm2_tile(0);
                next_w2(j < 3 ? j + 1 : 0);
                gelu_tile(1, j);
                if (j > 0) leave(0, j - 1, accp);
                accp = acc;
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {        // block B's GEMM2; the previous tile's results leave beside it
                const Acc2 acc = gemm2_tile(1);
                if (j < 3) next_w2(j + 1);
                leave(j > 0 ? 1 : 0, j > 0 ? j - 1 : 3, accp);
                accp = acc;
                __builtin_amdgcn_sched_barrier(0);
            }
            leave(1, 3, accp);
        };
        // the second half of a split ninth block joins the first in the ring (and, in the saving instance, leaves for HBM as the sum)
        auto ninth_add = [&](const f32x4_t (&part)[4], const Geo& ge) {
            if (ge.rp < 0) return;
#pragma unroll
            for (int mt2 = 0; mt2 < 4; ++mt2) {
                float4* rp4 = reinterpret_cast<float4*>(ring + ge.rp * LDR + 16 * mt2 + 4 * g);
                float4 r = *rp4;
                r = make_float4(__builtin_fmaf(part[mt2][0], ge.mk, r.x), __builtin_fmaf(part[mt2][1], ge.mk, r.y), __builtin_fmaf(part[mt2][2], ge.mk, r.z), __builtin_fmaf(part[mt2][3], ge.mk, r.w));
                *rp4 = r;
                if (SAVE && ge.inner) HS<BF>::st4(a1.h2, ge.prow + 16 * mt2, r);
            }
        };

        // ---- strip prologue: halo rows Y0 - 1, Y0 (36 pixels: blocks 0 .. 2, one per wave).  Its x vector (the workgroup's first strip: requested in
        // front of the table staging) and the first step's are in flight before anything is computed
        float4 xh[3];
        {
            const float4 xp = strip == seg0 ? xp_first : xload(Y0 - 1, wave < 3 ? wave : 0);
            xh[0] = xload(Y0 + 1, 2 * wave); xh[1] = xload(Y0 + 1, 2 * wave + 1); xh[2] = xload(Y0 + 1, 8);
            __syncthreads();     // the previous strip's spatial phase is done with the ring
            if (uwave < 3) halo(IC<1>{}, IC<0>{}, Y0 - 1, 2 * HX, wave, &xp, nullptr, nullptr);
            XSTAMP_AT(9, 2);
        }
#pragma unroll 1
        for (int y0 = Y0; y0 < Yend; y0 += TY) {
            const int si = (y0 - Y0) >> 3;
            // roles rotate with the step: `role` 3 owns tile rows 6, 7 and the second half of the ninth block, role 1 its first half
            const int role = (uwave + si) & 3, ty0 = 2 * role;
#ifdef LG_STAMPS
            const int stamp_si = si;
#endif
            XSTAMP(0);
            // the residual rows of the spatial phase, requested a phase ahead
            float4 xres[2];
#pragma unroll
            for (int r2 = 0; r2 < 2; ++r2) {
                const int y = min(y0 + ty0 + r2, h - 1), x = min(x0 + c, w - 1);
                xres[r2] = *reinterpret_cast<const float4*>(a2.x + ((b * h + y) * (long)w + x) * E + 4 * g);
            }
            halo_pair(y0 + 1, 2 * wave, xh);
            XSTAMP(1);
            f32x4_t part9[4];
            Geo geo9;
            if (role == 1) halo(IC<1>{}, IC<1>{}, y0 + 1, TY * HX, 8, xh + 2, nullptr, nullptr);
            if (role == 3) halo(IC<1>{}, IC<2>{}, y0 + 1, TY * HX, 8, xh + 2, part9, &geo9);
            XSTAMP(2);
            // next step's halo operands: in flight across the spatial phase (clamped addresses: harmless behind the last step)
            xh[0] = xload(y0 + TY + 1, 2 * wave); xh[1] = xload(y0 + TY + 1, 2 * wave + 1); xh[2] = xload(y0 + TY + 1, 8);
            __syncthreads();     // ring rows y0 - 1 .. y0 + 8 complete (but for the ninth block's second half)
            XSTAMP(3);
            if (role == 3) ninth_add(part9, geo9);
            // ---- spatial phase: tile rows ty0, ty0 + 1: dw3x3 over the ring -> gelu -> GEMM3 -> + bias + residual -> y (+ planar LN half)
            {
                const int sbase = (y0 - Y0) % RING;
                const float* rrow[4];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    int sl = sbase + ty0 + r4;
                    sl = sl >= RING ? sl - RING : sl;
                    sl = sl >= RING ? sl - RING : sl;
                    rrow[r4] = ring + (sl * HX + c) * LDR + 4 * g;
                }
                float h3[2][4][4];
                // sixteen sections (channel quad m, ring row r4); each requests the next one's three ring vectors, section (m, 1) the next quad's taps
                // (stored pair-interleaved, [quad][tap][channel of the quad]: one 16-byte read IS the two packed operands of a tap)
                float4 tq[9], tqn[9], rv[3], rvn[3], bq, bqn;
#pragma unroll
                for (int k = 0; k < 9; ++k) { tq[k] = *reinterpret_cast<const float4*>(sTaps + 36 * g + 4 * k); tqn[k] = tq[k]; }
                bq = *reinterpret_cast<const float4*>(sPar + P_DWB + 4 * g); bqn = bq;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) rv[dx] = *reinterpret_cast<const float4*>(rrow[0] + dx * LDR);
                lg_v2f acc01[2], acc23[2];
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    const int m = it >> 2, r4 = it & 3;
                    if (r4 == 0) {
                        acc01[0] = acc01[1] = (lg_v2f){bq.x, bq.y};
                        acc23[0] = acc23[1] = (lg_v2f){bq.z, bq.w};
                    }
                    if (it < 15) {
                        const int mn = (it + 1) >> 2, rn = (it + 1) & 3;
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) rvn[dx] = *reinterpret_cast<const float4*>(rrow[rn] + dx * LDR + 16 * mn);
                    }
                    if (r4 == 1 && m < 3) {
#pragma unroll
                        for (int k = 0; k < 9; ++k) tqn[k] = *reinterpret_cast<const float4*>(sTaps + 36 * (4 * (m + 1) + g) + 4 * k);
                        bqn = *reinterpret_cast<const float4*>(sPar + P_DWB + 16 * (m + 1) + 4 * g);
                    }
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const lg_v2f v01 = (lg_v2f){rv[dx].x, rv[dx].y}, v23 = (lg_v2f){rv[dx].z, rv[dx].w};
                        if (r4 <= 2) {
                            const float4 t4 = tq[r4 * 3 + dx];
                            acc01[0] = (lg_v2f){t4.x, t4.y} * v01 + acc01[0]; acc23[0] = (lg_v2f){t4.z, t4.w} * v23 + acc23[0];
                        }
                        if (r4 >= 1) {
                            const float4 t4 = tq[(r4 - 1) * 3 + dx];
                            acc01[1] = (lg_v2f){t4.x, t4.y} * v01 + acc01[1]; acc23[1] = (lg_v2f){t4.z, t4.w} * v23 + acc23[1];
                        }
                    }
                    // (a scheduling fence alone does not do it: the instruction order the scheduler starts from had the second row's chain of every quad
                    //  behind the first rows of all four, its twelve ring vectors spilled; an empty asm that "modifies" the sums pins them here)
                    asm volatile("" : "+v"(acc01[0]), "+v"(acc23[0]), "+v"(acc01[1]), "+v"(acc23[1]));
                    if (r4 == 3) {
#pragma unroll
                        for (int r2 = 0; r2 < 2; ++r2) { h3[r2][m][0] = acc01[r2].x; h3[r2][m][1] = acc01[r2].y; h3[r2][m][2] = acc23[r2].x; h3[r2][m][3] = acc23[r2].y; }
#pragma unroll
                        for (int k = 0; k < 9; ++k) tq[k] = tqn[k];
                        bq = bqn;
                    }
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) rv[dx] = rvn[dx];
                    __builtin_amdgcn_sched_barrier(0);
                }
                // GEMM3's fragments, bias, the next block's LayerNorm affine: requested in front of the GELUs
                u32x4_t w3h[2], w3l[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) { w3h[s] = sW[(NF1 + NF2 + 2 * s) * 64 + lane]; w3l[s] = sW[(NF1 + NF2 + 2 * s + 1) * 64 + lane]; }
                const float4 b3v = *reinterpret_cast<const float4*>(sPar + P_B3 + 4 * g);
                const float4 ng = *reinterpret_cast<const float4*>(sPar + P_N1G + 4 * g), nbv = *reinterpret_cast<const float4*>(sPar + P_N1B + 4 * g);
#pragma unroll
                for (int r2 = 0; r2 < 2; ++r2) {
                    const int y = y0 + ty0 + r2, x = x0 + c;
                    const bool ok = y < Yend && x < w;
                    uint32_t phi[4][2], plo[4][2];
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        if (SAVE && ok && a2.a3s) HS<BF>::st4(a2.a3s, ((b * h + y) * (long)w + x) * N1 + 16 * m + 4 * g, make_float4(h3[r2][m][0], h3[r2][m][1], h3[r2][m][2], h3[r2][m][3]));
                        const lg_v2f a01 = geluN<NP>((lg_v2f){h3[r2][m][0], h3[r2][m][1]}, gk3);
                        const lg_v2f a23 = geluN<NP>((lg_v2f){h3[r2][m][2], h3[r2][m][3]}, gk3);
                        pairN<NP>(a01.x, a01.y, phi[m][0], plo[m][0]);
                        pairN<NP>(a23.x, a23.y, phi[m][1], plo[m][1]);
                    }
                    f32x4_t o = {b3v.x, b3v.y, b3v.z, b3v.w};
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const u32x4_t bh = {phi[2 * s][0], phi[2 * s][1], phi[2 * s + 1][0], phi[2 * s + 1][1]};
                        const u32x4_t bl = {plo[2 * s][0], plo[2 * s][1], plo[2 * s + 1][0], plo[2 * s + 1][1]};
                        o = mfma3<NP>(w3h[s], w3l[s], bh, bl, o);
                    }
                    // ---- epilogue in registers: residual, store, LayerNorm statistics of the next block across the four lane groups
                    const float o0 = o[0] * inv3 + xres[r2].x, o1 = o[1] * inv3 + xres[r2].y, o2 = o[2] * inv3 + xres[r2].z, o3 = o[3] * inv3 + xres[r2].w;
                    if (ok) *reinterpret_cast<float4*>(a2.y + ((b * h + y) * (long)w + x) * E + 4 * g) = make_float4(o0, o1, o2, o3);
                    if (a2.g) {
                        const float s = xg_sum((o0 + o1) + (o2 + o3));
                        const float mu = s * (1.0f / E);
                        const float d0 = o0 - mu, d1 = o1 - mu, d2 = o2 - mu, d3 = o3 - mu;
                        const float vs = xg_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
                        const float rstd = __builtin_amdgcn_rsqf(vs * (1.0f / E) + LG_EPS);
                        if (ok && g >= 2) {      // channels 8..15 = the global-mixer half, planar [B, e/2, h, w]
                            const long hw = (long)h * w, sp = (long)y * w + x;
                            float* dst = a2.g + (b * (E / 2) + (4 * g - E / 2)) * hw + sp;
                            dst[0] = d0 * rstd * ng.x + nbv.x;
                            dst[hw] = d1 * rstd * ng.y + nbv.y;
                            dst[2 * hw] = d2 * rstd * ng.z + nbv.z;
                            dst[3 * hw] = d3 * rstd * ng.w + nbv.w;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            XSTAMP(4);
            __syncthreads();     // the ring rows this step read are free for the next step's halo pass
            XSTAMP(5);
        }   // steps of the strip
    }   // strips of this segment
    seg0 = seg1;
    } while (MULTI && seg0 < run1);   // segments (stages) of this workgroup
}

// The launch geometry (host only; lg_debug_stage_decision reports it).  n <= 1: one stage of B samples.
XrGeo ffn_xr_geometry(int h, int w, int B, int Bs, int n, int grid_cap) {
    // several stages in the launch: the strip height of ONE stage's launch, so that a workgroup gets whole strips of that size -- three at 3 x 32 pairs
    const bool multi = n > 1;
    XrGeo q{strip_geometry(h, w, B, multi ? Bs : B, xr::GRID, multi ? grid_cap : 0), 0};
    const int SH = q.SH;
    // uneven split of strip pairs (strip_geo in the kernel): only in the shapes it was measured in, exactly two workgroups per CU.  One stage: one strip per
    // workgroup.  Several: the 512 resident workgroups (a capped grid is smaller and keeps the even strip runs), each pair of them on a run of strip pairs.
    const bool shape_ok = xr::GRID == 512 && (q.strips_y & 1) == 0 && SH >= 32 && h % (2 * SH) == 0;
    if (!multi && xr::UNEVEN && q.nstrips == xr::GRID && shape_ok) q.dS = (SH * xr::UNEVEN / 64 + 7) / 8 * 8;
    if (multi && xr::MULTI_UNEVEN && q.grid == xr::GRID && (q.grid & 1) == 0 && shape_ok) q.dS = (SH * xr::MULTI_UNEVEN / 64 + 7) / 8 * 8;
    return q;
}

int launch_ffn_xr(const Ffn1Args& a1, const Ffn2Args& a2, hipStream_t s) {
    using namespace xr;
    ProfScope prof__(LG_K_FFN2, s, a1.sg.n);
    static DeviceOnce attr_once;
    if (int rc = lds_attr_once(attr_once, "ffn_xr", (int)LDS_BYTES,
                                     k_ffn_xr<0, 2>, k_ffn_xr<3, 2>, k_ffn_xr<0, 1>, k_ffn_xr<3, 1>, k_ffn_xr<0, 2, true>, k_ffn_xr<0, 1, true>)) return rc;
    if (!a1.hbf && !a1.scales) { lg_set_error("ffn_xr: the f16-pair instance needs the operand scales"); return -2; }
    const bool save = a1.h2 != nullptr;
    if (save && (a1.a1s || a1.g1s || a2.g3s)) { lg_set_error("ffn_xr: saves h2 / h3 (or h2 alone: a3s null, the backward re-computes h3) only"); return -2; }
    if ((long)a2.B * a2.h * a2.w * N1 >= (1ll << 32)) { lg_set_error("ffn_xr: hidden tensor of %ld elements exceeds the 32-bit save index", (long)a2.B * a2.h * a2.w * N1); return -2; }
    const bool multi = a1.sg.n > 1;
    if (multi && (save || a1.sg.Bs <= 0 || a2.B != a1.sg.n * a1.sg.Bs)) { lg_set_error("ffn_xr: B = %d is not %d stages of %d samples", a2.B, a1.sg.n, a1.sg.Bs); return -2; }
    const XrGeo geo = ffn_xr_geometry(a2.h, a2.w, a2.B, a1.sg.Bs, a1.sg.n, a1.sg.grid_cap);
    const int tiles_x = geo.tiles_x, strips_y = geo.strips_y, nstrips = geo.nstrips, SH = geo.SH, grid = geo.grid, dS = geo.dS;
    if (a1.hbf) {    // precision = 'bf16'
        if (save) k_ffn_xr<3, 1><<<grid, 256, LDS_BYTES, s>>>(a1, a2, tiles_x, strips_y, nstrips, SH, dS);
        else if (multi) k_ffn_xr<0, 1, true><<<grid, 256, LDS_BYTES, s>>>(a1, a2, tiles_x, strips_y, nstrips, SH, dS);
        else k_ffn_xr<0, 1><<<grid, 256, LDS_BYTES, s>>>(a1, a2, tiles_x, strips_y, nstrips, SH, dS);
    } else if (save) k_ffn_xr<3, 2><<<grid, 256, LDS_BYTES, s>>>(a1, a2, tiles_x, strips_y, nstrips, SH, dS);
    else if (multi) k_ffn_xr<0, 2, true><<<grid, 256, LDS_BYTES, s>>>(a1, a2, tiles_x, strips_y, nstrips, SH, dS);
    else k_ffn_xr<0, 2><<<grid, 256, LDS_BYTES, s>>>(a1, a2, tiles_x, strips_y, nstrips, SH, dS);
    LG_CHECK_LAUNCH();
    return 0;
}
