// k_ffn_dw_bwd_h: the spatial half of the feed_forward backward at e = 16 WITHOUT a saved h3 (round 6; VERDICT r5 lever b) -- reference
// models/common/LGT.py:91-109: net.4, the second GELU and the depthwise 3x3 of net.2.
//
//     h3  = dw3x3(h2) + b                  RE-COMPUTED on the halo pixels from an LDS ring of h2 (the forward saves h2 only: its saving launch
//                                          writes 134 MB less, -17 us each; this kernel reads h2 1.25 x instead of h3 1.125 x + h2 1 x)
//     dh3 = (W3^T dy) * gelu'(h3)          on the halo pixels, kept in a second LDS ring (never stored)
//     dh2 = dw3x3^T dh3                    -> HBM, the one tensor k_ffn1_bwd_xs reads
//     d dww[c][k] += h2(q) dh3(q - off_k),  d dwb[c] += dh3,  dW3 += dy (x) gelu(h3),  db3 += dy        (pixel sums)
//
// Two stencils in a row want two rings; at 64 hidden channels they do not fit beside each other twice per CU (49 + 54 KB), so the hidden
// channels are two independent HALVES (everything behind W3^T dy is per hidden channel): blockIdx.y = half, a workgroup walks DOWN a
// 16-column strip in 8-row steps with the rings of ITS 32 channels (26 + 29 KB; 74 KB in all: two workgroups per CU).  dy is read by both
// halves (the second read is an L2 hit).  Lane map of the halo pass as in k_ffn_xr: lane (g, c) = pixel c of a 16-pixel block; W3^T on the A
// side of the MFMA puts channels 16 mt + 4 g + v of that pixel into the lane (two 16-row tiles per half), where its h3 is re-computed from
// nine 16-byte ring reads per tile in the forward's own order of operations (bit for bit the forward's h3), gelu / gelu' are evaluated and
// dh3 leaves for the ring as 16-byte stores; dy needs no LDS on the way in (its four channels per lane ARE the B operand's k-slots).  dW3's
// pixel-axis contraction reads dy and gelu(h3) back by columns from small per-wave images (ds_read_b64_tr_b16), as k_ffn_dw_bwd_xs does.
// A step's nine halo blocks: wave w takes blocks 2 w, 2 w + 1 with both channel tiles; the ninth is split by tile between two waves whose
// roles rotate with the step.  The spatial phase (dh2 and the depthwise gradients: one row of four pixels per lane and step, sliding 3 x 3
// windows over the dh3 ring) reads its h2 from the ring too.  Three workgroup barriers per step.
#include "kernels.h"
#include "bwd_kernels.h"
#include "split_bf16.h"
#include "hstore.h"

#ifdef LG_STAMPS
__device__ unsigned long long g_dwh_stamps[1024 * 4 * 10 * 8];   // [workgroup (both halves)][wave][step][stamp]
#define HSTAMP(i) do { unsigned long long t__; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)); \
                       g_dwh_stamps[((((blockIdx.y * gridDim.x + blockIdx.x) & 1023) * 4 + wave) * 10 + (stamp_si < 9 ? stamp_si : 9)) * 8 + (i)] = t__; } while (0)
extern "C" __attribute__((visibility("default"))) int lg_debug_dwh_stamps(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_dwh_stamps), sizeof(g_dwh_stamps));
}
#else
#define HSTAMP(i) do { } while (0)
#endif
namespace dwh {

constexpr int E = 16, N1 = 64, NH = 32, NQ = NH / 4, TX = 16, TY = 8, HX = 18, HH = 20, RING = 10, LDC = NH + 8;   // ring pitch 40 floats: the spatial phase's (pixel group, quad) reads and the halo pass's (pixel, quad group) reads are both
                                                                                                    // conflict-free in the hardware's 16-lane groups (36 was 2-way almost everywhere: 23.5 M conflict cycles per launch)
constexpr int IMG_DY = 16 * 16, IMG_A3 = 16 * 16;                       // halves per piece: one 16-pixel block x 16 channels
constexpr int IMG_WAVE = 3 * IMG_DY + 3 * IMG_A3;                       // halves per wave: dy pieces | gelu(h3) pieces of ONE tile (the two tiles take turns)
constexpr size_t OFF_TAPS = 0;                                          // [8 quads][9 taps][4 channels of the quad] fp32
constexpr size_t OFF_DWB = OFF_TAPS + (size_t)NQ * 36 * 4;              // [32]
constexpr size_t OFF_W3F = OFF_DWB + (size_t)NH * 4;                    // W3^T fragments [2 tiles][3 pieces][64 lanes] 8-byte units
constexpr size_t OFF_IMG = OFF_W3F + (size_t)2 * 3 * 64 * 8;
constexpr size_t OFF_RD = OFF_IMG + (size_t)4 * IMG_WAVE * 2;           // dh3 ring [RING * HX][LDC]
constexpr size_t OFF_RH = OFF_RD + (size_t)RING * HX * LDC * 4;         // h2 ring  [RING * HH][LDC]
constexpr size_t LDS_BYTES = OFF_RH + (size_t)RING * HH * LDC * 4;
static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
static_assert(OFF_IMG % 16 == 0 && OFF_RD % 16 == 0 && OFF_RH % 16 == 0, "16-byte aligned LDS regions");
// slab row of a workgroup: [d dww 32 x 9 | d dwb 32 | dW3 16 x 32 | db3 16] of its channel half
constexpr int R_DB = NH * 9, R_W3 = R_DB + NH, R_B3 = R_W3 + E * NH, ROW = R_B3 + E;
static_assert(ROW == FFN_DW_BWD_H_ROW, "slab row (bwd_kernels.h)");
static_assert((size_t)(4 * NQ * 40 + 4 * E * NH + 4 * E) * 4 <= LDS_BYTES - OFF_RD, "the end-of-kernel reduction rows alias the rings");

template <int N>
struct IC { static constexpr int value = N; };

#define DWH_FENCE() __builtin_amdgcn_sched_barrier(0)

}  // namespace dwh

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_ffn_dw_bwd_h(FfnDwBwdXArgs a, int tiles_x, int strips_y, int nstrips, int SH) {
    using namespace dwh;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* sTaps = reinterpret_cast<float*>(smem_raw + OFF_TAPS);
    float* sDwb = reinterpret_cast<float*>(smem_raw + OFF_DWB);
    float* ringD = reinterpret_cast<float*>(smem_raw + OFF_RD);
    float* ringH = reinterpret_cast<float*>(smem_raw + OFF_RH);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c_ = lane & 15;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    uint16_t* imgDy = reinterpret_cast<uint16_t*>(smem_raw + OFF_IMG) + wave * IMG_WAVE;   // [3][16 px][16 ch]
    uint16_t* imgA3 = imgDy + 3 * IMG_DY;                                                  // [3][16 px][16 ch]
    const int h = a.h, w = a.w;
    const int hoff = blockIdx.y * NH;                  // this workgroup's channel half [hoff, hoff + 32) of the 64 hidden channels
    // ---- once per (persistent) workgroup: taps (pair-interleaved: one 16-byte read = the two packed operands of a tap), conv bias, W3^T fragments
    for (int k = threadIdx.x; k < NQ * 36; k += 256) sTaps[k] = a.dww[(hoff + 4 * (k / 36) + (k & 3)) * 9 + (k % 36) / 4];
    if (threadIdx.x < NH) sDwb[threadIdx.x] = a.dwb[hoff + threadIdx.x];
    u32x2_t* sW3 = reinterpret_cast<u32x2_t*>(smem_raw + OFF_W3F);      // (twelve registers held across the spatial phase otherwise: spills)
    if (wave < 2) {
        const WFrag16 f = load_wfrag16(a.w3t + (size_t)(hoff + 16 * wave) * E, E, 0);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) sW3[(wave * 3 + pc) * 64 + lane] = __builtin_bit_cast(u32x2_t, f.p[pc]);
    }
    // P2 roles: lane = (pixel group, channel quad q): group G = 8 wave + lane / 8 owns tile row G / 4, pixels 4 (G % 4) .. + 3
    const int q = lane & 7, G = 8 * wave + (lane >> 3), ty = G >> 2, txb = 4 * (G & 3);
    lg_v2f pw01[10], pw23[10];                         // d dww / d dwb partials of the lane's four P2 channels, as channel pairs
#pragma unroll
    for (int k = 0; k < 10; ++k) { pw01[k] = (lg_v2f){0.f, 0.f}; pw23[k] = (lg_v2f){0.f, 0.f}; }
    f32x4_t acc3[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // dW3[dy channel 4 g + v][hidden 16 mt + c]
    float4 sb3 = make_float4(0.f, 0.f, 0.f, 0.f);      // db3[4 g ..] of this lane's own pixels
    float dmx = 0.f;
    __syncthreads();

#pragma unroll 1
    for (int strip = blockIdx.x; strip < nstrips; strip += gridDim.x) {
        int t_ = strip;
        const int tx_i = t_ % tiles_x;
        t_ /= tiles_x;
        const int sy = t_ % strips_y;
        const long b = t_ / strips_y;
        const int x0 = tx_i * TX, Y0 = sy * SH, Yend = min(Y0 + SH, h);

        // dy of the lane's pixel of halo block blk of the row block starting at ya: unconditional, from a clamped address
        auto dyload = [&](int ya, int blk) -> float4 {
            const int m = 16 * blk + c_;
            const int hy = m / HX, hx = m - hy * HX;
            const int y = clampi(ya + hy, 0, h - 1), x = clampi(x0 + hx - 1, 0, w - 1);
            return *reinterpret_cast<const float4*>(a.dy + ((b * h + y) * (long)w + x) * E + 4 * g);
        };
        // h2 rows [row0, row0 + nrows) x columns [x0 - 2, x0 + 18) x this half's 32 channels: vector k of this thread (nrows * 160 in all)
        auto h2load = [&](int row0, int nrows, int k) -> float4 {
            const int idx = threadIdx.x + 256 * k, rr = idx / (HH * NQ), rem = idx - rr * (HH * NQ), col = rem >> 3, qd = rem & 7;
            const int y = row0 + min(rr, nrows - 1), x = x0 - 2 + col;
            const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(a.h2) + ((b * h + clampi(y, 0, h - 1)) * (long)w + clampi(x, 0, w - 1)) * N1 + hoff + 4 * qd);
            const bool in = y >= 0 && y < h && x >= 0 && x < w;      // dep_conv zero-pads h2
            return in ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        auto h2store = [&](int row0, int nrows, int k, const float4& v) {
            const int idx = threadIdx.x + 256 * k, rr = idx / (HH * NQ), rem = idx - rr * (HH * NQ), col = rem >> 3, qd = rem & 7;
            if (rr >= nrows) return;
            int sl = (row0 + rr - (Y0 - 2)) % RING;
            *reinterpret_cast<float4*>(ringH + (sl * HH + col) * LDC + 4 * qd) = v;
        };

        // dh3 of NB halo blocks (blk0 ..) x the channel tiles [MT0, MT0 + NMT) of halo rows [ya, ..) -> ringD; dW3 / db3 partials on the way
        auto halo = [&](auto nbc, auto mt0c, auto nmtc, int ya, int npx, int blk0, const float4* dyin) {
            constexpr int NB = decltype(nbc)::value, MT0 = decltype(mt0c)::value, NMT = decltype(nmtc)::value;
            int c = c_;
            asm volatile("" : "+v"(c));     // the block geometry is re-derived per call (as loop invariants of the step loop it would be hoisted and spilled)
            const int ringD0 = ((ya - Y0 + 1) % RING) * HX;
            int mm[NB], hoffs[NB][3];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int m = 16 * (blk0 + nb) + c;
                const int hy = m / HX, hx = m - hy * HX;
                mm[nb] = m;
                // h2 ring coordinates of the pixel's 3 x 3 neighbourhood: ring rows of image rows y - 1 .. y + 1, ring columns hx .. hx + 2
#pragma unroll
                for (int dy3 = 0; dy3 < 3; ++dy3) hoffs[nb][dy3] = (((ya - (Y0 - 2) + hy - 1 + dy3) % RING) * HH + hx) * LDC + 4 * g;
            }
            // ---- phase 1: h3 = dw3x3(h2) + b of every (block, tile) unit, in the forward's order of operations (k_ffn_xr / k_ffn_xs: rows, then
            // columns, packed channel pairs).  A tile's nine taps are read once for all blocks of the call; no GELU chain sits between the reads.
            lg_v2f H01[NB][NMT], H23[NB][NMT];
#pragma unroll
            for (int i = 0; i < NMT; ++i) {
                const int mt = MT0 + i;
                int toff = 4 * mt + g;                  // (an integer is laundered, not the pointer: a laundered pointer loses its address space and its reads become
                asm volatile("" : "+v"(toff));          //  flat loads that wait on BOTH counters) -- keeps the table reads inside the step loop
                const float4 bq = *reinterpret_cast<const float4*>(sDwb + 4 * toff);
                float4 tq[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) tq[k] = *reinterpret_cast<const float4*>(sTaps + 36 * toff + 4 * k);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    lg_v2f h01 = (lg_v2f){bq.x, bq.y}, h23 = (lg_v2f){bq.z, bq.w};
#pragma unroll
                    for (int dy3 = 0; dy3 < 3; ++dy3)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) {
                            const float4 v = *reinterpret_cast<const float4*>(ringH + hoffs[nb][dy3] + dx * LDC + 16 * mt);
                            const float4 t4 = tq[dy3 * 3 + dx];
                            h01 = (lg_v2f){t4.x, t4.y} * (lg_v2f){v.x, v.y} + h01;
                            h23 = (lg_v2f){t4.z, t4.w} * (lg_v2f){v.z, v.w} + h23;
                        }
                    asm volatile("" : "+v"(h01), "+v"(h23));
                    H01[nb][i] = h01; H23[nb][i] = h23;
                    DWH_FENCE();
                }
            }
            // ---- phase 2: per block: W3^T dy, gelu / gelu', dh3 -> ring, the images, dW3
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int m = mm[nb];
                const int hy = m / HX, hx = m - hy * HX;
                const int y = ya + hy, x = x0 + hx - 1;
                const bool in = m < npx && y >= 0 && y < h && x >= 0 && x < w;
                const bool own = in && hx >= 1 && hx <= TX && y >= Y0 && y < Yend;
                const float4 dr = dyin[nb];
                const float dv[4] = {in ? dr.x : 0.f, in ? dr.y : 0.f, in ? dr.z : 0.f, in ? dr.w : 0.f};   // dy = 0 outside the image: so is dh3
                if (own && MT0 == 0) { sb3.x += dv[0]; sb3.y += dv[1]; sb3.z += dv[2]; sb3.w += dv[3]; }
                u32x2_t q1, q2, q3;
                split3_x4(dv, q1, q2, q3);
                // dy pieces of the block's OWN pixels -> the wave's image (dW3's A operand: read back by columns)
                {
                    const float dm[4] = {own ? dv[0] : 0.f, own ? dv[1] : 0.f, own ? dv[2] : 0.f, own ? dv[3] : 0.f};
                    u32x2_t o1, o2, o3;
                    split3_x4(dm, o1, o2, o3);
                    uint16_t* dst = imgDy + c * 16 + 4 * g;
                    *reinterpret_cast<u32x2_t*>(dst) = o1;
                    *reinterpret_cast<u32x2_t*>(dst + IMG_DY) = o2;
                    *reinterpret_cast<u32x2_t*>(dst + 2 * IMG_DY) = o3;
                }
                int rp = ringD0 + m;
                rp = rp >= RING * HX ? rp - RING * HX : rp;
#pragma unroll
                for (int i = 0; i < NMT; ++i) {
                    const int mt = MT0 + i;
                    // (W3^T dy)[16 mt + 4 g + v][pixel c]
                    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                    WFrag16 wf;
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc) wf.p[pc] = __builtin_bit_cast(s16x4_t, sW3[(mt * 3 + pc) * 64 + lane]);
                    const s16x4_t dyq[3] = {__builtin_bit_cast(s16x4_t, q1), __builtin_bit_cast(s16x4_t, q2), __builtin_bit_cast(s16x4_t, q3)};
                    mfma_np16<3, true>(acc, wf.p, dyq);
                    lg_v2f a01, a23, g01, g23;
                    gelu2_both_f(H01[nb][i], a01, g01);
                    gelu2_both_f(H23[nb][i], a23, g23);
                    // dh3 (0 outside the image: dy is 0 there) -> ring
                    if (m < npx) *reinterpret_cast<float4*>(ringD + rp * LDC + 16 * mt + 4 * g) = make_float4(acc[0] * g01.x, acc[1] * g01.y, acc[2] * g23.x, acc[3] * g23.y);
                    // gelu(h3) of the OWN pixels -> the wave's [pixel][channel] image of this tile
                    const float av[4] = {own ? a01.x : 0.f, own ? a01.y : 0.f, own ? a23.x : 0.f, own ? a23.y : 0.f};   // (a select, not a product: beyond the block's last pixel the ring holds anything)
                    u32x2_t p1, p2, p3;
                    split3_x4(av, p1, p2, p3);
                    uint16_t* dst = imgA3 + c * 16 + 4 * g;
                    *reinterpret_cast<u32x2_t*>(dst) = p1;
                    *reinterpret_cast<u32x2_t*>(dst + IMG_A3) = p2;
                    *reinterpret_cast<u32x2_t*>(dst + 2 * IMG_A3) = p3;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    {   // dW3[dy channel][hidden 16 mt + .] += dy^T gelu(h3): both operands read by columns (K = the block's 16 pixels)
                        const int off = (4 * g + (c >> 2)) * 16 + 4 * (c & 3);
                        s16x4_t dt[3], at[3];
#pragma unroll
                        for (int pc = 0; pc < 3; ++pc) { dt[pc] = lds_tr4(imgDy + pc * IMG_DY + off); at[pc] = lds_tr4(imgA3 + pc * IMG_A3 + off); }
                        mfma_split16(acc3[mt], dt, at);
                    }
                    __builtin_amdgcn_wave_barrier();   // the image is rewritten by the next tile
                    DWH_FENCE();
                }
                __builtin_amdgcn_wave_barrier();   // the images are rewritten by the next block
                DWH_FENCE();
            }
        };

        // ---- strip prologue: h2 rows Y0 - 2 .. Y0 + 1, then dh3 of halo rows Y0 - 1, Y0 (36 pixels: blocks 0 .. 2, one per wave)
        {
            float4 hp[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) hp[k] = h2load(Y0 - 2, 4, k);
            const float4 dp = dyload(Y0 - 1, uwave < 3 ? uwave : 0);
            __syncthreads();     // the previous strip's spatial phase is done with both rings
#pragma unroll
            for (int k = 0; k < 3; ++k) h2store(Y0 - 2, 4, k, hp[k]);
            __syncthreads();
            if (uwave < 3) halo(IC<1>{}, IC<0>{}, IC<2>{}, Y0 - 1, 2 * HX, uwave, &dp);
        }
        float4 hn[5], dn[3];
#pragma unroll
        for (int k = 0; k < 5; ++k) hn[k] = h2load(Y0 + 2, TY, k);
        dn[0] = dyload(Y0 + 1, 2 * wave); dn[1] = dyload(Y0 + 1, 2 * wave + 1); dn[2] = dyload(Y0 + 1, 8);
#pragma unroll 1
        for (int y0 = Y0; y0 < Yend; y0 += TY) {
            const int si = (y0 - Y0) >> 3, role = (uwave + si) & 3;
#ifdef LG_STAMPS
            const int stamp_si = si;
#endif
            HSTAMP(0);
            __syncthreads();     // ring rows of h2 that this step overwrites (y0 - 8 .. y0 - 1) are dead: the previous step's spatial phase is done
#pragma unroll
            for (int k = 0; k < 5; ++k) h2store(y0 + 2, TY, k, hn[k]);
            __syncthreads();     // h2 rows y0 .. y0 + 9 complete
            HSTAMP(1);
            // next step's operands are requested IN FRONT of the halo pass (clamped addresses: harmless behind the last step): behind it the spatial
            // phase alone (~1 us) did not cover their HBM round trip
            float4 dnn[3];
#pragma unroll
            for (int k = 0; k < 5; ++k) hn[k] = h2load(y0 + TY + 2, TY, k);
            dnn[0] = dyload(y0 + TY + 1, 2 * wave); dnn[1] = dyload(y0 + TY + 1, 2 * wave + 1); dnn[2] = dyload(y0 + TY + 1, 8);
            halo(IC<2>{}, IC<0>{}, IC<2>{}, y0 + 1, TY * HX, 2 * wave, dn);
            if (role == 1) halo(IC<1>{}, IC<0>{}, IC<1>{}, y0 + 1, TY * HX, 8, dn + 2);
            if (role == 3) halo(IC<1>{}, IC<1>{}, IC<1>{}, y0 + 1, TY * HX, 8, dn + 2);
            dn[0] = dnn[0]; dn[1] = dnn[1]; dn[2] = dnn[2];
            HSTAMP(2);
            __syncthreads();     // dh3 rows y0 - 1 .. y0 + 8 complete
            HSTAMP(3);
            // ---- spatial phase: dh2 of four consecutive pixels of tile row ty, channels 4 q .. + 3: a 3 x 3 window of dh3 vectors slides over them
            {
                const int sbase = (y0 - Y0) % RING;            // dh3 ring slot of row y0 - 1
                const float* rrow[3];
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) {               // ring row ty + rr (relative to row y0 - 1) meets tap dy = 2 - rr
                    int sl = sbase + ty + rr;
                    sl = sl >= RING ? sl - RING : sl;
                    sl = sl >= RING ? sl - RING : sl;
                    rrow[rr] = ringD + (sl * HX + txb) * LDC + 4 * q;
                }
                const int y = y0 + ty;
                const float* hcen = ringH + (((y - (Y0 - 2)) % RING) * HH + txb + 2) * LDC + 4 * q;
                int qoff = 36 * q;
                asm volatile("" : "+v"(qoff));
                const float* tpq = sTaps + qoff;               // the quad's taps, read per window row (nine resident 16-byte vectors were 36 registers)
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const float4 hc = *reinterpret_cast<const float4*>(hcen + it * LDC);
                    const lg_v2f h01 = (lg_v2f){hc.x, hc.y}, h23 = (lg_v2f){hc.z, hc.w};
                    lg_v2f acc01 = (lg_v2f){0.f, 0.f}, acc23 = (lg_v2f){0.f, 0.f};
#pragma unroll
                    for (int rr = 0; rr < 3; ++rr) {           // one window row at a time: three dh3 vectors and their three taps (a resident 4 x 3 window + nine taps spilled)
                        float4 tq[3], gq[3];
#pragma unroll
                        for (int cc = 0; cc < 3; ++cc) {
                            tq[cc] = *reinterpret_cast<const float4*>(tpq + 4 * ((2 - rr) * 3 + (2 - cc)));
                            gq[cc] = *reinterpret_cast<const float4*>(rrow[rr] + (it + cc) * LDC);
                        }
#pragma unroll
                        for (int cc = 0; cc < 3; ++cc) {
                            // forward: h3(p) += w[dy][dx] h2(p + (dy-1, dx-1))  ->  h2(q) meets dh3(q - (dy-1, dx-1)) in both sums: halo column
                            // tx + 2 - dx = tx + cc, ring row ty + 2 - dy = ty + rr
                            const int k = (2 - rr) * 3 + (2 - cc);
                            const lg_v2f g01 = (lg_v2f){gq[cc].x, gq[cc].y}, g23 = (lg_v2f){gq[cc].z, gq[cc].w};
                            acc01 = (lg_v2f){tq[cc].x, tq[cc].y} * g01 + acc01;
                            acc23 = (lg_v2f){tq[cc].z, tq[cc].w} * g23 + acc23;
                            pw01[k] = h01 * g01 + pw01[k];
                            pw23[k] = h23 * g23 + pw23[k];
                            if (k == 4) { pw01[9] += g01; pw23[9] += g23; }
                        }
                    }
                    const int x = x0 + txb + it;
                    // (every output pixel of a step is inside the image: the launcher checks h % 8 == 0 and w % 16 == 0 -- a condition here split the
                    //  item into blocks in which the compiler formed dh2 and the gradient sums from separate copies of the operands)
                    *reinterpret_cast<float4*>(static_cast<float*>(a.dh2) + ((b * h + y) * (long)w + x) * N1 + hoff + 4 * q) = make_float4(acc01.x, acc01.y, acc23.x, acc23.y);
                    dmx = fmaxf(fmaxf(dmx, fmaxf(fabsf(acc01.x), fabsf(acc01.y))), fmaxf(fabsf(acc23.x), fabsf(acc23.y)));
                    DWH_FENCE();
                }
            }
            HSTAMP(4);
        }   // steps of the strip
        __syncthreads();
    }   // strips of this workgroup

    if (a.dh2_max) {     // one atomic per wave (non-negative floats order as their bit patterns)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dmx = fmaxf(dmx, __shfl_xor(dmx, off));
        if (lane == 0) atomicMax(reinterpret_cast<unsigned int*>(a.dh2_max), __float_as_uint(dmx));
    }
    // ---- this workgroup's partial sums -> its slab row [d dww 32 x 9 | d dwb 32 | dW3 16 x 32 | db3 16]
    float* row = a.slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ROW;
    float* red = ringD;   // [4 waves][8 quads][40] | [4 waves][16 x 32] | [4 waves][16]: the rings are dead (barrier at the end of the last strip)
    float* redW = red + 4 * NQ * 40;
    float* redB = redW + 4 * E * NH;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            float v = u == 0 ? pw01[k].x : (u == 1 ? pw01[k].y : (u == 2 ? pw23[k].x : pw23[k].y));
#pragma unroll
            for (int off = NQ; off < 64; off <<= 1) v += __shfl_xor(v, off);      // lanes with the same q hold the same channels
            if (lane < NQ) red[(wave * NQ + q) * 40 + u * 10 + k] = v;
        }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int v = 0; v < 4; ++v) redW[wave * E * NH + (4 * g + v) * NH + 16 * mt + c_] = acc3[mt][v];
    {
        float4 s4 = sb3;      // lanes with the same g hold the same dy channels
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            s4.x += __shfl_xor(s4.x, off); s4.y += __shfl_xor(s4.y, off); s4.z += __shfl_xor(s4.z, off); s4.w += __shfl_xor(s4.w, off);
        }
        if (c_ == 0) *reinterpret_cast<float4*>(redB + wave * E + 4 * g) = s4;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NQ * 40; i += 256) {
        float v = 0.f;
#pragma unroll
        for (int w8 = 0; w8 < 4; ++w8) v += red[w8 * NQ * 40 + i];
        const int qq = i / 40, rem = i - qq * 40, u = rem / 10, k = rem - u * 10;
        const int ch = 4 * qq + u;
        if (k < 9) row[ch * 9 + k] = v;
        else row[R_DB + ch] = v;
    }
    for (int i = threadIdx.x; i < E * NH; i += 256) row[R_W3 + i] = (redW[i] + redW[E * NH + i]) + (redW[2 * E * NH + i] + redW[3 * E * NH + i]);
    if (threadIdx.x < E) row[R_B3 + threadIdx.x] = (redB[threadIdx.x] + redB[E + threadIdx.x]) + (redB[2 * E + threadIdx.x] + redB[3 * E + threadIdx.x]);
}

int launch_ffn_dw_bwd_h(const FfnDwBwdXArgs& a, hipStream_t s) {
    using namespace dwh;
    ProfScope prof__(LG_K_FFN2_BWD, s);
    if (!a.dy || !a.h2 || !a.dh2 || !a.w3t || !a.dww || !a.dwb || !a.slab) { lg_set_error("ffn_dw_bwd_h: null argument"); return -2; }
    if (a.hbf) { lg_set_error("ffn_dw_bwd_h: fp32 storage only"); return -2; }
    if ((a.h & 7) || (a.w & 15)) { lg_set_error("ffn_dw_bwd_h: h must be a multiple of 8 and w of 16 (got %d x %d)", a.h, a.w); return -2; }
    static DeviceOnce attr_once;
    if (int rc = lds_attr_once(attr_once, "ffn_dw_bwd_h", (int)LDS_BYTES, k_ffn_dw_bwd_h)) return rc;
    const StripGeo geo = strip_geometry(a.h, a.w, a.B, a.B, FFN_DW_BWD_H_WGS, 0);   // a strip per resident workgroup (512 = two per CU; the two channel halves share them)
    const int tiles_x = geo.tiles_x, strips_y = geo.strips_y, nstrips = geo.nstrips, SH = geo.SH, gx = geo.grid;
    k_ffn_dw_bwd_h<<<dim3(gx, 2), 256, LDS_BYTES, s>>>(a, tiles_x, strips_y, nstrips, SH);
    LG_CHECK_LAUNCH();
    return reduce_ffn_dw_bwd_slab(a, E, 2, gx, R_DB, R_W3, R_B3, ROW, s);
}
