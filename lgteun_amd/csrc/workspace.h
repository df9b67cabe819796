// Workspace carving shared by forward and backward orchestrators.  The caller owns one flat buffer; this
// maps named activation tensors onto it deterministically from (plan, B, train).
#pragma once
#include "common.h"
#include "kernels.h"

struct Carver {
    char* base;
    size_t off;
    float* take(size_t nfloats) {
        size_t o = off;
        off += (nfloats * sizeof(float) + 255) & ~(size_t)255;
        return base ? reinterpret_cast<float*>(base + o) : nullptr;
    }
};

#define LG_MAX_K 16
#define LG_NBLK 5   // blocks of one LGT: encoder 0 1, bottleneck 2 (level 1), decoder 3 4

// The per-block prep slots: four tables of [K][LG_NBLK] rows, written once per forward call (k_fwd.hip: prep_stages) and read by the kernels of
// that (stage, block).  THE description of their layout: the row sizes here, the carving in carve(), the rows in NetBufs::*_row and
// NetBufs::block, the stage-to-stage strides of the multi-stage kernels in NetBufs::stage_strides.
constexpr size_t POS_TABLE = 2 * 64 * 64;   // floats of one pos_emb table [2][64][64] (posT; a row of the R3 backward's dpos slab too)
constexpr size_t FFN_SCALES_ROW = 8;        // floats of a block's row of ffn_scales
constexpr size_t ATTN_SCALES_ROW = 4;       // ... of attn_scales

struct BlockBufs {
    int e, h, w;       // channels / spatial size of this block
    float *xin, *xmid, *xout;
    float *g, *o2;     // planar [B,e/2,h,w]
    float *amp, *pha;  // saved spectrum [B,e/2,h,w/2+1] (train)
    float* sgn;        // saved sign of the irfft2 output [B,e/2,h,w] (train)
    float *att_o, *att_l;  // train: the local mixer's attention output [B,h,w,e/2] and score-row log-sum-exp [B,h,w,2] (k_attn_m -> k_attn_bwd_f)
    float *a1, *g1, *h2, *a3, *g3;  // [B,h,w,4e]: gelu(h1), gelu'(h1), h2, gelu(h3), gelu'(h3)  (a*, g* train only)
};

// One (stage, block) of an LGT, as every block function receives it: the block's buffers, its slots of the flat parameter / gradient buffers and
// its rows of the prep tables (NetBufs::block).  `b` is a copy: the per-op entries point xin / xmid / xout at their caller's tensors.
struct Blk {
    const lg_plan* pl;
    const float* P;
    float* G;          // null in the forward
    int st, j;
    BlockBufs b;
    float* fft_scratch;                     // NetBufs::fft_scratch
    const float *posT, *attn_scales;        // this block's rows
    float *ffn_scales, *wsplit;
    const float* p(int slot) const { return P + pl->blk(st, j, slot); }   // parameter slot B_*
    float* g(int slot) const { return G + pl->blk(st, j, slot); }         // its gradient
};
// ... and the LGT-level slots L_* of a stage
struct LgtSlots {
    const lg_plan* pl;
    const float* P;
    float* G;
    int st;
    const float* p(int slot) const { return P + pl->lgt(st, slot); }
    float* g(int slot) const { return G + pl->lgt(st, slot); }
};

struct NetBufs {
    float* Z[LG_MAX_K + 1];                          // Z_0 .. Z_K  [B,C,H,W]: Z[i] -> data step i -> Z[i+1] (= input of LGT i)
    float* X[LG_MAX_K];                              // chained mode: input of data step i (X[0] = Z[0], X[i] = output of LGT i-1)
    float *t1[LG_MAX_K], *r[LG_MAX_K], *s1[LG_MAX_K];  // data-step intermediates per stage
    float* pr;                                       // [B,H,W] scratch of the one-launch data step (k_dstep.hip): R Z - pan of the stage in flight
    float* posT;                                     // [K][LG_NBLK][POS_TABLE]
    BlockBufs blk[LG_NBLK];
    float* x0;        // embed output = blk[0].xin
    float* deadout;   // output of dead-stage LGTs (faithful mode)
    float* u_down;    // saved bicubic-downsampled encoder output [B,H/2,W/2,E] (train)
    float* t_up;      // saved up-path tensor [B,H,W,E] (train)
    float* fft_scratch;  // half-spectrum scratch of the FFT mixer's three-launch paths (FftRoute::scratch_floats); null where both levels run in LDS
    float* ffn_scales;   // [K][LG_NBLK][FFN_SCALES_ROW] operand scales of the f16-pair FFN arithmetic (k_ffn_prep.hip), written once per forward call
    float* attn_scales;  // [K][LG_NBLK][ATTN_SCALES_ROW] static operand scales of the local mixer's f16-pair products { s_y, s_w, s_q, s_k } (k_ffn_prep.hip), written once per forward call
    float* wsplit;       // [K][LG_NBLK][wsplit_slot] slots of pre-split (and pre-scaled) weight fragments of the e >= 32 FFN blocks (k_ffn_x32.hip), written once per forward call
    size_t set_off, set_bytes;  // the per-LGT activation set [set_off, set_off + set_bytes): train == 2 carves K of them back to back
    size_t live_s0;             // first sample of the live stage's slot in the transient forward buffers (live_view): (K-1) B with stage_batch, else 0
    size_t wsplit_slot;         // floats of one wsplit slot: sized for the widest block (level 1: e = 8 C)
    size_t bytes;
    static size_t row(int st, int j) { return (size_t)st * LG_NBLK + j; }
    float* posT_row(int st, int j) const { return posT + row(st, j) * POS_TABLE; }
    float* ffn_scales_row(int st, int j) const { return ffn_scales + row(st, j) * FFN_SCALES_ROW; }
    float* attn_scales_row(int st, int j) const { return attn_scales + row(st, j) * ATTN_SCALES_ROW; }
    float* wsplit_row(int st, int j) const { return wsplit + row(st, j) * wsplit_slot; }
    // from one stage's rows to the next one's, in the units the multi-stage kernels shift by (kernels.h: StageSel)
    void stage_strides(StageSel& sg) const {
        sg.fs_stride = (int)(LG_NBLK * FFN_SCALES_ROW); sg.as_stride = (int)(LG_NBLK * ATTN_SCALES_ROW); sg.ws_stride = (long)(LG_NBLK * wsplit_slot * sizeof(float));
    }
    Blk block(const lg_plan* pl, const float* P, float* G, int st, int j) const {
        return Blk{pl, P, G, st, j, blk[j], fft_scratch, posT_row(st, j), attn_scales_row(st, j), ffn_scales_row(st, j), wsplit_row(st, j)};
    }
};

// NetBufs of stage `i` when every stage keeps its own activation set (chained training): same layout, shifted by i sets
static inline NetBufs stage_view(const NetBufs& nb, int i) {
    NetBufs v = nb;
    const size_t sh = (size_t)i * nb.set_bytes;
    auto mv = [sh](float*& p) { if (p) p = reinterpret_cast<float*>(reinterpret_cast<char*>(p) + sh); };
    for (int j = 0; j < LG_NBLK; ++j) {
        BlockBufs& b = v.blk[j];
        mv(b.xin); mv(b.xmid); mv(b.xout); mv(b.g); mv(b.o2); mv(b.amp); mv(b.pha); mv(b.sgn); mv(b.att_o); mv(b.att_l);
        mv(b.a1); mv(b.g1); mv(b.h2); mv(b.a3); mv(b.g3);
    }
    mv(v.x0); mv(v.u_down); mv(v.t_up);
    return v;
}

// NetBufs of the LIVE stage (and of every single-stage call): a plan with stage_batch carves the transient forward buffers for K slots of B samples,
// dead stage i in slot i and the live stage ALWAYS in slot K-1 -- whether it rides behind the dead pass or runs alone, forward and backward alike.
// Saved tensors are B-sized and stay where they are; any other plan: nb itself.
static inline NetBufs live_view(const NetBufs& nb) {
    NetBufs v = nb;
    if (!nb.live_s0) return v;
    for (int j = 0; j < LG_NBLK; ++j) {
        BlockBufs& b = v.blk[j];
        const size_t px = nb.live_s0 * b.h * b.w;   // pixels in front of the slot
        b.xin += px * b.e; b.xmid += px * b.e; b.xout += px * b.e; b.g += px * (b.e / 2); b.o2 += px * (b.e / 2);
    }
    v.x0 = v.blk[0].xin;
    v.live_s0 = 0;   // (a view of a view is itself)
    return v;
}

// train: 0 = inference, 1 = training (one saved activation set: only the last stage's LGT is live),
// 2 = chained training (LG_FLAG_CHAINED: every stage's LGT is live and keeps its own set)
static inline void carve(const lg_plan* plan, int B, int train, void* base, NetBufs& nb) {
    const lg_config& c = plan->cfg;
    Carver cv{reinterpret_cast<char*>(base), 0};
    const size_t P0 = (size_t)c.H * c.W, P1 = P0 / 4, E = 4 * (size_t)c.C;
    // A plan whose dead stages run as one pass (lg_plan::stage_batch: K-1 >= 2 of them) carves the TRANSIENT forward buffers -- what a non-saving
    // LGT forward writes -- for K slots of B samples: stage s's part follows stage s-1's, so a kernel sees a plain batch of up to K B samples.  The live
    // stage owns slot K-1 on every path (live_view), the dead stages slots 0 .. K-2; deadout holds the K-1 dead outputs.  Saved tensors, the data steps'
    // buffers and every other plan (K = 2 among them) are unchanged.
    const bool slots = plan->stage_batch && train != 2;
    const size_t BT = (size_t)B * (slots ? c.K : 1);
    nb.live_s0 = slots ? (size_t)B * (c.K - 1) : 0;
    for (int i = 0; i <= c.K; ++i) nb.Z[i] = cv.take(B * c.C * P0);
    for (int i = 0; i < c.K; ++i) {
        nb.t1[i] = cv.take(B * c.C * P1);
        nb.r[i] = cv.take(B * c.C * P1 / 4);
        nb.s1[i] = cv.take(B * c.C * P1);
    }
    nb.pr = cv.take(B * P0);
    const size_t rows = NetBufs::row(c.K, 0);
    nb.posT = cv.take(rows * POS_TABLE);
    nb.ffn_scales = cv.take(rows * FFN_SCALES_ROW);
    nb.attn_scales = cv.take(rows * ATTN_SCALES_ROW);
    nb.wsplit_slot = ffn_wsplit_bytes((int)(2 * E)) / sizeof(float);
    nb.wsplit = cv.take(rows * nb.wsplit_slot);
    nb.deadout = cv.take((slots ? nb.live_s0 : (size_t)B) * c.C * P0);
    nb.X[0] = nb.Z[0];
    for (int i = 1; i < c.K; ++i) nb.X[i] = (train == 2) ? cv.take(B * c.C * P0) : nb.deadout;
    float* shared_h2 = nullptr;
    if (!train) shared_h2 = cv.take(B * P0 * 4 * E);  // largest (level-0) hidden tensor, reused by every block
    nb.set_off = cv.off;
    for (int j = 0; j < LG_NBLK; ++j) {
        BlockBufs& bb = nb.blk[j];
        const bool l1 = (j == 2);
        bb.e = (int)(l1 ? 2 * E : E);
        bb.h = l1 ? c.H / 2 : c.H;
        bb.w = l1 ? c.W / 2 : c.W;
        const size_t P = l1 ? P1 : P0, e = bb.e;
        bb.xin = nullptr;  // wired below
        bb.xmid = cv.take(BT * P * e);
        bb.xout = cv.take(BT * P * e);
        bb.g = cv.take(BT * P * e / 2);
        bb.o2 = cv.take(BT * P * e / 2);
        if (train) {
            bb.amp = cv.take(B * (e / 2) * bb.h * (bb.w / 2 + 1));
            bb.pha = cv.take(B * (e / 2) * bb.h * (bb.w / 2 + 1));
            bb.sgn = cv.take(B * P * e / 2);
            bb.att_o = cv.take(B * P * e / 2);
            bb.att_l = cv.take(B * P * 2);
            bb.a1 = cv.take(B * P * 4 * e);
            bb.g1 = cv.take(B * P * 4 * e);
            bb.h2 = cv.take(B * P * 4 * e);
            bb.a3 = cv.take(B * P * 4 * e);
            bb.g3 = cv.take(B * P * 4 * e);
        } else {
            bb.att_o = bb.att_l = nullptr;
            bb.amp = bb.pha = bb.sgn = bb.a1 = bb.g1 = bb.a3 = bb.g3 = nullptr;
            bb.h2 = shared_h2;
        }
    }
    nb.x0 = cv.take(BT * P0 * E);
    nb.blk[0].xin = nb.x0;
    nb.blk[1].xin = nb.blk[0].xout;
    nb.blk[2].xin = cv.take(BT * P1 * 2 * E);  // down output
    nb.blk[3].xin = cv.take(BT * P0 * E);      // up+fusion output
    nb.blk[4].xin = nb.blk[3].xout;
    nb.u_down = train ? cv.take(B * P1 * E) : nullptr;
    nb.t_up = train ? cv.take(B * P0 * E) : nullptr;
    nb.set_bytes = cv.off - nb.set_off;
    if (train == 2) cv.off += (size_t)(c.K - 1) * nb.set_bytes;
    {
        // level 0: B * E/2 planes of H x W; level 1: B * E planes of H/2 x W/2 -- level 0's is the larger whenever both need one
        const size_t f0 = BT * (E / 2) * plan->route.fft[0].scratch_floats, f1 = BT * E * plan->route.fft[1].scratch_floats;
        const size_t fl = f0 > f1 ? f0 : f1;
        nb.fft_scratch = fl ? cv.take(fl) : nullptr;
    }
    nb.bytes = cv.off;
}
