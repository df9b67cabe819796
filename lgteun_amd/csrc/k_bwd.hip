// Backward orchestration: autograd of Pansharpening.forward (reference models/unlg_former.py:50-67) over the live
// graph only -- the last stage's LGT and the K shared data steps (dead-stage LGTs never get a gradient).
#include <string.h>

#include "kernels.h"
#include "bwd_kernels.h"
#include "backward.h"

struct BwdBufs {
    float *dzA, *dzB, *gu3, *gs1, *gu1, *gr, *gd3, *gt1, *gd1;
    float *dx[3];
    float *dh2, *dh1, *y2, *do2, *dg, *dym, *cat, *y1, *dqkv;
    float *w3t[LG_NBLK], *w2t[LG_NBLK], *w1t[LG_NBLK], *wsp, *dt, *dskip, *v, *du;   // transposed FFN weights, one set per block of the LGT
    float* slab_arena;    // scratch of the deferred parameter-gradient reductions (ReduceQueue, bwd_kernels.h)
    float* attn_stats;    // [P0][2][4]: row statistics between the two launches of k_attn_bwd_core_m (LG_ATTN_BWD_CORE=m)
    size_t slab_cap;      // floats
    ReduceQueue rq;
    size_t bytes;
};

// the local mixer's pos_emb partial rows of one block: k_attn_bwd_f's rows (every parameter gradient of the half-block) or the three-kernel form's
static const size_t R3_DPOS_SLAB = 512 * POS_TABLE;   // (AttnBwdArgs::dpos_slab: room for the tables of 512 workgroups)
static size_t dpos_slab_floats() {
    const size_t f = (size_t)ATTN_BWD_F_WGS * ATTN_BWD_F_ROW;
    return f > R3_DPOS_SLAB ? f : R3_DPOS_SLAB;
}
static void carve_bwd(const lg_plan* plan, int B, void* base, BwdBufs& bb) {
    const lg_config& c = plan->cfg;
    Carver cv{reinterpret_cast<char*>(base), 0};
    const size_t P0 = (size_t)c.H * c.W * B, P1 = P0 / 4, E = 4 * (size_t)c.C, C = c.C;
    bb.dzA = cv.take(C * P0); bb.dzB = cv.take(C * P0); bb.gu3 = cv.take(C * P0);
    bb.gs1 = cv.take(C * P1); bb.gu1 = cv.take(C * P1); bb.gt1 = cv.take(C * P1); bb.gd1 = cv.take(C * P1);
    bb.gr = cv.take(C * P1 / 4); bb.gd3 = cv.take(C * P1 / 4);
    for (int i = 0; i < 3; ++i) bb.dx[i] = cv.take(P0 * E);
    bb.dh2 = cv.take(P0 * 4 * E); bb.dh1 = cv.take(P0 * 4 * E);
    bb.y2 = cv.take(P0 * E); bb.do2 = cv.take(P0 * E / 2); bb.dg = cv.take(P0 * E / 2);
    bb.dym = cv.take(P0 * E); bb.cat = cv.take(P0 * E); bb.y1 = cv.take(P0 * 16 > P0 * E / 2 ? P0 * 16 : P0 * E / 2);
    bb.dqkv = cv.take(P0 * 2 * E);
    bb.attn_stats = cv.take(P0 * 8);
    for (int j = 0; j < LG_NBLK; ++j) { bb.w3t[j] = cv.take(8 * E * 2 * E); bb.w2t[j] = cv.take(8 * E * 8 * E); bb.w1t[j] = cv.take(8 * E * 2 * E); }
    bb.wsp = cv.take(ffn_wsplit_bytes(32) / sizeof(float));   // pre-split W2^T / W1^T fragments of k_ffn1_bwd_x32 (e = 32 blocks)
    size_t sl = wgrad_slab_floats((int)(8 * E), (int)(8 * E), (long)P0);
    size_t sl2 = wgrad_slab_floats(64, 64, (long)P0);
    size_t sl3 = ffn_dw_bwd_slab_floats((int)E, B, c.H, c.W);
    if (sl2 > sl) sl = sl2;
    // per-workgroup partial-sum rows of the parameter-gradient reductions (bwd_kernels.h)
    size_t sl4 = chan_partial_floats(c.C, B, c.H, c.W);
    const size_t sl5 = (size_t)PIXEL_PART_WGS * (2 * 8 * c.C + 2 * c.C);
    if (sl5 > sl4) sl4 = sl5;
    if (sl4 > sl) sl = sl4;
    // arena: a whole LGT backward between flushes -- five blocks' worth of slabs (each: dw-conv partials + the three FFN weight gradients + the
    // small ones, and the local mixer's pos_emb partial rows); the weight-gradient slabs of the down / up / fusion convs ride in the blocks'
    // slack.  take() flushes by itself if a configuration needs more
    if (sl3 > sl) sl = sl3;
    for (const FfnRoute& fr : plan->route.ffn)   // slab rows of the fused FFN backward kernels (k_ffn_bwd_x.hip, k_ffn_dwbwd_x.hip): only of the paths this plan runs
        if (fr.px == FFN1_BWD_XS && ffn1_bwd_x_slab_floats(fr.e) > sl) sl = ffn1_bwd_x_slab_floats(fr.e);
    if (ffn_dw_bwd_x_slab_floats(16) > sl) sl = ffn_dw_bwd_x_slab_floats(16);
    if (ffn_dw_bwd_x_slab_floats(32) > sl) sl = ffn_dw_bwd_x_slab_floats(32);
    if (ffn_dw_bwd_h_slab_floats() > sl) sl = ffn_dw_bwd_h_slab_floats();
    bb.slab_cap = LG_NBLK * (4 * sl + dpos_slab_floats());
    bb.slab_arena = cv.take(bb.slab_cap);
    bb.dt = cv.take(P0 * E); bb.dskip = cv.take(P0 * E); bb.v = cv.take(P1 * E); bb.du = cv.take(P1 * E);
    bb.bytes = cv.off;
}

size_t bwd_workspace_bytes(const lg_plan* plan, int B) {
    BwdBufs bb;
    carve_bwd(plan, B, nullptr, bb);
    return bb.bytes;
}

#define RC(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

// deactivates the calling thread's reduce queue on every exit path (error returns included)
struct ReduceQueueScope {
    explicit ReduceQueueScope(BwdBufs& bb, hipStream_t s, bool per_block) {
        bb.rq.init(bb.slab_arena, bb.slab_cap, s, per_block);
        reduce_queue_begin(&bb.rq);
    }
    ~ReduceQueueScope() { (void)reduce_queue_end(); }
};

static int wgrad(const void* Y, int ldy, const void* X, int ldx, float* dW, int ldw, float* db, long P, int N, int K, int nv, int kv,
                 int ybf, int xbf, BwdBufs& bb, hipStream_t s, int xgelu = 0) {
    float* slab = bb.rq.take(wgrad_slab_floats(N, K, P));
    if (!slab) return -3;
    WgradArgs a;
    a.Y = Y; a.X = X; a.dW = dW; a.db = db; a.P = P; a.ldy = ldy; a.ldx = ldx; a.ldw = ldw; a.N = N; a.K = K;
    a.n_valid = nv; a.k_valid = kv; a.ybf = ybf; a.xbf = xbf; a.xgelu = xgelu;
    return launch_wgrad(a, slab, s);
}

// W3^T / W2^T / W1^T of the nk blocks k[] into bb.w?t[j], all in ONE launch (backward GEMMs read transposed weights).  The same launch sets word 6
// of the blocks' ffn_scales rows (max |dh2|, ffn_half_bwd) to zero: the forward's k_ffn_scales does so once, but a saved forward may be followed by more
// than one backward (retain_graph), and the second must not start from the first one's maximum
static int ffn_transposes(const Blk* blocks, int nk, BwdBufs& bb, hipStream_t s) {
    const float* tsrc[3 * LG_NBLK];
    float* tdst[3 * LG_NBLK];
    float* clear[LG_NBLK];
    int trows[3 * LG_NBLK], tcols[3 * LG_NBLK], n = 0, nclear = 0;
    for (int i = 0; i < nk; ++i) {
        const Blk& k = blocks[i];
        const int j = k.j, e = k.b.e, n1 = 4 * e;
        tsrc[n] = k.p(B_W3); tdst[n] = bb.w3t[j]; trows[n] = e; tcols[n] = n1; ++n;
        tsrc[n] = k.p(B_W2); tdst[n] = bb.w2t[j]; trows[n] = n1; tcols[n] = n1; ++n;
        tsrc[n] = k.p(B_W1); tdst[n] = bb.w1t[j]; trows[n] = n1; tcols[n] = e; ++n;
        if (k.pl->ffn(e).bwd_scales) clear[nclear++] = k.ffn_scales + 6;
    }
    return launch_transpose3(tsrc, tdst, trows, tcols, n, s, clear, nclear);
}

// feed_forward half-block backward: dy (grad wrt block output) -> tmp (grad wrt the mid activation); bb.w?t[j] hold the transposed weights.
// The spatial kernel of the block's route (dh2; the depthwise gradients; dW3 / db3 unless it is the tile kernel), then the pixelwise kernel
// (dx, the LayerNorm gradients; dW1 / dW2 when it is k_ffn1_bwd_xs), then the weight-gradient launches the route lists; dh2 is the only tensor
// between the halves
static int ffn_half_bwd(const Blk& k, BwdBufs& bb, const float* dy, float* tmp, int B, hipStream_t s) {
    const BlockBufs& fb = k.b;
    const FfnRoute& fr = k.pl->ffn(fb.e);
    const int j = k.j, e = fb.e, n1 = 4 * e;
    const int hbf = fr.hbf ? 1 : 0;   // bf16 storage of the hidden / saved FFN tensors
    const int pre = fr.pre ? 1 : 0;   // fb.a1 / fb.a3 hold h1 / h3 (fb.g1 / fb.g3 unused): GELU re-evaluated where needed
    const long Pn = (long)B * fb.h * fb.w;
    // f16-pair products in k_ffn1_bwd_xs (round 5): the forward's operand scales of this block + max |dh2|, which the spatial half leaves in word 6
    float* fsc = fr.bwd_scales ? k.ffn_scales : nullptr;
    if (fr.dw == FFN_DWBWD_TILE) {
        FfnDwBwdArgs fd;
        fd.dy = dy; fd.g3 = pre ? fb.a3 : fb.g3; fd.h2 = fb.h2; fd.dh2 = bb.dh2; fd.w3t = bb.w3t[j]; fd.dww = k.p(B_DWW);
        fd.slab_w = bb.rq.take(ffn_dw_bwd_slab_floats(e, B, fb.h, fb.w));
        if (!fd.slab_w) return -3;
        fd.slab_b = fd.slab_w + ffn_dw_bwd_slab_floats(e, B, fb.h, fb.w) / 10 * 9;
        fd.d_dww = k.g(B_DWW); fd.d_dwb = k.g(B_DWB);
        fd.B = B; fd.h = fb.h; fd.w = fb.w; fd.hbf = hbf; fd.pre = pre;
        RC(launch_ffn_dw_bwd(e, fd, s));
    } else {
        // the strip walk: dh3 in an LDS ring on the saved pre-activation h3, or (FFN_DWBWD_H, round 6) on h3 re-computed from h2 and the depthwise bias
        const bool h3re = fr.dw == FFN_DWBWD_H;
        FfnDwBwdXArgs fk;
        fk.dy = dy; fk.h3 = h3re ? nullptr : fb.a3; fk.h2 = fb.h2; fk.dh2 = bb.dh2; fk.w3t = bb.w3t[j]; fk.dww = k.p(B_DWW); fk.dwb = k.p(B_DWB);
        fk.slab = bb.rq.take(h3re ? ffn_dw_bwd_h_slab_floats() : ffn_dw_bwd_x_slab_floats(e));
        if (!fk.slab) return -3;
        fk.d_dww = k.g(B_DWW); fk.d_dwb = k.g(B_DWB); fk.d_w3 = k.g(B_W3); fk.d_b3 = k.g(B_B3);
        fk.B = B; fk.h = fb.h; fk.w = fb.w; fk.hbf = hbf;
        fk.dh2_max = fsc ? fsc + 6 : nullptr;
        RC(h3re ? launch_ffn_dw_bwd_h(fk, s) : launch_ffn_dw_bwd_xs(e, fk, s));
    }
    if (fr.px == FFN1_BWD_XS) {
        // one pass over dh2 re-computes h1 and yields dx, the LayerNorm gradients, dW1 / db1 and dW2 / db2
        Ffn1BwdXArgs fx;
        fx.scales = fsc;
        fx.dh2 = bb.dh2; fx.x = fb.xmid; fx.dy = dy; fx.dx = tmp;
        fx.w1 = k.p(B_W1); fx.b1 = k.p(B_B1); fx.w2t = bb.w2t[j]; fx.w1t = bb.w1t[j]; fx.ln2g = k.p(B_LN2G); fx.ln2b = k.p(B_LN2B);
        fx.slab = bb.rq.take(ffn1_bwd_x_slab_floats(e));
        if (!fx.slab) return -3;
        fx.d_w1 = k.g(B_W1); fx.d_b1 = k.g(B_B1); fx.d_w2 = k.g(B_W2); fx.d_b2 = k.g(B_B2); fx.d_ln2g = k.g(B_LN2G); fx.d_ln2b = k.g(B_LN2B);
        fx.P = Pn; fx.hbf = hbf;
        RC(launch_ffn1_bwd_xs(e, fx, s));
    } else {
        Ffn1BwdArgs f1;
        f1.dh2 = bb.dh2; f1.g1 = pre ? fb.a1 : fb.g1; f1.x = fb.xmid; f1.dy = dy; f1.dh1 = bb.dh1; f1.y2 = bb.y2; f1.dx = tmp;
        f1.w2t = bb.w2t[j]; f1.w1t = bb.w1t[j];
        f1.ln2g = k.p(B_LN2G); f1.ln2b = k.p(B_LN2B);
        f1.d_ln2g = k.g(B_LN2G); f1.d_ln2b = k.g(B_LN2B); f1.part = bb.rq.take((size_t)PIXEL_PART_WGS * 2 * e);
        if (!f1.part) return -3;
        f1.P = Pn; f1.hbf = hbf; f1.pre = pre;
        f1.w1 = nullptr; f1.wsplit = nullptr;
        if (fr.px == FFN1_BWD_X32) { f1.w1 = k.p(B_W1); f1.wsplit = bb.wsp; }
        f1.w1slab = nullptr; f1.d_w1 = nullptr; f1.d_b1 = nullptr;
        if (!fr.wgrad_w1) {   // dW1 / db1 come out of k_ffn1_bwd itself
            f1.w1slab = bb.rq.take((size_t)FFN1_BWD_WGS * ((size_t)n1 * e + n1));
            if (!f1.w1slab) return -3;
            f1.d_w1 = k.g(B_W1); f1.d_b1 = k.g(B_B1);
        }
        f1.w2slab = nullptr; f1.d_w2 = nullptr; f1.d_b2 = nullptr;   // (dW2 / db2: k_wgrad below)
        RC(launch_ffn1_bwd(e, fr.px, f1, s));
    }
    if (fr.wgrad_w2) RC(wgrad(bb.dh2, n1, fb.a1, n1, k.g(B_W2), n1, k.g(B_B2), Pn, n1, n1, n1, n1, hbf, hbf, bb, s, pre));
    if (fr.wgrad_w1) RC(wgrad(bb.dh1, n1, bb.y2, e, k.g(B_W1), e, k.g(B_B1), Pn, n1, e, n1, e, hbf, 0, bb, s));
    // last: dh2's two readers run right behind its producer (Infinity Cache), this one only needs the saved h3 / gelu(h3) and dy
    if (fr.wgrad_w3) RC(wgrad(dy, e, fb.a3, n1, k.g(B_W3), n1, k.g(B_B3), Pn, e, n1, e, n1, 0, hbf, bb, s, pre));
    return 0;
}

static int fft_bwd_call(const Blk& k, const float* do2, float* dg, int B, hipStream_t s, float* part) {
    const BlockBufs& fb = k.b;
    const int hc = fb.e / 2;
    FftBwdArgs fa;
    fa.do2 = do2; fa.sgn = fb.sgn; fa.amp = fb.amp; fa.pha = fb.pha; fa.dg = dg; fa.scratch = k.fft_scratch;
    fa.ampw = k.p(B_AMPW); fa.ampb = k.p(B_AMPB); fa.phaw = k.p(B_PHAW); fa.phab = k.p(B_PHAB);
    fa.d_ampw = k.g(B_AMPW); fa.d_ampb = k.g(B_AMPB); fa.d_phaw = k.g(B_PHAW); fa.d_phab = k.g(B_PHAB);
    fa.ch = hc; fa.planes = B * hc; fa.part = part;
    return launch_fftmix_bwd(k.pl->fft(fb.e), fa, s);
}

// mixer half-block backward: tmp (grad wrt the mid activation) -> dx_out (grad wrt block input)
static int mixer_half_bwd(const Blk& k, BwdBufs& bb, const float* tmp, float* dx_out, int B, int flags, uint64_t seed, hipStream_t s) {
    const BlockBufs& fb = k.b;
    const int e = fb.e, hc = e / 2;
    const long Pn = (long)B * fb.h * fb.w;
    const int drop = (flags & LG_FLAG_DROPOUT) ? 1 : 0;
    const MixerRoute& mr = k.pl->mixer(e);
    if (mr.bwd == ATTN_BWD_F) {
        // round 4: three launches per half-block -- proj^T towards the global mixer (+ dropout keep bits, proj bias gradient), the FFT-mixer
        // backward, and ONE kernel for everything else (flash passes, to_qkv^T, LayerNorm backward, dx, every parameter gradient)
        uint32_t* keep = drop ? reinterpret_cast<uint32_t*>(bb.dym) : nullptr;
        ProjO2BwdKArgs pk;
        pk.dy = tmp; pk.do2 = bb.do2; pk.keep = keep; pk.projw = k.p(B_PROJW);
        pk.slab = bb.rq.take((size_t)PROJ_O2_K_WGS * e);
        if (!pk.slab) return -3;
        pk.d_projb = k.g(B_PROJB); pk.HW = fb.h * fb.w; pk.total = Pn; pk.seed = mix_seed(seed, k.st, k.j);
        RC(launch_proj_o2_bwd_k(e, pk, s));
        float* fpart = bb.rq.take(k.pl->fft(e).bwd_part_floats((size_t)B * hc));
        if (!fpart) return -3;
        RC(fft_bwd_call(k, bb.do2, bb.dg, B, s, fpart));
        AttnBwdFArgs af;
        af.x = fb.xin; af.dy = tmp; af.keep = keep; af.o2 = fb.o2; af.dg = bb.dg; af.dx = dx_out;
        af.pos = k.p(B_POS); af.ln1g = k.p(B_LN1G); af.ln1b = k.p(B_LN1B); af.qkvw = k.p(B_QKVW); af.qkvb = k.p(B_QKVB); af.projw = k.p(B_PROJW);
        af.slab = bb.rq.take((size_t)ATTN_BWD_F_WGS * ATTN_BWD_F_ROW);   // a slab of its own per block: untouched until the pass's reduce launch
        if (!af.slab) return -3;
        af.d_pos = k.g(B_POS); af.d_qkvw = k.g(B_QKVW); af.d_qkvb = k.g(B_QKVB); af.d_projw = k.g(B_PROJW); af.d_ln1g = k.g(B_LN1G); af.d_ln1b = k.g(B_LN1B);
        af.B = B; af.h = fb.h; af.w = fb.w;
        if (mr.stats) { af.so = fb.att_o; af.sl = fb.att_l; }   // left by the forward's saving launch (block_mixer_fwd)
        return launch_attn_bwd_f(e, af, s);
    }
    ProjO2BwdArgs po;
    po.dy = tmp; po.do2 = bb.do2; po.dym = drop ? bb.dym : nullptr; po.projw = k.p(B_PROJW);
    po.HW = fb.h * fb.w; po.total = Pn; po.dropout = drop; po.seed = mix_seed(seed, k.st, k.j);
    RC(launch_proj_o2_bwd(e, po, s));
    const float* dym = drop ? bb.dym : tmp;
    float* fpart = bb.rq.take(k.pl->fft(e).bwd_part_floats((size_t)B * hc));
    if (!fpart) return -3;
    RC(fft_bwd_call(k, bb.do2, bb.dg, B, s, fpart));
    AttnBwdArgs at;
    at.x = fb.xin; at.dy = tmp; at.dym = dym; at.o2 = fb.o2; at.dg = bb.dg; at.dx = dx_out;
    at.cat = bb.cat; at.y1 = bb.y1; at.dqkv = bb.dqkv;
    at.pos = k.p(B_POS); at.dpos_slab = bb.rq.take(R3_DPOS_SLAB);
    if (!at.dpos_slab) return -3;
    at.ln1g = k.p(B_LN1G); at.ln1b = k.p(B_LN1B); at.qkvw = k.p(B_QKVW); at.qkvb = k.p(B_QKVB); at.projw = k.p(B_PROJW);
    at.d_ln1g = k.g(B_LN1G); at.d_ln1b = k.g(B_LN1B); at.part = bb.rq.take(attn_bwd_part_floats(e));
    at.d_qkvw = k.g(B_QKVW); at.d_qkvb = k.g(B_QKVB);
    if (attn_bwd_fuses_qkv(e)) at.y1 = nullptr;   // the epilogue kernel forms y1 itself and accumulates the to_qkv weight gradient
    if (!at.part) return -3;
    at.B = B; at.h = fb.h; at.w = fb.w; at.core_m = mr.bwd == ATTN_BWD_R3_CORE_M ? 1 : 0; at.stats = bb.attn_stats;
    if (mr.stats) { at.so = fb.att_o; at.sl = fb.att_l; }   // left by the forward's saving launch (block_mixer_fwd)
    RC(launch_attn_bwd(e, at, s));
    const int grid = attn_bwd_grid(e, B, fb.h, fb.w);
    RC(launch_reduce_slab(at.dpos_slab, grid, 1, POS_TABLE, k.g(B_POS), POS_TABLE, 1, POS_TABLE, s));
    RC(wgrad(dym, e, bb.cat, e, k.g(B_PROJW), e, k.g(B_PROJB), Pn, e, e, e, e, 0, 0, bb, s));
    if (!attn_bwd_fuses_qkv(e)) {
        const int y1ld = (hc + 15) / 16 * 16, dqld = (3 * hc + 15) / 16 * 16;
        RC(wgrad(bb.dqkv, dqld, bb.y1, y1ld, k.g(B_QKVW), hc, k.g(B_QKVB), Pn, dqld, y1ld, 3 * hc, hc, 0, 0,
                 bb, s));
    }
    return 0;
}

static int block_bwd(const Blk& k, BwdBufs& bb, const float* dy, float* tmp, float* dx_out, int B, int flags, uint64_t seed, hipStream_t s) {
    RC(ffn_half_bwd(k, bb, dy, tmp, B, s));
    RC(mixer_half_bwd(k, bb, tmp, dx_out, B, flags, seed, s));
    return bb.rq.block_end();   // (per_block form: one reduce launch per block; merged form: the pass's launch takes these jobs)
}

// per-op backward entry (tests): which 0: global mixer (dy, dx planar), 1: mixer half-block, 2: ffn half-block
int op_block_bwd(const Blk& k, int which, const float* dy, float* dx, void* bwd_ws, int B, hipStream_t s) {
    BwdBufs bb;
    carve_bwd(k.pl, B, bwd_ws, bb);
    if (which == 0) return fft_bwd_call(k, dy, dx, B, s, bb.slab_arena);   // no queue: summed at once
    ReduceQueueScope rqs(bb, s, k.pl->route.reduce_per_block);
    int rc = which == 1 ? 0 : ffn_transposes(&k, 1, bb, s);
    if (!rc) rc = which == 1 ? mixer_half_bwd(k, bb, dy, dx, B, 0, 0, s) : ffn_half_bwd(k, bb, dy, dx, B, s);
    const int rc2 = reduce_queue_end();
    return rc ? rc : rc2;
}

// zin: the tensor the forward data step of stage st consumed (nb.Z[st]; nb.X[st] in chained mode)
static int data_step_bwd(const lg_plan* pl, const float* P, float* G, int st, const NetBufs& nb, BwdBufs& bb, const float* zin,
                         const float* pan, const float* g, float* dz, int B, hipStream_t s) {
    const lg_config& c = pl->cfg;
    const int planes = B * c.C, H = c.H, W = c.W;
    if (pl->route.dstep_fused) {
        // one pixelwise + one plane-in-LDS launch (k_dstep.hip) instead of the nine tile launches below
        DstepBwdArgs a;
        a.g = g; a.z = zin; a.pan = pan; a.t1 = nb.t1[st]; a.r = nb.r[st]; a.s1 = nb.s1[st]; a.dz = dz;
        a.d1w = P + pl->shared(S_D1W); a.d3w = P + pl->shared(S_D3W); a.dt1w = P + pl->shared(S_DT1W); a.dt3w = P + pl->shared(S_DT3W);
        a.dt3b = P + pl->shared(S_DT3B);
        a.rw = P + pl->shared(S_RW); a.rb = P + pl->shared(S_RB); a.rtw = P + pl->shared(S_RTW); a.rtb = P + pl->shared(S_RTB);
        a.eta = P + pl->eta(st);
        a.B = B; a.C = c.C; a.N = H;
        float* part = bb.rq.take(dstep_bwd_part_floats(c.C, B, H));
        if (!part) return -3;
        const size_t bc = (size_t)B * c.C;
        a.part_top = part; a.part_dt1 = part + 14 * bc; a.part_d3 = part + 24 * bc; a.part_d1 = part + 34 * bc; a.part_pre = part + 44 * bc;
        DstepBwdGrads gg;
        gg.d1w = G + pl->shared(S_D1W); gg.d1b = G + pl->shared(S_D1B); gg.d3w = G + pl->shared(S_D3W); gg.d3b = G + pl->shared(S_D3B);
        gg.dt1w = G + pl->shared(S_DT1W); gg.dt1b = G + pl->shared(S_DT1B); gg.dt3w = G + pl->shared(S_DT3W); gg.dt3b = G + pl->shared(S_DT3B);
        gg.rw = G + pl->shared(S_RW); gg.rb = G + pl->shared(S_RB); gg.rtw = G + pl->shared(S_RTW); gg.rtb = G + pl->shared(S_RTB);
        gg.eta = G + pl->eta(st);
        RC(launch_dstep_bwd(a, gg, s));
        return bb.rq.block_end();   // the K stages share these parameters: per_block form, one launch per stage; merged form, one chain per parameter
    }
    DstepTopArgs t;
    t.g = g; t.s1 = nb.s1[st]; t.z = zin; t.pan = pan; t.gu = bb.gu3; t.dz = dz;
    t.w9 = P + pl->shared(S_DT3W); t.b9 = P + pl->shared(S_DT3B);
    t.rw = P + pl->shared(S_RW); t.rb = P + pl->shared(S_RB); t.rtw = P + pl->shared(S_RTW); t.rtb = P + pl->shared(S_RTB);
    t.eta = P + pl->eta(st);
    t.dw9 = G + pl->shared(S_DT3W); t.dbias = G + pl->shared(S_DT3B);
    t.drw = G + pl->shared(S_RW); t.drb = G + pl->shared(S_RB); t.drtw = G + pl->shared(S_RTW); t.drtb = G + pl->shared(S_RTB);
    t.deta = G + pl->eta(st);
    t.C = c.C; t.B = B; t.H = H; t.W = W; t.part = bb.rq.take(chan_partial_floats(c.C, B, H, W));
    if (!t.part) return -3;
    RC(launch_dstep_top_bwd(t, s));
    // s1 = dw(up(r)): grad wrt s1, then through the DT.1 conv
    RC(launch_resample_adj(1, bb.gu3, bb.gs1, planes, H / 2, W / 2, 0, s));
    DwBwdArgs d;
    d.C = c.C; d.planes = planes;
    d.gout = bb.gs1; d.in = nb.r[st]; d.gin = bb.gu1; d.w9 = P + pl->shared(S_DT1W);
    d.dw9 = G + pl->shared(S_DT1W); d.dbias = G + pl->shared(S_DT1B);
    d.hi = H / 4; d.wi = W / 4; d.n_h = H / 2; d.n_w = W / 2;
    d.part = bb.rq.take(chan_partial_floats(c.C, B, H, W));
    if (!d.part) return -3;
    RC(launch_dw_bwd(1, d, s));
    RC(launch_resample_adj(1, bb.gu1, bb.gr, planes, H / 4, W / 4, 0, s));
    // r = dw(down(t1)) - ms
    d.gout = bb.gr; d.in = nb.t1[st]; d.gin = bb.gd3; d.w9 = P + pl->shared(S_D3W);
    d.dw9 = G + pl->shared(S_D3W); d.dbias = G + pl->shared(S_D3B);
    d.hi = H / 2; d.wi = W / 2; d.n_h = H / 4; d.n_w = W / 4;
    d.part = bb.rq.take(chan_partial_floats(c.C, B, H, W));
    if (!d.part) return -3;
    RC(launch_dw_bwd(0, d, s));
    RC(launch_resample_adj(0, bb.gd3, bb.gt1, planes, H / 2, W / 2, 0, s));
    // t1 = dw(down(Z))
    d.gout = bb.gt1; d.in = zin; d.gin = bb.gd1; d.w9 = P + pl->shared(S_D1W);
    d.dw9 = G + pl->shared(S_D1W); d.dbias = G + pl->shared(S_D1B);
    d.hi = H; d.wi = W; d.n_h = H / 2; d.n_w = W / 2;
    d.part = bb.rq.take(chan_partial_floats(c.C, B, H, W));
    if (!d.part) return -3;
    RC(launch_dw_bwd(0, d, s));
    RC(launch_resample_adj(0, bb.gd1, dz, planes, H, W, 1, s));
    return bb.rq.block_end();   // the K stages share these parameters: per_block form, one launch per stage; merged form, one chain per parameter
}

// backward of stage st's LGT (LGT.py:314-344, reversed) from the activation set `nb` holds: dout = gradient wrt the LGT's
// output, zin = the LGT's input; leaves the gradient wrt zin in bb.dzA
static int lgt_bwd(const lg_plan* pl, const float* P, float* G, int st, const NetBufs& nb, BwdBufs& bb, const float* dout,
                   const float* zin, int B, int flags, uint64_t seed, hipStream_t s) {
    const lg_config& c = pl->cfg;
    const int E = 4 * c.C;
    const long P0 = (long)B * c.H * c.W, P1 = P0 / 4;
    const LgtSlots L{pl, P, G, st};
    Blk k[LG_NBLK];
    for (int j = 0; j < LG_NBLK; ++j) k[j] = nb.block(pl, P, G, st, j);
    float *A = bb.dx[0], *Bf = bb.dx[1], *Cf = bb.dx[2];
    RC(ffn_transposes(k, LG_NBLK, bb, s));
    TailBwdArgs tb;
    tb.dout = dout; tb.x = nb.blk[4].xout; tb.dx = A; tb.dz = bb.dzA; tb.w = L.p(L_TAILW);
    tb.d_w = L.g(L_TAILW); tb.d_b = L.g(L_TAILB);   // the conv's own weight gradient comes out of the same kernel
    tb.HW = c.H * c.W; tb.total = P0; tb.part = bb.rq.take(tail_bwd_part_floats(c.C));
    if (!tb.part) return -3;
    RC(launch_tail_bwd(c.C, tb, s));
    RC(block_bwd(k[4], bb, A, Bf, Cf, B, flags, seed, s));
    RC(block_bwd(k[3], bb, Cf, Bf, A, B, flags, seed, s));
    // up + fusion
    UpFuseBwdArgs ub;
    ub.dy = A; ub.dt = bb.dt; ub.dskip = bb.dskip; ub.v = bb.v; ub.dxb = Bf; ub.tmp = Cf;   // Cf is free until the bottleneck block
    ub.fw = L.p(L_FUSEW); ub.upw = L.p(L_UPW);
    ub.B = B; ub.H = c.H; ub.W = c.W;
    RC(launch_upfuse_bwd_a(E, ub, s));
    RC(wgrad(A, E, nb.t_up, E, L.g(L_FUSEW), 2 * E, L.g(L_FUSEB), P0, E, E, E, E, 0, 0, bb, s));
    RC(wgrad(A, E, nb.blk[1].xout, E, L.g(L_FUSEW) + E, 2 * E, nullptr, P0, E, E, E, E, 0, 0, bb, s));
    RC(launch_upfuse_bwd_b(E, ub, s));
    RC(wgrad(bb.v, E, nb.blk[2].xout, 2 * E, L.g(L_UPW), 2 * E, L.g(L_UPB), P1, E, 2 * E, E, 2 * E, 0, 0, bb, s));
    // bottleneck
    RC(block_bwd(k[2], bb, Bf, Cf, A, B, flags, seed, s));
    // down
    DownBwdArgs db;
    db.dy = A; db.du = bb.du; db.dskip = bb.dskip; db.dx = Bf; db.w = L.p(L_DOWNW);
    db.B = B; db.H = c.H; db.W = c.W;
    RC(launch_down_bwd_a(E, db, s));
    RC(wgrad(A, 2 * E, nb.u_down, E, L.g(L_DOWNW), E, L.g(L_DOWNB), P1, 2 * E, E, 2 * E, E, 0, 0, bb, s));
    RC(launch_down_bwd_b(E, db, s));
    // encoder
    RC(block_bwd(k[1], bb, Bf, Cf, A, B, flags, seed, s));
    RC(block_bwd(k[0], bb, A, Bf, Cf, B, flags, seed, s));
    // patch embed
    EmbedBwdArgs eb;
    eb.dx = Cf; eb.z = zin; eb.dz = bb.dzA;
    eb.dww = L.p(L_PE_DWW); eb.dwb = L.p(L_PE_DWB); eb.w = L.p(L_PE_W); eb.b = L.p(L_PE_B); eb.lng = L.p(L_PE_LNG);
    eb.d_dww = L.g(L_PE_DWW); eb.d_dwb = L.g(L_PE_DWB); eb.d_lng = L.g(L_PE_LNG); eb.d_lnb = L.g(L_PE_LNB);
    eb.d_w = L.g(L_PE_W); eb.d_b = L.g(L_PE_B);   // the conv's own weight gradient comes out of the same kernel
    eb.HW = c.H * c.W; eb.total = P0; eb.part = bb.rq.take(embed_bwd_part_floats(c.C));
    if (!eb.part) return -3;
    RC(launch_embed_bwd(c.C, eb, s));
    return 0;
}

// per-op backward entries (tests): one data step / one LGT in isolation.  The forward of the same piece has just filled `nb`
// (data step: nb.t1 / r / s1 [st]; LGT: the saved activation set).
int op_data_step_bwd(const lg_plan* pl, const float* P, float* G, int st, NetBufs& nb, void* bwd_ws, const float* z_in, const float* pan,
                     const float* g, float* dz, int B, hipStream_t s) {
    BwdBufs bb;
    carve_bwd(pl, B, bwd_ws, bb);
    ReduceQueueScope rqs(bb, s, pl->route.reduce_per_block);
    const int rc = data_step_bwd(pl, P, G, st, nb, bb, z_in, pan, g, dz, B, s);
    const int rc2 = reduce_queue_end();
    return rc ? rc : rc2;
}

int op_lgt_bwd(const lg_plan* pl, const float* P, float* G, int st, NetBufs& nb, void* bwd_ws, const float* z, const float* dout, float* dz,
               int B, int flags, uint64_t seed, hipStream_t s) {
    BwdBufs bb;
    carve_bwd(pl, B, bwd_ws, bb);
    bb.dzA = dz;                       // lgt_bwd leaves the gradient wrt the LGT's input here
    ReduceQueueScope rqs(bb, s, pl->route.reduce_per_block);
    const int rc = lgt_bwd(pl, P, G, st, nb, bb, dout, z, B, flags, seed, s);
    const int rc2 = reduce_queue_end();
    return rc ? rc : rc2;
}

int net_backward(const lg_plan* pl, const float* P, float* G, const float* ms, const float* pan, const float* dout, NetBufs& nb,
                 void* bwd_ws, int B, int flags, uint64_t seed, hipStream_t s) {
    (void)ms;
    const lg_config& c = pl->cfg;
    BwdBufs bb;
    carve_bwd(pl, B, bwd_ws, bb);
    ReduceQueueScope rqs(bb, s, pl->route.reduce_per_block);
    if (flags & LG_FLAG_CHAINED) {
        // intended unfolding (every stage live): LGT_i then data step i, last stage first; each LGT reads its own activation set
        const float* g = dout;
        for (int i = c.K - 1; i >= 0; --i) {
            const NetBufs sv = stage_view(nb, i);
            RC(lgt_bwd(pl, P, G, i, sv, bb, g, nb.Z[i + 1], B, flags, seed, s));
            if (!bb.rq.per_block) RC(bb.rq.flush());   // merged form: one launch per LGT and per data step here (the arena holds one LGT pass)
            RC(data_step_bwd(pl, P, G, i, nb, bb, nb.X[i], pan, bb.dzA, bb.dzB, B, s));
            RC(bb.rq.flush());
            g = bb.dzB;
        }
        return reduce_queue_end();
    }
    const bool do_lgt = !(flags & (LG_FLAG_BWD_LGT | LG_FLAG_BWD_DATA)) || (flags & LG_FLAG_BWD_LGT);
    const bool do_data = !(flags & (LG_FLAG_BWD_LGT | LG_FLAG_BWD_DATA)) || (flags & LG_FLAG_BWD_DATA);
    // ---------------- LGT of the last stage: the only live one
    if (do_lgt) RC(lgt_bwd(pl, P, G, c.K - 1, live_view(nb), bb, dout, nb.Z[c.K], B, flags, seed, s));   // its xin / xmid / xout: slot K-1 (workspace.h)
    if (!do_data) return reduce_queue_end();
    // merged form: the LGT's gradients are complete here (LG_FLAG_BWD_LGT / _DATA, the two-bucket all-reduce), the K data steps follow in ONE launch
    if (do_lgt && !bb.rq.per_block) RC(bb.rq.flush());
    // ---------------- K shared data steps, last to first (unlg_former.py:56-61); input gradient: bb.dzA
    float* g = bb.dzA;
    float* dz = bb.dzB;
    for (int i = c.K - 1; i >= 0; --i) {
        RC(data_step_bwd(pl, P, G, i, nb, bb, nb.Z[i], pan, g, dz, B, s));
        float* t = g; g = dz; dz = t;
    }
    return reduce_queue_end();
}
