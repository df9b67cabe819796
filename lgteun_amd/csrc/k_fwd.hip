// Forward orchestration (Pansharpening.forward, reference models/unlg_former.py:50-67): lgteun_forward, lgteun_dead_forward and the pieces the
// per-op entries of api.hip run on their own (forward.h).  Host code only: every kernel is behind a launcher of kernels.h.
#include <string.h>

#include "abi.h"
#include "forward.h"
#include "net_args.h"

int data_step_fwd(const lg_plan* pl, const float* P, int stage, const float* z_in, const float* ms, const float* pan,
                  float* z_out, float* t1, float* r, float* s1, float* pr, int B, hipStream_t s) {
    const lg_config& c = pl->cfg;
    const int planes = B * c.C, H = c.H, W = c.W;
    if (pl->route.dstep_fused) {
        DstepFwdArgs f;
        f.z = z_in; f.ms = ms; f.pan = pan; f.zout = z_out; f.t1 = t1; f.r = r; f.s1 = s1; f.pr = pr;
        f.d1w = P + pl->shared(S_D1W); f.d1b = P + pl->shared(S_D1B); f.d3w = P + pl->shared(S_D3W); f.d3b = P + pl->shared(S_D3B);
        f.dt1w = P + pl->shared(S_DT1W); f.dt1b = P + pl->shared(S_DT1B); f.dt3w = P + pl->shared(S_DT3W); f.dt3b = P + pl->shared(S_DT3B);
        f.rw = P + pl->shared(S_RW); f.rb = P + pl->shared(S_RB); f.rtw = P + pl->shared(S_RTW); f.rtb = P + pl->shared(S_RTB);
        f.eta = P + pl->eta(stage);
        f.B = B; f.C = c.C; f.N = H;
        return launch_dstep_fwd(f, s);
    }
    DwArgs a;
    memset(&a, 0, sizeof(a));
    a.C = c.C; a.planes = planes;
    int rc;
    // D: x0.5, dw3, x0.5, dw3  (unlg_former.py:29-30) ; then "- ms" (unlg_former.py:58)
    a.in = z_in; a.out = t1; a.w9 = P + pl->shared(S_D1W); a.bias = P + pl->shared(S_D1B);
    a.hi = H; a.wi = W; a.ho = H / 2; a.wo = W / 2;
    if ((rc = launch_resample_dw(0, 0, a, s))) return rc;
    a.in = t1; a.out = r; a.w9 = P + pl->shared(S_D3W); a.bias = P + pl->shared(S_D3B); a.sub = ms;
    a.hi = H / 2; a.wi = W / 2; a.ho = H / 4; a.wo = W / 4;
    if ((rc = launch_resample_dw(0, 1, a, s))) return rc;
    // DT: x2, dw3, x2, dw3 (unlg_former.py:32-33)
    a.in = r; a.out = s1; a.w9 = P + pl->shared(S_DT1W); a.bias = P + pl->shared(S_DT1B); a.sub = nullptr;
    a.hi = H / 4; a.wi = W / 4; a.ho = H / 2; a.wo = W / 2;
    if ((rc = launch_resample_dw(1, 0, a, s))) return rc;
    // last DT stage fused with pan term and the update (unlg_former.py:59-61)
    a.in = s1; a.out = z_out; a.w9 = P + pl->shared(S_DT3W); a.bias = P + pl->shared(S_DT3B);
    a.z = z_in; a.pan = pan; a.rw = P + pl->shared(S_RW); a.rb = P + pl->shared(S_RB);
    a.rtw = P + pl->shared(S_RTW); a.rtb = P + pl->shared(S_RTB); a.eta = P + pl->eta(stage);
    a.hi = H / 2; a.wi = W / 2; a.ho = H; a.wo = W;
    return launch_resample_dw(1, 2, a, s);
}

// the two launches of a block's mixer: the global (FFT) half, a plane kernel, and the local half + proj + residual, a persistent one
static int mixer_fft_fwd(const Blk& k, int B, int flags, hipStream_t s, const StageSel& sg) {
    const lg_plan* pl = k.pl;
    const BlockBufs& bb = k.b;
    FftArgs f;
    f.g = bb.g; f.o = bb.o2;
    f.amp = (flags & LG_FLAG_SAVE) ? bb.amp : nullptr;
    f.pha = (flags & LG_FLAG_SAVE) ? bb.pha : nullptr;
    f.sgn = (flags & LG_FLAG_SAVE) ? bb.sgn : nullptr;
    f.scratch = k.fft_scratch;
    f.ampw = k.p(B_AMPW); f.ampb = k.p(B_AMPB); f.phaw = k.p(B_PHAW); f.phab = k.p(B_PHAB);
    f.ch = bb.e / 2; f.planes = B * f.ch;
    f.sg = sg;
    return launch_fftmix(pl->fft(bb.e), f, s);
}
static int mixer_local_fwd(const Blk& k, int B, int flags, uint64_t seed, hipStream_t s, const StageSel& sg) {
    const lg_plan* pl = k.pl;
    const BlockBufs& bb = k.b;
    const MixerRoute& mr = pl->mixer(bb.e);
    AttnArgs t;
    t.x = bb.xin; t.o2 = bb.o2; t.y = bb.xmid; t.posT = k.posT; t.pos = k.p(B_POS);
    t.bf16 = mr.bf16 ? 1 : 0;
    t.ln1g = k.p(B_LN1G); t.ln1b = k.p(B_LN1B); t.qkvw = k.p(B_QKVW); t.qkvb = k.p(B_QKVB); t.projw = k.p(B_PROJW); t.projb = k.p(B_PROJB);
    t.B = B; t.h = bb.h; t.w = bb.w;
    t.dropout = (flags & LG_FLAG_DROPOUT) ? 1 : 0;
    t.seed = mix_seed(seed, k.st, k.j);
    t.sg = sg; t.sg.seed = seed; t.sg.stage0 = k.st; t.sg.blk = k.j;   // several stages: the kernel keys each stage's mask itself
    t.scales = mr.f16x2 ? k.attn_scales : nullptr;   // written by prep_stages for the stages of this call
    if ((flags & LG_FLAG_SAVE) && mr.stats) { t.save_o = bb.att_o; t.save_l = bb.att_l; }
    if (sg.n > 1 && mr.fwd == ATTN_FWD_VALU) { lg_set_error("mixer: the vector-pipe kernel takes one stage per launch"); return -2; }
    return mr.fwd == ATTN_FWD_VALU ? launch_attn(bb.e, t, s) : launch_attn_m(bb.e, t, s);
}
int block_mixer_fwd(const Blk& k, int B, int flags, uint64_t seed, hipStream_t s, const StageSel& sg) {
    if (int rc = mixer_fft_fwd(k, B, flags, s, sg)) return rc;
    return mixer_local_fwd(k, B, flags, seed, s, sg);
}

// next: the block whose mixer reads this FFN's output directly (its LN1 + planar split ride in this FFN's epilogue), or null
int block_ffn_fwd(const Blk& k, const Blk* next, int B, int flags, hipStream_t s, const StageSel& sg) {
    int rc;
    const BlockBufs& bb = k.b;
    const FfnRoute& fr = k.pl->ffn(bb.e);
    const unsigned saves = (flags & LG_FLAG_SAVE) ? fr.saves : 0;   // the slots the backward's route reads (route.h)
    Ffn1Args a1;
    a1.x = bb.xmid; a1.a1s = (saves & FFN_SLOT_A1) ? bb.a1 : nullptr; a1.g1s = (saves & FFN_SLOT_G1) ? bb.g1 : nullptr;
    a1.ln2g = k.p(B_LN2G); a1.ln2b = k.p(B_LN2B); a1.w1 = k.p(B_W1); a1.b1 = k.p(B_B1); a1.w2 = k.p(B_W2); a1.b2 = k.p(B_B2);
    a1.P = (long)B * bb.h * bb.w;
    a1.hbf = fr.hbf ? 1 : 0;
    a1.kernel = fr.fwd[(flags & LG_FLAG_SAVE) ? 1 : 0];
    a1.wsplit = k.wsplit;   // this block's slot, filled by prep_stages
    a1.wsplit_ready = bb.e >= 32 ? 1 : 0;
    a1.scales = fr.scales ? k.ffn_scales : nullptr;   // written by prep_stages for the stages of this call
    Ffn2Args a2;
    a2.h2 = bb.h2; a2.x = bb.xmid; a2.a3s = (saves & FFN_SLOT_A3) ? bb.a3 : nullptr; a2.g3s = (saves & FFN_SLOT_G3) ? bb.g3 : nullptr; a2.y = bb.xout;   // g3s null with a3s set: a3 receives the PRE-activation h3
    a2.g = next ? next->b.g : nullptr;
    a2.dww = k.p(B_DWW); a2.dwb = k.p(B_DWB); a2.w3 = k.p(B_W3); a2.b3 = k.p(B_B3);
    a2.n1g = next ? next->p(B_LN1G) : nullptr;
    a2.n1b = next ? next->p(B_LN1B) : nullptr;
    a2.B = B; a2.h = bb.h; a2.w = bb.w; a2.hbf = a1.hbf;
    a1.h2 = bb.h2;
    a1.sg = sg;
    if (sg.n > 1 && a1.kernel != FFN_FWD_XR && a1.kernel != FFN_FWD_X32) { lg_set_error("ffn: this route's kernel takes one stage per launch"); return -2; }
    if (a1.kernel == FFN_FWD_UNFUSED) {
        if ((rc = launch_ffn1(bb.e, a1, s))) return rc;
        return launch_ffn2(bb.e, a2, s);
    }
    // fused kernels (e <= 32): h2 only leaves the chip when the backward needs it; e = 64 passes it through HBM between its two kernels
    if (!saves && bb.e != 64) a1.h2 = nullptr;
    return launch_ffn_fused(bb.e, a1, a2, s);
}

// what the LGTs of stages [st0, st1) need in front of their first kernel, into the rows of their blocks (workspace.h) -- one launch each for all
// stages of the call (a launch per stage was 5 us + a launch gap each): the transposed pos_emb tables (round 2's vector-pipe mixer, LG_ATTN_FWD=valu,
// alone reads them), the operand scales of the f16-pair FFN arithmetic, and the pre-split weight fragments of every e >= 32 block, behind the scales
// they are multiplied by (round 5: one launch per forward call instead of one in front of every FFN launch)
int prep_stages(const lg_plan* pl, const float* P, int st0, int st1, const NetBufs& nb, hipStream_t s) {
    if (st1 <= st0) return 0;
    const float* psrc[LG_NBLK * LG_MAX_K];
    float* pdst[LG_NBLK * LG_MAX_K];
    FfnPrepJob jobs[LG_NBLK * LG_MAX_K];
    SplitWJob sj[LG_NBLK * LG_MAX_K];
    int n = 0, ns = 0, rc;
    for (int st = st0; st < st1; ++st)
        for (int j = 0; j < LG_NBLK; ++j, ++n) {
            const Blk k = nb.block(pl, P, nullptr, st, j);
            psrc[n] = k.p(B_POS); pdst[n] = nb.posT_row(st, j);
            FfnPrepJob& q = jobs[n];
            q.ln2g = k.p(B_LN2G); q.ln2b = k.p(B_LN2B); q.w1 = k.p(B_W1); q.b1 = k.p(B_B1); q.w2 = k.p(B_W2); q.b2 = k.p(B_B2);
            q.dww = k.p(B_DWW); q.dwb = k.p(B_DWB); q.w3 = k.p(B_W3);
            q.e = k.b.e;
            q.ln1g = k.p(B_LN1G); q.ln1b = k.p(B_LN1B); q.qkvw = k.p(B_QKVW); q.qkvb = k.p(B_QKVB);
            if (k.b.e < 32 || k.b.e % 32) continue;
            SplitWJob& w = sj[ns++];
            w.w1 = k.p(B_W1); w.w2 = k.p(B_W2); w.w3 = k.p(B_W3);
            w.e = k.b.e; w.np = pl->ffn(k.b.e).wsplit_np;
            w.scales = w.np == 2 ? k.ffn_scales : nullptr;
            w.out = k.wsplit;
        }
    if (pl->route.mix[0].fwd == ATTN_FWD_VALU && (rc = launch_pos_transpose_n(n, psrc, pdst, s))) return rc;
    if (pl->route.ffn[0].scales &&   // (the same at both levels)
        (rc = launch_ffn_scales(n, jobs, nb.ffn_scales_row(st0, 0), s, pl->route.mix[0].f16x2 ? nb.attn_scales_row(st0, 0) : nullptr))) return rc;
    return ns ? launch_split_w_jobs(ns, sj, s) : 0;
}

// LGT.forward (LGT.py:314-344) on z -> out with the buffers of `nb`, whose rows of this stage the caller has filled (prep_stages)
// nst > 1: the LGTs of stages stage .. stage + nst - 1 in ONE pass, every kernel launched once over nst * B samples (kernels.h: StageSel) -- stage
// stage + i reads z + i * zstride, writes out + i * B C H W and uses samples [i B, (i + 1) B) of every buffer of `nb` (workspace.h carves them
// that large for a plan with stage_batch).
// live_out == null: never with LG_FLAG_SAVE, only dead stages run this way.
// live_out != null: the LIVE stage rides along as the last of the nst = K stages (stage = 0; its slot K-1 is the one live_view(nb) names).  The plane and
// pixel kernels -- embed, FFT mixer, down, up + fusion, tail -- launch once over all K B samples and save (LG_FLAG_SAVE) from sample (K-1) B on only; the
// persistent kernels -- local mixer, FFN -- launch twice, the same two launches a dead pass and a live pass make: the live stage's own (saving) launch on
// slot K-1 and the multi-stage non-saving instance over the K-1 dead stages (per block: the live pair first, see `block` below).  The last stage's output
// goes to live_out.
int lgt_fwd(const lg_plan* pl, const float* P, int stage, const float* z, float* out, const NetBufs& nb, int B, int flags, uint64_t seed,
            hipStream_t s, int nst, long zstride, int grid_cap, float* live_out) {
    const lg_config& c = pl->cfg;
    const int E = 4 * c.C;
    const bool ride = live_out != nullptr;
    int rc;
    StageSel sg;
    if (nst > 1) {
        if (!pl->stage_batch || (!ride && (flags & LG_FLAG_SAVE))) { lg_set_error("lgt_fwd: this plan / call runs one stage per pass"); return -2; }
        sg.n = nst; sg.Bs = B; sg.pstride = pl->stage_stride; sg.zstride = zstride; sg.grid_cap = grid_cap;
        nb.stage_strides(sg);
    }
    if (ride && (stage != 0 || nst != c.K || nb.live_s0 != (size_t)(nst - 1) * B)) { lg_set_error("lgt_fwd: the live stage rides behind all K-1 dead ones, in slot K-1"); return -2; }
    const int Bs = B, fdead = flags & ~LG_FLAG_SAVE;
    StageSel sgd = sg;           // the persistent kernels' dead launch: stages 0 .. nst - 2
    if (ride) { sg.s0 = (nst - 1) * Bs; sgd.n = nst - 1; }
    B *= nst;   // what every plane / pixel kernel below sees: a plain batch
    const LgtSlots L{pl, P, nullptr, stage};
    Blk k[LG_NBLK], kl[LG_NBLK];   // kl: the live stage's blocks (ride)
    const NetBufs lv = ride ? live_view(nb) : nb;
    for (int j = 0; j < LG_NBLK; ++j) { k[j] = nb.block(pl, P, nullptr, stage, j); kl[j] = lv.block(pl, P, nullptr, stage + nst - 1, j); }
    // one LGB block j: mixer, then FFN; next: the block whose LN1 + planar split ride in this FFN's epilogue, or -1.  Riding: the FFT mixer over all K B samples,
    // then the live stage's persistent pair (local mixer, FFN: saving), then the dead stages' -- the launch that follows reads K-1 stages' worth of what the dead
    // pair wrote last and finds it in the caches; behind the live pair's saved tensors it would not
    auto block = [&](int j, int next) -> int {
        int r;
        if (!ride) return (r = block_mixer_fwd(k[j], B, flags, seed, s, sg)) ? r : block_ffn_fwd(k[j], next < 0 ? nullptr : &k[next], B, flags, s, sg);
        if ((r = mixer_fft_fwd(k[j], B, flags, s, sg))) return r;
        if ((r = mixer_local_fwd(kl[j], Bs, flags, seed, s, StageSel())) || (r = block_ffn_fwd(kl[j], next < 0 ? nullptr : &kl[next], Bs, flags, s, StageSel()))) return r;
        if ((r = mixer_local_fwd(k[j], sgd.n * Bs, fdead, seed, s, sgd))) return r;
        return block_ffn_fwd(k[j], next < 0 ? nullptr : &k[next], sgd.n * Bs, fdead, s, sgd);
    };
    EmbedArgs ea;
    ea.z = z; ea.x = nb.x0; ea.g = nb.blk[0].g;
    ea.dww = L.p(L_PE_DWW); ea.dwb = L.p(L_PE_DWB); ea.w = L.p(L_PE_W); ea.b = L.p(L_PE_B); ea.lng = L.p(L_PE_LNG); ea.lnb = L.p(L_PE_LNB);
    ea.n1g = k[0].p(B_LN1G); ea.n1b = k[0].p(B_LN1B);
    ea.HW = c.H * c.W; ea.total = (long)B * c.H * c.W; ea.sg = sg;
    if ((rc = launch_embed(c.C, ea, s))) return rc;
    // encoder LGB (2 blocks)
    if ((rc = block(0, 1))) return rc;
    if ((rc = block(1, -1))) return rc;
    // down
    DownArgs da;
    da.x = nb.blk[1].xout; da.y = nb.blk[2].xin; da.g = nb.blk[2].g;
    da.u_save = (flags & LG_FLAG_SAVE) ? nb.u_down : nullptr;
    da.w = L.p(L_DOWNW); da.b = L.p(L_DOWNB);
    da.n1g = k[2].p(B_LN1G); da.n1b = k[2].p(B_LN1B);
    da.B = B; da.H = c.H; da.W = c.W; da.sg = sg;
    if ((rc = launch_down(E, da, s))) return rc;
    // bottleneck
    if ((rc = block(2, -1))) return rc;
    // up + fusion
    UpFuseArgs ua;
    ua.xb = nb.blk[2].xout; ua.skip = nb.blk[1].xout; ua.y = nb.blk[3].xin; ua.g = nb.blk[3].g;
    ua.t_save = (flags & LG_FLAG_SAVE) ? nb.t_up : nullptr;
    ua.upw = L.p(L_UPW); ua.upb = L.p(L_UPB); ua.fw = L.p(L_FUSEW); ua.fb = L.p(L_FUSEB);
    ua.n1g = k[3].p(B_LN1G); ua.n1b = k[3].p(B_LN1B);
    ua.B = B; ua.H = c.H; ua.W = c.W; ua.sg = sg;
    if ((rc = launch_upfuse(E, ua, s))) return rc;
    // decoder LGB (2 blocks)
    if ((rc = block(3, 4))) return rc;
    if ((rc = block(4, -1))) return rc;
    // tail
    TailArgs ta;
    ta.x = nb.blk[4].xout; ta.z = z; ta.out = out; ta.out_last = live_out;
    ta.w = L.p(L_TAILW); ta.b = L.p(L_TAILB);
    ta.HW = c.H * c.W; ta.total = (long)B * c.H * c.W; ta.sg = sg;
    return launch_tail(c.C, ta, s);
}

// where dead stage i's output goes: a plan with stage_batch has room for all K-1 of them (the batched pass writes them side by side), any other one slot
static float* dead_out(const lg_plan* pl, const NetBufs& nb, int i, int B) {
    return nb.deadout + (pl->stage_batch ? (size_t)i * B * pl->cfg.C * pl->cfg.H * pl->cfg.W : 0);
}
// do the K-1 dead-stage LGT forwards of this plan / call run as one pass?
static bool dead_as_one_pass(const lg_plan* pl, int flags) { return pl->stage_batch && !(flags & LG_FLAG_STAGEWISE); }
// the K-1 dead-stage LGT forwards behind the data steps: non-saving, Z[1 ..] in, deadout[0 ..] out -- one pass (lgt_fwd with nst = K-1) or one by one
static int dead_stages(const lg_plan* pl, const float* P, const NetBufs& nb, int B, int flags, uint64_t seed, hipStream_t s) {
    flags &= ~LG_FLAG_SAVE;
    if (dead_as_one_pass(pl, flags)) return lgt_fwd(pl, P, 0, nb.Z[1], nb.deadout, nb, B, flags, seed, s, pl->cfg.K - 1, (long)(nb.Z[2] - nb.Z[1]));
    for (int i = 0; i + 1 < pl->cfg.K; ++i)
        if (int rc = lgt_fwd(pl, P, i, nb.Z[i + 1], dead_out(pl, nb, i, B), nb, B, flags, seed, s)) return rc;
    return 0;
}

extern "C" int lgteun_forward(const lg_plan* plan, const float* params, const float* ms, const float* pan, float* out,
                              void* workspace, size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream) {
    const bool chained = (flags & LG_FLAG_CHAINED) != 0;
    const int train = (flags & LG_FLAG_SAVE) ? (chained ? 2 : 1) : 0;
    NetArgs v("forward");
    v.plan(plan).f32(params, "params").f32(ms, "ms").f32(pan, "pan").f32(out, "out").flags(flags, LG_FLAGS_FORWARD);
    if (v.batch(B, train).workspace(workspace, workspace_bytes, B, train).rc) return v.rc;
    hipStream_t s = (hipStream_t)stream;
    const lg_config& c = plan->cfg;
    NetBufs nb;
    carve(plan, B, train, workspace, nb);
    int rc;
    // the rows of every stage whose LGT runs in this call
    const bool all_stages = chained || ((flags & LG_FLAG_FAITHFUL) && !(flags & LG_FLAG_DEFER_DEAD));
    if ((rc = prep_stages(plan, params, all_stages ? 0 : c.K - 1, c.K, nb, s))) return rc;
    // Z0 = bicubic x4 (unlg_former.py:53)
    if ((rc = launch_resample(2, ms, nb.Z[0], B * c.C, c.H / 4, c.W / 4, s))) return rc;
    if (chained) {
        // intended unfolding: X_{i+1} = LGT_i(data_step_i(X_i)); every stage saves into its own activation set when training
        for (int i = 0; i < c.K; ++i) {
            if ((rc = data_step_fwd(plan, params, i, nb.X[i], ms, pan, nb.Z[i + 1], nb.t1[i], nb.r[i], nb.s1[i], nb.pr, B, s))) return rc;
            NetBufs sv = (train == 2) ? stage_view(nb, i) : nb;
            if ((rc = lgt_fwd(plan, params, i, nb.Z[i + 1], i == c.K - 1 ? out : nb.X[i + 1], sv, B, flags, seed, s))) return rc;
        }
        return 0;
    }
    // The reference executes the LGTs of stages 0 .. K-2 and discards their result (unlg_former.py:63-67).  They read Z[1] .. Z[K-1], which
    // the data steps alone produce, so with two or more of them (and a route whose kernels can: lg_plan_stage_batch) the K data steps run first and the
    // dead stages follow as ONE pass over (K-1) B samples; LG_FLAG_STAGEWISE keeps them one by one, each behind its data step.
    const bool dead = (flags & LG_FLAG_FAITHFUL) && !(flags & LG_FLAG_DEFER_DEAD) && c.K > 1;
    const bool one_pass = dead && dead_as_one_pass(plan, flags);
    for (int i = 0; i < c.K; ++i) {
        if ((rc = data_step_fwd(plan, params, i, nb.Z[i], ms, pan, nb.Z[i + 1], nb.t1[i], nb.r[i], nb.s1[i], nb.pr, B, s))) return rc;
        if (i < c.K - 1 && dead && !one_pass &&
            (rc = lgt_fwd(plan, params, i, nb.Z[i + 1], dead_out(plan, nb, i, B), nb, B, flags & ~LG_FLAG_SAVE, seed, s))) return rc;
    }
    // One pass: the live stage rides along in the plane and pixel launches of the dead ones (lgt_fwd: live_out), 1 024 instead of 768 + 256 planes of
    // the level-0 FFT mixer at B = 32; LG_FLAG_LIVE_APART keeps the dead pass and the live pass apart.  Either way, and on every other path, the live
    // stage's transient buffers are slot K-1 (workspace.h: live_view) -- the backward reads them there.
    if (one_pass && !(flags & LG_FLAG_LIVE_APART))
        return lgt_fwd(plan, params, 0, nb.Z[1], nb.deadout, nb, B, flags, seed, s, c.K, (long)(nb.Z[2] - nb.Z[1]), 0, out);
    if (one_pass && (rc = dead_stages(plan, params, nb, B, flags, seed, s))) return rc;
    return lgt_fwd(plan, params, c.K - 1, nb.Z[c.K], out, live_view(nb), B, flags, seed, s);
}

extern "C" int lgteun_dead_forward(const lg_plan* plan, const float* params, void* workspace, size_t workspace_bytes, int32_t B,
                                   int32_t flags, uint64_t seed, void* stream) {
    const int train = (flags & LG_FLAG_SAVE) ? 1 : 0;
    NetArgs v("dead_forward");
    v.plan(plan).f32(params, "params").flags(flags, LG_FLAGS_FORWARD);
    if (!v.rc && ((flags & LG_FLAG_CHAINED) || !(flags & LG_FLAG_FAITHFUL))) v.fail(-2, "flags: only the faithful unfolding has dead stages");
    if (v.batch(B, train).workspace(workspace, workspace_bytes, B, train).rc) return v.rc;
    NetBufs nb;
    carve(plan, B, train, workspace, nb);
    if (int rc = prep_stages(plan, params, 0, plan->cfg.K - 1, nb, (hipStream_t)stream)) return rc;
    return dead_stages(plan, params, nb, B, flags, seed, (hipStream_t)stream);
}
