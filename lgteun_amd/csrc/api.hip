// C ABI entry points (include/lgteun_hip.h): plan, forward orchestration, per-op entries, the optimizer steps; one-line forwards to the rest.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <atomic>
#include <mutex>

// only the C ABI of include/lgteun_hip.h is exported from the shared object (everything else: -fvisibility=hidden)
#pragma GCC visibility push(default)
#include "../../include/lgteun_hip.h"
#pragma GCC visibility pop

#include "kernels.h"
#include "workspace.h"
#include "backward.h"

static thread_local char g_err[512] = "";

void lg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ------------------------------------------------------------------------------------------------
// live per-kernel timing
// ------------------------------------------------------------------------------------------------
// The ONE piece of mutable process-global state of the library (documented in the header): the event table of the timing
// facility.  `kid` is atomic so that the launch path pays one relaxed load while profiling is off; everything else is under the mutex.
static struct {
    std::atomic<int> kid{0};
    std::atomic<int> paused{0};
    int cap = 0, n = 0;
    int64_t units = 0;         // stage-sized launches the n timed launches stand for (ProfScope: a launch over S stages counts S)
    hipEvent_t* ev = nullptr;  // 2 per launch
    std::mutex mu;
} g_prof;

void lg_prof_begin(int kid, hipStream_t s) {
    if (kid != g_prof.kid.load(std::memory_order_relaxed) || g_prof.paused.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (kid != g_prof.kid.load(std::memory_order_relaxed) || g_prof.n >= g_prof.cap) return;
    hipEventRecord(g_prof.ev[2 * g_prof.n], s);
}
void lg_prof_end(int kid, hipStream_t s, int units) {
    if (kid != g_prof.kid.load(std::memory_order_relaxed) || g_prof.paused.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (kid != g_prof.kid.load(std::memory_order_relaxed) || g_prof.n >= g_prof.cap) return;
    hipEventRecord(g_prof.ev[2 * g_prof.n + 1], s);
    g_prof.n++;
    g_prof.units += units;
}
static void prof_disable_locked() {
    for (int i = 0; i < 2 * g_prof.cap; ++i) hipEventDestroy(g_prof.ev[i]);
    free(g_prof.ev);
    g_prof.ev = nullptr;
    g_prof.cap = g_prof.n = 0;
    g_prof.units = 0;
    g_prof.kid.store(0);
    g_prof.paused.store(0);
}
extern "C" void lg_prof_disable(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    prof_disable_locked();
}
extern "C" int lg_prof_enable(int32_t kernel_id, int32_t max_launches) {
    if (kernel_id <= 0 || kernel_id >= LG_K_COUNT || max_launches <= 0) { lg_set_error("prof_enable: invalid argument"); return -1; }
    std::lock_guard<std::mutex> lk(g_prof.mu);
    prof_disable_locked();
    g_prof.ev = (hipEvent_t*)malloc(sizeof(hipEvent_t) * 2 * max_launches);
    for (int i = 0; i < 2 * max_launches; ++i) {
        hipError_t e = hipEventCreate(&g_prof.ev[i]);
        if (e != hipSuccess) { lg_set_error("prof_enable: hipEventCreate: %s", hipGetErrorString(e)); return (int)e; }
    }
    g_prof.cap = max_launches;
    g_prof.kid.store(kernel_id);
    return 0;
}
// sampling: while paused, launches are neither timed nor counted (an event pair costs ~2 us of stream time; a caller that times whole
// steps around the kernels keeps that out of most of them).  Toggle between launches of the profiled kernel only.
extern "C" void lg_prof_pause(int32_t paused) { g_prof.paused.store(paused ? 1 : 0); }
extern "C" int lg_prof_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.n = 0;
    g_prof.units = 0;
    return 0;
}
extern "C" int lg_prof_read(double* total_ms, int64_t* launches) {
    if (!total_ms || !launches) { lg_set_error("prof_read: null argument"); return -1; }
    std::lock_guard<std::mutex> lk(g_prof.mu);
    double tot = 0.0;
    for (int i = 0; i < g_prof.n; ++i) {
        hipError_t e = hipEventSynchronize(g_prof.ev[2 * i + 1]);
        if (e != hipSuccess) { lg_set_error("prof_read: %s", hipGetErrorString(e)); return (int)e; }
        float ms = 0.f;
        hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]);
        tot += ms;
    }
    *total_ms = tot;
    *launches = g_prof.units;
    return 0;
}
extern "C" const char* lg_kernel_name(int32_t k) {
    static const char* names[LG_K_COUNT] = {"none", "k_ffn1", "fused FFN forward (k_ffn_xr e=16 / k_ffn_x32 e=32 / k_ffn1_x64+k_ffn2_x64 e=64)", "k_fftmix", "k_attn", "k_upfuse", "k_down", "k_embed", "k_tail",
                                            "k_resample_dw", "k_ffn1_bwd", "k_ffn2_bwd", "k_fftmix_bwd", "k_attn_bwd", "k_wgrad", "k_batch_assemble", "k_scene_gather", "k_scene_blend"};
    return (k >= 0 && k < LG_K_COUNT) ? names[k] : "?";
}

extern "C" const char* lg_version(void) { return "lgteun_hip 0.2 (gfx950)"; }
extern "C" int32_t lg_abi_version(void) { return LG_ABI_VERSION; }
extern "C" const char* lg_last_error(void) { return g_err; }

static void lg_plan_stage_batch(lg_plan* p);
extern "C" int lg_plan_create(const lg_config* cfg, const int64_t* offsets, int32_t n_offsets, lg_plan** out) {
    if (!cfg || !offsets || !out) { lg_set_error("plan_create: null argument"); return -1; }
    if (cfg->C != 4 && cfg->C != 8) { lg_set_error("plan_create: C must be 4 or 8 (got %d)", cfg->C); return -2; }
    if (cfg->precision != 0 && cfg->precision != 1) { lg_set_error("plan_create: precision must be 0 (fp32) or 1 (bf16 hidden storage)"); return -2; }
    if (cfg->K < 1 || cfg->K > LG_MAX_K) { lg_set_error("plan_create: K out of range (%d)", cfg->K); return -2; }
    if (cfg->H % 16 || cfg->W % 16 || cfg->H <= 0 || cfg->W <= 0) { lg_set_error("plan_create: H,W must be positive multiples of 16"); return -2; }
    if (cfg->H > 1024 || cfg->W > 1024) {   // FFT mixer: Bluestein lines of up to 1024 points (square powers of two <= 512: radix-2 paths)
        lg_set_error("plan_create: PAN sizes up to 1024x1024 are supported (got %dx%d)", cfg->H, cfg->W);
        return -2;
    }
    const int expect = S_NSHARED + cfg->K + L_NSLOT * cfg->K;
    if (n_offsets != expect) { lg_set_error("plan_create: expected %d offsets, got %d", expect, n_offsets); return -2; }
    for (int i = 0; i < n_offsets; ++i)
        if (offsets[i] < 0 || (offsets[i] & 3)) { lg_set_error("plan_create: offset %d (=%lld) must be a non-negative multiple of 4 floats", i, (long long)offsets[i]); return -2; }
    LgRoute route;   // A/B switches come in through lg_config.variant (the library reads no environment variable)
    if (int rc = lg_resolve_route(*cfg, &route)) return rc;
    lg_plan* p = new lg_plan;
    p->cfg = *cfg;
    p->n_offsets = n_offsets;
    p->route = route;
    p->off = (int64_t*)malloc(sizeof(int64_t) * n_offsets);
    memcpy(p->off, offsets, sizeof(int64_t) * n_offsets);
    lg_plan_stage_batch(p);
    *out = p;
    return 0;
}

// Decided once per plan: can the forward kernels of its route take the samples of several stages in one launch (kernels.h: StageSel), and is there
// anything to gain (two or more dead stages)?  The parameter offsets must be affine in the stage, the FFT mixer the real-input in-LDS kernel, the
// FFN / mixer kernels the persistent ones of the C = 4 route, and no workgroup's tile may straddle two samples.  Otherwise the dead stages run one by one.
static void lg_plan_stage_batch(lg_plan* p) {
    const lg_config& c = p->cfg;
    const LgRoute& r = p->route;
    p->stage_stride = c.K > 1 ? p->lgt(1, 0) - p->lgt(0, 0) : 0;
    bool ok = c.K - 1 >= 2 && c.C == 4 && p->stage_stride > 0;
    for (int st = 1; ok && st < c.K; ++st)
        for (int slot = 0; slot < L_NSLOT; ++slot)
            if (p->lgt(st, slot) - p->lgt(0, slot) != st * p->stage_stride) { ok = false; break; }
    ok = ok && r.ffn[0].fwd[0] == FFN_FWD_XR && r.ffn[1].fwd[0] == FFN_FWD_X32 && r.mix[0].fwd == ATTN_FWD_M && r.mix[1].fwd == ATTN_FWD_M && !r.fft_full;
    ok = ok && (r.ffn[1].scales || r.ffn[1].hbf);                        // (k_ffn_x32's three-piece arithmetic has no multi-stage instance)
    ok = ok && !fft_is_generic(c.H, c.W) && c.H <= 128;                 // both levels' planes in LDS
    ok = ok && ((c.H / 16) * (c.W / 16)) % 4 == 0;                      // level 1: whole window quads per sample (k_attn_m); the pixel kernels' tiles follow
    p->stage_batch = ok;
}

extern "C" void lg_plan_destroy(lg_plan* plan) {
    if (!plan) return;
    free(plan->off);
    delete plan;
}

extern "C" int lg_plan_describe(const lg_plan* plan, char* buf, size_t n) {
    if (!plan) { lg_set_error("plan_describe: null argument"); return -1; }
    return lg_describe_route(plan->cfg, plan->route, buf, n);
}

extern "C" size_t lg_workspace_bytes(const lg_plan* plan, int32_t B, int32_t train) {
    if (!plan || B <= 0 || train < 0 || train > 2) return 0;
    NetBufs nb;
    carve(plan, B, train, nullptr, nb);
    size_t fwd = nb.bytes;
    if (train) fwd += bwd_workspace_bytes(plan, B);
    return fwd;
}

extern "C" int lg_workspace_deadout(const lg_plan* plan, int32_t B, int32_t train, size_t* offset, size_t* stage_stride) {
    if (!plan || B <= 0 || train < 0 || train > 2 || !offset || !stage_stride) { lg_set_error("workspace_deadout: invalid argument"); return -1; }
    NetBufs nb;
    char base[1];   // carve() only adds offsets to the base it is given
    carve(plan, B, train, base, nb);
    *offset = (size_t)(reinterpret_cast<char*>(nb.deadout) - base);
    *stage_stride = (plan->stage_batch && train != 2) ? (size_t)B * plan->cfg.C * plan->cfg.H * plan->cfg.W * sizeof(float) : 0;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// forward pieces
// ------------------------------------------------------------------------------------------------
static int data_step_fwd(const lg_plan* pl, const float* P, int stage, const float* z_in, const float* ms, const float* pan,
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

static int block_mixer_fwd(const Blk& k, int B, int flags, uint64_t seed, hipStream_t s, const StageSel& sg = StageSel()) {
    int rc;
    const lg_plan* pl = k.pl;
    const BlockBufs& bb = k.b;
    const MixerRoute& mr = pl->mixer(bb.e);
    FftArgs f;
    f.g = bb.g; f.o = bb.o2;
    f.amp = (flags & LG_FLAG_SAVE) ? bb.amp : nullptr;
    f.pha = (flags & LG_FLAG_SAVE) ? bb.pha : nullptr;
    f.sgn = (flags & LG_FLAG_SAVE) ? bb.sgn : nullptr;
    f.scratch = k.fft_scratch;
    f.ampw = k.p(B_AMPW); f.ampb = k.p(B_AMPB); f.phaw = k.p(B_PHAW); f.phab = k.p(B_PHAB);
    f.ch = bb.e / 2; f.planes = B * f.ch; f.n = bb.h; f.h = bb.h; f.w = bb.w; f.full = pl->route.fft_full;
    f.sg = sg;
    if ((rc = launch_fftmix(f, s))) return rc;
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

// next: the block whose mixer reads this FFN's output directly (its LN1 + planar split ride in this FFN's epilogue), or null
static int block_ffn_fwd(const Blk& k, const Blk* next, int B, int flags, hipStream_t s, const StageSel& sg = StageSel()) {
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
static int prep_stages(const lg_plan* pl, const float* P, int st0, int st1, const NetBufs& nb, hipStream_t s) {
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
// that large for a plan with stage_batch).  Never with LG_FLAG_SAVE: only dead stages run this way.
static int lgt_fwd(const lg_plan* pl, const float* P, int stage, const float* z, float* out, const NetBufs& nb, int B, int flags,
                   uint64_t seed, hipStream_t s, int nst = 1, long zstride = 0, int grid_cap = 0) {
    const lg_config& c = pl->cfg;
    const int E = 4 * c.C;
    int rc;
    StageSel sg;
    if (nst > 1) {
        if (!pl->stage_batch || (flags & LG_FLAG_SAVE)) { lg_set_error("lgt_fwd: this plan / call runs one stage per pass"); return -2; }
        sg.n = nst; sg.Bs = B; sg.pstride = pl->stage_stride; sg.zstride = zstride; sg.grid_cap = grid_cap;
        nb.stage_strides(sg);
    }
    B *= nst;   // what every kernel below sees: a plain batch
    const LgtSlots L{pl, P, nullptr, stage};
    Blk k[LG_NBLK];
    for (int j = 0; j < LG_NBLK; ++j) k[j] = nb.block(pl, P, nullptr, stage, j);
    EmbedArgs ea;
    ea.z = z; ea.x = nb.x0; ea.g = nb.blk[0].g;
    ea.dww = L.p(L_PE_DWW); ea.dwb = L.p(L_PE_DWB); ea.w = L.p(L_PE_W); ea.b = L.p(L_PE_B); ea.lng = L.p(L_PE_LNG); ea.lnb = L.p(L_PE_LNB);
    ea.n1g = k[0].p(B_LN1G); ea.n1b = k[0].p(B_LN1B);
    ea.HW = c.H * c.W; ea.total = (long)B * c.H * c.W; ea.sg = sg;
    if ((rc = launch_embed(c.C, ea, s))) return rc;
    // encoder LGB (2 blocks)
    if ((rc = block_mixer_fwd(k[0], B, flags, seed, s, sg)) || (rc = block_ffn_fwd(k[0], &k[1], B, flags, s, sg))) return rc;
    if ((rc = block_mixer_fwd(k[1], B, flags, seed, s, sg)) || (rc = block_ffn_fwd(k[1], nullptr, B, flags, s, sg))) return rc;
    // down
    DownArgs da;
    da.x = nb.blk[1].xout; da.y = nb.blk[2].xin; da.g = nb.blk[2].g;
    da.u_save = (flags & LG_FLAG_SAVE) ? nb.u_down : nullptr;
    da.w = L.p(L_DOWNW); da.b = L.p(L_DOWNB);
    da.n1g = k[2].p(B_LN1G); da.n1b = k[2].p(B_LN1B);
    da.B = B; da.H = c.H; da.W = c.W; da.sg = sg;
    if ((rc = launch_down(E, da, s))) return rc;
    // bottleneck
    if ((rc = block_mixer_fwd(k[2], B, flags, seed, s, sg)) || (rc = block_ffn_fwd(k[2], nullptr, B, flags, s, sg))) return rc;
    // up + fusion
    UpFuseArgs ua;
    ua.xb = nb.blk[2].xout; ua.skip = nb.blk[1].xout; ua.y = nb.blk[3].xin; ua.g = nb.blk[3].g;
    ua.t_save = (flags & LG_FLAG_SAVE) ? nb.t_up : nullptr;
    ua.upw = L.p(L_UPW); ua.upb = L.p(L_UPB); ua.fw = L.p(L_FUSEW); ua.fb = L.p(L_FUSEB);
    ua.n1g = k[3].p(B_LN1G); ua.n1b = k[3].p(B_LN1B);
    ua.B = B; ua.H = c.H; ua.W = c.W; ua.sg = sg;
    if ((rc = launch_upfuse(E, ua, s))) return rc;
    // decoder LGB (2 blocks)
    if ((rc = block_mixer_fwd(k[3], B, flags, seed, s, sg)) || (rc = block_ffn_fwd(k[3], &k[4], B, flags, s, sg))) return rc;
    if ((rc = block_mixer_fwd(k[4], B, flags, seed, s, sg)) || (rc = block_ffn_fwd(k[4], nullptr, B, flags, s, sg))) return rc;
    // tail
    TailArgs ta;
    ta.x = nb.blk[4].xout; ta.z = z; ta.out = out;
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

// the workspace of entry `who` carved into nb, or -3 if the caller's is too small for (plan, B, train)
static int carve_checked(const char* who, const lg_plan* plan, int B, int train, void* workspace, size_t workspace_bytes, NetBufs& nb) {
    if (workspace_bytes < lg_workspace_bytes(plan, B, train)) { lg_set_error("%s: workspace too small", who); return -3; }
    carve(plan, B, train, workspace, nb);
    return 0;
}

extern "C" int lgteun_forward(const lg_plan* plan, const float* params, const float* ms, const float* pan, float* out,
                              void* workspace, size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream) {
    if (!plan || !params || !ms || !pan || !out || !workspace || B <= 0) { lg_set_error("forward: null/invalid argument"); return -1; }
    const bool chained = (flags & LG_FLAG_CHAINED) != 0;
    const int train = (flags & LG_FLAG_SAVE) ? (chained ? 2 : 1) : 0;
    if (workspace_bytes < lg_workspace_bytes(plan, B, train)) {   // (the one entry that reports both sizes)
        lg_set_error("forward: workspace too small (%zu < %zu)", workspace_bytes, lg_workspace_bytes(plan, B, train));
        return -3;
    }
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
    if (one_pass && (rc = dead_stages(plan, params, nb, B, flags, seed, s))) return rc;
    return lgt_fwd(plan, params, c.K - 1, nb.Z[c.K], out, nb, B, flags, seed, s);
}

extern "C" int lgteun_dead_forward(const lg_plan* plan, const float* params, void* workspace, size_t workspace_bytes, int32_t B,
                                   int32_t flags, uint64_t seed, void* stream) {
    if (!plan || !params || !workspace || B <= 0) { lg_set_error("dead_forward: null/invalid argument"); return -1; }
    if ((flags & LG_FLAG_CHAINED) || !(flags & LG_FLAG_FAITHFUL)) { lg_set_error("dead_forward: only the faithful unfolding has dead stages"); return -2; }
    NetBufs nb;
    if (int rc = carve_checked("dead_forward", plan, B, (flags & LG_FLAG_SAVE) ? 1 : 0, workspace, workspace_bytes, nb)) return rc;
    if (int rc = prep_stages(plan, params, 0, plan->cfg.K - 1, nb, (hipStream_t)stream)) return rc;
    return dead_stages(plan, params, nb, B, flags, seed, (hipStream_t)stream);
}

extern "C" int lgteun_backward(const lg_plan* plan, const float* params, float* grads, const float* ms, const float* pan,
                               const float* dout, void* workspace, size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed,
                               void* stream) {
    if (!plan || !params || !grads || !ms || !pan || !dout || !workspace || B <= 0) { lg_set_error("backward: null/invalid argument"); return -1; }
    if ((flags & LG_FLAG_CHAINED) && (flags & (LG_FLAG_BWD_LGT | LG_FLAG_BWD_DATA))) {
        lg_set_error("backward: LG_FLAG_BWD_LGT / LG_FLAG_BWD_DATA do not apply to LG_FLAG_CHAINED");
        return -2;
    }
    NetBufs nb;
    if (int rc = carve_checked("backward", plan, B, (flags & LG_FLAG_CHAINED) ? 2 : 1, workspace, workspace_bytes, nb)) return rc;
    return net_backward(plan, params, grads, ms, pan, dout, nb, (char*)workspace + nb.bytes, B, flags, seed, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// per-op entry points
// ------------------------------------------------------------------------------------------------
extern "C" int lg_op_resample(const float* x, float* y, int32_t planes, int32_t hi, int32_t wi, int32_t mode, void* stream) {
    if (!x || !y || planes <= 0 || hi <= 0 || wi <= 0 || mode < 0 || mode > 2) { lg_set_error("op_resample: invalid argument"); return -1; }
    if (mode == 0 && ((hi & 1) || (wi & 1))) { lg_set_error("op_resample: x0.5 needs even sizes"); return -2; }
    return launch_resample(mode, x, y, planes, hi, wi, (hipStream_t)stream);
}

extern "C" int lg_op_data_step(const lg_plan* plan, const float* params, int32_t stage, const float* z_in, const float* ms,
                               const float* pan, float* z_out, float* tmp, int32_t B, void* stream) {
    if (!plan || !params || !z_in || !ms || !pan || !z_out || !tmp || stage < 0 || stage >= plan->cfg.K) { lg_set_error("op_data_step: invalid argument"); return -1; }
    const lg_config& c = plan->cfg;
    size_t q = (size_t)B * c.C * c.H * c.W / 4;
    return data_step_fwd(plan, params, stage, z_in, ms, pan, z_out, tmp, tmp + q, tmp + 2 * q, tmp + 3 * q, B, (hipStream_t)stream);
}

extern "C" int lg_op_lgt(const lg_plan* plan, const float* params, int32_t stage, const float* z, float* out, void* workspace,
                         size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream) {
    if (!plan || !params || !z || !out || !workspace || stage < 0 || stage >= plan->cfg.K) { lg_set_error("op_lgt: invalid argument"); return -1; }
    NetBufs nb;
    if (int rc = carve_checked("op_lgt", plan, B, (flags & LG_FLAG_SAVE) ? 1 : 0, workspace, workspace_bytes, nb)) return rc;
    if (int rc = prep_stages(plan, params, stage, stage + 1, nb, (hipStream_t)stream)) return rc;
    return lgt_fwd(plan, params, stage, z, out, nb, B, flags, seed, (hipStream_t)stream);
}

extern "C" int lg_op_lgt_stages(const lg_plan* plan, const float* params, int32_t stage0, int32_t n, const float* z, float* out, void* workspace,
                                size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, int32_t grid_cap, void* stream) {
    if (!plan || !params || !z || !out || !workspace || B <= 0 || stage0 < 0 || n < 1 || stage0 + n > plan->cfg.K || grid_cap < 0) { lg_set_error("op_lgt_stages: invalid argument"); return -1; }
    if (flags & ~LG_FLAG_DROPOUT) { lg_set_error("op_lgt_stages: only LG_FLAG_DROPOUT applies (nothing is saved)"); return -2; }
    if (n > 1 && (!plan->stage_batch || n > plan->cfg.K - 1)) { lg_set_error("op_lgt_stages: this plan runs one stage per pass (lg_plan_stage_batch), or n > K-1"); return -2; }
    NetBufs nb;
    if (int rc = carve_checked("op_lgt_stages", plan, B, 0, workspace, workspace_bytes, nb)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = prep_stages(plan, params, stage0, stage0 + n, nb, s)) return rc;
    return lgt_fwd(plan, params, stage0, z, out, nb, B, flags, seed, s, n, (long)B * plan->cfg.C * plan->cfg.H * plan->cfg.W, grid_cap);
}

// debug exports (tests/test_stage_runs_cpu.py; host only, no device, no launch): the partition of a persistent multi-stage launch, from the functions
// the kernels call (kernels.h: stage_run_*), and the launchers' decision for a shape
extern "C" int lg_debug_stage_runs(int32_t kind, int32_t units, int32_t per_stage, int32_t grid, int32_t split, int32_t* out, int32_t n_out) {
    if (kind < 0 || kind > 1 || units <= 0 || per_stage <= 0 || units % per_stage || grid <= 0 || !out || n_out < 0 || (int64_t)units * grid >= (1ll << 31)) {
        lg_set_error("debug_stage_runs: invalid argument");
        return -1;
    }
    const bool uneven = kind == 0 ? split != 0 : split != 4;
    if (!uneven && grid > units) { lg_set_error("debug_stage_runs: more workgroups than units"); return -1; }
    // (what the launchers guarantee: a pair of strips per pair of workgroups, two quads per CU)
    if (uneven && ((grid & 1) || (kind == 0 ? 2 * units < grid : units < grid) || (kind == 1 && (split < 1 || split > 7)))) { lg_set_error("debug_stage_runs: an uneven split needs an even grid, a unit per workgroup and 1 <= eighths <= 7"); return -2; }
    int rows = 0;
    for (int wg = 0; wg < grid; ++wg) {
        const StageRun r = !uneven ? stage_run_even(units, grid, wg) : (kind == 0 ? stage_run_pairs(units, grid, wg) : stage_run_chunk(units, grid, wg, split));
        int seg0 = r.run0;
        do {   // the kernels' segment loop
            const int st = seg0 / per_stage, seg1 = stage_seg_end(st, r.run1, per_stage);
            if (rows < n_out) { int32_t* o = out + 5 * (size_t)rows; o[0] = wg; o[1] = seg0; o[2] = seg1; o[3] = st; o[4] = r.base; }
            ++rows;
            seg0 = seg1;
        } while (seg0 < r.run1);
    }
    return rows;
}

extern "C" int lg_debug_stage_decision(int32_t kind, int32_t h, int32_t w, int32_t Bs, int32_t n, int32_t grid_cap, int32_t* out8) {
    if ((kind != 0 && kind != 8 && kind != 16) || h <= 0 || w <= 0 || Bs <= 0 || n < 1 || grid_cap < 0 || !out8 || (int64_t)Bs * n * h * w >= (1ll << 31)) { lg_set_error("debug_stage_decision: invalid argument"); return -1; }
    if (kind == 0) {
        const XrGeo q = ffn_xr_geometry(h, w, Bs * n, Bs, n, grid_cap);
        const int sh = q.dS ? 1 : 0;
        const int32_t o[8] = {q.dS != 0, q.dS, q.nstrips >> sh, (Bs * q.tiles_x * q.strips_y) >> sh, q.grid, q.SH, q.tiles_x, q.strips_y};
        memcpy(out8, o, sizeof(o));
    } else {
        if ((h & 7) || (w & 7) || (Bs * (h / 8) * (w / 8)) % 4) { lg_set_error("debug_stage_decision: not whole window quads per stage"); return -2; }
        const AttnMGeo q = attn_m_geometry(kind, h, w, Bs * n, n, grid_cap, 2);   // two resident workgroups per CU: what the runtime reports for HC <= 16
        const int32_t o[8] = {q.uneven != 0, q.uneven ? q.uneven : 4, q.nquads, q.nquads / n, q.grid, q.nwin, 0, 0};
        memcpy(out8, o, sizeof(o));
    }
    return 0;
}

extern "C" int lg_op_block(const lg_plan* plan, const float* params, int32_t stage, int32_t blk, int32_t which, const float* x,
                           float* y, void* workspace, size_t workspace_bytes, int32_t B, void* stream) {
    if (!plan || !params || !x || !y || !workspace || stage < 0 || stage >= plan->cfg.K || blk < 0 || blk > 4 || which < 0 || which > 2) {
        lg_set_error("op_block: invalid argument");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    NetBufs nb;
    int rc;
    if ((rc = carve_checked("op_block", plan, B, 0, workspace, workspace_bytes, nb))) return rc;
    Blk k = nb.block(plan, params, nullptr, stage, blk);
    BlockBufs& bb = k.b;
    if (which == 0 || which == 1) {
        // LN1 + planar split of the global half (normally emitted by the producing kernel's epilogue)
        if ((rc = launch_ln_split(bb.e, x, k.p(B_LN1G), k.p(B_LN1B), bb.g, B, bb.h * bb.w, s))) return rc;
    }
    if (which == 0) {
        FftArgs f;
        f.g = bb.g; f.o = y; f.amp = nullptr; f.pha = nullptr; f.sgn = nullptr; f.scratch = nb.fft_scratch;
        f.ampw = k.p(B_AMPW); f.ampb = k.p(B_AMPB); f.phaw = k.p(B_PHAW); f.phab = k.p(B_PHAB);
        f.ch = bb.e / 2; f.planes = B * f.ch; f.n = bb.h; f.h = bb.h; f.w = bb.w; f.full = plan->route.fft_full;
        return launch_fftmix(f, s);
    }
    if ((rc = prep_stages(plan, params, stage, stage + 1, nb, s))) return rc;   // the block's rows: pos_emb table and static operand scales (mixer), operand scales and weight fragments (FFN)
    if (which == 1) {
        bb.xin = const_cast<float*>(x);
        bb.xmid = y;
        return block_mixer_fwd(k, B, 0, 0, s);
    }
    bb.xmid = const_cast<float*>(x);
    bb.xout = y;
    return block_ffn_fwd(k, nullptr, B, 0, s);
}

extern "C" int lg_op_block_bwd(const lg_plan* plan, const float* params, float* grads, int32_t stage, int32_t blk, int32_t which,
                               const float* x, const float* dy, float* dx, void* workspace, size_t workspace_bytes, int32_t B,
                               void* stream) {
    if (!plan || !params || !grads || !x || !dy || !dx || !workspace || stage < 0 || stage >= plan->cfg.K || blk < 0 || blk > 4 ||
        which < 0 || which > 2) {
        lg_set_error("op_block_bwd: invalid argument");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    NetBufs nb;
    int rc;
    if ((rc = carve_checked("op_block_bwd", plan, B, 1, workspace, workspace_bytes, nb))) return rc;
    Blk k = nb.block(plan, params, grads, stage, blk);
    BlockBufs& bb = k.b;
    // forward of the half-block with everything saved
    if (which == 0 || which == 1) {
        if ((rc = launch_ln_split(bb.e, x, k.p(B_LN1G), k.p(B_LN1B), bb.g, B, bb.h * bb.w, s))) return rc;
        if ((rc = prep_stages(plan, params, stage, stage + 1, nb, s))) return rc;   // the mixer's pos_emb table and static operand scales
        bb.xin = const_cast<float*>(x);
        if ((rc = block_mixer_fwd(k, B, LG_FLAG_SAVE, 0, s))) return rc;
    } else {
        bb.xmid = const_cast<float*>(x);
        if ((rc = prep_stages(plan, params, stage, stage + 1, nb, s))) return rc;
        if ((rc = block_ffn_fwd(k, nullptr, B, LG_FLAG_SAVE, s))) return rc;
    }
    return op_block_bwd(k, which, dy, dx, (char*)workspace + nb.bytes, B, s);
}

extern "C" int lg_op_data_step_bwd(const lg_plan* plan, const float* params, float* grads, int32_t stage, const float* z_in,
                                   const float* ms, const float* pan, const float* dz_out, float* dz_in, void* workspace,
                                   size_t workspace_bytes, int32_t B, void* stream) {
    if (!plan || !params || !grads || !z_in || !ms || !pan || !dz_out || !dz_in || !workspace || B <= 0 || stage < 0 || stage >= plan->cfg.K) {
        lg_set_error("op_data_step_bwd: invalid argument");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    NetBufs nb;
    int rc;
    if ((rc = carve_checked("op_data_step_bwd", plan, B, 1, workspace, workspace_bytes, nb))) return rc;
    // forward of the step: fills the intermediates its backward reads (t1, r, s1)
    if ((rc = data_step_fwd(plan, params, stage, z_in, ms, pan, nb.Z[stage + 1], nb.t1[stage], nb.r[stage], nb.s1[stage], nb.pr, B, s))) return rc;
    return op_data_step_bwd(plan, params, grads, stage, nb, (char*)workspace + nb.bytes, z_in, pan, dz_out, dz_in, B, s);
}

extern "C" int lg_op_lgt_bwd(const lg_plan* plan, const float* params, float* grads, int32_t stage, const float* z, const float* dout,
                             float* dz, void* workspace, size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream) {
    if (!plan || !params || !grads || !z || !dout || !dz || !workspace || B <= 0 || stage < 0 || stage >= plan->cfg.K) {
        lg_set_error("op_lgt_bwd: invalid argument");
        return -1;
    }
    if (flags & ~LG_FLAG_DROPOUT) { lg_set_error("op_lgt_bwd: only LG_FLAG_DROPOUT applies"); return -2; }
    hipStream_t s = (hipStream_t)stream;
    NetBufs nb;
    int rc;
    if ((rc = carve_checked("op_lgt_bwd", plan, B, 1, workspace, workspace_bytes, nb))) return rc;
    if ((rc = prep_stages(plan, params, stage, stage + 1, nb, s))) return rc;
    if ((rc = lgt_fwd(plan, params, stage, z, nb.deadout, nb, B, flags | LG_FLAG_SAVE, seed, s))) return rc;
    return op_lgt_bwd(plan, params, grads, stage, nb, (char*)workspace + nb.bytes, z, dout, dz, B, flags, seed, s);
}

// ------------------------------------------------------------------------------------------------
// the train-mode dropout mask, exported for the fp64 oracle
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dropout_mask(uint64_t seed, long first, long n, float* __restrict__ out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) out[i] = dropout_scale(seed, (uint64_t)(first + i));
}
extern "C" int lg_dropout_mask(uint64_t seed, int32_t stage, int32_t blk, int64_t first, int64_t n, float* out, void* stream) {
    if (!out || n < 0 || first < 0 || stage < 0 || stage >= LG_MAX_K || blk < 0 || blk > 4) { lg_set_error("dropout_mask: invalid argument"); return -1; }
    if (n == 0) return 0;
    const int grid = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    k_dropout_mask<<<grid, 256, 0, (hipStream_t)stream>>>(mix_seed(seed, stage, blk), first, n, out);
    LG_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// l1 / l2 training losses (k_recloss.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int lg_l1_loss(const float* out, const float* gt, float* dout, float* loss_accum, int64_t n_local, int64_t n_global,
                          float scale, void* stream) {
    return launch_l1_loss(out, gt, dout, loss_accum, n_local, n_global, scale, (hipStream_t)stream);
}
extern "C" int lg_l2_loss(const float* out, const float* gt, float* dout, float* loss_accum, int64_t n_local, int64_t n_global,
                          float scale, void* stream) {
    return launch_l2_loss(out, gt, dout, loss_accum, n_local, n_global, scale, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// device-resident dataset (k_batch.hip), Wald degradation (k_wald.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int lg_pyr_down2(const void* pan, float* pan_l, int64_t planes, int32_t H, int32_t W, int32_t dtype, void* stream) {
    return launch_pyr_down2(pan, pan_l, planes, H, W, dtype, (hipStream_t)stream);
}
extern "C" int lg_batch_assemble(const void* pan, const void* lr, const void* mul, const float* pan_l, int64_t N, const int32_t* idx, int64_t idx_offset,
                                 const uint32_t* flips, float* o_pan, float* o_lr, float* o_mul, float* o_pan_l, int32_t B, int32_t C, int32_t H, int32_t W,
                                 int32_t h, int32_t w, int32_t dtype, float divisor, int32_t n_div, float post_scale, void* stream) {
    return launch_batch_assemble(pan, lr, mul, pan_l, N, idx, idx_offset, flips, o_pan, o_lr, o_mul, o_pan_l, B, C, H, W, h, w, dtype, divisor, n_div,
                                 post_scale, (hipStream_t)stream);
}
extern "C" int lg_fir_decimate4(const void* in, void* out, const double* taps, int64_t planes, int32_t H, int32_t W, int32_t n_taps, int32_t phase,
                                int32_t dtype, int32_t out_f32, void* stream) {
    return launch_fir_decimate4(in, out, taps, planes, H, W, n_taps, phase, dtype, out_f32, (hipStream_t)stream);
}
extern "C" int lg_window_assemble(const void* pan, const void* lr, const void* mul, const int32_t* origins, int64_t n_windows, int64_t first,
                                  const uint32_t* flips, float* o_pan, float* o_lr, float* o_mul, float* o_pan_l, int32_t B, int32_t C, int32_t Hs,
                                  int32_t Ws, int32_t P, int32_t Q, int32_t dtype, float divisor, int32_t n_div, float post_scale, void* stream) {
    return launch_window_assemble(pan, lr, mul, origins, n_windows, first, flips, o_pan, o_lr, o_mul, o_pan_l, B, C, Hs, Ws, P, Q, dtype, divisor,
                                  n_div, post_scale, (hipStream_t)stream);
}
extern "C" int lg_scene_gather(const void* pan, const void* ms, const int32_t* origins, int64_t n_tiles, int64_t first, float* o_pan, float* o_ms,
                               int32_t B, int32_t C, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t dtype, float divisor, int32_t n_div,
                               float post_scale, void* stream) {
    return launch_scene_gather(pan, ms, origins, n_tiles, first, o_pan, o_ms, B, C, H, W, th, tw, dtype, divisor, n_div, post_scale, (hipStream_t)stream);
}
extern "C" int lg_scene_blend(const float* tiles, float* scene, int64_t first, int32_t B, int32_t C, int32_t H, int32_t W, int32_t th, int32_t tw,
                              int32_t overlap, void* stream) {
    return launch_scene_blend(tiles, scene, first, B, C, H, W, th, tw, overlap, (hipStream_t)stream);
}
extern "C" int lg_scene_to_u16(const float* src, uint16_t* dst, int64_t n, float scale, void* stream) {
    return launch_scene_to_u16(src, dst, n, scale, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// evaluation indices (k_iqa.hip)
// ------------------------------------------------------------------------------------------------
extern "C" size_t lg_iqa_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t no_ref) {
    return iqa_workspace_bytes(B, C, H, W, no_ref);
}
extern "C" int lg_iqa_ref(const float* pred, const float* gt, double* out, int32_t B, int32_t C, int32_t H, int32_t W, float scale,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return launch_iqa_ref(pred, gt, out, B, C, H, W, scale, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int lg_iqa_no_ref(const float* pred, const float* pan, const float* ms, double* out, int32_t B, int32_t C, int32_t H, int32_t W,
                             float scale, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_iqa_no_ref(pred, pan, ms, out, B, C, H, W, scale, workspace, workspace_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam single-tensor semantics) over ranges of the flat buffers
// ------------------------------------------------------------------------------------------------
// The controls of a train step (lg_optim_step_ex), compile-time like the option sets: CTL_CLIP reads the gradient as
// fl(fl(g * grad_scale) * *clip) -- the coefficient is loaded once per thread, from DEVICE memory -- and CTL_EMA updates an average of the
// weights behind the parameter update, ema = fma(w, p_new - ema, ema) (torch._foreach_lerp_ for a weight below 0.5).  CTL = 0 is the kernel
// lg_adam_step / lg_optim_step launch: nothing of the controls is in it.
enum { CTL_CLIP = 1, CTL_EMA = 2 };
struct ctl_args {
    const float* clip;   // CTL_CLIP: the clip coefficient, out + 1 of lg_grad_norm
    float* ema;          // CTL_EMA: laid out like params
    float w;             // CTL_EMA: 1 - decay, taken in fp64 and rounded once
};

template <int CTL>
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, const int64_t* __restrict__ ranges, float step_size, float b1,
                                              float b2, float inv_bc2_sqrt, float eps, float gscale, ctl_args c) {
    const int64_t lo = ranges[2 * blockIdx.y], hi = ranges[2 * blockIdx.y + 1];
    float coef = 1.0f;
    if constexpr ((CTL & CTL_CLIP) != 0) coef = *c.clip;
    for (int64_t i = lo + blockIdx.x * 256L + threadIdx.x; i < hi; i += (int64_t)gridDim.x * 256L) {
        float gi = g[i] * gscale;
        if constexpr ((CTL & CTL_CLIP) != 0) gi = gi * coef;
        float mi = b1 * m[i] + (1.0f - b1) * gi;
        float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
        const float pn = p[i] - step_size * (mi / denom);
        p[i] = pn;
        if constexpr ((CTL & CTL_EMA) != 0) {
            const float e = c.ema[i];
            c.ema[i] = __builtin_fmaf(c.w, pn - e, e);
        }
    }
}

// lg_adam_step, and the plain-Adam route of lg_optim_step_ex: the same scalars, rounded at the same places
static int launch_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* ranges, int32_t n_ranges,
                       int64_t max_range, int32_t step, float lr, float beta1, float beta2, float eps, float grad_scale, const ctl_args& c,
                       hipStream_t st) {
    double bc1 = 1.0 - pow((double)beta1, (double)step);
    double bc2 = 1.0 - pow((double)beta2, (double)step);
    int gx = (int)((max_range + 255) / 256);
    if (gx < 1) gx = 1;
    if (gx > 512) gx = 512;
    dim3 grid(gx, n_ranges);
    const float step_size = (float)(lr / bc1), inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
#define LG_ADAM_GO(CTL) k_adam<CTL><<<grid, 256, 0, st>>>(params, grads, exp_avg, exp_avg_sq, ranges, step_size, beta1, beta2, inv_bc2_sqrt, eps, grad_scale, c)
    switch ((c.clip ? CTL_CLIP : 0) | (c.ema ? CTL_EMA : 0)) {
        case 0: LG_ADAM_GO(0); break;
        case CTL_CLIP: LG_ADAM_GO(CTL_CLIP); break;
        case CTL_EMA: LG_ADAM_GO(CTL_EMA); break;
        default: LG_ADAM_GO(CTL_CLIP | CTL_EMA); break;
    }
#undef LG_ADAM_GO
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* ranges,
                            int32_t n_ranges, int64_t max_range, int32_t step, float lr, float beta1, float beta2, float eps,
                            float grad_scale, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !ranges || n_ranges <= 0 || step < 1) { lg_set_error("adam_step: invalid argument"); return -1; }
    return launch_adam(params, grads, exp_avg, exp_avg_sq, ranges, n_ranges, max_range, step, lr, beta1, beta2, eps, grad_scale,
                       ctl_args{nullptr, nullptr, 0.f}, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// torch.optim single-tensor steps (Adam / AdamW / SGD / RMSprop with their options) over ranges of the flat buffers
// (base_model.py:116-135 passes torch's keyword arguments through).  One instance per option set: ALGO and the bits of OPT are
// compile-time, so no element branches on an option.  The operation order is torch's (_single_tensor_adam / _sgd / _rmsprop).
// ------------------------------------------------------------------------------------------------
enum { OPT_WD = 1, OPT_ALT = 2, OPT_MOM = 4, OPT_FIRST = 8 };   // ALT: amsgrad (Adam, AdamW) / nesterov (SGD) / centered (RMSprop)
struct optim_args {
    float lr;          // Adam, AdamW: lr / (1 - beta1^step)
    float h0, h1;      // Adam, AdamW: beta1, beta2; SGD: momentum, dampening; RMSprop: alpha, momentum
    float c0, c1;      // 1 - h0, 1 - h1: taken in fp64 and rounded once, like torch's Python-side `1 - beta`
    float eps, wd, gscale;
    float bc2_sqrt;    // Adam, AdamW: sqrt(1 - beta2^step)
    float decay;       // AdamW: 1 - lr * weight_decay
};

// Rounding: every torch op of the multi-tensor (foreach) form the device route runs is one rounding step here -- `a * s`, `b * c`,
// `b / c`, sqrt are rounded on their own, `a + s * x` (add with alpha, addcmul, addcdiv, lerp) is one fused multiply-add as the
// compiler contracts it in torch's kernels -- so that a run fed the same gradients lands on the same bits as `fused=False`.
// Contraction is switched off for the kernel and every fma is written out.
#ifndef LG_OPT_FMA
#define LG_OPT_FMA(a, b, c) __builtin_fmaf(a, b, c)
#endif
template <int ALGO, int OPT, int CTL>
__global__ __launch_bounds__(256) void k_optim(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                               float* __restrict__ s1, float* __restrict__ s2, const int64_t* __restrict__ ranges,
                                               optim_args a, ctl_args c) {
#pragma clang fp contract(off)
    const int64_t lo = ranges[2 * blockIdx.y], hi = ranges[2 * blockIdx.y + 1];
    float coef = 1.0f;
    if constexpr ((CTL & CTL_CLIP) != 0) coef = *c.clip;
    for (int64_t i = lo + blockIdx.x * 256L + threadIdx.x; i < hi; i += (int64_t)gridDim.x * 256L) {
        float pi = p[i];
        float gi = g[i] * a.gscale;
        if constexpr ((CTL & CTL_CLIP) != 0) gi = gi * coef;                         // g.mul_(clip_coef) of clip_grad_norm_: one more rounding
        if constexpr (ALGO == LG_OPT_ADAMW) pi = pi * a.decay;                       // _foreach_mul_(params, 1 - lr * weight_decay)
        else if constexpr ((OPT & OPT_WD) != 0) gi = LG_OPT_FMA(a.wd, pi, gi);       // _foreach_add(grads, params, alpha=weight_decay)
        if constexpr (ALGO == LG_OPT_ADAM || ALGO == LG_OPT_ADAMW) {
            float mi = s0[i];
            mi = LG_OPT_FMA(a.c0, gi - mi, mi);                                      // _foreach_lerp_(exp_avgs, grads, 1 - beta1)
            const float vb = s1[i] * a.h1;                                           // _foreach_mul_(exp_avg_sqs, beta2)
            float vi = LG_OPT_FMA(a.c1, gi * gi, vb);                                // _foreach_addcmul_(exp_avg_sqs, grads, grads, 1 - beta2)
            s0[i] = mi;
            s1[i] = vi;
            if constexpr ((OPT & OPT_ALT) != 0) { vi = fmaxf(s2[i], vi); s2[i] = vi; }
            float denom = sqrtf(vi) / a.bc2_sqrt;
            denom = denom + a.eps;
            pi = LG_OPT_FMA(-a.lr, mi / denom, pi);                                  // _foreach_addcdiv_(params, exp_avgs, denom, -step_size)
        } else if constexpr (ALGO == LG_OPT_SGD) {
            if constexpr ((OPT & OPT_MOM) != 0) {
                float bi;
                if constexpr ((OPT & OPT_FIRST) != 0) bi = gi;                       // torch: the first buffer is a clone of the gradient
                else bi = LG_OPT_FMA(a.c1, gi, s0[i] * a.h0);                        // _foreach_mul_(bufs, momentum); _foreach_add_(bufs, grads, alpha=1 - dampening)
                s0[i] = bi;
                if constexpr ((OPT & OPT_ALT) != 0) gi = LG_OPT_FMA(a.h0, bi, gi);   // _foreach_add_(grads, bufs, alpha=momentum)
                else gi = bi;
            }
            pi = LG_OPT_FMA(-a.lr, gi, pi);                                          // _foreach_add_(params, grads, alpha=-lr)
        } else {
            const float vb = s0[i] * a.h0;                                           // _foreach_mul_(square_avgs, alpha)
            const float vi = LG_OPT_FMA(a.c0, gi * gi, vb);                          // _foreach_addcmul_(square_avgs, grads, grads, value=1 - alpha)
            s0[i] = vi;
            float avg;
            if constexpr ((OPT & OPT_ALT) != 0) {
                float ci = s2[i];
                ci = LG_OPT_FMA(a.c0, gi - ci, ci);                                  // _foreach_lerp_(grad_avgs, grads, 1 - alpha)
                s2[i] = ci;
                avg = sqrtf(LG_OPT_FMA(-1.0f, ci * ci, vi));                         // _foreach_addcmul(square_avgs, grad_avgs, grad_avgs, value=-1), sqrt
            } else {
                avg = sqrtf(vi);
            }
            avg = avg + a.eps;
            if constexpr ((OPT & OPT_MOM) != 0) {
                const float bi = LG_OPT_FMA(1.0f, gi / avg, s1[i] * a.h1);           // _foreach_mul_(bufs, momentum); _foreach_addcdiv_(bufs, grads, avg)
                s1[i] = bi;
                pi = LG_OPT_FMA(-a.lr, bi, pi);                                      // _foreach_add_(params, bufs, alpha=-lr)
            } else {
                pi = LG_OPT_FMA(-a.lr, gi / avg, pi);                                // _foreach_addcdiv_(params, grads, avg, value=-lr)
            }
        }
        p[i] = pi;
        if constexpr ((CTL & CTL_EMA) != 0) {
            const float e = c.ema[i];
            c.ema[i] = LG_OPT_FMA(c.w, pi - e, e);                                   // _foreach_lerp_(ema, params, 1 - decay)
        }
    }
}

template <int ALGO, int OPT>
static void launch_optim(dim3 grid, hipStream_t st, float* p, const float* g, float* s0, float* s1, float* s2, const int64_t* ranges,
                         const optim_args& a, const ctl_args& c) {
    switch ((c.clip ? CTL_CLIP : 0) | (c.ema ? CTL_EMA : 0)) {
        case 0: k_optim<ALGO, OPT, 0><<<grid, 256, 0, st>>>(p, g, s0, s1, s2, ranges, a, c); break;
        case CTL_CLIP: k_optim<ALGO, OPT, CTL_CLIP><<<grid, 256, 0, st>>>(p, g, s0, s1, s2, ranges, a, c); break;
        case CTL_EMA: k_optim<ALGO, OPT, CTL_EMA><<<grid, 256, 0, st>>>(p, g, s0, s1, s2, ranges, a, c); break;
        default: k_optim<ALGO, OPT, CTL_CLIP | CTL_EMA><<<grid, 256, 0, st>>>(p, g, s0, s1, s2, ranges, a, c); break;
    }
}

static int optim_step(float* params, const float* grads, float* state0, float* state1, float* state2, const int64_t* ranges,
                      int32_t n_ranges, int64_t max_range, int32_t step, int32_t algo, int32_t flags, double lr, double h0, double h1,
                      double eps, double weight_decay, double grad_scale, const ctl_args& c, void* stream) {
    if (!params || !grads || !ranges || n_ranges <= 0 || step < 1 || algo < LG_OPT_ADAM || algo > LG_OPT_RMSPROP ||
        (flags & ~(LG_OPT_AMSGRAD | LG_OPT_NESTEROV | LG_OPT_CENTERED))) { lg_set_error("optim_step: invalid argument"); return -1; }
    const bool adam = algo == LG_OPT_ADAM || algo == LG_OPT_ADAMW;
    const int own = adam ? LG_OPT_AMSGRAD : (algo == LG_OPT_SGD ? LG_OPT_NESTEROV : LG_OPT_CENTERED);
    if (flags & ~own) { lg_set_error("optim_step: the flag belongs to another algorithm"); return -1; }
    int opt = (weight_decay != 0.0 && algo != LG_OPT_ADAMW ? OPT_WD : 0) | (flags ? OPT_ALT : 0);
    if (algo == LG_OPT_SGD && h0 != 0.0) opt |= OPT_MOM | (step == 1 ? OPT_FIRST : 0);
    if (algo == LG_OPT_RMSPROP && h1 > 0.0) opt |= OPT_MOM;
    if (algo == LG_OPT_SGD && (opt & OPT_ALT) && !(opt & OPT_MOM)) { lg_set_error("optim_step: nesterov needs a momentum"); return -1; }
    // the state buffers this option set reads and writes
    const bool need0 = algo != LG_OPT_SGD || (opt & OPT_MOM), need1 = adam || (algo == LG_OPT_RMSPROP && (opt & OPT_MOM));
    const bool need2 = algo != LG_OPT_SGD && (opt & OPT_ALT);
    if ((need0 && !state0) || (need1 && !state1) || (need2 && !state2)) { lg_set_error("optim_step: a state buffer of this option set is missing"); return -1; }
    // the scalars are torch's Python floats: every derived one is taken in fp64 and rounded to fp32 once, where torch hands it to a tensor op
    optim_args a = {(float)lr, (float)h0, (float)h1, (float)(1.0 - h0), (float)(1.0 - h1), (float)eps, (float)weight_decay, (float)grad_scale,
                    1.f, 1.f};
    if (adam) {
        a.lr = (float)(lr / (1.0 - pow(h0, (double)step)));
        a.bc2_sqrt = (float)sqrt(1.0 - pow(h1, (double)step));
        a.decay = (float)(1.0 - lr * weight_decay);
    }
    int gx = (int)((max_range + 255) / 256);
    if (gx < 1) gx = 1;
    if (gx > 512) gx = 512;
    const dim3 grid(gx, n_ranges);
    const hipStream_t st = (hipStream_t)stream;
#define LG_OPT_CASE(A, O) case (A) * 16 + (O): launch_optim<A, O>(grid, st, params, grads, state0, state1, state2, ranges, a, c); break;
    switch (algo * 16 + opt) {
        LG_OPT_CASE(LG_OPT_ADAM, 0) LG_OPT_CASE(LG_OPT_ADAM, OPT_WD) LG_OPT_CASE(LG_OPT_ADAM, OPT_ALT) LG_OPT_CASE(LG_OPT_ADAM, OPT_WD | OPT_ALT)
        LG_OPT_CASE(LG_OPT_ADAMW, 0) LG_OPT_CASE(LG_OPT_ADAMW, OPT_ALT)
        LG_OPT_CASE(LG_OPT_SGD, 0) LG_OPT_CASE(LG_OPT_SGD, OPT_WD)
        LG_OPT_CASE(LG_OPT_SGD, OPT_MOM) LG_OPT_CASE(LG_OPT_SGD, OPT_MOM | OPT_WD)
        LG_OPT_CASE(LG_OPT_SGD, OPT_MOM | OPT_FIRST) LG_OPT_CASE(LG_OPT_SGD, OPT_MOM | OPT_FIRST | OPT_WD)
        LG_OPT_CASE(LG_OPT_SGD, OPT_MOM | OPT_ALT) LG_OPT_CASE(LG_OPT_SGD, OPT_MOM | OPT_ALT | OPT_WD)
        LG_OPT_CASE(LG_OPT_SGD, OPT_MOM | OPT_ALT | OPT_FIRST) LG_OPT_CASE(LG_OPT_SGD, OPT_MOM | OPT_ALT | OPT_FIRST | OPT_WD)
        LG_OPT_CASE(LG_OPT_RMSPROP, 0) LG_OPT_CASE(LG_OPT_RMSPROP, OPT_WD) LG_OPT_CASE(LG_OPT_RMSPROP, OPT_ALT) LG_OPT_CASE(LG_OPT_RMSPROP, OPT_ALT | OPT_WD)
        LG_OPT_CASE(LG_OPT_RMSPROP, OPT_MOM) LG_OPT_CASE(LG_OPT_RMSPROP, OPT_MOM | OPT_WD)
        LG_OPT_CASE(LG_OPT_RMSPROP, OPT_MOM | OPT_ALT) LG_OPT_CASE(LG_OPT_RMSPROP, OPT_MOM | OPT_ALT | OPT_WD)
        default: lg_set_error("optim_step: no kernel for this option set"); return -1;
    }
#undef LG_OPT_CASE
    LG_CHECK_LAUNCH();
    return 0;
}

extern "C" int lg_optim_step(float* params, const float* grads, float* state0, float* state1, float* state2, const int64_t* ranges,
                             int32_t n_ranges, int64_t max_range, int32_t step, int32_t algo, int32_t flags, double lr, double h0, double h1,
                             double eps, double weight_decay, double grad_scale, void* stream) {
    return optim_step(params, grads, state0, state1, state2, ranges, n_ranges, max_range, step, algo, flags, lr, h0, h1, eps, weight_decay,
                      grad_scale, ctl_args{nullptr, nullptr, 0.f}, stream);
}

// ------------------------------------------------------------------------------------------------
// the controls of a train step: gradient norm + clip coefficient (k_gradnorm.hip), clipped / averaging optimizer step
// ------------------------------------------------------------------------------------------------
extern "C" size_t lg_qnr_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) { return qnr_workspace_bytes(B, C, H, W); }
extern "C" int lg_qnr_stats(const float* out, const float* pan, const float* ms, const float* pan_l, double* q, double* table, int32_t B,
                            int32_t C, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_qnr_stats(out, pan, ms, pan_l, q, table, B, C, H, W, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int lg_qnr_grad(const float* out, const float* pan, const double* table, float* dout, float* loss_accum, double* indices, int32_t B,
                           int64_t B_global, int32_t C, int32_t H, int32_t W, float scale, int32_t accumulate, const void* workspace,
                           size_t workspace_bytes, void* stream) {
    return launch_qnr_grad(out, pan, table, dout, loss_accum, indices, B, B_global, C, H, W, scale, accumulate, workspace, workspace_bytes,
                           (hipStream_t)stream);
}
extern "C" size_t lg_recloss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) { return recloss_workspace_bytes(B, C, H, W); }
extern "C" int lg_sam_loss(const float* out, const float* gt, float* dout, float* loss_accum, int32_t B, int64_t B_global, int32_t C, int32_t H,
                           int32_t W, float scale, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_sam_loss(out, gt, dout, loss_accum, B, B_global, C, H, W, scale, accumulate, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int lg_ssim_loss(const float* out, const float* gt, float* dout, float* loss_accum, int32_t B, int64_t B_global, int32_t C, int32_t H,
                            int32_t W, float scale, float data_range, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_ssim_loss(out, gt, dout, loss_accum, B, B_global, C, H, W, scale, data_range, accumulate, workspace, workspace_bytes,
                            (hipStream_t)stream);
}
extern "C" size_t lg_grad_norm_workspace_bytes(int32_t n_ranges, int64_t max_range) { return grad_norm_workspace_bytes(n_ranges, max_range); }
extern "C" int lg_grad_norm(const float* grads, const int64_t* ranges, int32_t n_ranges, int64_t max_range, double max_norm, float* out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    return launch_grad_norm(grads, ranges, n_ranges, max_range, max_norm, out, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lg_optim_step_ex(float* params, const float* grads, float* state0, float* state1, float* state2, const int64_t* ranges,
                                int32_t n_ranges, int64_t max_range, int32_t step, int32_t algo, int32_t flags, double lr, double h0,
                                double h1, double eps, double weight_decay, double grad_scale, const float* clip_coef, float* ema,
                                double ema_decay, int32_t plain_adam, void* stream) {
    if (ema && !(ema_decay > 0.5 && ema_decay < 1.0)) { lg_set_error("optim_step_ex: ema_decay must lie in (0.5, 1) when ema is given"); return -1; }
    if (((uintptr_t)clip_coef | (uintptr_t)ema) & 3) { lg_set_error("optim_step_ex: clip_coef and ema must be 4-byte aligned"); return -1; }
    if (plain_adam != 0 && plain_adam != 1) { lg_set_error("optim_step_ex: plain_adam must be 0 or 1"); return -1; }
    const ctl_args c = {clip_coef, ema, ema ? (float)(1.0 - ema_decay) : 0.f};
    if (!plain_adam)
        return optim_step(params, grads, state0, state1, state2, ranges, n_ranges, max_range, step, algo, flags, lr, h0, h1, eps, weight_decay,
                          grad_scale, c, stream);
    if (algo != LG_OPT_ADAM || flags != 0 || weight_decay != 0.0) {
        lg_set_error("optim_step_ex: plain_adam is algo LG_OPT_ADAM without weight decay and amsgrad");
        return -1;
    }
    if (!params || !grads || !state0 || !state1 || !ranges || n_ranges <= 0 || step < 1) { lg_set_error("optim_step_ex: invalid argument"); return -1; }
    // lg_adam_step takes its scalars as floats: round them first, so that the bias corrections see what that entry point sees
    return launch_adam(params, grads, state0, state1, ranges, n_ranges, max_range, step, (float)lr, (float)h0, (float)h1, (float)eps,
                       (float)grad_scale, c, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// the classical baselines (k_classical.hip)
// ------------------------------------------------------------------------------------------------
extern "C" size_t lg_classical_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t method) {
    return classical_workspace_bytes(B, C, h, w, method);
}
extern "C" int lg_interp23_up4(const float* ms, float* out, int32_t B, int32_t C, int32_t h, int32_t w, void* stream) {
    return launch_interp23_up4(ms, out, B, C, h, w, (hipStream_t)stream);
}
extern "C" int lg_sfim(const float* ms, const float* pan, float* out, int32_t B, int32_t C, int32_t h, int32_t w, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return launch_sfim(ms, pan, out, B, C, h, w, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int lg_gsa(const float* ms, const float* pan, float* out, double* stats, int32_t B, int32_t C, int32_t h, int32_t w, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return launch_gsa(ms, pan, out, stats, B, C, h, w, workspace, workspace_bytes, (hipStream_t)stream);
}
