// C ABI entry points (include/lgteun_hip.h), host code only -- no kernel and no launch in this file: the error text, plan and workspace sizing,
// lgteun_backward, the per-op and debug entries.  Every other entry point sits beside the code it runs: k_fwd.hip, prof.hip, k_optim.hip, k_*.hip.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "abi.h"
#include "kernels.h"
#include "workspace.h"
#include "forward.h"
#include "backward.h"
#include "net_args.h"

static thread_local char g_err[512] = "";

void lg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ------------------------------------------------------------------------------------------------
// the network entries' argument contract (net_args.h; include/lgteun_hip.h states it)
// ------------------------------------------------------------------------------------------------
// The largest batch: B_max = min(floor(65535 / C), floor((2^31 - 1) / (S * 16 C * H * W))), S = K for (C = 4, K >= 3, H and W <= 128, train != 2) --
// a superset of the plans whose dead stages run as one pass (lg_plan_stage_batch), which hand S B samples to one launch -- else 1.  Read off every
// launcher and kernel a network route reaches; nothing above it was ever launched to find it.  The limiting sites:
//   planes B C in a grid's y or z, which HIP documents up to 65535 (x: 2^31 - 1):
//     k_pixel.hip:131       launch_resample_dw: dim3 grid(.., .., a.planes) -- the data step's four forward tile launches (every plan but 64^2 / 128^2)
//     k_bwd_pixel.hip:101   launch_resample_adj: dim3 grid(.., planes), and the launcher's own refusal of planes > 65535 at :90
//     k_bwd_pixel.hip:200   resample + depthwise backward: dim3 grid(.., .., a.planes)
//     k_bwd_pixel.hip:306   the update's backward: dim3 grid(.., .., a.B * a.C)
//     k_fwd.hip:12, k_bwd.hip:278   const int planes = B * c.C feeds all of them
//   elements of the largest tensor one launch addresses, the FFN's hidden tensor [S B, H, W, 16 C], in a 32-bit index:
//     k_ffn_xr.hip:717      launch_ffn_xr refuses a2.B * h * w * N1 >= 2^32 (a2.B = S B in the batched pass): the kernel's 32-bit save index
//     api.hip               lg_debug_stage_decision refuses Bs * n * h * w >= 2^31: the persistent kernels count pixels and strips in int
//     k_pixel.hip:621       launch_upfuse: const int grid = a.B * tiles_x * tiles_y;  k_ffn.hip:254 the same;  k_bwd_pixel.hip:766 const int rows = a.B * a.H
//     k_fft.hip:1220-1288   the FFT mixer: S B 4C planes in grid x, 512 or 1024 threads each -- threads per launch stay below 2^32
//   Every other product of B in the launchers is taken in long or size_t (k_bwd.hip:30, :122, :198, :347; k_fwd.hip:92, :196, :226; workspace.h).
// The element bound is signed (2^31) where k_ffn_xr.hip's own is unsigned (2^32): every int index into any tensor of the call stays positive, whichever
// kernel forms it.  With it 16 x 16 planes give B <= 16383 (C = 4) and 8191 (C = 8) from the grid limit; from 256 x 256 up the element bound is the
// smaller one (C = 4, K = 4, 128 x 128: 511; 1024 x 1024: 31 / 15).
int64_t lg_net_max_batch(const lg_config& c, int train) {
    const int64_t S = (c.C == 4 && c.K >= 3 && c.H <= 128 && c.W <= 128 && train != 2) ? c.K : 1;
    const int64_t by_grid = 65535 / c.C, by_index = ((1ll << 31) - 1) / (S * 16 * c.C * c.H * c.W);
    return by_grid < by_index ? by_grid : by_index;
}

NetArgs& NetArgs::fail(int code, const char* fmt, ...) {
    char what[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(what, sizeof(what), fmt, ap);
    va_end(ap);
    lg_set_error("%s: %s", who, what);
    rc = code;
    return *this;
}
NetArgs& NetArgs::batch(int B, int train) {
    if (rc) return *this;
    const long long top = lg_net_max_batch(pl->cfg, train);
    return (B >= 1 && B <= top) ? *this : fail(-1, "B must be in 1 .. %lld for this plan (got %d)", top, B);
}
NetArgs& NetArgs::flags(int fl, int allowed) {
    if (rc) return *this;
    if (fl & ~LG_FLAGS_DEFINED) return fail(-1, "flags has bits the header does not define (0x%x)", (unsigned)(fl & ~LG_FLAGS_DEFINED));
    if (fl & ~allowed) return fail(-2, "flags 0x%x do not apply to this entry (it takes 0x%x)", (unsigned)(fl & ~allowed), (unsigned)allowed);
    return *this;
}
NetArgs& NetArgs::workspace(const void* ws, size_t bytes, int B, int train) {
    ptr(ws, "workspace").aligned(ws, "workspace", 256);
    if (rc) return *this;
    const size_t need = lg_workspace_bytes(pl, B, train);
    return bytes >= need ? *this : fail(-3, "workspace too small (workspace_bytes %zu < %zu)", bytes, need);
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
    ok = ok && r.ffn[0].fwd[0] == FFN_FWD_XR && r.ffn[1].fwd[0] == FFN_FWD_X32 && r.mix[0].fwd == ATTN_FWD_M && r.mix[1].fwd == ATTN_FWD_M;
    ok = ok && (r.ffn[1].scales || r.ffn[1].hbf);                        // (k_ffn_x32's three-piece arithmetic has no multi-stage instance)
    ok = ok && r.fft[0].path == FFT_PATH_LDS_R && r.fft[1].path == FFT_PATH_LDS_R;   // the one FFT kernel that takes several stages
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
    if (!plan || train < 0 || train > 2 || B <= 0 || B > lg_net_max_batch(plan->cfg, train)) return 0;
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

extern "C" int lg_debug_live_slot(const lg_plan* plan, int32_t B, int32_t train, size_t* out53) {
    if (!plan || B <= 0 || train < 0 || train > 2 || !out53) { lg_set_error("debug_live_slot: invalid argument"); return -1; }
    NetBufs nb;
    char base[1];   // carve() only adds offsets to the base it is given
    carve(plan, B, train, base, nb);
    const NetBufs lv = live_view(nb);
    size_t* o = out53;
    *o++ = nb.bytes; *o++ = train ? bwd_workspace_bytes(plan, B) : 0; *o++ = nb.live_s0;
    auto off = [&](const float* p) { return (size_t)(reinterpret_cast<const char*>(p) - base); };
    for (int j = 0; j < LG_NBLK; ++j) {
        const BlockBufs &a = nb.blk[j], &l = lv.blk[j];
        const float* pa[5] = {a.xin, a.xmid, a.xout, a.g, a.o2};
        const float* pl[5] = {l.xin, l.xmid, l.xout, l.g, l.o2};
        for (int f = 0; f < 5; ++f) { *o++ = off(pa[f]); *o++ = off(pl[f]); }
    }
    return 0;
}

extern "C" int lgteun_backward(const lg_plan* plan, const float* params, float* grads, const float* ms, const float* pan,
                               const float* dout, void* workspace, size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed,
                               void* stream) {
    const int train = (flags & LG_FLAG_CHAINED) ? 2 : 1;
    NetArgs v("backward");
    v.plan(plan).f32(params, "params").f32(grads, "grads").f32(ms, "ms").f32(pan, "pan").f32(dout, "dout").flags(flags, LG_FLAGS_DEFINED);
    if (!v.rc && (flags & LG_FLAG_CHAINED) && (flags & (LG_FLAG_BWD_LGT | LG_FLAG_BWD_DATA))) v.fail(-2, "flags: LG_FLAG_BWD_LGT / LG_FLAG_BWD_DATA do not apply to LG_FLAG_CHAINED");
    if (v.batch(B, train).workspace(workspace, workspace_bytes, B, train).rc) return v.rc;
    NetBufs nb;
    carve(plan, B, train, workspace, nb);
    return net_backward(plan, params, grads, ms, pan, dout, nb, (char*)workspace + nb.bytes, B, flags, seed, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// per-op entry points
// ------------------------------------------------------------------------------------------------
extern "C" int lg_op_resample(const float* x, float* y, int32_t planes, int32_t hi, int32_t wi, int32_t mode, void* stream) {
    // k_pixel.hip:15-38: a one-dimensional grid of at most 4096 workgroups strides over planes * ho * wo outputs in long -- the plane count is in no grid
    // dimension; inside a plane the taps are indexed in int (common.h: resample_at, yy * wi + x), so a plane holds fewer than 2^31 / 16 inputs
    NetArgs v("op_resample");
    v.f32(x, "x").f32(y, "y").range(mode, "mode", 0, 2).range(planes, "planes", 1, 0x7fffffff).range(hi, "hi", 1, 0x7fffffff).range(wi, "wi", 1, 0x7fffffff);
    if (!v.rc && (long long)hi * wi >= (1ll << 27)) v.fail(-1, "hi * wi must be below 2^27 (got %lld)", (long long)hi * wi);
    if (!v.rc && mode == 0 && ((hi & 1) || (wi & 1))) v.fail(-2, "hi and wi: x0.5 needs even sizes");
    if (v.rc) return v.rc;
    return launch_resample(mode, x, y, planes, hi, wi, (hipStream_t)stream);
}

extern "C" int lg_op_data_step(const lg_plan* plan, const float* params, int32_t stage, const float* z_in, const float* ms,
                               const float* pan, float* z_out, float* tmp, int32_t B, void* stream) {
    NetArgs v("op_data_step");
    v.plan(plan).f32(params, "params").stage(stage).f32(z_in, "z_in").f32(ms, "ms").f32(pan, "pan").f32(z_out, "z_out").f32(tmp, "tmp");
    if (v.batch(B, 0).rc) return v.rc;
    const lg_config& c = plan->cfg;
    size_t q = (size_t)B * c.C * c.H * c.W / 4;
    return data_step_fwd(plan, params, stage, z_in, ms, pan, z_out, tmp, tmp + q, tmp + 2 * q, tmp + 3 * q, B, (hipStream_t)stream);
}

extern "C" int lg_op_lgt(const lg_plan* plan, const float* params, int32_t stage, const float* z, float* out, void* workspace,
                         size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream) {
    const int train = (flags & LG_FLAG_SAVE) ? 1 : 0;
    NetArgs v("op_lgt");
    v.plan(plan).f32(params, "params").stage(stage).f32(z, "z").f32(out, "out").flags(flags, LG_FLAG_SAVE | LG_FLAG_DROPOUT);
    if (v.batch(B, train).workspace(workspace, workspace_bytes, B, train).rc) return v.rc;
    NetBufs nb;
    carve(plan, B, train, workspace, nb);
    nb = live_view(nb);   // a single stage runs where the live stage does: slot K-1 of the transient buffers (workspace.h)
    if (int rc = prep_stages(plan, params, stage, stage + 1, nb, (hipStream_t)stream)) return rc;
    return lgt_fwd(plan, params, stage, z, out, nb, B, flags, seed, (hipStream_t)stream);
}

extern "C" int lg_op_lgt_stages(const lg_plan* plan, const float* params, int32_t stage0, int32_t n, const float* z, float* out, void* workspace,
                                size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, int32_t grid_cap, void* stream) {
    NetArgs v("op_lgt_stages");
    v.plan(plan).f32(params, "params");
    if (!v.rc) v.range(stage0, "stage0", 0, plan->cfg.K - 1).range(n, "n", 1, plan->cfg.K - stage0);
    v.f32(z, "z").f32(out, "out").range(grid_cap, "grid_cap", 0, 0x7fffffff).flags(flags, LG_FLAG_DROPOUT);
    if (!v.rc && n > 1 && (!plan->stage_batch || n > plan->cfg.K - 1)) v.fail(-2, "n: this plan runs one stage per pass (lg_plan_stage_batch), or n > K-1");
    if (v.batch(B, 0).workspace(workspace, workspace_bytes, B, 0).rc) return v.rc;
    NetBufs nb;
    carve(plan, B, 0, workspace, nb);
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
    NetArgs v("op_block");
    v.plan(plan).f32(params, "params").stage(stage).range(blk, "blk", 0, LG_NBLK - 1).range(which, "which", 0, 2).f32(x, "x").f32(y, "y");
    if (v.batch(B, 0).workspace(workspace, workspace_bytes, B, 0).rc) return v.rc;
    hipStream_t s = (hipStream_t)stream;
    NetBufs nb;
    int rc;
    carve(plan, B, 0, workspace, nb);
    nb = live_view(nb);   // a single stage runs where the live stage does: slot K-1 of the transient buffers (workspace.h)
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
        f.ch = bb.e / 2; f.planes = B * f.ch;
        return launch_fftmix(plan->fft(bb.e), f, s);
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
    NetArgs v("op_block_bwd");
    v.plan(plan).f32(params, "params").f32(grads, "grads").stage(stage).range(blk, "blk", 0, LG_NBLK - 1).range(which, "which", 0, 2).f32(x, "x").f32(dy, "dy").f32(dx, "dx");
    if (v.batch(B, 1).workspace(workspace, workspace_bytes, B, 1).rc) return v.rc;
    hipStream_t s = (hipStream_t)stream;
    NetBufs nb;
    int rc;
    carve(plan, B, 1, workspace, nb);
    nb = live_view(nb);   // a single stage runs where the live stage does: slot K-1 of the transient buffers (workspace.h)
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
    NetArgs v("op_data_step_bwd");
    v.plan(plan).f32(params, "params").f32(grads, "grads").stage(stage).f32(z_in, "z_in").f32(ms, "ms").f32(pan, "pan").f32(dz_out, "dz_out").f32(dz_in, "dz_in");
    if (v.batch(B, 1).workspace(workspace, workspace_bytes, B, 1).rc) return v.rc;
    hipStream_t s = (hipStream_t)stream;
    NetBufs nb;
    int rc;
    carve(plan, B, 1, workspace, nb);
    // forward of the step: fills the intermediates its backward reads (t1, r, s1)
    if ((rc = data_step_fwd(plan, params, stage, z_in, ms, pan, nb.Z[stage + 1], nb.t1[stage], nb.r[stage], nb.s1[stage], nb.pr, B, s))) return rc;
    return op_data_step_bwd(plan, params, grads, stage, nb, (char*)workspace + nb.bytes, z_in, pan, dz_out, dz_in, B, s);
}

extern "C" int lg_op_lgt_bwd(const lg_plan* plan, const float* params, float* grads, int32_t stage, const float* z, const float* dout,
                             float* dz, void* workspace, size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream) {
    NetArgs v("op_lgt_bwd");
    v.plan(plan).f32(params, "params").f32(grads, "grads").stage(stage).f32(z, "z").f32(dout, "dout").f32(dz, "dz").flags(flags, LG_FLAG_DROPOUT);
    if (v.batch(B, 1).workspace(workspace, workspace_bytes, B, 1).rc) return v.rc;
    hipStream_t s = (hipStream_t)stream;
    NetBufs nb;
    int rc;
    carve(plan, B, 1, workspace, nb);
    nb = live_view(nb);   // a single stage runs where the live stage does: slot K-1 of the transient buffers (workspace.h)
    if ((rc = prep_stages(plan, params, stage, stage + 1, nb, s))) return rc;
    if ((rc = lgt_fwd(plan, params, stage, z, nb.deadout, nb, B, flags | LG_FLAG_SAVE, seed, s))) return rc;
    return op_lgt_bwd(plan, params, grads, stage, nb, (char*)workspace + nb.bytes, z, dout, dz, B, flags, seed, s);
}
