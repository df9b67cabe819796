// lg_resolve_route: the ONE place that turns lg_config.variant / precision / C / H / W into kernels (host code only).
//
// bit (include/lgteun_hip.h)     Python side (_lib.variant_from_env)   effect
// LG_VAR_FFN_IMPL_MASK           LG_FFN_IMPL = strip                   1 (LG_VAR_FFN_STRIP, precision = 0 only): round 1's f32-MFMA kernels -- k_ffn_strip at e = 16,
//                                                                      k_ffn_fused at e = 32, k_ffn1 + k_ffn2 at e = 64; the backward then runs round 2's tile
//                                                                      kernels on the five-tensor save.  2 and 3 are not carried: lg_plan_create rejects them
// LG_VAR_FFN_SAVE3 / _SAVE5      LG_FFN_SAVE = 3 | 5                   e = 16: keep h1 / h2 / h3 (3; precision = 1: as 5) or gelu(h1), gelu'(h1), h2, gelu(h3),
//                                                                      gelu'(h3) (5) instead of h2 / h3 (default: h1 re-computed by k_ffn1_bwd_xs)
// LG_VAR_FFN_BWD32_PAIR          LG_FFN_BWD32 = pair                   e = 32 pixelwise half: k_ffn1_bwd_x32 + k_wgrad on saved gelu(h1) / gelu'(h1) instead of k_ffn1_bwd_xs<32>
// LG_VAR_FFN_DWBWD_TILE          LG_FFN_DWBWD = tile                   spatial half: the tile kernel k_ffn_dw_bwd + k_wgrad for dW3 instead of k_ffn_dw_bwd_xs
//                                                                      (fp32 storage; e = 32 level-1 planes whose width is 8 mod 16 take it anyway: a strip is 16 wide)
// LG_VAR_ATTN_BWD_R3             LG_ATTN_BWD = r3                      e = 16 local-mixer backward: round 3's three-kernel form instead of k_attn_bwd_f
// LG_VAR_DSTEP_TILES             LG_DSTEP = tiles                      data step: the tile kernels also where the one-launch form exists (square planes of 128 or 64)
// LG_VAR_ATTN_FWD_VALU           LG_ATTN_FWD = valu                    local-mixer forward: the vector-pipe k_attn instead of the matrix-pipe k_attn_m
// LG_VAR_FFN_BF16X3              LG_FFN_SPLIT = bf16x3                 fused FFN forward (and with it the local mixer, whose scales ride in the same prep launch):
//                                                                      three bf16 pieces / six products instead of f16 pairs with operand scales
// LG_VAR_FFT_FULL                LG_FFT = full                         global mixer, planes that run in LDS (square powers of two up to 128): the complex-row kernels
//                                                                      instead of the real-input ones.  The path itself follows from the plane's size alone
//                                                                      (resolve_fft); lg_plan_describe names it per level: fft=k_fftmix_r | k_fftmix | split | bluestein
// LG_VAR_FFN_BWD_BF16X3          LG_FFN_BWD_SPLIT = bf16x3             k_ffn1_bwd_xs: three bf16 pieces instead of f16 pairs
// LG_VAR_ATTN_BWD_CORE_M         LG_ATTN_BWD_CORE = m                  e = 32 local-mixer backward core: k_attn_bwd_core_m (re-derives the row statistics) instead of k_attn_bwd_core
// LG_VAR_FFN_XS                  LG_FFN_FWD = xs                       e = 16 fused FFN forward: the channel-split k_ffn_xs instead of the register chain k_ffn_xr
// LG_VAR_ATTN_BF16X3             LG_ATTN_SPLIT = bf16x3                k_attn_m: to_qkv and Q K^T on three bf16 pieces instead of f16 pairs with static scales
// LG_VAR_FFN_H3_RECOMPUTE        LG_FFN_H3 = recompute                 e = 16, default save form, f16 pairs, k_ffn_xr: save h2 ONLY; k_ffn_dw_bwd_h re-computes h3
// LG_VAR_ATTN_BWD_RESTATS        LG_ATTN_BWD_STATS = recompute         the local-mixer backward re-derives the softmax row statistics instead of reading the forward's
// LG_VAR_REDUCE_PER_BLOCK        LG_REDUCE = per_block                 parameter-gradient reduces: one launch per block and data step instead of one per pass
#include <stdio.h>

#include "kernels.h"
#include "bwd_kernels.h"

static void resolve_ffn(const lg_config& cfg, int e, int h, int w, FfnRoute& f) {
    const uint32_t v = cfg.variant;
    const int impl = (int)(v & LG_VAR_FFN_IMPL_MASK);
    const uint32_t sv = v & LG_VAR_FFN_SAVE_MASK;
    const bool split = impl == 0;   // the split-arithmetic kernels of rounds 2 - 6; otherwise (precision = 0 only) round 1's f32-MFMA kernels with round 2's tile backward
    const bool strips = (h & 7) == 0 && (w & 15) == 0;   // a strip is 16 columns wide, every output pixel of a step inside the plane (level 0: always)
    f.e = e; f.h = h; f.w = w;
    // precision = 1 applies where a plain-bf16 kernel exists: the e = 64 half-blocks have only the round-1 f32-MFMA pair in that form (436 + 372 us
    // against 123 + 95 us for the split-bf16 k_ffn_x64 pair), so they run the default kernels with fp32 storage in both modes
    f.hbf = cfg.precision == 1 && e != 64;
    f.scales = cfg.precision == 0 && split && !(v & LG_VAR_FFN_BF16X3);
    f.arith = !split ? FFN_ARITH_F32 : f.hbf ? FFN_ARITH_BF16 : f.scales ? FFN_ARITH_F16X2 : FFN_ARITH_BF16X3;
    f.wsplit_np = e < 32 ? 0 : f.hbf ? 1 : f.scales ? 2 : 3;   // (prep_stages fills the slot of every e >= 32 block, whichever kernel runs)

    // ---- backward.  e = 16 keeps h2 / h3 (save form 2), h1 / h2 / h3 (3, fp32 storage only) or the five GELU-free tensors (5, and every other width)
    const int save_form = (e != 16 || !split) ? 5 : sv == LG_VAR_FFN_SAVE5 ? 5 : (sv == LG_VAR_FFN_SAVE3 ? (cfg.precision == 0 ? 3 : 5) : 2);
    f.pre = save_form != 5;
    f.px = (e == 16 && save_form == 2) || (e == 32 && split && !(v & LG_VAR_FFN_BWD32_PAIR)) ? FFN1_BWD_XS : (e == 32 && split) ? FFN1_BWD_X32 : FFN1_BWD_TILE;
    const bool dw_tile = (v & LG_VAR_FFN_DWBWD_TILE) && !(e == 16 && f.hbf);   // (the bf16 strip kernel has no tile counterpart behind k_ffn1_bwd_xs<16>)
    f.dw = ((e == 16 && save_form == 2) || (e == 32 && split)) && !dw_tile && strips ? FFN_DWBWD_XS : FFN_DWBWD_TILE;
    const bool xr_built = split && !(v & LG_VAR_FFN_XS) && (f.hbf || f.scales);   // k_ffn_xr has bf16 and f16-pair instances
    if (e == 16 && f.dw == FFN_DWBWD_XS && (v & LG_VAR_FFN_H3_RECOMPUTE) && xr_built && !f.hbf) f.dw = FFN_DWBWD_H;
    f.bwd_scales = f.px == FFN1_BWD_XS && f.dw != FFN_DWBWD_TILE && f.scales && !(v & LG_VAR_FFN_BWD_BF16X3);
    f.wgrad_w2 = f.px != FFN1_BWD_XS;
    f.wgrad_w1 = f.px != FFN1_BWD_XS && !ffn1_bwd_fuses_w1(e);
    f.wgrad_w3 = f.dw == FFN_DWBWD_TILE;

    // ---- what the backward reads is what the saving forward writes
    f.saves = FFN_SLOT_H2;
    if (f.dw == FFN_DWBWD_XS || f.wgrad_w3) f.saves |= FFN_SLOT_A3;
    if (f.dw == FFN_DWBWD_TILE && !f.pre) f.saves |= FFN_SLOT_G3;
    if (f.px != FFN1_BWD_XS) f.saves |= FFN_SLOT_A1 | (f.pre ? 0 : FFN_SLOT_G1);

    // ---- forward
    FfnFwdKernel k;
    if (e == 16) k = split ? FFN_FWD_XS : FFN_FWD_STRIP;
    else if (e == 32) k = split ? FFN_FWD_X32 : FFN_FWD_TILE;
    else k = split ? FFN_FWD_X64 : FFN_FWD_UNFUSED;
    f.fwd[0] = f.fwd[1] = k;
    if (e == 16 && xr_built) {   // the register chain where it exists: nothing saved, or h2 (/ h3)
        f.fwd[0] = FFN_FWD_XR;
        if (!(f.saves & ~(unsigned)(FFN_SLOT_H2 | FFN_SLOT_A3))) f.fwd[1] = FFN_FWD_XR;
    }
}

static void resolve_mixer(const lg_config& cfg, int e, MixerRoute& m) {
    const uint32_t v = cfg.variant;
    m.e = e;
    m.fwd = (v & LG_VAR_ATTN_FWD_VALU) ? ATTN_FWD_VALU : ATTN_FWD_M;
    m.bf16 = cfg.precision == 1;
    // (the scales ride in the FFN prep launch: the f16-pair FFN arithmetic must be on)
    m.f16x2 = cfg.precision == 0 && m.fwd == ATTN_FWD_M && !(v & LG_VAR_ATTN_BF16X3) && !(v & LG_VAR_FFN_IMPL_MASK) && !(v & LG_VAR_FFN_BF16X3);
    m.bwd = (attn_bwd_fused(e) && !(v & LG_VAR_ATTN_BWD_R3)) ? ATTN_BWD_F : (e == 32 && (v & LG_VAR_ATTN_BWD_CORE_M)) ? ATTN_BWD_R3_CORE_M : ATTN_BWD_R3;
    // fp32-equivalent mode, matrix-pipe forward: the row log-sum-exp and the attention output go from k_attn_m to k_attn_bwd_f / k_attn_bwd_core
    m.stats = cfg.precision == 0 && m.fwd == ATTN_FWD_M && !(v & LG_VAR_ATTN_BWD_RESTATS) && m.bwd != ATTN_BWD_R3_CORE_M;
}

// THE size rule of the global mixer: a square power of two of 8 .. 512 stays radix-2 -- in LDS up to 128, through HBM above -- and every other plane
// takes Bluestein lines.  LG_VAR_FFT_FULL swaps the in-LDS kernel pair and touches nothing else.
static void resolve_fft(const lg_config& cfg, int h, int w, FftRoute& f) {
    const bool pow2 = h == w && (h & (h - 1)) == 0 && h >= 8 && h <= 512;
    f.h = h; f.w = w; f.lg = 0;
    while (pow2 && (1 << f.lg) < h) ++f.lg;
    f.path = !pow2 ? FFT_PATH_BLUESTEIN : h > 128 ? FFT_PATH_SPLIT : (cfg.variant & LG_VAR_FFT_FULL) ? FFT_PATH_LDS_C : FFT_PATH_LDS_R;
    // columns a workgroup of the column launch transforms; the in-LDS kernels hold the whole plane
    const int cols_per_wg = f.path == FFT_PATH_SPLIT ? fft_split_cols_per_wg(h) : f.path == FFT_PATH_BLUESTEIN ? fft_bluestein_lines_per_wg(h) : 0;
    f.col_groups = cols_per_wg ? (w / 2 + 1 + cols_per_wg - 1) / cols_per_wg : 1;
    f.scratch_floats = cols_per_wg ? (size_t)h * (w / 2 + 1) * 2 : 0;
}

int lg_resolve_route(const lg_config& cfg, LgRoute* r) {
    const uint32_t v = cfg.variant;
    if (v & ~LG_VAR_ALL) { lg_set_error("plan_create: unknown variant bits 0x%x", v & ~LG_VAR_ALL); return -2; }
    if ((v & LG_VAR_FFN_SAVE_MASK) == LG_VAR_FFN_SAVE_MASK) { lg_set_error("plan_create: invalid FFN save variant"); return -2; }
    if ((v & LG_VAR_FFN_IMPL_MASK) > LG_VAR_FFN_STRIP) { lg_set_error("plan_create: FFN implementation field (LG_VAR_FFN_IMPL_MASK) = %u: only 0 and LG_VAR_FFN_STRIP exist", v & LG_VAR_FFN_IMPL_MASK); return -2; }
    if (cfg.precision == 1 && (v & LG_VAR_FFN_IMPL_MASK)) { lg_set_error("plan_create: FFN implementation field (LG_VAR_FFN_IMPL_MASK): LG_VAR_FFN_STRIP is an fp32 kernel set, precision = 1 has none"); return -2; }
    const int E = 4 * cfg.C;
    resolve_ffn(cfg, E, cfg.H, cfg.W, r->ffn[0]);
    resolve_ffn(cfg, 2 * E, cfg.H / 2, cfg.W / 2, r->ffn[1]);
    resolve_mixer(cfg, E, r->mix[0]);
    resolve_mixer(cfg, 2 * E, r->mix[1]);
    resolve_fft(cfg, cfg.H, cfg.W, r->fft[0]);
    resolve_fft(cfg, cfg.H / 2, cfg.W / 2, r->fft[1]);
    r->dstep_fused = !(v & LG_VAR_DSTEP_TILES) && dstep_fused_ok(cfg.C, cfg.H, cfg.W);
    r->reduce_per_block = (v & LG_VAR_REDUCE_PER_BLOCK) != 0;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// lg_plan_describe: the routes as text, one line per level and mode
// ------------------------------------------------------------------------------------------------
static const char* slots_text(unsigned slots, bool a1_pre, bool a3_pre, char (&buf)[48]) {
    int n = 0;
    buf[0] = 0;
    auto add = [&](unsigned bit, const char* name) { if (slots & bit) n += snprintf(buf + n, sizeof(buf) - n, "%s%s", n ? "," : "", name); };
    add(FFN_SLOT_A1, a1_pre ? "a1:h1" : "a1"); add(FFN_SLOT_G1, "g1"); add(FFN_SLOT_H2, "h2"); add(FFN_SLOT_A3, a3_pre ? "a3:h3" : "a3"); add(FFN_SLOT_G3, "g3");
    return n ? buf : "-";
}

int lg_describe_route(const lg_config& cfg, const LgRoute& r, char* buf, size_t n) {
    static const char* const fwd_names[] = {"k_ffn_xr", "k_ffn_xs", "k_ffn_x32", "k_ffn1_x64+k_ffn2_x64", "k_ffn_strip", "k_ffn_fused", "k_ffn1+k_ffn2"};
    static const char* const arith_names[] = {"f32", "bf16", "f16x2", "bf16x3"};
    static const char* const dw_names[] = {"k_ffn_dw_bwd_xs", "k_ffn_dw_bwd_h", "k_ffn_dw_bwd"};
    static const char* const px_names[] = {"k_ffn1_bwd_xs", "k_ffn1_bwd_x32", "k_ffn1_bwd"};
    static const char* const fft_names[] = {"k_fftmix_r", "k_fftmix", "split", "bluestein"};
    static const char* const attn_bwd_names[] = {"k_attn_bwd_f", "k_attn_bwd_core+k_attn_bwd_epi", "k_attn_bwd_core_m+k_attn_bwd_epi"};
    size_t off = 0;
    bool full = false;
    auto put = [&](const char* fmt, auto... a) {
        const int k = snprintf(buf + off, n - off, fmt, a...);
        if (k < 0 || (size_t)k >= n - off) full = true; else off += (size_t)k;
    };
    if (!buf || n == 0) { lg_set_error("plan_describe: null argument"); return -1; }
    put("net C=%d %dx%d precision=%d variant=0x%x: dstep=%s fft=%s reduce=%s\n", cfg.C, cfg.H, cfg.W, cfg.precision, cfg.variant,
        r.dstep_fused ? "fused" : "tiles", (cfg.variant & LG_VAR_FFT_FULL) ? "k_fftmix" : "k_fftmix_r", r.reduce_per_block ? "per_block" : "merged");
    for (int l = 0; l < 2 && !full; ++l) {
        const FfnRoute& f = r.ffn[l];
        const MixerRoute& m = r.mix[l];
        const char* attn = m.fwd == ATTN_FWD_M ? "k_attn_m" : "k_attn";
        const char* attn_arith = m.fwd == ATTN_FWD_VALU ? "f32" : m.bf16 ? "bf16" : m.f16x2 ? "f16x2" : "bf16x3";
        char sb[48];
        put("L%d e=%d %dx%d fwd: ffn=%s arith=%s hidden=%s | mixer=%s arith=%s | fft=%s\n", l, f.e, f.h, f.w, fwd_names[f.fwd[0]], arith_names[f.arith],
            f.hbf ? "bf16" : "fp32", attn, attn_arith, fft_names[r.fft[l].path]);
        put("L%d e=%d %dx%d save: ffn=%s writes=%s | mixer=%s writes=%s\n", l, f.e, f.h, f.w, fwd_names[f.fwd[1]],
            slots_text(f.saves, f.pre, f.a3_pre(), sb), attn, m.stats ? "o,l" : "-");
        unsigned reads = FFN_SLOT_H2;   // by kernel: the spatial half, the pixelwise half, the weight-gradient launches
        if (f.dw == FFN_DWBWD_XS) reads |= FFN_SLOT_A3;
        if (f.dw == FFN_DWBWD_TILE) reads |= f.pre ? FFN_SLOT_A3 : FFN_SLOT_G3;
        if (f.px != FFN1_BWD_XS) reads |= f.pre ? FFN_SLOT_A1 : FFN_SLOT_G1;
        if (f.wgrad_w2) reads |= FFN_SLOT_A1;
        if (f.wgrad_w3) reads |= FFN_SLOT_A3;
        put("L%d e=%d %dx%d bwd: ffn=%s+%s%s%s%s arith=%s reads=%s | mixer=%s stats=%s\n", l, f.e, f.h, f.w, dw_names[f.dw], px_names[f.px],
            f.wgrad_w2 ? "+k_wgrad(W2)" : "", f.wgrad_w1 ? "+k_wgrad(W1)" : "", f.wgrad_w3 ? "+k_wgrad(W3)" : "",
            f.px == FFN1_BWD_TILE ? "f32" : f.px == FFN1_BWD_X32 ? "bf16x3" : f.hbf ? "bf16" : f.bwd_scales ? "f16x2" : "bf16x3", slots_text(reads, f.pre, f.a3_pre(), sb), attn_bwd_names[m.bwd],
            m.stats ? "saved" : "recomputed");
    }
    if (full) { lg_set_error("plan_describe: buffer of %zu bytes is too small", n); return -3; }
    return 0;
}
