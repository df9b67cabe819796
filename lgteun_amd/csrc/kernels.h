// Internal launcher declarations (one per fused kernel).  All pointers are device pointers.
#pragma once
#include "common.h"

// ---------------- data module (reference models/unlg_former.py:29-37,58-61) ----------------
struct DwArgs {
    const float* in;    // [planes, hi, wi]
    float* out;         // [planes, ho, wo]
    const float* w9;    // [C,1,3,3]
    const float* bias;  // [C]
    const float* sub;   // EPI 1: subtract [planes, ho, wo]
    // EPI 2 (data-step update): out = z - eta * (val + RT(R(z) - pan))
    const float* z;     // [B, C, ho, wo]
    const float* pan;   // [B, 1, ho, wo]
    const float* rw;    // [1,C,1,1]
    const float* rb;    // [1]
    const float* rtw;   // [C,1,1,1]
    const float* rtb;   // [C]
    const float* eta;   // scalar
    int C, planes, hi, wi, ho, wo;
};
// MODE 0: x0.5, 1: x2 ; EPI 0: none, 1: minus sub, 2: data-step update
int launch_resample_dw(int mode, int epi, const DwArgs& a, hipStream_t s);
int launch_resample(int mode, const float* x, float* y, int planes, int hi, int wi, hipStream_t s);
// the whole proximal-gradient step of a stage in ONE launch (k_dstep.hip): planes that fit the LDS of a CU (square, 128 or 64 wide)
struct DstepFwdArgs {
    const float* z;      // Z_i [B,C,N,N]
    const float* ms;     // [B,C,N/4,N/4]
    const float* pan;    // [B,1,N,N]
    float* zout;         // [B,C,N,N]
    float *t1, *r, *s1;  // the chain's intermediates (what the backward reads): [B,C,N/2,N/2], [B,C,N/4,N/4], [B,C,N/2,N/2]
    float* pr;           // scratch [B,N,N]: R Z - pan of the sample (written by the pixelwise launch in front of the plane kernel)
    const float *d1w, *d1b, *d3w, *d3b, *dt1w, *dt1b, *dt3w, *dt3b, *rw, *rb, *rtw, *rtb, *eta;
    int B, C, N;
};
bool dstep_fused_ok(int C, int H, int W);
int launch_dstep_fwd(const DstepFwdArgs& a, hipStream_t s);

// ---------------- several stages in one launch (the dead-stage LGT forwards of a faithful step, k_fwd.hip: lgt_fwd) ----------------
// A forward kernel of the LGT sees a plain batch of n * Bs samples; sample b belongs to stage b / Bs, and a workgroup moves its weight, scale and
// table pointers by (b / Bs) x the stage strides before it stages anything.  The K LGTs have identical shapes, so every tensor of the flat
// parameter buffer has the SAME stride from one stage to the next (lg_plan::stage_stride).  n <= 1: one stage, every shift is zero.
struct StageSel {
    int n = 1;           // stages in the launch
    int Bs = 0;          // samples per stage
    long pstride = 0;    // floats between a parameter tensor of stage s and the same tensor of stage s + 1
    long zstride = 0;    // floats between the LGT inputs z of two consecutive stages
    int fs_stride = 0;   // floats between the stages' rows of ffn_scales
    int as_stride = 0;   // ... of attn_scales
    long ws_stride = 0;  // bytes between the stages' rows of wsplit
    int grid_cap = 0;    // test entry (lg_op_lgt_stages): upper bound of a persistent kernel's grid, 0 = none
    int s0 = 0;          // the plane and pixel kernels: the launch's save pointers (FftArgs::amp / pha / sgn, DownArgs::u_save, UpFuseArgs::t_save) hold samples
                         // s0 .. only, indexed from s0 -- the live stage riding behind the dead ones (k_fwd.hip: lgt_fwd).  0: every sample saves
    // dropout: the mask of stage s is keyed by mix_seed(seed, stage0 + s, blk) and counts its elements from the start of the stage's own tensor
    uint64_t seed = 0;
    int stage0 = 0, blk = 0;
};
#ifdef __HIPCC__
// stage of sample b (workgroup-uniform).  Integer division runs on the vector pipe, so its result is moved to a scalar register: left in a vector
// register it would drag every shifted pointer, and every load through one, onto the vector side.
__device__ __forceinline__ int stage_of(const StageSel& sg, int b) { return sg.n > 1 ? __builtin_amdgcn_readfirstlane(b / sg.Bs) : 0; }
// ... of the workgroup, where a sample is `per_sample` consecutive workgroups (or other units) and `unit` this workgroup's
__device__ __forceinline__ int stage_of_unit(const StageSel& sg, int unit, int per_sample) { return sg.n > 1 ? __builtin_amdgcn_readfirstlane(unit / (per_sample * sg.Bs)) : 0; }

// ---- the units (strips, strip pairs, window quads) a workgroup of a persistent multi-stage launch walks: the run [run0, run1) of ascending units, cut
// into one segment per stage.  ONE copy of the arithmetic for the kernels and for the host (lg_debug_stage_runs; tests/test_stage_runs_cpu.py).
struct StageRun { int run0, run1, base; };   // base: k_ffn_xr only -- strip index = unit + base
// `half` workgroups share the units evenly -- workgroup j takes [j units / half, (j + 1) units / half) -- and a workgroup j + half past them takes the run of
// workgroup j again, at base `units`   (half x units < 2^32: the launchers check it)
__host__ __device__ inline StageRun stage_run_halves(int units, int half, int wg) {
    const int first = wg < half ? 1 : 0, j = wg - (first ? 0 : half);
    return {(int)((unsigned)j * (unsigned)units / (unsigned)half), (int)(((unsigned)j + 1u) * (unsigned)units / (unsigned)half), first ? 0 : units};
}
// even: workgroup wg of `grid` takes units [wg units / grid, (wg + 1) units / grid)
__host__ __device__ inline StageRun stage_run_even(int units, int grid, int wg) { return stage_run_halves(units, grid, wg); }
// k_ffn_xr, uneven strip pairs (strip_geo with dS != 0: pair p = the tall strip p and the short strip p + npairs): workgroups j and j + grid / 2 -- the two
// of a CU -- walk the SAME run of pairs, the first (the one the arbiter favours) their tall strips, the second their short ones
__host__ __device__ inline StageRun stage_run_pairs(int npairs, int grid, int wg) { return stage_run_halves(npairs, grid >> 1, wg); }
// k_attn_m, uneven quads: chunk c of grid / 2 (one per CU) is cut u : 8 - u between workgroups c and c + grid / 2, to the nearest whole quad and with at
// least one quad each (an empty run would stage the tables of a stage that does not exist).  The launcher asks for >= 2 quads per chunk.  u = 0: even runs.
__host__ __device__ inline StageRun stage_run_chunk(int units, int grid, int wg, int u) {
    const StageRun ch = stage_run_halves(units, u ? grid >> 1 : grid, wg);
    if (!u) return ch;
    const int len = ch.run1 - ch.run0;
    int n1 = (len * u + 4) >> 3;
    n1 = n1 > len - 1 ? len - 1 : n1;
    n1 = n1 < 1 ? 1 : n1;
    return ch.base ? StageRun{ch.run0 + n1, ch.run1, 0} : StageRun{ch.run0, ch.run0 + n1, 0};
}
// end of the segment that starts at unit seg0 of stage st (= seg0 / per_stage)
__host__ __device__ inline int stage_seg_end(int st, int run1, int per_stage) { return run1 < (st + 1) * per_stage ? run1 : (st + 1) * per_stage; }
#endif

// the launchers' geometry as host functions (no device, no launch): what lg_debug_stage_decision reports
// The strip walkers (k_ffn_xs, k_ffn_strip, k_ffn_x32, k_ffn_xr, k_ffn_dw_bwd_xs, k_ffn_dw_bwd_h): 16-column strips of SH rows, dealt to a persistent grid.
// Strip height: the tallest multiple of 8 rows that still yields a strip per resident workgroup (`wgs`), at least 16.  Bh: the batch that sets the height --
// B, or with several stages in the launch the samples of ONE stage, so that a workgroup gets whole strips of that stage's own launch.  grid_cap: 0 = none.
struct StripGeo { int tiles_x, SH, strips_y, nstrips, grid; };
inline StripGeo strip_geometry(int h, int w, int B, int Bh, int wgs, int grid_cap) {
    StripGeo q;
    q.tiles_x = (w + 15) / 16;
    q.SH = (h + 7) / 8 * 8;
    while (q.SH > 16 && (long)Bh * q.tiles_x * ((h + q.SH - 1) / q.SH) < wgs) q.SH = (q.SH / 2 + 7) / 8 * 8;
    q.strips_y = (h + q.SH - 1) / q.SH;
    q.nstrips = B * q.tiles_x * q.strips_y;
    q.grid = q.nstrips < wgs ? q.nstrips : wgs;
    if (grid_cap > 0 && q.grid > grid_cap) q.grid = grid_cap;
    return q;
}
struct XrGeo : StripGeo { int dS; };
XrGeo ffn_xr_geometry(int h, int w, int B, int Bs, int n, int grid_cap);                       // k_ffn_xr.hip; n <= 1: one stage of B samples
struct AttnMGeo { int nwin, nquads, grid, uneven; };                                           // uneven: eighths of a CU's quads to its first workgroup, 0 = even
AttnMGeo attn_m_geometry(int HC, int h, int w, int B, int n, int grid_cap, int per_cu);        // k_attn_m.hip; HC = e / 2 in { 8, 16, 32 }

// ---------------- LGT pixelwise pieces (reference models/common/LGT.py) ----------------
struct EmbedArgs {
    const float* z;  // [B,C,H,W]
    float* x;        // [B,H,W,E]
    float* g;        // [B,E/2,H,W] LN1(next block)(x)[..., E/2:]  (nullable)
    const float *dww, *dwb, *w, *b, *lng, *lnb, *n1g, *n1b;
    int HW;
    long total;  // B*H*W
    StageSel sg;
};
int launch_embed(int C, const EmbedArgs& a, hipStream_t s);

struct DownArgs {
    const float* x;  // [B,H,W,E]
    float* y;        // [B,H/2,W/2,2E]
    float* g;        // [B,E,H/2,W/2]
    float* u_save;   // optional [B,H/2,W/2,E]: the resampled conv input (for the weight gradient)
    const float *w, *b, *n1g, *n1b;
    int B, H, W;  // input size
    StageSel sg;
};
int launch_down(int E, const DownArgs& a, hipStream_t s);

struct UpFuseArgs {
    const float* xb;    // [B,H/2,W/2,2E]
    const float* skip;  // [B,H,W,E]
    float* y;           // [B,H,W,E]
    float* g;           // [B,E/2,H,W]
    float* t_save;      // optional [B,H,W,E]: up-path tensor after its 1x1 conv (for the weight gradient)
    const float *upw, *upb, *fw, *fb, *n1g, *n1b;
    int B, H, W;  // output size
    StageSel sg;
};
int launch_upfuse(int E, const UpFuseArgs& a, hipStream_t s);

struct TailArgs {
    const float* x;  // [B,H,W,E]
    const float* z;  // [B,C,H,W]
    float* out;      // [B,C,H,W]
    float* out_last = nullptr;   // several stages: where the LAST stage's [Bs,C,H,W] goes instead of its part of `out` (the live stage: the caller's tensor); null: `out`
    const float *w, *b;
    int HW;
    long total;
    StageSel sg;
};
int launch_tail(int C, const TailArgs& a, hipStream_t s);

// ---------------- global (FFT) mixer, LGT.py:149-180 ----------------
struct FftArgs {
    const float* g;   // [B,ch,n,n] planar, LayerNorm-ed global half
    float* o;         // [B,ch,n,n] planar: abs(irfft2(...))
    float* amp;       // optional save [B,ch,n,n/2+1]
    float* pha;       // optional save
    float* sgn;       // optional save: sign of the irfft2 output [B,ch,n,n]
    float* scratch;   // three-launch paths only: half-spectrum scratch [planes][h][w/2+1] complex (FftRoute::scratch_floats per plane)
    const float *ampw, *ampb, *phaw, *phab;  // [ch]
    int planes, ch;
    int unread_[4] = {0, 0, 0, 0};   // no kernel and no launcher reads these (once n, h, w, full: FftRoute holds them now); they keep the kernels' argument layout
    StageSel sg;       // k_fftmix_r only
};
int launch_fftmix(const FftRoute& r, const FftArgs& a, hipStream_t s);   // r: the level's route -- path, plane, grids (route.h)
// what resolve_fft (route.hip) takes from k_fft.hip: columns per workgroup of the column launch of the split / the Bluestein path, planes of height n
int fft_split_cols_per_wg(int n);
int fft_bluestein_lines_per_wg(int n);

// ---------------- local mixer + proj + residual, LGT.py:112-146,183-219,231-248 ----------------
struct AttnArgs {
    const float* x;     // [B,h,w,e]
    const float* o2;    // [B,e/2,h,w] planar global-mixer output
    float* y;           // [B,h,w,e] = x + dropout(proj(cat(attn, o2)))
    const float* posT;  // [2,64,64] transposed pos_emb: posT[h][j][i] = pos[h][i][j]   (k_attn, the vector-pipe kernel)
    const float* pos;   // [2,64,64] pos_emb as stored: pos[h][i][j]                      (k_attn_m, the matrix-pipe kernel)
    const float *ln1g, *ln1b, *qkvw, *qkvb, *projw, *projb;
    int B, h, w;
    int dropout;
    uint64_t seed;
    int bf16;           // k_attn_m: 1 = one round-to-nearest piece per operand (precision = 'bf16'), 0 = fp32-equivalent split arithmetic
    float* save_o = nullptr;         // k_attn_m, e = 16, saving launch (round 6): [P,e/2] attention output before proj (head-major = the local half of cat) and
    float* save_l = nullptr;         // [P,2] log2-domain log-sum-exp of the score rows, for k_attn_bwd_f (which then skips its reduction pass); null: not written
    const float* scales = nullptr;   // k_attn_m: this block's static operand scales { s_y, s_w, s_q, s_k } (k_ffn_prep.hip, round 6): to_qkv and Q K^T on f16 pairs; nullptr: bf16 triples
    StageSel sg;                     // k_attn_m only
};
int launch_attn(int e, const AttnArgs& a, hipStream_t s);     // round 2's kernel: lane = token, every product on the vector pipe (LG_VAR_ATTN_FWD_VALU)
int launch_attn_m(int e, const AttnArgs& a, hipStream_t s);   // round 5: every product on the matrix pipe (k_attn_m.hip)
// posT[blk] for nblk blocks: src pointers via offsets into params
int launch_pos_transpose_n(int n, const float* const* pos, float* const* posT, hipStream_t s);   // n <= 5 * LG_MAX_K tables in one launch

// ---------------- feed_forward, LGT.py:91-109 ----------------
struct Ffn1Args {
    const float* x;  // [P, e]   (P = B*h*w)
    void* a1s;       // optional save [P,4e]: gelu(h1)        (conv input of W2 for its weight gradient)
    void* g1s;       // optional save [P,4e]: gelu'(h1)       (backward never re-evaluates GELU)
    void* h2;        // [P,4e] = W2 gelu(W1 LN(x) + b1) + b2
    int hbf;         // hidden storage: 0 fp32, 1 bf16 (hstore.h)
    int kernel;      // host only: the FfnFwdKernel of the block's route (route.h); launch_ffn_fused switches on it
    const float *ln2g, *ln2b, *w1, *b1, *w2, *b2;
    long P;
    void* wsplit;    // workspace scratch for pre-split weight fragments (ffn_wsplit_bytes; k_ffn_x32.hip), or nullptr
    int wsplit_ready = 0;   // 1: the fragments are in `wsplit` already (prep launch of the forward call: launch_split_w_jobs); 0: the launcher splits in front of its kernel
    const float* scales;   // this block's operand scales { s_x, s_a1, s_a3, s_w1, s_w2, s_w3 } (k_ffn_prep.hip): the f16-pair arithmetic (NP = 2) of the
                           // fused forward kernels; nullptr = the three-piece bf16 arithmetic (NP = 3)
    StageSel sg;           // k_ffn_xr / k_ffn_x32 only (covers the Ffn2Args of the same launch too)
};
// operand scales of the f16-pair FFN arithmetic: one job per block, all in one launch (k_ffn_prep.hip); out[job][8]
struct FfnPrepJob { const float *ln2g, *ln2b, *w1, *b1, *w2, *b2, *dww, *dwb, *w3; int e; const float *ln1g, *ln1b, *qkvw, *qkvb; };   // ln1 / qkv: the local mixer's static scales (attn_out)
#define LG_MAX_FFN_PREP_JOBS 40
struct FfnPrepTable { FfnPrepJob j[LG_MAX_FFN_PREP_JOBS]; };
int launch_ffn_scales(int n, const FfnPrepJob* jobs, float* out, hipStream_t s, float* attn_out = nullptr);   // attn_out[job][4] = { s_y, s_w, s_q, s_k } (nullptr: not computed)
// pre-split weight fragments of the e >= 32 FFN blocks: one job per block, all blocks of a forward call in ONE launch (k_ffn_x32.hip)
struct SplitWJob { const float *w1, *w2, *w3, *scales; void* out; int e, np; };
struct SplitWTable { SplitWJob j[LG_MAX_FFN_PREP_JOBS]; };
int launch_split_w_jobs(int n, const SplitWJob* jobs, hipStream_t s);
int launch_ffn1(int e, const Ffn1Args& a, hipStream_t s);   // k_ffn1 + k_ffn2 (FFN_FWD_UNFUSED): e = 64, fp32 storage
struct Ffn2Args {
    const void* h2;   // [B,h,w,4e]
    const float* x;   // [B,h,w,e] residual input
    void* a3s;        // optional save [B,h,w,4e]: gelu(h3)
    void* g3s;        // optional save [B,h,w,4e]: gelu'(h3)
    int hbf;          // hidden storage: 0 fp32, 1 bf16
    float* y;         // [B,h,w,e]
    float* g;         // optional [B,e/2,h,w] LN1(next block)(y) global half
    const float *dww, *dwb, *w3, *b3, *n1g, *n1b;
    int B, h, w;
};
int launch_ffn2(int e, const Ffn2Args& a, hipStream_t s);
// fused feed_forward half-block (h2 stays in LDS): runs a1.kernel; -2 when the save pointers are not the ones that kernel writes
int launch_ffn_fused(int e, const Ffn1Args& a1, const Ffn2Args& a2, hipStream_t s);
int launch_ffn_xs(const Ffn1Args& a1, const Ffn2Args& a2, hipStream_t s);   // e = 16, fp32 storage (k_ffn_x.hip)
int launch_ffn_xr(const Ffn1Args& a1, const Ffn2Args& a2, hipStream_t s);   // e = 16, f16 pairs, fp32 storage: the register chain (k_ffn_xr.hip, round 6)
int launch_ffn_x32(const Ffn1Args& a1, const Ffn2Args& a2, hipStream_t s);  // e = 32, fp32 storage (k_ffn_x32.hip)
size_t ffn_wsplit_bytes(int e);   // bytes of a1.wsplit for hidden width 4e
// pre-split weight fragments: np = 3 three bf16 pieces, np = 1 one RNE bf16 piece, np = 2 f16 pairs of W * scales[3 + which matrix] (k_ffn_prep.hip)
int launch_split_w(const float* w1, const float* w2, const float* w3, void* out, int e, int np, hipStream_t s, const float* scales = nullptr);
int launch_ffn_x64(const Ffn1Args& a1, const Ffn2Args& a2, hipStream_t s);  // e = 64: two kernels (h2 through HBM), split-bf16 GEMMs (k_ffn_x64.hip)

// test helper: g[B,e/2,HW] = LayerNorm(x)[..., e/2:] (the epilogue the producing kernels fuse)
int launch_ln_split(int e, const float* x, const float* n1g, const float* n1b, float* g, int B, int HW, hipStream_t s);
