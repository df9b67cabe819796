/*
 * lgteun_hip.h -- C ABI of the MI355X-native (gfx950) LGTEUN unfolding hot path.
 *
 * The reference (lms-07/LGTEUN) has no FFI: its hot path is a Python nn.Module,
 *   Pansharpening.forward            models/unlg_former.py:50-67
 *   LGT.forward and its sub-modules  models/common/LGT.py:64-344
 *   sampling_/dep_conv/point_conv    models/common/basic_module_unformer_v2.py:13-53
 *   L1 loss + Adam + StepLR          models/unlg_former.py:87-113, models/base/base_model.py:116-147
 * This library replaces the ATen op sequences behind those lines.  It is bound from Python with
 * ctypes (lgteun_amd/_lib.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked host.
 *  - the caller (PyTorch) owns all memory: parameters, gradients, optimizer state, workspace -- with ONE exception, the
 *    reduce-image cache below.  Plans are immutable after creation.
 *  - all work of a call -- kernels and copies -- is enqueued on `stream` (a hipStream_t passed as void*), and the call returns without
 *    waiting for the device, EXCEPT the two cases listed under "may synchronise" below.  tests/test_gpu_streams.py holds every entry to
 *    this: called on a stream that is still asleep, it must return at once and read inputs that arrive on that stream later.
 *  - calls on different streams, or from different host threads, do not interact as long as they share no buffer: a workspace, a
 *    gradient buffer or a loss scalar belongs to one stream at a time (tests/test_gpu_streams.py, test_gpu_threads.py: bitwise the
 *    results of each call sequence run alone).  lg_last_error is per thread.  The library's mutable process-global state, all of it:
 *      (a) per-device once-bits (one 64-bit mask per kernel family, indexed by hipGetDevice() & 63, so devices 64 apart share a bit):
 *          "dynamic-LDS attribute set" and "twiddles uploaded", and a per-device cache of the compute-unit count.  A race between
 *          threads only repeats an idempotent call.
 *      (b) __constant__ c_tw512, the 256 twiddles of the radix-2 FFT paths: written once per device by a hipMemcpyToSymbol at the first
 *          FFT-mixer launch there, read-only afterwards.
 *      (c) 64 fp64 accumulator slots in device memory (a __device__ array of the code object, per device) and one process-wide
 *          round-robin counter: lg_l2_loss launch number n uses slot n mod 64 and hands it back zeroed.  Two lg_l2_loss launches
 *          collide only if 64 or more were issued -- on any streams, threads and devices of the process -- between them while the
 *          first had not finished: keep fewer than 64 lg_l2_loss launches pending.
 *      (d) the reduce-image cache of lgteun_backward / lg_op_*_bwd (default variant: LG_VAR_REDUCE_PER_BLOCK clear): per device 16
 *          job tables (630 KB) that the LIBRARY allocates with hipMalloc at the first backward on that device and never frees, with
 *          host copies, behind one process-wide mutex.  A table is the list of gradient reductions of one launch and is found again by
 *          content; the content is a function of (plan, B, flags, the workspace pointer, the gradient-buffer pointer) and, for a
 *          per-op entry, of its stage, block and piece.
 *      (e) process-wide atomic counters of the reduce queue (a debug export reads them) and the mutex-protected event table of the
 *          opt-in timing facility (lg_prof_*; off by default).
 *    Host-side staging of a call (the reduce queue, its job table) is thread_local.
 *  - a call may synchronise, and only then:
 *      1. FIRST USE PER DEVICE of a kernel family: hipFuncSetAttribute, the twiddle upload (b), the hipMalloc of (d).  These may wait
 *         for work pending on the device.  Warm every entry you use once per device (any shape of the same C) before relying on 2.
 *      2. a backward whose job table is NOT in the cache (d) -- a new combination of (plan, B, flags, workspace pointer, gradient
 *         pointer), or one evicted by 16 newer ones (slots are reused in the order they were filled) -- drains the WHOLE DEVICE
 *         (hipDeviceSynchronize), uploads the table on `stream` and waits for `stream`.  A training loop that keeps its workspace and
 *         gradient buffer (Engine.train_step does) misses twice, in its first step, and never again; a caller whose buffers move from
 *         step to step pays a device drain in every backward.  Results are the same either way.
 *    Everything else -- every forward, loss, optimizer, metric, classical, data-preparation and scene entry, and a backward whose
 *    table is cached -- allocates nothing and synchronises nothing.
 *  - arguments are validated before any HIP call; a rejected call launches and writes nothing.  The network entries' ranges -- the batch bound, the
 *    alignment of tensors and workspace, the flag bits each entry takes -- stand at lg_workspace_bytes below (tests/test_net_abi_cpu.py,
 *    tests/test_gpu_net_limits.py); the entries around the network state theirs in their own blocks (tests/test_abi_limits_cpu.py, test_gpu_abi_limits.py).
 *  - return value: 0 ok; <0 invalid argument / unsupported shape (see lg_last_error());
 *    >0 a hipError_t.  Nothing throws across the boundary.
 *  - parameters live in ONE flat fp32 buffer; `offsets[i]` (in floats) locates the i-th tensor of
 *    Pansharpening.state_dict() in its canonical order (12 shared, K eta, 119 per stage;
 *    SURVEY.md section 8b).  Gradients use the same offsets in a second flat buffer.
 *  - module I/O is NCHW fp32 like the reference: ms [B,C,h,w], pan [B,1,4h,4w], out [B,C,4h,4w].
 */
#ifndef LGTEUN_HIP_H
#define LGTEUN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_TENSORS_SHARED 12
#define LG_TENSORS_PER_STAGE 119

/* flags for lgteun_forward */
#define LG_FLAG_FAITHFUL 1 /* run every stage's LGT like the reference does (results of stages 0..K-2 are dead) */
#define LG_FLAG_SAVE 2     /* keep what lgteun_backward needs in the workspace */
#define LG_FLAG_DROPOUT 4  /* training-mode Dropout(0.1) after LGMixer.proj (LGT.py:198,215), counter-hash RNG */

/* flags for lgteun_backward: run only a part (lets the caller start the gradient all-reduce of the LGT bucket
 * while the data-step backward still runs).  Neither bit set = both parts. */
#define LG_FLAG_BWD_LGT 8
#define LG_FLAG_BWD_DATA 16

/* forward + backward: the INTENDED unfolding, default off: stage i+1's data step consumes LGT_i's output
 * instead of the data step's own output (the reference feeds `Z`, not `Z_`, forward: unlg_former.py:56-67), so every stage's
 * LGT is live, every parameter gets a gradient, and training keeps one saved activation set per stage
 * (lg_workspace_bytes(..., train = 2)).  Overrides LG_FLAG_FAITHFUL; LG_FLAG_BWD_LGT / _DATA do not apply (the K LGT and
 * data-step backwards interleave) and are rejected. */
#define LG_FLAG_CHAINED 32

/* forward, with LG_FLAG_FAITHFUL: leave the K-1 dead-stage LGT forwards (the reference executes them and discards the
 * result) to a later lgteun_dead_forward call.  They depend on nothing but the data-step outputs, so a training step can enqueue them
 * on a second stream BEHIND the LGT backward (they reuse the LGT activation buffers) and beside the K data-step backwards + Adam --
 * a chain of ~40 small latency-bound launches that leaves most of the GPU idle.  Same kernels, same work, same results. */
#define LG_FLAG_DEFER_DEAD 64

/* forward / dead_forward, with LG_FLAG_FAITHFUL: run the K-1 dead-stage LGT forwards ONE BY ONE (in lgteun_forward each behind its data step),
 * as the library did before it had the batched pass.  Default (bit clear), for a plan with two or more dead stages whose route's forward kernels can take the
 * samples of several stages in one launch (C = 4, planes up to 128 x 128): the K data steps first, then the dead stages as ONE pass over
 * (K-1) B samples -- every kernel launched once, each workgroup choosing its stage's weights by its sample -- then the live stage.  Same work,
 * same arithmetic, bitwise the same results; other plans run one by one whatever the bit says. */
#define LG_FLAG_STAGEWISE 128

/* forward, with LG_FLAG_FAITHFUL on a plan that runs its dead stages as one pass (and neither LG_FLAG_STAGEWISE nor LG_FLAG_DEFER_DEAD): keep the
 * dead pass and the live stage's pass APART, one after the other, as the library ran them before the live stage rode along.  Default (bit clear):
 * the plane and pixel kernels -- patch embedding, FFT mixer, down, up + fusion, tail -- launch ONCE over all K B samples, stages 0 .. K-2 dead and
 * stage K-1 live (it alone saves for the backward, and its output goes to `out`); the persistent local-mixer and FFN kernels still launch twice,
 * non-saving over the (K-1) B dead samples and saving over the live B.  At C = 4, B = 32, 128 x 128 the level-0 FFT mixer then runs 1 024 planes in
 * two full rounds of the chip instead of 768 in one and a half plus 256 at one plane per CU.  Same work, same arithmetic, bitwise the same results.
 * Such a plan keeps the transient forward buffers of K stages of B samples side by side: dead stage i in slot i, the live stage ALWAYS in slot K-1,
 * whichever of these paths ran it; lgteun_backward reads it there.  (Other plans -- K = 2, C = 8, chained training -- have one slot, as before.) */
#define LG_FLAG_LIVE_APART 256

/* kernel ids for the live HIP-event timing facility (lg_prof_*) */
enum lg_kernel_id {
    LG_K_NONE = 0, LG_K_FFN1, LG_K_FFN2, LG_K_FFT, LG_K_ATTN, LG_K_UPFUSE, LG_K_DOWN, LG_K_EMBED, LG_K_TAIL, LG_K_DATASTEP,
    LG_K_FFN1_BWD, LG_K_FFN2_BWD, LG_K_FFT_BWD, LG_K_ATTN_BWD, LG_K_WGRAD, LG_K_BATCH, LG_K_SCENE_GATHER, LG_K_SCENE_BLEND, LG_K_COUNT
};

typedef struct lg_config {
    int32_t C;       /* MS bands: 4 or 8                      (cfg.ms_chans, unlg_former.py:24) */
    int32_t K;       /* unfolding stages                      (stage kwarg, unlg_former.py:22)  */
    int32_t H, W;    /* PAN size = 4 x MS size: multiples of 16, 16..1024 (LGT.py needs 8-px windows at both levels).  Square powers
                      * of two up to 512 take the radix-2 FFT paths (plane in LDS up to 128, split above); everything else
                      * (400x400 full-resolution scenes, rectangles) the Bluestein path -- same results, slower mixer */
    int32_t precision; /* 0 = fp32 storage/compute (parity mode); 1 = bf16 storage of FFN hidden tensors */
    uint32_t variant;  /* 0 = the product path.  LG_VAR_* bits select A/B kernels that compute the SAME function (tests compare them with
                        * the default; the library itself reads no environment variable).  Words the library does not carry are rejected. */
} lg_config;

/* lg_config.variant: A/B switches (all default off).  lg_plan_create resolves them, with precision, C and the plane sizes, into the plan's
 * kernel routes in ONE function (lgteun_amd/csrc/route.hip: lg_resolve_route; the table of bit -> LG_* environment name -> effect is
 * there); lg_plan_describe shows the result. */
#define LG_VAR_FFN_IMPL_MASK 3u   /* fused FFN forward: 0 = split-bf16 kernels; 1 = the exact f32-MFMA strip kernel (v_mfma_f32_16x16x4_f32: bit
                                   * for bit an fp32 fma chain -- the yardstick of the arithmetic-criterion test), precision = 0 only;
                                   * 2 and 3 name nothing: lg_plan_create rejects them */
#define LG_VAR_FFN_STRIP 1u
#define LG_VAR_FFN_SAVE_MASK (3u << 2) /* what the live stage's e = 16 FFN keeps for the backward: 0 = h2, h3 (default); 1 = h1, h2, h3; 2 = the
                                        * five-tensor GELU-free form */
#define LG_VAR_FFN_SAVE3 (1u << 2)
#define LG_VAR_FFN_SAVE5 (2u << 2)
#define LG_VAR_FFN_BWD32_PAIR (1u << 4) /* e = 32 FFN backward, pixelwise half: round 2's k_ffn1_bwd_x32 + two weight-gradient launches instead of k_ffn1_bwd_xs<32> */
#define LG_VAR_FFN_DWBWD_TILE (1u << 5) /* e = 16 FFN backward, spatial half: round 2's tile kernel + weight-gradient launch */
#define LG_VAR_ATTN_BWD_R3 (1u << 6)    /* e = 16 local-mixer backward: round 3's three-kernel form instead of k_attn_bwd_f */
#define LG_VAR_DSTEP_TILES (1u << 7)    /* data step: the tile kernels (four launches forward, nine backward) also where the one-launch form exists */
#define LG_VAR_ATTN_FWD_VALU (1u << 8)  /* local-mixer forward: round 2's vector-pipe kernel k_attn (lane = token, fp32 FMAs) instead of the matrix-pipe k_attn_m */
#define LG_VAR_FFN_BF16X3 (1u << 9)     /* fused FFN forward: round 2's three-piece bf16 split (six products) instead of the f16 pairs (three products) */
#define LG_VAR_FFT_FULL (1u << 10)     /* global mixer on planes up to 128 x 128: round 1-4's complex-row in-LDS kernels k_fftmix / k_fftmix_bwd instead of the real-input k_fftmix_r / k_fftmix_bwd_r */
#define LG_VAR_FFN_BWD_BF16X3 (1u << 11) /* FFN backward (k_ffn1_bwd_xs): three bf16 pieces / six products (rounds 3 - 4) instead of f16 pairs / three products with scaled operands */
#define LG_VAR_ATTN_BWD_CORE_M (1u << 12) /* e = 32 local-mixer backward core: the matrix-pipe k_attn_bwd_core_m (round 5; same results, not faster yet: DESIGN.md 3.3) instead of the vector-pipe k_attn_bwd_core */
#define LG_VAR_FFN_XS (1u << 13)        /* fused FFN forward at e = 16: the channel-split k_ffn_xs of rounds 2 - 5 (LN(x) / gelu(h1) pieces through LDS, eleven barriers per step) instead of the register-chain k_ffn_xr (round 6) */
#define LG_VAR_ATTN_BF16X3 (1u << 14)  /* local-mixer forward (k_attn_m): to_qkv and Q K^T on three bf16 pieces / six products (round 5) instead of f16 pairs with static operand scales (round 6) */
#define LG_VAR_FFN_H3_RECOMPUTE (1u << 15)  /* e = 16 FFN of the live stage: save h2 ONLY and re-compute h3 in the backward (k_ffn_dw_bwd_h, round 6: the saving forward launch -17 us, the backward kernel +70 us: opt-in) instead of saving h2 and h3 (k_ffn_dw_bwd_xs) */
#define LG_VAR_ATTN_BWD_RESTATS (1u << 16)  /* e = 16 local mixer of the live stage: k_attn_bwd_f re-derives the softmax row statistics and the attention output with a reduction pass of its own (rounds 4 - 5) instead of reading what k_attn_m's saving launch left (round 6: log-sum-exp + attention output, 40 bytes per pixel) */
#define LG_VAR_REDUCE_PER_BLOCK (1u << 17)  /* parameter-gradient reductions of a backward pass: one launch per LGT block and per data step, job table as a kernel argument (rounds 2 - 6: nine launches per c2 step) instead of one launch for the LGT and one for the K data steps with the table in device memory; bitwise the same gradients */
#define LG_VAR_ALL 0x3ffffu

typedef struct lg_plan lg_plan; /* host-side, immutable after creation */

const char* lg_version(void);
/* Bumped whenever a struct layout, an argument meaning or a caller-provided buffer size changes (2: lg_config.variant, the data step's
 * tmp of 3*B*C*H*W/4 + B*H*W floats).  Additions keep it: lg_op_lgt_stages, lg_workspace_deadout, LG_FLAG_STAGEWISE, LG_FLAG_LIVE_APART, the lg_debug_stage_* entries and lg_debug_live_slot and the classical baselines (lg_classical_workspace_bytes, lg_interp23_up4, lg_sfim, lg_gsa, then lg_wavelet, lg_wavelet_taps, then lg_mtfglp_workspace_bytes, lg_mtf_glp, then lg_bdsd_workspace_bytes, lg_bdsd, then lg_atrous_workspace_bytes, lg_atrous, lg_atrous_taps with their own new struct lg_atrous_args, then lg_mtf_hr_workspace_bytes, lg_mtf_hr with their own new struct lg_mtf_hr_args) came without a bump (no existing struct,
 * argument or caller-sized buffer changed: workspaces are sized by lg_workspace_bytes, which grew for the plans that batch their dead stages).  A binding checks it at load time -- lgteun_amd/_lib.py does -- instead of passing a stale struct. */
#define LG_ABI_VERSION 2
int32_t lg_abi_version(void);
const char* lg_last_error(void); /* thread-local, host string */

/* offsets: host array of n_offsets = 12 + K + 119*K int64 (float offsets into the flat parameter buffer). */
int lg_plan_create(const lg_config* cfg, const int64_t* offsets, int32_t n_offsets, lg_plan** out);
void lg_plan_destroy(lg_plan* plan);
/* The kernel routes the plan resolved from its configuration, as a short stable text in the HOST buffer buf[n]: one "net" line, then per level
 * (L0: e = 4C at H x W, L1: e = 8C at H/2 x W/2) a line for the plain forward, the LG_FLAG_SAVE forward (with the save slots it writes) and
 * the backward (with the slots it reads).  -3 when n is too small (1 KiB is enough). */
int lg_plan_describe(const lg_plan* plan, char* buf, size_t n);
/* bytes of workspace lgteun_forward/backward need for batch B: train = 0 forward only, 1 = forward with LG_FLAG_SAVE + backward,
 * 2 = the same with LG_FLAG_CHAINED (K saved activation sets).
 * A plan that runs its dead stages as one pass (C = 4, K >= 3, planes up to 128 x 128; LG_FLAG_STAGEWISE above) keeps the transient LGT forward
 * buffers of K stages side by side, train = 0 and 1 alike (LG_FLAG_LIVE_APART above): C = 4, K = 4, 128 x 128, B = 32 needs 2 263 MiB (train = 0) /
 * 6 482 MiB (train = 1), 512 MiB more than with K - 1 slots.  Saved tensors stay B-sized; K = 2, C = 8 and train = 2 sizes are unchanged.
 * The workspace contract of every entry that takes one (lgteun_forward / _backward / _dead_forward, lg_op_*), pinned bit for bit by
 * tests/test_gpu_workspace_contract.py:
 *  - what the workspace holds ON ENTRY is arbitrary -- zeros, NaNs, huge values, what an earlier call on other inputs left: every region is
 *    written in a call before that call reads it, and results do not depend on it.  It holds data only (floats, bf16, keep-bit words), never an
 *    index or a pointer.  It is 256-byte aligned (the entries check it); bytes beyond lg_workspace_bytes are not written and change nothing.
 *  - a call with workspace_bytes below lg_workspace_bytes, or a null workspace, returns an error and launches nothing.
 *  - between a forward with LG_FLAG_SAVE and its backward (same plan, B, flags, seed, pointer) the WHOLE workspace must stay untouched: the
 *    saved activation set(s), the data steps' intermediates and the per-block tables of that forward live there.  Nothing else has to survive
 *    from one call to the next.
 *
 * The network entries' argument contract -- lgteun_forward / _backward / _dead_forward, lg_op_resample, lg_op_data_step, lg_op_lgt, lg_op_lgt_stages,
 * lg_op_block, lg_op_block_bwd, lg_op_data_step_bwd, lg_op_lgt_bwd, lg_l1_loss, lg_l2_loss, lg_adam_step, lg_optim_step(_ex) and lg_dropout_mask --
 * held by tests/test_net_abi_cpu.py (every argument one step outside its range, on the host) and tests/test_gpu_net_limits.py (the accepted side at
 * the bound, on the device).  Arguments are validated before any HIP call, by one shared helper (lgteun_amd/csrc/net_args.h), and lg_last_error
 * names the entry and the offending argument; a rejected call launches and writes nothing.  -1: null or out of range, -2: unsupported (a defined
 * flag that does not apply, a shape the plan cannot run), -3: workspace too small.
 *  - batch: 1 <= B <= B_max(C, K, H, W, train) = min( floor(65535 / C), floor((2^31 - 1) / (S * 16 * C * H * W)) ), with S = K if C = 4, K >= 3,
 *    H <= 128, W <= 128 and train != 2 (the plans that may run the samples of K stages in one launch), else S = 1.  The first term keeps the B C
 *    planes of the data step inside a grid's y / z dimension (65535); the second keeps every element index of the largest tensor a launch addresses,
 *    the FFN's hidden [S B, H, W, 16 C], in a signed 32-bit int.  16 x 16: 16383 (C = 4) / 8191 (C = 8); C = 4, K = 4, 128 x 128: 511; 1024 x 1024:
 *    31 / 15.  The derivation, site by site, is the comment of lg_net_max_batch in lgteun_amd/csrc/api.hip.  lg_workspace_bytes returns 0 outside the range.
 *    lg_op_resample: 1 <= planes, hi, wi and hi * wi < 2^27 (the plane count is in no grid dimension; taps are indexed in int inside a plane).
 *    lg_adam_step / lg_optim_step(_ex): 1 <= n_ranges <= 65535 (a grid's y).  lg_l1_loss / lg_l2_loss / lg_dropout_mask index in 64 bits: any n.
 *  - alignment: every float tensor (params, grads, inputs, outputs, tmp, the optimizer's state buffers, lg_dropout_mask's out) 16 bytes, `ranges`
 *    8 bytes, loss_accum / clip_coef / ema 4 bytes.  The network and loss kernels read and write float4 and need it; the optimizer kernels and
 *    k_dropout_mask index element by element and would take any float -- for them the rule is the uniform contract, not a kernel's need.  The workspace 256 bytes: carve() places every region at a multiple of 256
 *    bytes from its base and the kernels rely on the regions' alignment, not on the base's.
 *  - flags: a bit the header does not define (bit 9 and up) is rejected by every entry.  lgteun_forward and lgteun_dead_forward take every defined
 *    bit but LG_FLAG_BWD_LGT / LG_FLAG_BWD_DATA (dead_forward also needs LG_FLAG_FAITHFUL without LG_FLAG_CHAINED); lgteun_backward takes every
 *    defined bit, LG_FLAG_BWD_* not together with LG_FLAG_CHAINED; lg_op_lgt takes LG_FLAG_SAVE and LG_FLAG_DROPOUT; lg_op_lgt_stages and lg_op_lgt_bwd
 *    LG_FLAG_DROPOUT alone.
 *  - stage in 0 .. K-1 (lg_dropout_mask: 0 .. 15), blk in 0 .. 4, which in 0 .. 2, n in 1 .. K - stage0, grid_cap >= 0. */
size_t lg_workspace_bytes(const lg_plan* plan, int32_t B, int32_t train);

/* Pansharpening.forward (unlg_former.py:50-67).  seed: dropout counter seed (used with LG_FLAG_DROPOUT). */
int lgteun_forward(const lg_plan* plan, const float* params, const float* ms, const float* pan, float* out,
                   void* workspace, size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream);

/* The dead-stage LGT forwards a forward with LG_FLAG_FAITHFUL | LG_FLAG_DEFER_DEAD left out (unlg_former.py:63-67 for stages
 * 0..K-2): same workspace, B, flags and seed as that forward.  Overwrites the LGT activation set, so it must be ordered behind the
 * LGT part of lgteun_backward (LG_FLAG_BWD_LGT) and before the next forward on the workspace; reads only dead-stage parameters
 * (Adam never touches those) and the data-step outputs. */
int lgteun_dead_forward(const lg_plan* plan, const float* params, void* workspace, size_t workspace_bytes, int32_t B, int32_t flags,
                        uint64_t seed, void* stream);

/* Backward of the same graph (autograd of unlg_former.py:50-67): needs the workspace of a forward run
 * with LG_FLAG_SAVE.  dout [B,C,H,W].  Accumulates (+=) into `grads` for the live tensors only
 * (shared D/DT/R/RT, eta, last stage's LGT); dead-stage slots are never written.
 * A backward reads the saved forward and leaves it as it found it, so it MAY run more than once per forward (autograd's retain_graph): every
 * run gives the bits of a fresh forward + backward with its dout (the one word a backward accumulates in the forward's tables, max |dh2| in
 * ffn_scales, is reset by the backward itself).  Not behind lgteun_dead_forward, which overwrites the activation set (above). */
int lgteun_backward(const lg_plan* plan, const float* params, float* grads, const float* ms, const float* pan,
                    const float* dout, void* workspace, size_t workspace_bytes, int32_t B, int32_t flags,
                    uint64_t seed, void* stream);

/* nn.L1Loss(mean) forward+backward (losses.py:19-40; unlg_former.py:99-104): loss_sum[0] += sum|out-gt|/N and
 * dout = sign(out-gt) * scale / N.   N = number of elements of the GLOBAL batch (DDP: pass n_global). */
int lg_l1_loss(const float* out, const float* gt, float* dout, float* loss_accum, int64_t n_local, int64_t n_global,
               float scale, void* stream);

/* torch.optim.Adam step (base_model.py:123-124; no weight decay / amsgrad) over [begin,end) float ranges of the
 * flat buffers.  ranges: DEVICE int64 pairs, n_ranges of them (the live tensors).  step is 1-based. */
int lg_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* ranges,
                 int32_t n_ranges, int64_t max_range, int32_t step, float lr, float beta1, float beta2, float eps,
                 float grad_scale, void* stream);

/* nn.MSELoss(mean) forward+backward (losses.py:19-40 with type 'l2'; unlg_former.py:99-104): the contract of lg_l1_loss with
 * loss_accum[0] += sum (out-gt)^2 / N and dout = 2 (out-gt) * scale / N.   N = number of elements of the GLOBAL batch (DDP: pass
 * n_global).  The sum is carried in fp64; loss_accum takes one float add per call.  dout is rounded as torch's MSE backward rounds it:
 * (fl(2 / N) * (out-gt)) * scale. */
int lg_l2_loss(const float* out, const float* gt, float* dout, float* loss_accum, int64_t n_local, int64_t n_global,
               float scale, void* stream);

/* One step of torch.optim's single-tensor Adam / AdamW / SGD / RMSprop (base_model.py:116-135 hands torch's keyword arguments
 * through) over [begin,end) float ranges of the flat buffers, one launch.  ranges: DEVICE int64 pairs as for lg_adam_step; step is
 * 1-based (bias corrections; the SGD momentum buffer of step 1 is the gradient itself).  Hyper-parameters per algorithm:
 *   LG_OPT_ADAM, LG_OPT_ADAMW  h0 = beta1, h1 = beta2; flag LG_OPT_AMSGRAD; weight_decay is L2 (Adam) or decoupled (AdamW)
 *                              state0 = exp_avg, state1 = exp_avg_sq, state2 = max_exp_avg_sq (amsgrad only)
 *   LG_OPT_SGD                 h0 = momentum, h1 = dampening; flag LG_OPT_NESTEROV; state0 = momentum buffer (momentum != 0 only)
 *   LG_OPT_RMSPROP             h0 = alpha, h1 = momentum; flag LG_OPT_CENTERED; eps is added after the square root
 *                              state0 = square_avg, state1 = momentum buffer (momentum > 0 only), state2 = grad_avg (centered only)
 * State buffers are caller-owned fp32 buffers laid out like params; those an option set does not use may be NULL.
 * Gradients are read as grads * grad_scale.  The scalars are fp64, as torch holds them: 1 - beta, lr / bias_correction1 and 1 - lr *
 * weight_decay are taken in fp64 and rounded to fp32 once.  Every op of torch's multi-tensor form is one rounding step of the kernel, so a
 * step fed the same gradients gives the bits torch's device kernels give. */
#define LG_OPT_ADAM 0
#define LG_OPT_ADAMW 1
#define LG_OPT_SGD 2
#define LG_OPT_RMSPROP 3
#define LG_OPT_AMSGRAD 1
#define LG_OPT_NESTEROV 2
#define LG_OPT_CENTERED 4
int lg_optim_step(float* params, const float* grads, float* state0, float* state1, float* state2, const int64_t* ranges,
                  int32_t n_ranges, int64_t max_range, int32_t step, int32_t algo, int32_t flags, double lr, double h0, double h1,
                  double eps, double weight_decay, double grad_scale, void* stream);

/* L2 norm of `grads` over [begin,end) float ranges (DEVICE int64 pairs, as for lg_optim_step) and the clip coefficient of
 * torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False), both left in device memory:
 *   out[0] = (float)sqrt(sum of squares), squares and sum carried in fp64;
 *   out[1] = min(1, (float)max_norm / (out[0] + 1e-6f)) in fp32, with torch.clamp's handling of a NaN (it stays a NaN).
 * Non-finite gradients propagate as torch's do: an infinite norm gives the coefficient 0, a NaN gives NaN.  Two launches: one fp64 partial
 * per workgroup into `workspace`, then a fixed-order finishing pass -- no floating-point atomics, so the same call gives the same bits.
 * Nothing outside the ranges is read; a range may begin and end at any float offset and be of any length.  workspace: 8-byte aligned,
 * lg_grad_norm_workspace_bytes(n_ranges, max_range) bytes (0 for arguments lg_grad_norm rejects); its content need not survive the call. */
size_t lg_grad_norm_workspace_bytes(int32_t n_ranges, int64_t max_range);
int lg_grad_norm(const float* grads, const int64_t* ranges, int32_t n_ranges, int64_t max_range, double max_norm, float* out,
                 void* workspace, size_t workspace_bytes, void* stream);

/* lg_optim_step with the controls of a train step, still ONE launch.  With clip_coef == NULL, ema == NULL and plain_adam == 0 it is
 * lg_optim_step, bit for bit.
 *   clip_coef   DEVICE pointer or NULL (out + 1 of lg_grad_norm): gradients are read as fl(fl(grads * grad_scale) * *clip_coef), the
 *               rounding `g.mul_(clip_coef)` in front of torch's optimizer gives.  No host synchronisation: the kernel loads it.
 *   ema         NULL, or an fp32 buffer laid out like params: behind the parameter update, every element of the ranges takes
 *               ema = fma(1 - ema_decay, p_new - ema, ema) with 1 - ema_decay taken in fp64 and rounded once -- torch._foreach_lerp_(ema,
 *               params, 1 - ema_decay), which has this form for a weight below 0.5: ema_decay must lie in (0.5, 1).  Elements outside the
 *               ranges are neither read nor written.
 *   plain_adam  1: the arithmetic of lg_adam_step (algo LG_OPT_ADAM, weight_decay 0, no flag; state0 = exp_avg, state1 = exp_avg_sq;
 *               lr, h0, h1, eps and grad_scale rounded to fp32 first, as that entry point takes them) extended the same way, so that
 *               switching a control on does not move a plain-Adam run onto lg_optim_step's bits.  0: lg_optim_step's. */
int lg_optim_step_ex(float* params, const float* grads, float* state0, float* state1, float* state2, const int64_t* ranges,
                     int32_t n_ranges, int64_t max_range, int32_t step, int32_t algo, int32_t flags, double lr, double h0, double h1,
                     double eps, double weight_decay, double grad_scale, const float* clip_coef, float* ema, double ema_decay,
                     int32_t plain_adam, void* stream);

/* Live per-kernel timing: when enabled for `kernel_id`, every launch of that kernel is bracketed by hipEvents recorded on
 * the stream it is launched on.  lg_prof_read synchronises on the recorded events and returns the summed device time (ms)
 * and the number of launches since lg_prof_enable / lg_prof_reset -- counted in launches of ONE stage's samples: a launch over the samples
 * of S dead stages (LG_FLAG_STAGEWISE clear) counts S, so time / launches stays the time per stage-sized launch.  Host-side event objects are the only thing the library
 * ever creates; lg_prof_disable destroys them. */
int lg_prof_enable(int32_t kernel_id, int32_t max_launches);
int lg_prof_reset(void);
void lg_prof_pause(int32_t paused);   /* 1: launches are neither timed nor counted until lg_prof_pause(0) (sampling: an event pair costs ~2 us of stream time) */
int lg_prof_read(double* total_ms, int64_t* launches);
void lg_prof_disable(void);
const char* lg_kernel_name(int32_t kernel_id);

/* The dropout the LGMixers apply in train mode (nn.Dropout(0.1) behind proj, LGT.py:197-198,215): out[i] = 0 or 1/0.9 = the factor of
 * element i (= pixel * e + channel, NHWC) of block `blk` of stage `stage` under `seed` -- a counter hash, so forward and backward draw the
 * same mask without storing it, and an integrator can reproduce it.  n elements from index `first`; out is a device pointer. */
int lg_dropout_mask(uint64_t seed, int32_t stage, int32_t blk, int64_t first, int64_t n, float* out, void* stream);

/* ---- per-op entry points (unit-tested against the oracle; same kernels the orchestrators launch) ----
 * tests/test_gpu_composition.py holds the orchestrators to them: a network composed by hand from lg_op_resample, lg_op_data_step, lg_op_lgt,
 * lg_op_lgt_bwd and lg_op_data_step_bwd gives the bits of lgteun_forward / lgteun_dead_forward / lgteun_backward, faithful, live and chained. */
/* bmu.sampling_ bicubic (basic_module_unformer_v2.py:21-23): mode 0: x0.5, 1: x2, 2: x4.  x [planes,hi,wi]. */
int lg_op_resample(const float* x, float* y, int32_t planes, int32_t hi, int32_t wi, int32_t mode, void* stream);
/* one data step (unlg_former.py:58-61) for stage `stage`: z_in -> z_out [B,C,H,W]; tmp: 3*B*C*H*W/4 + B*H*W floats (the chain's three
 * intermediates t1 | r | . | s1 in quarters of B*C*H*W/4, then the per-sample plane R Z - pan of the one-launch form). */
int lg_op_data_step(const lg_plan* plan, const float* params, int32_t stage, const float* z_in, const float* ms,
                    const float* pan, float* z_out, float* tmp, int32_t B, void* stream);
/* one LGT forward (LGT.py:314-344) with stage `stage`'s weights: z [B,C,H,W] -> out [B,C,H,W]. */
int lg_op_lgt(const lg_plan* plan, const float* params, int32_t stage, const float* z, float* out, void* workspace,
              size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream);
/* n LGT forwards (LGT.py:314-344) with the weights of stages stage0 .. stage0 + n - 1, as the reference issues them for the stages whose
 * result it discards (unlg_former.py:56-67): z [n,B,C,H,W] -> out [n,B,C,H,W], nothing saved, as ONE pass over n B samples -- every
 * kernel launched once.  n > 1 needs a plan whose dead stages run that way (C = 4, K >= 3, planes up to 128 x 128; n <= K-1) and is an
 * error otherwise.  flags: 0 or LG_FLAG_DROPOUT: stage s's masks are those of lg_op_lgt(stage s) with the same seed.  grid_cap > 0 bounds
 * the grid of the persistent kernels (fused FFN, local mixer), so that a small shape gives a workgroup samples of two stages; 0: no bound.
 * The workspace is that of lg_workspace_bytes(plan, B, 0). */
int lg_op_lgt_stages(const lg_plan* plan, const float* params, int32_t stage0, int32_t n, const float* z, float* out, void* workspace,
                     size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, int32_t grid_cap, void* stream);
/* Where a forward with LG_FLAG_FAITHFUL leaves the discarded LGT outputs inside its workspace (train as for lg_workspace_bytes): stage i's
 * [B,C,H,W] at byte offset *offset + i * *stage_stride.  *stage_stride is 0 for a plan that keeps one slot (every dead stage overwrites the
 * previous one's). */
int lg_workspace_deadout(const lg_plan* plan, int32_t B, int32_t train, size_t* offset, size_t* stage_stride);
/* Debug, host only: where the transient forward buffers lie in the workspace of (plan, B, train), as byte offsets.  out53 = { end offset of the
 * forward carving, bytes of the backward's part behind it (0 for train = 0), first sample of the live stage's slot ((K-1) B for a plan that keeps K
 * slots, else 0), then for each of the five blocks and each of its buffers xin, xmid, xout, g, o2 the pair { offset of slot 0, offset of the live
 * stage's slot } }.  lg_workspace_bytes = out53[0] + out53[1]. */
int lg_debug_live_slot(const lg_plan* plan, int32_t B, int32_t train, size_t* out53);
/* Debug, host only (no device, no launch): the units the workgroups of a persistent multi-stage launch walk, from the functions the kernels call.
 * kind 0: the fused FFN (k_ffn_xr) -- split 0: `units` strips in even runs; split != 0: `units` strip PAIRS, the two workgroups w and w + grid/2
 * on the same run of pairs, the second at strip base `units`.  kind 1: the local mixer (k_attn_m) -- `units` window quads; split = eighths of a
 * CU's chunk to its first workgroup, 4 = even runs.  per_stage: units of one stage.  out: rows of five int32 { workgroup, seg0, seg1, stage,
 * strip base }, one per (workgroup, stage segment) in workgroup order; at most n_out rows are written.  Returns the number of rows, < 0 on error. */
int lg_debug_stage_runs(int32_t kind, int32_t units, int32_t per_stage, int32_t grid, int32_t split, int32_t* out, int32_t n_out);
/* ... and the launchers' decision for n stages of Bs samples on h x w planes under grid_cap (lg_op_lgt_stages).  kind 0: k_ffn_xr, out8 =
 * { uneven, rows shifted dS, units, units per stage, grid, strip height, column tiles, strips per column }; kind 8 / 16: k_attn_m<8|16> with
 * two resident workgroups per CU, out8 = { uneven, eighths, quads, quads per stage, grid, windows, 0, 0 }.  units / split are what
 * lg_debug_stage_runs takes. */
int lg_debug_stage_decision(int32_t kind, int32_t h, int32_t w, int32_t Bs, int32_t n, int32_t grid_cap, int32_t* out8);
/* pieces of one LGB block `blk` (0,1: encoder; 2: bottleneck; 3,4: decoder) of stage `stage`, on NHWC x:
 *  which = 0: global_mixer on LN(x)[..., e/2:]  -> y planar [B,e/2,h,w]        (LGT.py:149-180)
 *          1: x + LGMixer(LN(x))                -> y [B,h,w,e]                 (LGT.py:183-219,231-248)
 *          2: x + feed_forward(LN(x))           -> y [B,h,w,e]                 (LGT.py:91-109)
 *  h,w,e are implied by blk (level 0: H,W,4C; level 1: H/2,W/2,8C). */
int lg_op_block(const lg_plan* plan, const float* params, int32_t stage, int32_t blk, int32_t which, const float* x,
                float* y, void* workspace, size_t workspace_bytes, int32_t B, void* stream);

/* backward of the same pieces (autograd of the lines cited at lg_op_block): runs the half-block forward on x with
 * everything saved, then its backward for upstream gradient dy.  which = 0: dy, dx planar [B,e/2,h,w] (gradient wrt the
 * LayerNorm-ed global half); 1, 2: dy, dx NHWC [B,h,w,e].  Parameter gradients accumulate (+=) into grads.
 * workspace: lg_workspace_bytes(plan, B, 1). */
int lg_op_block_bwd(const lg_plan* plan, const float* params, float* grads, int32_t stage, int32_t blk, int32_t which,
                    const float* x, const float* dy, float* dx, void* workspace, size_t workspace_bytes, int32_t B,
                    void* stream);

/* backward of one data step (autograd of unlg_former.py:58-61 with D :29-30, DT :32-33, R :36, RT :37): runs the step's forward
 * on z_in (to have its intermediates), then maps dz_out (gradient wrt the step's output) to dz_in (gradient wrt z_in, including the
 * identity path) and accumulates (+=) the gradients of D / DT / R / RT and eta[stage] into grads.  workspace:
 * lg_workspace_bytes(plan, B, 1). */
int lg_op_data_step_bwd(const lg_plan* plan, const float* params, float* grads, int32_t stage, const float* z_in, const float* ms,
                        const float* pan, const float* dz_out, float* dz_in, void* workspace, size_t workspace_bytes, int32_t B,
                        void* stream);
/* backward of one LGT (autograd of LGT.py:314-344; covers patch_embedding :64-88, down :280-281, up + fusion :294-295,337-338 and
 * tail :302-303,342 besides the five blocks): runs the LGT forward on z with everything saved, then maps dout to dz (gradient wrt z)
 * and accumulates (+=) the 119 parameter gradients of stage `stage` into grads.  flags: 0 or LG_FLAG_DROPOUT (with seed). */
int lg_op_lgt_bwd(const lg_plan* plan, const float* params, float* grads, int32_t stage, const float* z, const float* dout, float* dz,
                  void* workspace, size_t workspace_bytes, int32_t B, int32_t flags, uint64_t seed, void* stream);

/* ---- evaluation indices of lgteun_amd/metrics.py (reference models/base/metrics.py:22-182, 271-333, 409-425) in fp64 on the device ----
 * Same definitions as the host functions; only the order of summation differs.  Every input element is first multiplied by `scale` in
 * fp32 (2^bit_depth - 0.5 for normalised inputs, as data_denormalize does; 1 for digital numbers), then widened to fp64.  Reductions
 * are per-workgroup partials in the workspace plus a fixed-order pass (no atomics): repeated calls give the same bits, and row b of a
 * batch equals the row of image b scored alone.  Shapes: 1 <= B <= 65535; 2 <= C <= LG_IQA_MAX_BANDS; LG_IQA_SSIM_TAPS (one SSIM window) <= H, W
 * <= 8192; the no-reference indices also need H, W >= LG_IQA_QNR_BLOCK and multiples of LG_IQA_RATIO. */
#define LG_IQA_PEAK 2047.5     /* dynamic range of PSNR / SSIM (11-bit data)          metrics.PEAK */
#define LG_IQA_SSIM_TAPS 11    /* SSIM: Gaussian window taps                          metrics.SSIM_TAPS */
#define LG_IQA_SSIM_SIGMA 1.5  /*       and its sigma                                 metrics.SSIM_SIGMA */
#define LG_IQA_Q_BLOCK 8       /* Q: box window of the reduced-resolution pass        metrics.Q_BLOCK */
#define LG_IQA_RATIO 4         /* ERGAS ratio = PAN / MS resolution                   metrics.ERGAS_RATIO */
#define LG_IQA_QNR_BLOCK 32    /* Q window of D_lambda / D_s                          metrics.QNR_BLOCK */
#define LG_IQA_MTF_TAPS 41     /* PAN low-pass (window-method MTF filter) taps        metrics.MTF_TAPS */
#define LG_IQA_MTF_GAIN 0.15   /*   and its gain at the MS Nyquist frequency          metrics.MTF_GAIN_PAN */
#define LG_IQA_MAX_BANDS 16
/* bytes of workspace a call on [B, C, H, W] images needs (no_ref = 0: lg_iqa_ref, 1: lg_iqa_no_ref); 0 for a shape the indices
 * are not defined for */
size_t lg_iqa_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t no_ref);
/* metrics.ref_evaluate of every image: pred, gt [B,C,H,W] fp32 -> out [B,5] fp64 = PSNR, SSIM, Q, SAM, ERGAS */
int lg_iqa_ref(const float* pred, const float* gt, double* out, int32_t B, int32_t C, int32_t H, int32_t W, float scale,
               void* workspace, size_t workspace_bytes, void* stream);
/* metrics.no_ref_evaluate of every image: pred [B,C,H,W], pan [B,1,H,W], ms [B,C,H/4,W/4] fp32 -> out [B,3] fp64 = D_lambda, D_s, QNR */
int lg_iqa_no_ref(const float* pred, const float* pan, const float* ms, double* out, int32_t B, int32_t C, int32_t H, int32_t W,
                  float scale, void* workspace, size_t workspace_bytes, void* stream);
/* the LG_IQA_MTF_TAPS taps of lg_iqa_no_ref's PAN low-pass into the HOST array out41: metrics.mtf_taps(LG_IQA_MTF_GAIN), the row sums of
 * the reference's 41 x 41 window-method filter (Gaussian frequency samples, inverse DFT, radial Kaiser window with beta 0.5, normalised).
 * Host code: computed once, no device call.  An addition without an ABI bump, like lg_wavelet_taps. */
int lg_iqa_mtf_taps(double* out41);

/* ---- the extended indices (metrics.ref_evaluate_ext / no_ref_evaluate_ext; kernels in lgteun_amd/csrc/k_iqa_ext.hip; definitions:
 * DESIGN.md 3.8.1) ----  The conventions of the block above: every element times `scale` in fp32 first, fp64 after that, per-workgroup partials
 * in the workspace plus a fixed-order pass, no atomics, a partition that depends on the shape only -- repeated calls give the same bits and
 * row b of a batch equals the row of image b scored alone.  Arguments are validated before any HIP call and lg_last_error says why; a rejected
 * call launches and writes nothing.  Shapes: 1 <= B <= 65535; 2 <= C <= LG_IQA_Q2N_MAX_BANDS; LG_IQA_Q2N_BLOCK <= H, W <= 8192.  The workspace is
 * 8-byte aligned; what it held before does not matter.
 *   Q2n  the hypercomplex Q on N = 2, 4 or 8 components (the smallest N >= C; bands C .. N-1 are zero planes), the mean over the non-overlapping
 *        32 x 32 blocks of the image extended to multiples of 32 by mirroring (lines L-1, L-2, ... follow line L-1; rows first).  Per block and
 *        band the ground truth's mean a and deviation c (two passes, n - 1; c = 0 counts as 1) map BOTH images: v -> (v - a) / c + 1.  A block's
 *        sums are one tree of pairwise additions, the one metrics._block_sum restates, so a flat block takes the host's t3 == 0 branch.
 *   SCC  sum FG / sqrt(sum F^2 sum G^2) of the Sobel magnitudes at the (H-2)(W-2) interior pixels of all bands; 1 if both sums of squares are
 *        zero, 0 if exactly one is.
 *   CC   the mean over bands of Pearson's r (centred moments, two passes); NaN if a band of either image is constant (min == max). */
#define LG_IQA_Q2N_BLOCK 32     /* Q2n block side                                     metrics.Q2N_BLOCK */
#define LG_IQA_Q2N_MAX_BANDS 8  /* octonions: Q8                                      metrics.Q2N_MAX_BANDS */
/* bytes of workspace lg_iqa_ref_ext / lg_iqa_q2n need for [B, C, H, W] images; 0 for a shape they reject */
size_t lg_iqa_ext_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
/* pred, gt [B,C,H,W] fp32 -> out [B,3] fp64 = Q2n(gt, pred), SCC, CC: the three columns metrics.ref_evaluate_ext adds to lg_iqa_ref's five */
int lg_iqa_ref_ext(const float* pred, const float* gt, double* out, int32_t B, int32_t C, int32_t H, int32_t W, float scale,
                   void* workspace, size_t workspace_bytes, void* stream);
/* gt, fused [B,C,H,W] fp32 -> out [B] fp64 = Q2n alone (gt's per-block statistics map both images).  D_lambda_K = 1 - Q2n(ms, the fused
 * image low-passed per band by its MTF-matched Gaussian and decimated: lg_fir_decimate4 on fused * scale), composed in device_metrics.py. */
int lg_iqa_q2n(const float* gt, const float* fused, double* out, int32_t B, int32_t C, int32_t H, int32_t W, float scale,
               void* workspace, size_t workspace_bytes, void* stream);

/* ---- the no-reference training loss 1 - QNR and its gradient (Engine.train_step with noref_weight; kernels in lgteun_amd/csrc/k_qnr.hip) ----
 * The reference's QNRLoss (models/base/losses.py:141-153) over D_lambda_torch / D_s_torch / QIndex_torch (models/base/metrics.py:336-397):
 * NOT the 32-pixel-block indices of lg_iqa_no_ref.  out [B,C,H,W] is the fused image, pan [B,1,H,W], ms [B,C,H/4,W/4], pan_l [B,1,H/4,W/4],
 * fp32.  Per sample n and pair (a, b), with E the mean over the sample's pixels,
 *   Q_n(a, b) = 4 cov E[a] E[b] / ((var_a + var_b) (E[a]^2 + E[b]^2) + 1e-8)                                    (metrics.py:347-355)
 * and over the P = C (C - 1) / 2 + C pairs -- the band pairs i < j in row-major order, then the C band-to-PAN pairs -- the table
 *   d[p] = mean_n Q_n,fused[p] - mean_n Q_n,ms[p]   (fused: (out_i, out_j) | (out_i, pan); ms: (ms_i, ms_j) | (ms_i, pan_l)),
 *   D_lambda = mean_{i<j} |d_ij| (:358-376), D_s = mean_i |d_iP| (:379-397), loss = 1 - (1 - D_lambda) (1 - D_s) (losses.py:150-153).
 * The signs of d are known only after the batch mean -- under data parallelism after every rank has contributed -- so the call is split:
 * lg_qnr_stats leaves THIS rank's sums in `table`, the caller SUM-all-reduces the P doubles (or does nothing on one rank), lg_qnr_grad
 * takes the result with B_global = the samples behind it.  All sums are fp64 (the product of two fp32 values is exact there): per-workgroup
 * partials in the workspace and fixed-order finishing passes, no atomics, so the same call gives the same bits every time; the number of
 * workgroups per sample depends on H and W only, so a sample's q row has the same bits alone and inside any batch.
 * Both calls validate their arguments before any HIP call and name the offending one in lg_last_error: C is 4 or 8; H and W are multiples
 * of 4 in 8 .. 65536; 1 <= B <= 65535; float tensors 16-byte aligned, doubles and the workspace 8-byte aligned.  All indexing is 64-bit.  They
 * allocate nothing and synchronise nothing. */
/* bytes of workspace both calls need for [B, C, H, W]; 0 for shapes the calls reject */
size_t lg_qnr_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
/* q [B,2,P] (may be NULL): Q_n of every pair, fused side then MS side; table [P] = sum_n (Q_n,fused[p] - Q_n,ms[p]) over this call's samples,
 * n ascending.  Leaves Q and dQ_fused / d(E[a], E[b], E[aa], E[bb], E[ab]) of every sample in the workspace for lg_qnr_grad. */
int lg_qnr_stats(const float* out, const float* pan, const float* ms, const float* pan_l, double* q, double* table, int32_t B, int32_t C,
                 int32_t H, int32_t W, void* workspace, size_t workspace_bytes, void* stream);
/* table: the sum over all B_global samples (B_global >= B).  With d = table / B_global and sign(0) = 0 as torch.abs differentiates,
 *   g[n,i,p] = d loss / d out[n,i,p] = alpha_ni + sum_j beta_nij out[n,j,p] + gamma_ni pan[n,p]
 * (every moment is linear in the pixels; the per-sample coefficients come from the stored derivatives, the signs and the factors
 * (1 - D_s) / (C (C - 1) / 2 B_global) and (1 - D_lambda) / (C B_global)), evaluated in fp64 and rounded once:
 * dout = fl32(scale g), or with accumulate = 1 dout = dout + fl32(scale g) in fp32.  loss_accum[0] += (float)(loss B / B_global), this
 * rank's share, by a plain read-add-write of one lane; `scale` applies to dout only, as in lg_l1_loss.  indices [3] (may be NULL) =
 * D_lambda, D_s, loss.  Reads only what lg_qnr_stats left for the same (B, C, H, W) in that workspace. */
int lg_qnr_grad(const float* out, const float* pan, const double* table, float* dout, float* loss_accum, double* indices, int32_t B,
                int64_t B_global, int32_t C, int32_t H, int32_t W, float scale, int32_t accumulate, const void* workspace,
                size_t workspace_bytes, void* stream);

/* ---- the spectral (SAM) and the structural (1 - SSIM) training loss and their gradients (Engine.train_step with spectral_weight /
 * struct_weight; kernels in lgteun_amd/csrc/k_recloss.hip; the definitions are lgteun_amd/losses.py SAMLoss / SSIMLoss) ----
 * The contract of lg_l1_loss -- out, gt, dout [B,C,H,W] fp32, B_global the samples of all ranks, `scale` on dout only -- plus `accumulate`
 * (0: dout = fl32(scale g); 1: dout = dout + fl32(scale g) in fp32, after an earlier term wrote dout) and the caller's loss_accum:
 * loss_accum[0] += (float)(this rank's share of the global mean), one read-add-write of one lane.  Both losses are means over the global
 * batch, so the shares of the ranks add up and no collective is needed.  All arithmetic is fp64, rounded to fp32 once per dout element;
 * per-workgroup fp64 partials in the workspace and a one-workgroup finish in a fixed order, no atomics: the same call gives the same bits, and a
 * sample's dout has the same bits alone and inside any batch.  Arguments are validated before any HIP call and the offending one is named
 * in lg_last_error: C is 4 or 8; W is a multiple of 4; H, W <= 65536; 1 <= B <= 65535; float tensors 16-byte aligned, the workspace 8-byte aligned.  All
 * indexing is 64-bit.  The calls allocate nothing and synchronise nothing. */
/* bytes of workspace either call needs for [B, C, H, W]; 0 for C not in {4, 8} or W not a multiple of 4.  lg_ssim_loss also needs H and W
 * of at least 11 (one window) and says so itself: for smaller images the size returned is lg_sam_loss's. */
size_t lg_recloss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
/* the mean over all B_global H W pixels of the angle between out[n,:,p] and gt[n,:,p], in radians.  Per pixel o^ = o / |o|, g^ = g / |g|,
 * c = <o^, g^>, u = g^ - c o^, s = |u|: theta = atan2(s, c), d theta / d o = -u / (s |o|) (acos is never differentiated).  As metrics.sam
 * clips the cosine to [0, 1]: a pixel with c <= 0, |o| = 0 or |g| = 0 counts pi / 2 and has no gradient; one with s < 1e-6 counts its theta
 * and has no gradient (u is rounding noise there). */
int lg_sam_loss(const float* out, const float* gt, float* dout, float* loss_accum, int32_t B, int64_t B_global, int32_t C, int32_t H, int32_t W,
                float scale, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* 1 - the mean of the SSIM map over every image, band and window that lies fully inside the image (metrics._ssim_band: 11-tap Gaussian of
 * sigma 1.5, c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2).  With the window sums m1 = sum g x, m2 = sum g x^2, m3 = sum g x y
 * (x = out, y = gt) and T the transposed separable Gaussian, d loss / d x(p) = -(T(dS/dm1) + 2 x T(dS/dm2) + y T(dS/dm3))(p) / windows. */
int lg_ssim_loss(const float* out, const float* gt, float* dout, float* loss_accum, int32_t B, int64_t B_global, int32_t C, int32_t H, int32_t W,
                 float scale, float data_range, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- device-resident dataset (lgteun_amd/resident.py; kernels in lgteun_amd/csrc/k_batch.hip) ----
 * The store holds a whole data set on the device in the files' sample type: pan [N,1,H,W], lr [N,C,h,w], mul [N,C,H,W] (optional) and the
 * fp32 pan_l [N,1,h,w], with H = 4 h and W = 4 w.  Arguments are validated before any HIP call. */
#define LG_DT_U8 0
#define LG_DT_U16 1
#define LG_DT_F32 2
/* input_pan_l of `planes` PAN planes [H, W] of sample type `dtype`: two levels of the 5 x 5 binomial pyramid ([1 4 6 4 1] / 16 per axis,
 * BORDER_REFLECT_101, even rows and columns) -> pan_l [planes, H/4, W/4] fp32.  Integer planes are computed in integer arithmetic (exact; one
 * rounding, to fp32), float planes in fp64.  H, W: multiples of 4, at least 8. */
int lg_pyr_down2(const void* pan, float* pan_l, int64_t planes, int32_t H, int32_t W, int32_t dtype, void* stream);
/* One training / evaluation batch in one launch: item b of the outputs is store item idx[idx_offset + b] (a DEVICE int32 list; values are
 * clamped into 0 .. N-1), converted to fp32, flipped as the device word *flips says (bit 0: up-down, bit 1: left-right; flips == NULL: no
 * flip) and scaled: n_div (0, 1 or 2) correctly rounded fp32 divisions by `divisor`, then one fp32 multiplication by post_scale unless it
 * is 1.  Outputs are contiguous fp32 NCHW: o_pan [B,1,H,W], o_lr [B,C,h,w], o_mul [B,C,H,W] (NULL together with mul), o_pan_l [B,1,h,w].
 * All arrays 16-byte aligned.  1 <= B <= 65535, 1 <= C <= 16, h, w <= 8192, 1 <= N < 2^31; an item's 16-byte chunks are counted in 32 bits:
 * (C + 1) (H ceil(W / 4) + h w) < 2^31. */
int lg_batch_assemble(const void* pan, const void* lr, const void* mul, const float* pan_l, int64_t N, const int32_t* idx, int64_t idx_offset,
                      const uint32_t* flips, float* o_pan, float* o_lr, float* o_mul, float* o_pan_l, int32_t B, int32_t C, int32_t H, int32_t W,
                      int32_t h, int32_t w, int32_t dtype, float divisor, int32_t n_div, float post_scale, void* stream);

/* ---- training from a raw scene (lgteun_amd/wald.py; kernels in lgteun_amd/csrc/k_wald.hip and k_batch.hip) ----
 * Arguments are validated before any HIP call; the calls allocate nothing and synchronise nothing. */
/* Wald's degradation: a separable FIR low-pass and decimation by 4 of `planes` planes [H, W] of sample type `dtype`.  taps: a DEVICE array
 * [planes, n_taps] of fp64, one row per plane, used on both axes; n_taps odd, in 1 .. 63.  Output (i, j) of a plane is the filtered plane at
 * (4 i + phase, 4 j + phase), phase in 0 .. 3; indices past the border are clamped into the plane (replicate).  H, W: multiples of 4 in
 * 8 .. 65536.  fp64 arithmetic: the row pass, then the column pass, each sum_k taps[k] * x[. + k - n_taps / 2] with every product and every
 * sum rounded on its own, in ascending k from 0.0.  out [planes, H/4, W/4]: fp32 (out_f32 = 1: the fp64 value rounded once) or the input's
 * integer type (out_f32 = 0, integer planes only: round half to even, saturated to the type's range, NaN -> 0).  An output's bits depend on
 * its own samples and taps only, not on the launch geometry or on the other planes of the call. */
int lg_fir_decimate4(const void* in, void* out, const double* taps, int64_t planes, int32_t H, int32_t W, int32_t n_taps, int32_t phase,
                     int32_t dtype, int32_t out_f32, void* stream);
/* One training / evaluation batch cut out of ONE device-resident scene in two launches (gather, window pyramid): pan [1,Hs,Ws],
 * lr [C,Hs/4,Ws/4], mul [C,Hs,Ws] (NULL together with o_mul) in sample type `dtype`; Hs, Ws multiples of 4 in 8 .. 65536.  Item b is the
 * P x Q window (multiples of 4 in 8 .. 4096, not larger than the scene) at origin first + b of `origins`, a DEVICE int32 list of n_windows
 * pairs (oy, ox) in PAN pixels, multiples of 4; values are clamped into the scene and rounded down to the 4-pixel grid, so no value becomes
 * an address outside it.  o_pan [B,1,P,Q], o_lr [B,C,P/4,Q/4], o_mul [B,C,P,Q], o_pan_l [B,1,P/4,Q/4]: contiguous fp32, every one bit for
 * bit what lg_batch_assemble writes for a store whose item b is that window (pan_l by lg_pyr_down2 of the window: the pyramid reflects at
 * the WINDOW's border), with the same flip word and (divisor, n_div, post_scale).  Scene and output arrays 16-byte aligned (window rows
 * need not be).  No atomics.  1 <= B <= 65535, 1 <= C <= 16. */
int lg_window_assemble(const void* pan, const void* lr, const void* mul, const int32_t* origins, int64_t n_windows, int64_t first,
                       const uint32_t* flips, float* o_pan, float* o_lr, float* o_mul, float* o_pan_l, int32_t B, int32_t C, int32_t Hs, int32_t Ws,
                       int32_t P, int32_t Q, int32_t dtype, float divisor, int32_t n_div, float post_scale, void* stream);

/* ---- tiled scene fusion (lgteun_amd/scene.py; kernels in lgteun_amd/csrc/k_scene.hip) ----
 * A scene larger than one plan (or off the 16-pixel grid) is cut into overlapping tiles, the tiles go through lgteun_forward in batches and
 * the outputs are blended back.  The scene is device-resident in the files' sample type: pan [1,H,W], ms [C,H/4,W/4]; H, W multiples of 4
 * in 16 .. 65536.  Tiles are th x tw PAN pixels, multiples of 16 in 16 .. 1024, not larger than the scene.  The grid of scene.tile_grid: per
 * axis of length L with tile t and stride s = t - overlap, n = 1 if L == t else ceil((L - t) / s) + 1 tiles at origins min(i * s, L - t);
 * tiles are numbered row-major (index = iy * nx + ix).  Arguments are validated before any HIP call; the calls allocate nothing and
 * synchronise nothing. */
/* Tile batch `first .. first + B - 1` of the origin list (a DEVICE int32 list of n_tiles pairs (oy, ox) in PAN pixels, multiples of 4; values
 * are clamped into the scene and rounded down to the 4-pixel grid, so no value becomes an address outside it) -> o_pan [B,1,th,tw],
 * o_ms [B,C,th/4,tw/4], contiguous fp32, scaled like lg_batch_assemble scales: n_div (0, 1 or 2) correctly rounded fp32 divisions by
 * `divisor`, then one fp32 multiplication by post_scale unless it is 1 (the same device function).  Scene and tile arrays 16-byte aligned.
 * 1 <= B <= 65535, 1 <= C <= 16. */
int lg_scene_gather(const void* pan, const void* ms, const int32_t* origins, int64_t n_tiles, int64_t first, float* o_pan, float* o_ms,
                    int32_t B, int32_t C, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t dtype, float divisor, int32_t n_div,
                    float post_scale, void* stream);
/* Adds the outputs `tiles` [B,C,th,tw] of grid tiles first .. first + B - 1 into scene [C,H,W] (fp32).  Call it for consecutive batches in
 * ascending order on one stream, every tile of the grid exactly once.  overlap: a multiple of 4 in 0 .. min(th, tw) / 2.  The weight of local
 * coordinate u on an axis of tile side t is (float)min(min(u, t - 1 - u) + 1, overlap + 1) / (float)(overlap + 1), a tile's weight the fp32
 * product w(y) * w(x).  After the last batch
 *   (a) a pixel holds (sum_k w_k v_k) / (sum_k w_k) over its covering tiles k in ascending index: the numerator is w_0 v_0 continued by
 *       fmaf(w_k, v_k, .) in that order, the denominator (sum_y w(y)) * (sum_x w(x)) with both sums in ascending order, and the one
 *       division is correctly rounded;
 *   (b) a pixel that one tile alone covers holds that tile's value, bit for bit;
 *   (c) the bits do not depend on how the tile list was cut into batches (between launches the scene holds the running numerator);
 *   (d) the scene needs no initialisation: a pixel's lowest-index cover writes it without reading it.
 * No atomics: within a launch exactly one lane writes a pixel.  tiles and scene 16-byte aligned. */
int lg_scene_blend(const float* tiles, float* scene, int64_t first, int32_t B, int32_t C, int32_t H, int32_t W, int32_t th, int32_t tw,
                   int32_t overlap, void* stream);
/* dst[i] = clip(rint(src[i] * scale), 0, 65535) with one fp32 multiplication and round-half-even (NaN -> 0): data_denormalize followed by the
 * TIFF writer's conversion.  n: a multiple of 4; src 16-byte, dst 8-byte aligned. */
int lg_scene_to_u16(const float* src, uint16_t* dst, int64_t n, float scale, void* stream);

/* ---- the classical baselines: SFIM and GSA (global regression) on the 23-tap interpolator x4 (lgteun_amd/classical.py; kernels in
 * lgteun_amd/csrc/k_classical.hip; the definitions are DESIGN.md 3.12) ----
 * ms [B,C,h,w], pan [B,1,4h,4w], out [B,C,4h,4w]: contiguous fp32, normalised to [0, 1].  Every sample is fused on its own.  All arithmetic is
 * fp64 with one rounding per output element; the moments are per-workgroup partials in the workspace plus a fixed-order pass (no atomics):
 * repeated calls give the same bits, and sample b of a batch has the bits of that sample fused alone.  The workspace needs no
 * initialisation.  2 <= C <= LG_IQA_MAX_BANDS; 4 <= h, w <= 4096; 1 <= B <= 65535; float tensors 16-byte aligned, workspace and stats 8-byte
 * aligned.  Arguments are validated before any HIP call, the offender is named in lg_last_error; all indexing is 64-bit; the calls allocate
 * nothing and synchronise nothing. */
#define LG_CLASSICAL_SFIM 0
#define LG_CLASSICAL_GSA 1
/* bytes of workspace lg_sfim (method LG_CLASSICAL_SFIM) / lg_gsa (LG_CLASSICAL_GSA) needs; 0 for a shape or method the calls reject */
size_t lg_classical_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t method);
/* u = interp23(ms): two x2 levels of zero insertion and the circular 23-tap half-band interpolator along rows, then columns; ms sample (i, j)
 * sits at u(4 i + 2, 4 j + 2) */
int lg_interp23_up4(const float* ms, float* out, int32_t B, int32_t C, int32_t h, int32_t w, void* stream);
/* out_k = clip(u_k p_k / (box5(p_k) + 1e-8), 0, 1), p_k = (pan - mean pan) std(u_k) / std(pan) + mean u_k (both std divide by N - 1), box5 the
 * circular 5 x 5 mean.  A constant PAN has scale 0. */
int lg_sfim(const float* ms, const float* pan, float* out, int32_t B, int32_t C, int32_t h, int32_t w, void* workspace, size_t workspace_bytes,
            void* stream);
/* out_k = clip(u_k + g_k (p~ - I0), 0, 1): p~ = pan - mean pan, I0 = sum_k alpha_k (u_k - mean u_k), alpha the least-squares fit of the 2 x 2
 * centre means of p~ by [ms_k - mean ms_k, 1], g_k = cov(I0, u_k) / var(I0) (covariance / (N - 1), variance / N).  stats: NULL or a device
 * array [B, 2 C + 1] of fp64 that receives alpha (C + 1 values, the intercept last), then g.  A sample whose regression is singular or whose
 * I0 has no variance gets alpha_0..C-1 = g = 0: out = clip(u). */
int lg_gsa(const float* ms, const float* pan, float* out, double* stats, int32_t B, int32_t C, int32_t h, int32_t w, void* workspace,
           size_t workspace_bytes, void* stream);
/* ---- the third classical baseline: Wavelet, the two-level Haar substitution ----
 * out_k(y, x) = clip(pan(y, x) - P(y / 4, x / 4) + M_k(y / 4, x / 4), 0, 1): the level-2 Haar approximation of PAN replaced by that of u_k = interp23(ms_k).
 * The sides are 4h x 4w, so both levels split evenly: P is the 4 x 4 block mean of PAN, M_k that of u_k, and M_k = sum_a sum_b t_a t_b
 * ms_k((i - a) mod h, (j - b) mod w) with the 17 taps of lg_wavelet_taps.  One launch, no workspace, no method code (the method has no global statistic:
 * lg_classical_workspace_bytes knows no third method); tensors, limits, checks and guarantees are those of lg_sfim. */
int lg_wavelet(const float* ms, const float* pan, float* out, int32_t B, int32_t C, int32_t h, int32_t w, void* stream);
/* out17: a HOST array that receives the taps lg_wavelet uses, by offset -8 .. 8: the block means of the response of interp23 to a unit impulse */
int lg_wavelet_taps(double* out17);
/* ---- MTF-GLP: the generalised Laplacian pyramid with an MTF-matched Gaussian, three injection rules (lgteun_amd/mtf_glp.py) ----
 * With u_k = interp23(ms)_k and SFIM's statistics (mu = mean pan, m_k = mean u_k, a_k = std(u_k) / std(pan), both std over N - 1; a_k = 0 for a constant
 * PAN): p_k = a_k (pan - mu) + m_k; D_f(i, j) = sum_a sum_b t_f[a] t_f[b] pan(clamp(4 i + 2 + a - r), clamp(4 j + 2 + b - r)) with r = n_taps / 2 (replicate
 * border, the rule of lg_fir_decimate4 at phase 2); q_k = a_k (D_k - mu) + m_k; L_k = interp23(q_k) (circular).  Then, clipped to [0, 1] with one rounding:
 *   LG_MTFGLP_GLP  out_k = u_k + (p_k - L_k)
 *   LG_MTFGLP_HPM  out_k = u_k p_k / (L_k + 1e-8)
 *   LG_MTFGLP_CBD  out_k = u_k + g_k (p_k - L_k), g_k = sum (u_k - m_k)(L_k - mean L_k) / sum (L_k - mean L_k)^2; g_k = 0 where a_k = 0, where the
 *                  denominator is not positive or not finite, or where the quotient is not finite: out_k = clip(u_k) bit for bit.
 * taps: a DEVICE array [n_filters, n_taps] of fp64 (wald.mtf_taps: rows that sum to 1); n_filters is 1 (one filtered plane serves every band) or C; n_taps odd,
 * in 1 .. 63.  stats: NULL or a device array [B, 2 C] of fp64 that receives a, then g (1 for GLP and HPM).  Launches: SFIM's moments and finish, one low-pass
 * that writes D as fp64 [B, n_filters, h, w] into the workspace, for CBD a second moments pass and its finish, and the apply pass; neither u nor L is stored.
 * Tensors, limits, alignment, checks and guarantees (same bits on every call, a sample's bits do not depend on its batch, the workspace needs no initialisation)
 * are those of lg_sfim; taps 8-byte aligned. */
#define LG_MTFGLP_GLP 0
#define LG_MTFGLP_HPM 1
#define LG_MTFGLP_CBD 2
/* bytes of workspace lg_mtf_glp needs; 0 for anything the call rejects */
size_t lg_mtfglp_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t n_filters, int32_t mode);
int lg_mtf_glp(const float* ms, const float* pan, float* out, double* stats, const double* taps, int32_t n_filters, int32_t n_taps, int32_t mode, int32_t B,
               int32_t C, int32_t h, int32_t w, void* workspace, size_t workspace_bytes, void* stream);
/* ---- A trous: ATWT and AWLP, the detail of PAN against its two-level undecimated B3-spline low-pass (lgteun_amd/atrous.py) ----
 * With u_k = interp23(ms)_k, N = 16 h w and SFIM's statistics (mu = mean pan, s_k = std(u_k) over N - 1): P_L = PAN filtered along rows, then columns, by the 13
 * taps (1, 4, 10, 20, 31, 40, 44, 40, 31, 20, 10, 4, 1) / 256 at offsets -6 .. 6, indices modulo the sides (the cascade of (1, 4, 6, 4, 1) / 16 at unit step and at
 * step 2; a scene's rim of 6 pixels wraps, where toolboxes mirror); d = pan - P_L; a_k = s_k / std(pan) (LG_ATROUS_MATCH_PAN) or s_k / s_L with
 * s_L^2 = sum (P_L - mu)^2 / (N - 1) (LG_ATROUS_MATCH_LOWPASS), 0 where that variance is not > 0.  Then, clipped to [0, 1] with one rounding:
 *   LG_ATROUS_ATWT  out_k = u_k + a_k d
 *   LG_ATROUS_AWLP  out_k = u_k + a_k d u_k / (U + 1e-8), U = the mean of u over the bands; the injection is 0 where U + 1e-8 is not > 0 or not finite
 * PAN enters every sum minus the sample's first pixel: a constant PAN has d = 0 and a = 0 exactly and out = clip(u) bit for bit.  The compute entry takes ONE
 * pointer to an argument block; struct_bytes must be sizeof(lg_atrous_args), any other value is rejected.  stats: NULL or a device array [B, C + 1] of fp64 that
 * receives a (C), then the reference deviation, std(pan) or s_L.  Launches: SFIM's moments and finish, for LG_ATROUS_MATCH_LOWPASS the pass that sums
 * (P_L - mu)^2 and its finish, and the apply pass; neither u nor P_L is stored.  Tensors, limits, alignment, checks (every one before any HIP call: a rejected
 * call launches and writes nothing, its message starts with "atrous:" and names the argument) and guarantees (same bits on every call, a sample's bits do not
 * depend on its batch, the workspace needs no initialisation) are those of lg_sfim. */
#define LG_ATROUS_ATWT 0
#define LG_ATROUS_AWLP 1
#define LG_ATROUS_MATCH_PAN 0
#define LG_ATROUS_MATCH_LOWPASS 1
typedef struct {
    uint32_t struct_bytes;            /* sizeof of this struct; any other value is rejected */
    int32_t rule, match, B, C, h, w;
    const float *ms, *pan; float* out; double* stats;   /* stats may be NULL */
    void* workspace; size_t workspace_bytes; void* stream;
} lg_atrous_args;
/* bytes of workspace the compute entry needs for `match`; 0 for anything the call rejects */
size_t lg_atrous_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t match);
int lg_atrous(const lg_atrous_args* args);
/* out13: a HOST array that receives the 13 taps the kernels use, by offset -6 .. 6, from the same constexpr */
int lg_atrous_taps(double* out13);
/* ---- MTF-HR: the regression-based and haze-corrected members of the MTF-GLP family: FS, HPM-R, HPM-H, BT-H (lgteun_amd/mtf_hr.py) ----
 * With u_k = interp23(ms)_k, N = 16 h w, m_k = mean u_k, mu = mean pan, D_f = lg_mtf_glp's plane of the RAW pan under the taps of filter f (f = k, or 0 when
 * n_filters is 1), L_k = interp23(D_k - pan(0, 0)) + pan(0, 0) (no histogram matching; the pivot keeps a constant PAN exact), l_k = mean L_k and H_k = the minimum of ms_k over the sample's h w pixels (the haze):
 *   LG_MTFHR_FS     out_k = u_k + g_k (pan - L_k), g_k = sum (u_k - m_k)(pan - mu) / sum (L_k - l_k)(pan - mu)
 *   LG_MTFHR_HPM_R  out_k = u_k r, r = (g_k pan + b_k) / (g_k L_k + b_k), g_k = sum (u_k - m_k)(L_k - l_k) / sum (L_k - l_k)^2, b_k = m_k - g_k l_k
 *   LG_MTFHR_HPM_H  out_k = (u_k - H_k) r + H_k, r = (pan - H_P,k) / (L_k - H_P,k), H_P,k = mean D_k + sum_j s_j (H_j - mean ms_j) with s the slopes of the
 *                   least-squares fit [ms_1 .. ms_C, 1] -> D_k over the h w MS pixels (Cholesky solve of the centred normal equations)
 *   LG_MTFHR_BT_H   out_k = (u_k - H_k) r + H_k, r = (pan - H_I) / sum_j w_j (u_j - H_j), w the slopes and w_0 the intercept of the same fit to the one plane
 *                   D (taps: PAN's own MTF), H_I = w_0 + sum_j w_j H_j; n_filters must be 1
 * clipped to [0, 1] with one rounding.  g_k = 0 where its denominator is not > 0 or not finite or the quotient is not finite; r = 1 (no injection at that
 * pixel) where its denominator is not > 0 or the quotient is not finite; a non-positive Cholesky pivot or a slope that is not finite gives slopes 0 (the
 * intercept is then mean D).  PAN enters the filter and every sum minus the sample's first pixel: a constant PAN gives g = 0 and, for FS and HPM-R,
 * out = clip(u) bit for bit.  The compute entry takes ONE pointer to an argument block; struct_bytes must be sizeof(lg_mtf_hr_args).  taps: a DEVICE array
 * [n_filters, n_taps] of fp64 (wald.mtf_taps), n_filters 1 or C, n_taps odd, in 1 .. 63.  stats: NULL or a device array [B, 2 C + 2] of fp64, unused slots
 * written as 0: FS g; HPM_R g, b; HPM_H H, H_P; BT_H H, w_1 .. w_C, w_0, H_I.  Launches: FS / HPM_R -- SFIM's moments and finish, the low-pass (D as fp64
 * [B, n_filters, h, w] in the workspace), a second moments pass and its finish, the apply pass; HPM_H / BT_H -- the low-pass, a Gram pass at the MS scale, the
 * solve, the apply pass.  Neither u nor L is stored.  Tensors, limits, alignment, checks (every one before any HIP call: a rejected call launches and writes
 * nothing, its message starts with "mtf_hr:" and names the argument) and guarantees (same bits on every call, a sample's bits do not depend on its batch, one
 * filtered plane and the same taps C times give the same bits, the workspace needs no initialisation) are those of lg_mtf_glp. */
#define LG_MTFHR_FS 0
#define LG_MTFHR_HPM_R 1
#define LG_MTFHR_HPM_H 2
#define LG_MTFHR_BT_H 3
typedef struct {
    uint32_t struct_bytes;            /* sizeof of this struct; any other value is rejected */
    int32_t rule, n_filters, n_taps, B, C, h, w;
    const float *ms, *pan; float* out; double* stats;   /* stats may be NULL */
    const double* taps;
    void* workspace; size_t workspace_bytes; void* stream;
} lg_mtf_hr_args;
/* bytes of workspace the compute entry needs; 0 for anything the call rejects */
size_t lg_mtf_hr_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t n_filters, int32_t rule);
int lg_mtf_hr(const lg_mtf_hr_args* args);
/* ---- BDSD: the band-dependent spatial detail method, global or block-wise (lgteun_amd/bdsd.py) ----
 * With u_k = interp23(ms)_k, A_k(i, j) = sum_a sum_b t_k[a] t_k[b] ms_k(clamp(i + a - r), clamp(j + b - r)) (the band low-passed on its own grid, replicate
 * border, r = n_taps / 2) and D = the raw PAN filtered with taps_pan at (4 i + 2, 4 j + 2) (lg_mtf_glp's rule): per block and band the weights gamma_k in
 * R^(C + 1) minimise sum (ms_k - A_k - x' gamma)^2 over the block's MS pixels, x = [A_1 .. A_C, D] (no intercept), by a Cholesky solve of the normal equations
 * in fp64; out_k = clip(u_k + sum_j gamma_k[j] u_j + gamma_k[C] pan, 0, 1) with one rounding, gamma that of the block the PAN pixel lies in.
 * block: 0 = one block is the whole sample (needs h w >= 2 (C + 1)); else the block's side in PAN pixels, a multiple of 32 that divides 4 h and 4 w; block
 * (I, J) holds the MS pixels i / (block / 4) = I, j / (block / 4) = J.  A block with a pivot d_j <= 1e-12 G_jj, a pivot or a weight that is not finite has
 * gamma = 0: its output is clip(u) bit for bit.  taps_ms: a DEVICE array [n_filters, n_taps] of fp64, n_filters 1 (one filter for every band) or C; taps_pan:
 * [n_taps]; rows sum to 1 (wald.mtf_taps); n_taps odd, in 1 .. 63.  stats: NULL or a device array [B, 4 h / block, 4 w / block, C, C + 1] of fp64 ([B, 1, 1, C,
 * C + 1] for block 0) that receives gamma.  Launches: the low-pass of PAN and of the bands (fp64 [B, h, w] and [B, C, h, w] in the workspace), the Gram pass,
 * the solve, the apply pass; neither u nor A is stored at PAN size.  Tensors, limits, alignment, checks and guarantees (same bits on every call, a sample's
 * bits do not depend on its batch, the workspace needs no initialisation, a rejected call writes nothing) are those of lg_mtf_glp. */
/* bytes of workspace lg_bdsd needs; 0 for anything the call rejects */
size_t lg_bdsd_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t block);
int lg_bdsd(const float* ms, const float* pan, float* out, double* stats, const double* taps_ms, int32_t n_filters, const double* taps_pan, int32_t n_taps,
            int32_t block, int32_t B, int32_t C, int32_t h, int32_t w, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the component-substitution baselines: generalised IHS, Brovey, Gram-Schmidt, PCA (lgteun_amd/cs.py) ----
 * Per sample, with u = interp23(ms), N = 16 h w, m_k = mean u_k, m_p = mean pan, Sigma = cov of the bands of u, r_k = cov(u_k, pan), v_p = var(pan) (all over
 * N - 1): intensity weights w -- 1 / C or the caller's `weights` for IHS, Brovey and GS, for PCA the unit eigenvector of Sigma's largest eigenvalue, signed so
 * that w'r >= 0 (if w'r = 0: sum w >= 0) -- I = sum_k w_k (u_k - m_k), m_I = sum_k w_k m_k, v_I = w'Sigma w, a = sqrt(v_I / v_p), P = a (pan - m_p).  Then
 *   LG_CS_IHS     out_k = clip(u_k + (P - I))                        g_k = 1
 *   LG_CS_BROVEY  out_k = clip(u_k (P + m_I) / (I + m_I + 2^-52))    g_k = 1 in stats
 *   LG_CS_GS      out_k = clip(u_k + g_k (P - I))                    g_k = (Sigma w)_k / v_I
 *   LG_CS_PCA     out_k = clip(u_k + g_k (P - I))                    g_k = w_k
 * clipped to [0, 1] by fmin(fmax()) with one rounding to fp32.  A sample with v_p <= 0, v_I <= 0, a not finite or (PCA) a largest eigenvalue <= 0 is
 * degenerate: out = clip(u) bit for bit (stats: a = 0, g = 0).  PAN and every band enter the moments minus their first sample, so a constant PAN or band has
 * exactly zero moments.  weights: a HOST array of C finite doubles, used as given (not normalised), or NULL; must be NULL for LG_CS_PCA.  stats: NULL or a
 * device array [B, 2 C + 2] of fp64 that receives w (C), g (C), a, m_I.  The moments are formed at the MS scale (the adjoint of interp23 on PAN, its Gram
 * operator on ms: lg_cs_taps), u only in the apply pass and never stored.  Launches: the adjoint pass, the Gram pass, the finish, the apply pass.  Tensors,
 * limits, alignment, checks and guarantees (same bits on every call, a sample's bits do not depend on its batch, the workspace needs no initialisation, a
 * rejected call launches nothing) are those of lg_sfim. */
#define LG_CS_IHS 0
#define LG_CS_BROVEY 1
#define LG_CS_GS 2
#define LG_CS_PCA 3
/* bytes of workspace lg_cs needs; 0 for a shape the call rejects */
size_t lg_cs_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w);
int lg_cs(const float* ms, const float* pan, float* out, double* stats, const double* weights, int32_t mode, int32_t B, int32_t C, int32_t h, int32_t w,
          void* workspace, size_t workspace_bytes, void* stream);
/* HOST arrays: t67 receives interp23's 1-D impulse response by offset -33 .. 33 (u(y) = sum_i t(y - 4 i - 2) ms(i), circular), r33 its Gram taps R(d) = sum_m
 * t(m) t(m - 4 d) by offset -16 .. 16 */
int lg_cs_taps(double* t67, double* r33);

#ifdef __cplusplus
}
#endif
#endif
