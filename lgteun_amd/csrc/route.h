// Kernel routes of a plan: which kernel runs for every half-block, what the saving forward leaves for the backward and what the
// backward reads.  lg_resolve_route (route.hip) fills them ONCE, in lg_plan_create, from lg_config.variant / precision / C / H / W;
// the orchestrators (k_fwd.hip, k_bwd.hip) and the launchers that choose between kernels read the route and nothing else.
#pragma once
#include <stddef.h>
#include "abi.h"

// level 0: the four e = 4C blocks at H x W; level 1: the bottleneck block, e = 8C at H/2 x W/2
enum FfnFwdKernel {
    FFN_FWD_XR,         // k_ffn_xr: register chain, e = 16 (nothing, h2 or h2 / h3 saved)
    FFN_FWD_XS,         // k_ffn_xs: channel-split strip kernel, e = 16 (every save form)
    FFN_FWD_X32,        // k_ffn_x32, e = 32
    FFN_FWD_X64,        // k_ffn1_x64 + k_ffn2_x64, e = 64 (h2 through HBM)
    FFN_FWD_STRIP,      // k_ffn_strip: f32-MFMA strip kernel, e = 16
    FFN_FWD_TILE,       // k_ffn_fused: round 1's f32-MFMA tile kernel, e = 32
    FFN_FWD_UNFUSED     // k_ffn1 + k_ffn2
};
enum FfnArith { FFN_ARITH_F32, FFN_ARITH_BF16, FFN_ARITH_F16X2, FFN_ARITH_BF16X3 };   // f32 MFMA | one bf16 piece | f16 pairs with operand scales | three bf16 pieces
enum FfnSlot { FFN_SLOT_A1 = 1, FFN_SLOT_G1 = 2, FFN_SLOT_H2 = 4, FFN_SLOT_A3 = 8, FFN_SLOT_G3 = 16 };   // the five save slots of BlockBufs (workspace.h)
enum FfnDwBwdKernel { FFN_DWBWD_XS, FFN_DWBWD_H, FFN_DWBWD_TILE };   // spatial half: k_ffn_dw_bwd_xs | k_ffn_dw_bwd_h (h3 re-computed) | k_ffn_dw_bwd
enum Ffn1BwdKernel { FFN1_BWD_XS, FFN1_BWD_X32, FFN1_BWD_TILE };      // pixelwise half: k_ffn1_bwd_xs | k_ffn1_bwd_x32 | k_ffn1_bwd

struct FfnRoute {
    int e, h, w;
    // ---- forward
    FfnFwdKernel fwd[2];   // [0]: nothing saved, [1]: LG_FLAG_SAVE
    FfnArith arith;
    bool hbf;              // bf16 storage of the hidden / saved tensors
    bool scales;           // the kernels take the block's operand scales (k_ffn_prep.hip)
    int wsplit_np;         // e >= 32: pieces per weight of the block's pre-split fragments (prep_stages); 0: none
    unsigned saves;        // FfnSlot bits the saving forward writes = the slots the backward below reads
    bool pre;              // e = 16: the a1 / a3 slots hold the PRE-activations h1 / h3 (GELU re-evaluated by the backward)
    bool a3_pre() const { return pre || dw == FFN_DWBWD_XS; }   // (the strip-walking spatial half always reads the pre-activation h3)
    // ---- backward
    FfnDwBwdKernel dw;     // FFN_DWBWD_XS / _H: dW3 / db3 come out of the spatial kernel
    Ffn1BwdKernel px;      // FFN1_BWD_XS: dW1 / dW2 come out of the pixelwise kernel
    bool bwd_scales;       // f16-pair products in k_ffn1_bwd_xs: the forward's operand scales + max |dh2| left by the spatial kernel
    bool wgrad_w2, wgrad_w1, wgrad_w3;   // k_wgrad launches behind the pixelwise kernel, in this order
};

enum AttnFwdKernel { ATTN_FWD_M, ATTN_FWD_VALU };                       // k_attn_m (matrix pipe) | k_attn (vector pipe)
enum AttnBwdKernel { ATTN_BWD_F, ATTN_BWD_R3, ATTN_BWD_R3_CORE_M };     // k_attn_bwd_f | k_attn_bwd_core + k_attn_bwd_epi | k_attn_bwd_core_m + k_attn_bwd_epi
struct MixerRoute {
    int e;
    AttnFwdKernel fwd;
    bool bf16;         // one bf16 piece per operand (precision = 1)
    bool f16x2;        // to_qkv and Q K^T on f16 pairs with static scales (k_ffn_prep.hip) instead of three bf16 pieces
    bool stats;        // the saving forward leaves the row log-sum-exp and the attention output; the backward reads them instead of re-deriving them
    AttnBwdKernel bwd;
};

// The global (FFT) mixer of a level.  The plane's size picks the path -- resolve_fft (route.hip) holds that rule and nothing else does: workspace.h sizes the
// scratch, k_bwd.hip the partial sums and k_fft.hip's launchers their grids from what is written here.
enum FftPath {
    FFT_PATH_LDS_R,       // k_fftmix_r / k_fftmix_bwd_r: real-input in-LDS kernels, one launch per direction
    FFT_PATH_LDS_C,       // k_fftmix / k_fftmix_bwd: complex-row in-LDS kernels (LG_VAR_FFT_FULL)
    FFT_PATH_SPLIT,       // rows -> half spectrum in HBM -> columns + edit -> rows: three launches, radix-2 (256 x 256, 512 x 512)
    FFT_PATH_BLUESTEIN    // the same three launches on Bluestein lines: every other plane
};
struct FftRoute {
    FftPath path;
    int h, w;                // the plane
    int lg;                  // log2 h on the three power-of-two paths (h = w there); 0: Bluestein
    int col_groups;          // column groups per plane: grid.y of the column launch of the three-launch paths = partial rows a plane's backward writes (in LDS: 1)
    size_t scratch_floats;   // per plane: the half spectrum h x (w/2 + 1), complex, of the three-launch paths; in LDS: 0
    size_t bwd_part_floats(size_t planes) const { return planes * col_groups * 4; }   // FftBwdArgs::part: four parameter-gradient partial sums per row
};

struct LgRoute {
    FfnRoute ffn[2];     // by level
    MixerRoute mix[2];
    FftRoute fft[2];
    bool dstep_fused;        // the one-launch data step (k_dstep.hip) instead of the tile kernels
    bool reduce_per_block;   // one parameter-gradient reduce launch per block instead of one per pass
};

// 0, or -2 with lg_set_error for a variant word the library does not carry
int lg_resolve_route(const lg_config& cfg, LgRoute* r);
int lg_describe_route(const lg_config& cfg, const LgRoute& r, char* buf, size_t n);
