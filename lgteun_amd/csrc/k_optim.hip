// The optimizer steps over [begin, end) ranges of the flat buffers: k_adam (lg_adam_step), k_optim (lg_optim_step: torch.optim's Adam / AdamW / SGD / RMSprop)
// and both with the controls of a train step (lg_optim_step_ex: the clip coefficient k_gradnorm.hip left in device memory, a weight EMA).  One launch per step.
#include <math.h>

#include "abi.h"
#include "common.h"
#include "net_args.h"

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

// What every optimizer entry checks first (the network entries' argument contract, include/lgteun_hip.h): the flat buffers are float tensors -- not null
// where the entry always reads them, 16-byte aligned (the contract's uniform rule for float tensors; these kernels themselves would take any float) --, `ranges` holds int64 pairs, and n_ranges is the grid's y (k_adam / k_optim: dim3 grid(gx, n_ranges)),
// which HIP documents up to 65535.  Inside a range the kernels index element by element in int64, so a range may begin at any float.
static int optim_args_ok(const char* who, const float* params, const float* grads, const float* s0, const float* s1, const float* s2, const int64_t* ranges,
                         int32_t n_ranges, int32_t step) {
    NetArgs v(who);
    auto need = [&](const void* p, const char* name) { if (!v.rc && !p) v.fail(-1, "invalid argument: %s is NULL", name); };
    need(params, "params"); need(grads, "grads"); need(ranges, "ranges");
    v.aligned(params, "params", 16).aligned(grads, "grads", 16).aligned(s0, "state0", 16).aligned(s1, "state1", 16).aligned(s2, "state2", 16).aligned(ranges, "ranges", 8);
    if (!v.rc && (n_ranges < 1 || n_ranges > 65535)) v.fail(-1, "invalid argument: n_ranges must be in 1 .. 65535 (got %d)", n_ranges);
    if (!v.rc && step < 1) v.fail(-1, "invalid argument: step must be at least 1 (got %d)", step);
    return v.rc;
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
    if (int rc = optim_args_ok("adam_step", params, grads, exp_avg, exp_avg_sq, nullptr, ranges, n_ranges, step)) return rc;
    if (!exp_avg || !exp_avg_sq) { lg_set_error("adam_step: invalid argument: %s is NULL", !exp_avg ? "exp_avg" : "exp_avg_sq"); return -1; }
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
#define LG_OPT_FMA(a, b, c) __builtin_fmaf(a, b, c)
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
    if (int rc = optim_args_ok("optim_step", params, grads, state0, state1, state2, ranges, n_ranges, step)) return rc;
    if (algo < LG_OPT_ADAM || algo > LG_OPT_RMSPROP) { lg_set_error("optim_step: invalid argument: algo must be in 0 .. 3 (got %d)", algo); return -1; }
    if (flags & ~(LG_OPT_AMSGRAD | LG_OPT_NESTEROV | LG_OPT_CENTERED)) { lg_set_error("optim_step: invalid argument: flags has bits the header does not define (0x%x)", (unsigned)flags); return -1; }
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
    if ((need0 && !state0) || (need1 && !state1) || (need2 && !state2)) {
        lg_set_error("optim_step: %s is NULL: a state buffer of this option set is missing", (need0 && !state0) ? "state0" : ((need1 && !state1) ? "state1" : "state2"));
        return -1;
    }
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
    if (int rc = optim_args_ok("optim_step_ex", params, grads, state0, state1, nullptr, ranges, n_ranges, step)) return rc;
    if (!state0 || !state1) { lg_set_error("optim_step_ex: invalid argument: %s is NULL", !state0 ? "state0" : "state1"); return -1; }
    // lg_adam_step takes its scalars as floats: round them first, so that the bias corrections see what that entry point sees
    return launch_adam(params, grads, state0, state1, ranges, n_ranges, max_range, step, (float)lr, (float)h0, (float)h1, (float)eps,
                       (float)grad_scale, c, (hipStream_t)stream);
}
