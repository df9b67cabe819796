// Global L2 norm of the flat gradient buffer over [begin, end) ranges and the clip coefficient of torch.nn.utils.clip_grad_norm_
// (Engine.train_step with TrainControls.max_grad_norm), both left in DEVICE memory: the optimizer launch reads the coefficient through a
// pointer, so clipping puts no host synchronisation into the step.
//
//   k_gradnorm_part    grid (gx, n_ranges) like the optimizer launch: workgroup (x, y) strides through range y and writes ONE fp64 partial,
//                      partial[y * gx + x] (0 for a workgroup the range does not reach).  The square of an fp32 value is exact in fp64;
//                      the lanes of a wave meet by shuffles, the four waves in LDS, both in a fixed order (reduce.h block_sum4).
//   k_gradnorm_finish  one workgroup adds the partials in a fixed order (reduce.h partials_sum) and writes
//                      out[0] = (float)sqrt(sum), out[1] = min(1, max_norm / (out[0] + 1e-6)) in fp32.
// No floating-point atomics anywhere, so the same call gives the same bits every time (the convention of reduce.h).  Scalar 4-byte
// loads: a range may begin and end at any float offset, and nothing outside [begin, end) is read.
#include "abi.h"
#include "common.h"
#include "reduce.h"

#define GN_NT 256      // block_sum4 and partials_sum are written for this
#define GN_MAX_GX 512

__global__ __launch_bounds__(GN_NT) void k_gradnorm_part(const float* __restrict__ g, const int64_t* __restrict__ ranges,
                                                         double* __restrict__ partial) {
    __shared__ double sm[GN_NT / 64];
    const int64_t lo = ranges[2 * blockIdx.y], hi = ranges[2 * blockIdx.y + 1];
    const int64_t stride = (int64_t)gridDim.x * GN_NT;
    double acc = 0.0;
    int64_t i = lo + (int64_t)blockIdx.x * GN_NT + threadIdx.x;
    for (; i + 3 * stride < hi; i += 4 * stride) {          // four loads in flight; the order of the adds is fixed
        const double a = (double)g[i], b = (double)g[i + stride], c = (double)g[i + 2 * stride], d = (double)g[i + 3 * stride];
        acc += a * a;
        acc += b * b;
        acc += c * c;
        acc += d * d;
    }
    for (; i < hi; i += stride) {
        const double a = (double)g[i];
        acc += a * a;
    }
    const double total = block_sum4(acc, sm);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(GN_NT) void k_gradnorm_finish(const double* __restrict__ partial, int n_partial, float max_norm,
                                                           float* __restrict__ out) {
    __shared__ double sm[GN_NT / 64];
    const double total = partials_sum(partial, n_partial, sm);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        const float q = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = q < 1.0f ? q : (q != q ? q : 1.0f);        // clamp(max = 1) as torch takes it: a NaN stays a NaN (fminf would drop it)
    }
}

static int gn_grid_x(int64_t max_range) {
    int64_t gx = (max_range + GN_NT - 1) / GN_NT;
    return (int)(gx < 1 ? 1 : (gx > GN_MAX_GX ? GN_MAX_GX : gx));
}

extern "C" size_t lg_grad_norm_workspace_bytes(int32_t n_ranges, int64_t max_range) {
    if (n_ranges <= 0 || n_ranges > 65535 || max_range <= 0) return 0;
    return (size_t)n_ranges * gn_grid_x(max_range) * sizeof(double);
}

extern "C" int lg_grad_norm(const float* grads, const int64_t* ranges, int32_t n_ranges, int64_t max_range, double max_norm, float* out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* why = nullptr;
    if (!grads || !ranges || !out || !workspace) why = "null pointer";
    else if (n_ranges <= 0 || n_ranges > 65535) why = "n_ranges must be in 1 .. 65535";
    else if (max_range <= 0) why = "max_range must be positive";
    else if (!(max_norm > 0.0)) why = "max_norm must be positive";
    else if ((uintptr_t)workspace & 7) why = "the workspace must be 8-byte aligned";
    else if (((uintptr_t)grads | (uintptr_t)out) & 3) why = "grads and out must be 4-byte aligned";
    else if (workspace_bytes < lg_grad_norm_workspace_bytes(n_ranges, max_range)) why = "workspace too small (lg_grad_norm_workspace_bytes)";
    if (why) { lg_set_error("grad_norm: %s", why); return -1; }
    const int gx = gn_grid_x(max_range);
    const hipStream_t s = (hipStream_t)stream;
    k_gradnorm_part<<<dim3(gx, n_ranges), GN_NT, 0, s>>>(grads, ranges, (double*)workspace);
    LG_CHECK_LAUNCH();
    k_gradnorm_finish<<<1, GN_NT, 0, s>>>((const double*)workspace, gx * n_ranges, (float)max_norm, out);
    LG_CHECK_LAUNCH();
    return 0;
}
