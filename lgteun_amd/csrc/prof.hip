// The opt-in live per-kernel timing of the C ABI (lg_prof_*, lg_kernel_name) and what the launchers call around a kernel (common.h: ProfScope).  Host code only.
#include <stdlib.h>
#include <mutex>

#include "abi.h"
#include "common.h"

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
