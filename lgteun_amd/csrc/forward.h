// Forward orchestration (Pansharpening.forward, reference models/unlg_former.py:50-67): what the per-op entries of api.hip call (k_fwd.hip).
#pragma once
#include "common.h"
#include "workspace.h"

int data_step_fwd(const lg_plan* pl, const float* P, int stage, const float* z_in, const float* ms, const float* pan,
                  float* z_out, float* t1, float* r, float* s1, float* pr, int B, hipStream_t s);
int prep_stages(const lg_plan* pl, const float* P, int st0, int st1, const NetBufs& nb, hipStream_t s);
int block_mixer_fwd(const Blk& k, int B, int flags, uint64_t seed, hipStream_t s, const StageSel& sg = StageSel());
int block_ffn_fwd(const Blk& k, const Blk* next, int B, int flags, hipStream_t s, const StageSel& sg = StageSel());
int lgt_fwd(const lg_plan* pl, const float* P, int stage, const float* z, float* out, const NetBufs& nb, int B, int flags, uint64_t seed,
            hipStream_t s, int nst = 1, long zstride = 0, int grid_cap = 0, float* live_out = nullptr);
