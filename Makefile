# Builds the gfx950 HIP library (C ABI in include/lgteun_hip.h) in-tree.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
CSRC  := lgteun_amd/csrc
SRCS  := $(CSRC)/api.hip $(CSRC)/prof.hip $(CSRC)/route.hip $(CSRC)/k_fwd.hip $(CSRC)/k_pixel.hip $(CSRC)/k_dstep.hip $(CSRC)/k_fft.hip $(CSRC)/k_attn.hip $(CSRC)/k_attn_m.hip $(CSRC)/k_ffn.hip $(CSRC)/k_ffn_prep.hip $(CSRC)/k_ffn_x.hip $(CSRC)/k_ffn_xr.hip $(CSRC)/k_ffn_x32.hip $(CSRC)/k_ffn_x64.hip $(CSRC)/k_bwd.hip $(CSRC)/k_bwd_pixel.hip $(CSRC)/k_wgrad.hip $(CSRC)/k_ffn_bwd.hip $(CSRC)/k_ffn_bwd_x.hip $(CSRC)/k_ffn_dwbwd_x.hip $(CSRC)/k_ffn_dwbwd_h.hip $(CSRC)/k_ffn1_bwd_x32.hip $(CSRC)/k_attn_bwd.hip $(CSRC)/k_attn_bwd_f.hip $(CSRC)/k_attn_bwd_m.hip $(CSRC)/k_iqa.hip $(CSRC)/k_iqa_ext.hip $(CSRC)/k_batch.hip $(CSRC)/k_scene.hip $(CSRC)/k_wald.hip $(CSRC)/k_gradnorm.hip $(CSRC)/k_optim.hip $(CSRC)/k_qnr.hip $(CSRC)/k_recloss.hip $(CSRC)/k_classical.hip $(CSRC)/k_cs.hip
LIB   := lgteun_amd/_lgteun_hip.so
OBJS  := $(SRCS:.hip=.o)
# -fno-slp-vectorize: the SLP vectoriser turns scalar fp32 chains into v_pk_mul_f32 / v_pk_add_f32 pairs; packed fp32 issues at
# half rate on gfx950 and the pairing blocks mul+add -> fma contraction (k_attn: 3140 VALU instructions, 502 of them packed,
# vs 3099 unpacked).  Measured on one box, alternating runs: 9.28 -> 9.10 ms/step fp32, 8.96 -> 8.68 bf16 mode.
FLAGS := -O3 -std=c++17 -fno-slp-vectorize -fPIC -fvisibility=hidden --offload-arch=$(ARCH) -Wall -Wno-unused-function -Wno-unused-value

all: $(LIB)

# k_attn_m.hip: matrix-core results straight into VGPRs (the default form parks them in AGPRs at this register pressure: one
# v_accvgpr_read per value) and no canonicalising v_max in front of the softmax's fmaxf chain
$(CSRC)/k_attn_m.o: FLAGS += -mllvm -amdgpu-mfma-vgpr-form -fno-honor-nans
$(CSRC)/k_attn_bwd_m.o: FLAGS += -mllvm -amdgpu-mfma-vgpr-form -fno-honor-nans
# k_ffn_xr: the iterative ILP scheduler instead of the default max-occupancy one (the kernel is pinned at two waves per SIMD anyway): 77.25 -> 76.36 us
# per fused-FFN launch, 5.134 -> 5.119 ms per step (same-box A/B; max-ilp measures the same; neither pays in k_attn_m, k_ffn1_bwd_xs, k_fftmix_r, k_attn_bwd_f)
$(CSRC)/k_ffn_xr.o: FLAGS += -mllvm -amdgpu-sched-strategy=iterative-ilp

# prerequisites come from the compiler (-MMD writes one .d file per object: every header a source includes, hstore.h too)
# (every object also depends on this file: a changed flag must rebuild what it applies to)
$(CSRC)/%.o: $(CSRC)/%.hip Makefile
	$(HIPCC) $(FLAGS) -MMD -MP -c $< -o $@

-include $(OBJS:.o=.d)

$(LIB): $(OBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(OBJS) -o $@

clean:
	rm -f $(CSRC)/*.o $(CSRC)/*.d $(LIB)
.PHONY: all clean
