"""ctypes binding of the gfx950 HIP library (C ABI: include/lgteun_hip.h).

Loaded lazily so modules stay picklable (the reference pickles whole module objects,
models/base/base_model.py:354-369).  There is NO fallback: if the shared object is missing the
product path raises -- the CPU restatement in oracle/ is test infrastructure only.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('LGTEUN_HIP_LIB') or os.path.join(_HERE, '_lgteun_hip.so')   # override: diagnostic builds (tools/build_stamps.sh)

LG_FLAG_FAITHFUL = 1
LG_FLAG_SAVE = 2
LG_FLAG_DROPOUT = 4
LG_FLAG_BWD_LGT = 8
LG_FLAG_BWD_DATA = 16
LG_FLAG_CHAINED = 32
LG_FLAG_DEFER_DEAD = 64
LG_FLAG_STAGEWISE = 128
LG_FLAG_LIVE_APART = 256
KERNEL_IDS = {n: i for i, n in enumerate(['none', 'ffn1', 'ffn', 'fft', 'attn', 'upfuse', 'down', 'embed', 'tail', 'datastep', 'ffn1_bwd',
                                           'ffn2_bwd', 'fft_bwd', 'attn_bwd', 'wgrad', 'batch', 'scene_gather', 'scene_blend'])}


class LgConfig(ctypes.Structure):
    _fields_ = [('C', c_int32), ('K', c_int32), ('H', c_int32), ('W', c_int32), ('precision', c_int32), ('variant', ctypes.c_uint32)]


class LgAtrousArgs(ctypes.Structure):
    """lg_atrous_args: the argument block of lg_atrous; struct_bytes = ctypes.sizeof(LgAtrousArgs)"""
    _fields_ = [('struct_bytes', ctypes.c_uint32), ('rule', c_int32), ('match', c_int32), ('B', c_int32), ('C', c_int32), ('h', c_int32), ('w', c_int32),
                ('ms', c_void_p), ('pan', c_void_p), ('out', c_void_p), ('stats', c_void_p), ('workspace', c_void_p), ('workspace_bytes', c_size_t),
                ('stream', c_void_p)]


class LgMtfHrArgs(ctypes.Structure):
    """lg_mtf_hr_args: the argument block of lg_mtf_hr; struct_bytes = ctypes.sizeof(LgMtfHrArgs)"""
    _fields_ = [('struct_bytes', ctypes.c_uint32), ('rule', c_int32), ('n_filters', c_int32), ('n_taps', c_int32), ('B', c_int32), ('C', c_int32),
                ('h', c_int32), ('w', c_int32), ('ms', c_void_p), ('pan', c_void_p), ('out', c_void_p), ('stats', c_void_p), ('taps', c_void_p),
                ('workspace', c_void_p), ('workspace_bytes', c_size_t), ('stream', c_void_p)]


# lg_config.variant bits (include/lgteun_hip.h): A/B kernels that compute the same function as the product path
LG_VAR_FFN_STRIP = 1
LG_VAR_FFN_SAVE3, LG_VAR_FFN_SAVE5 = 1 << 2, 2 << 2
LG_VAR_FFN_BWD32_PAIR, LG_VAR_FFN_DWBWD_TILE, LG_VAR_ATTN_BWD_R3 = 1 << 4, 1 << 5, 1 << 6
LG_VAR_DSTEP_TILES = 1 << 7
LG_VAR_ATTN_FWD_VALU = 1 << 8
LG_VAR_FFN_BF16X3 = 1 << 9
LG_VAR_FFT_FULL = 1 << 10
LG_VAR_FFN_BWD_BF16X3 = 1 << 11
LG_VAR_ATTN_BWD_CORE_M = 1 << 12
LG_VAR_FFN_XS = 1 << 13
LG_VAR_ATTN_BF16X3 = 1 << 14
LG_VAR_FFN_H3_RECOMPUTE = 1 << 15
LG_VAR_ATTN_BWD_RESTATS = 1 << 16
LG_VAR_REDUCE_PER_BLOCK = 1 << 17
LG_OPT_ADAM, LG_OPT_ADAMW, LG_OPT_SGD, LG_OPT_RMSPROP = 0, 1, 2, 3      # lg_optim_step: algo
LG_OPT_AMSGRAD, LG_OPT_NESTEROV, LG_OPT_CENTERED = 1, 2, 4             # lg_optim_step: flags
LG_DT_U8, LG_DT_U16, LG_DT_F32 = 0, 1, 2                                # lg_pyr_down2 / lg_batch_assemble: sample type of the store
LG_CLASSICAL_SFIM, LG_CLASSICAL_GSA = 0, 1                              # lg_classical_workspace_bytes: method
LG_MTFGLP_GLP, LG_MTFGLP_HPM, LG_MTFGLP_CBD = 0, 1, 2                   # lg_mtf_glp: mode (the injection rule)
LG_CS_IHS, LG_CS_BROVEY, LG_CS_GS, LG_CS_PCA = 0, 1, 2, 3                  # lg_cs: mode (the method)
LG_ATROUS_ATWT, LG_ATROUS_AWLP = 0, 1                                   # lg_atrous_args.rule
LG_ATROUS_MATCH_PAN, LG_ATROUS_MATCH_LOWPASS = 0, 1                     # lg_atrous_args.match
LG_MTFHR_FS, LG_MTFHR_HPM_R, LG_MTFHR_HPM_H, LG_MTFHR_BT_H = 0, 1, 2, 3    # lg_mtf_hr_args.rule
LG_ABI_VERSION = 2   # include/lgteun_hip.h: checked against lg_abi_version() when the library is loaded


def variant_from_env(env=None):
    """the variant word of a new plan from the diagnostic LG_* environment variables (read HERE, on the Python side, when an Engine
    builds a plan -- the shared library itself never looks at the environment).  Unset = 0 = the product path."""
    env = os.environ if env is None else env
    # ('tile' and 'xp' named kernels the library no longer carries: they keep their field values, which lg_plan_create rejects by name)
    v = {'strip': LG_VAR_FFN_STRIP, 'tile': 2, 'xp': 3}.get(env.get('LG_FFN_IMPL', ''), 0)
    v |= {'3': LG_VAR_FFN_SAVE3, '5': LG_VAR_FFN_SAVE5}.get(env.get('LG_FFN_SAVE', ''), 0)
    if env.get('LG_FFN_BWD32') == 'pair':
        v |= LG_VAR_FFN_BWD32_PAIR
    if env.get('LG_FFN_DWBWD') == 'tile':
        v |= LG_VAR_FFN_DWBWD_TILE
    if env.get('LG_ATTN_BWD') in ('old', 'r3'):
        v |= LG_VAR_ATTN_BWD_R3
    if env.get('LG_DSTEP') == 'tiles':
        v |= LG_VAR_DSTEP_TILES
    if env.get('LG_ATTN_FWD', '') == 'valu':
        v |= LG_VAR_ATTN_FWD_VALU
    if env.get('LG_FFN_SPLIT', '') == 'bf16x3':
        v |= LG_VAR_FFN_BF16X3
    if env.get('LG_FFT', '') == 'full':
        v |= LG_VAR_FFT_FULL
    if env.get('LG_FFN_BWD_SPLIT', '') == 'bf16x3':
        v |= LG_VAR_FFN_BWD_BF16X3
    if env.get('LG_ATTN_BWD_CORE', '') == 'm':
        v |= LG_VAR_ATTN_BWD_CORE_M
    if env.get('LG_FFN_FWD', '') == 'xs':
        v |= LG_VAR_FFN_XS
    if env.get('LG_ATTN_SPLIT', '') == 'bf16x3':
        v |= LG_VAR_ATTN_BF16X3
    if env.get('LG_FFN_H3', '') == 'recompute':
        v |= LG_VAR_FFN_H3_RECOMPUTE
    if env.get('LG_ATTN_BWD_STATS', '') == 'recompute':
        v |= LG_VAR_ATTN_BWD_RESTATS
    if env.get('LG_REDUCE', '') == 'per_block':
        v |= LG_VAR_REDUCE_PER_BLOCK
    return v


class LgteunHipError(RuntimeError):
    pass


_lib = None

# name -> (restype, argtypes); every symbol include/lgteun_hip.h declares
SIGNATURES = {
    'lg_version': (c_char_p, []),
    'lg_abi_version': (c_int32, []),
    'lg_last_error': (c_char_p, []),
    'lg_plan_create': (c_int32, [POINTER(LgConfig), POINTER(c_int64), c_int32, POINTER(c_void_p)]),
    'lg_plan_destroy': (None, [c_void_p]),
    'lg_plan_describe': (c_int32, [c_void_p, c_char_p, c_size_t]),
    'lg_workspace_bytes': (c_size_t, [c_void_p, c_int32, c_int32]),
    'lgteun_forward': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_int32,
                                 c_uint64, c_void_p]),
    'lgteun_backward': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32,
                                  c_int32, c_uint64, c_void_p]),
    'lgteun_dead_forward': (c_int32, [c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_int32, c_uint64, c_void_p]),
    'lg_l1_loss': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_void_p]),
    'lg_adam_step': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_float, c_float,
                               c_float, c_float, c_float, c_void_p]),
    'lg_l2_loss': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_void_p]),
    'lg_optim_step': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32,
                                c_double, c_double, c_double, c_double, c_double, c_double, c_void_p]),
    'lg_grad_norm_workspace_bytes': (c_size_t, [c_int32, c_int64]),
    'lg_grad_norm': (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    'lg_optim_step_ex': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32,
                                   c_double, c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_double, c_int32,
                                   c_void_p]),
    'lg_op_resample': (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    'lg_op_data_step': (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                  c_void_p]),
    'lg_op_lgt': (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_int32, c_uint64,
                            c_void_p]),
    'lg_op_lgt_stages': (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_int32, c_uint64,
                                   c_int32, c_void_p]),
    'lg_debug_stage_runs': (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32]),
    'lg_debug_stage_decision': (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    'lg_workspace_deadout': (c_int32, [c_void_p, c_int32, c_int32, POINTER(c_size_t), POINTER(c_size_t)]),
    'lg_debug_live_slot': (c_int32, [c_void_p, c_int32, c_int32, POINTER(c_size_t)]),
    'lg_op_block': (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_int32,
                              c_void_p]),
    'lg_dropout_mask': (c_int32, [c_uint64, c_int32, c_int32, c_int64, c_int64, c_void_p, c_void_p]),
    'lg_prof_enable': (c_int32, [c_int32, c_int32]),
    'lg_prof_reset': (c_int32, []),
    'lg_prof_pause': (None, [c_int32]),
    'lg_prof_read': (c_int32, [POINTER(ctypes.c_double), POINTER(c_int64)]),
    'lg_prof_disable': (None, []),
    'lg_kernel_name': (c_char_p, [c_int32]),
    'lg_op_data_step_bwd': (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_int32, c_void_p]),
    'lg_op_lgt_bwd': (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_int32,
                                c_uint64, c_void_p]),
    'lg_op_block_bwd': (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_size_t, c_int32, c_void_p]),
    'lg_iqa_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    'lg_iqa_ref': (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_size_t, c_void_p]),
    'lg_iqa_no_ref': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_size_t,
                                c_void_p]),
    'lg_iqa_mtf_taps': (c_int32, [c_void_p]),
    'lg_iqa_ext_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    'lg_iqa_ref_ext': (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_size_t, c_void_p]),
    'lg_iqa_q2n': (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_size_t, c_void_p]),
    'lg_qnr_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    'lg_qnr_stats': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t,
                               c_void_p]),
    'lg_qnr_grad': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32, c_float,
                              c_int32, c_void_p, c_size_t, c_void_p]),
    'lg_recloss_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    'lg_sam_loss': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32, c_float, c_int32, c_void_p,
                              c_size_t, c_void_p]),
    'lg_ssim_loss': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32, c_float, c_float, c_int32,
                               c_void_p, c_size_t, c_void_p]),
    'lg_pyr_down2': (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p]),
    'lg_batch_assemble': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, c_float, c_void_p]),
    'lg_fir_decimate4': (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    'lg_window_assemble': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, c_float, c_void_p]),
    'lg_scene_gather': (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                  c_int32, c_int32, c_float, c_int32, c_float, c_void_p]),
    'lg_scene_blend': (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    'lg_scene_to_u16': (c_int32, [c_void_p, c_void_p, c_int64, c_float, c_void_p]),
    'lg_classical_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    'lg_interp23_up4': (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    'lg_sfim': (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    'lg_gsa': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    'lg_wavelet': (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    'lg_wavelet_taps': (c_int32, [c_void_p]),
    'lg_mtfglp_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    'lg_mtf_glp': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                             c_size_t, c_void_p]),
    'lg_bdsd_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    'lg_bdsd': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                          c_size_t, c_void_p]),
    'lg_cs_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    'lg_cs': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_double), c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    'lg_cs_taps': (c_int32, [POINTER(c_double), POINTER(c_double)]),
    'lg_atrous_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    'lg_atrous': (c_int32, [POINTER(LgAtrousArgs)]),
    'lg_atrous_taps': (c_int32, [POINTER(c_double)]),
    'lg_mtf_hr_workspace_bytes': (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    'lg_mtf_hr': (c_int32, [POINTER(LgMtfHrArgs)]),
}


def lib():
    """Load (once) and return the ctypes library.  Raises LgteunHipError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LgteunHipError(
                f'HIP extension not built: {LIB_PATH} is missing. Run `make` (or __graft_entry__.build()). '
                'lgteun_amd has no CPU/PyTorch fallback.')
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        got = int(L.lg_abi_version())
        if got != LG_ABI_VERSION:   # a stale .so next to newer Python (or the reverse) would read structs / buffers of the other layout
            raise LgteunHipError(f'{LIB_PATH}: ABI version {got}, this binding was written for {LG_ABI_VERSION} (include/lgteun_hip.h): rebuild with `make`')
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().lg_last_error().decode(errors='replace')
        raise LgteunHipError(f'{what} failed (rc={rc}): {msg}')
