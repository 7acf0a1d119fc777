"""ctypes binding of libskyemb.so (the C ABI declared in include/skyemb.h).

The product path has NO fallback: if the HIP library is missing or fails to load,
every op raises ``SkyembLibraryError``.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

# torch bundles its own HIP runtime (torch/lib/libamdhip64.so).  It must be in the process BEFORE
# libskyemb.so is dlopen'ed so that both resolve to ONE runtime (otherwise kernels launched on
# torch's streams fail with "no ROCm-capable device is detected").
import torch  # noqa: F401  (import order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("SKYEMB_LIB") or os.path.join(_HERE, "libskyemb.so")   # SKYEMB_LIB: experiment builds
CSRC = os.path.join(_HERE, "csrc")

BF16, F32, F16 = 0, 1, 2
ABI_VERSION = 111          # skyemb_version() of the library this binding was written against (csrc/api.cpp)
KC, RC = 0, 1
ACT_NONE, ACT_GELU, ACT_DGELU = 0, 1, 2
COMBINE_MIN, COMBINE_MEAN, COMBINE_MAX = 0, 1, 2       # SKYEMB_COMBINE_*: how the token scores of an image are combined
METRIC_MSE, METRIC_MAE = 1, 2                          # SKYEMB_METRIC_*: the distance metrics of the patch-token search
# SKYEMB_MHA_*: kernel families of skyemb_mha_plan, and its switch bits
MHA_LDS, MHA_STREAM, MHA_MFMA_PACKED, MHA_MFMA_SINGLE, MHA_MFMA_STRIP, MHA_MFMA_LONG = range(6)
MHA_SW_NO_MFMA, MHA_SW_WPB1, MHA_SW_WPB4 = 1, 2, 4
# SKYEMB_PF_*: skyemb_prefilter_plan's request kinds, bank kinds and the "SKYEMB_PREFILTER_LO is unset" value of its lo switch
PF_ROWS, PF_TOKENS, PF_TOKENS_MEAN = range(3)
PF_BANK_F32, PF_BANK_F16, PF_BANK_BF16 = range(3)
PF_LO_UNSET, PF_MAX_SLICES = 2, 6
PROBE_CHUNKS, PROBE_MAX_F, PROBE_MIN_K, PROBE_MAX_K = 32, 4096, 3, 16   # SKYEMB_PROBE_*: limits of the linear-probe fits


class SkyembLibraryError(RuntimeError):
    pass


class SkyembError(RuntimeError):
    pass


c_i32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
c_f64 = ctypes.c_double


class GemmArgs(ctypes.Structure):
    _fields_ = [
        ("A", c_vp), ("B", c_vp), ("lda", c_i64), ("ldb", c_i64), ("a_layout", c_i32), ("b_layout", c_i32),
        ("M", c_i32), ("N", c_i32), ("K", c_i32), ("dtype", c_i32), ("alpha", c_f32),
        ("bias", c_vp), ("table", c_vp), ("tab_row", c_vp), ("ldt", c_i64), ("dst_row", c_vp),
        ("resid", c_vp), ("ldr", c_i64), ("aux", c_vp), ("ldaux", c_i64), ("act", c_i32),
        ("out_f32", c_vp), ("ldo32", c_i64), ("out", c_vp), ("ldo", c_i64), ("out2", c_vp), ("ldo2", c_i64),
        ("tile", c_i32), ("colsum_a", c_vp), ("ws", c_vp), ("ws_bytes", c_i64), ("split_k", c_i32), ("prefetch_wgs", c_i32),
        ("prefetch", c_vp), ("prefetch_bytes", c_i64),
    ]


class AdamwDesc(ctypes.Structure):
    """skyemb_adamw_desc (include/skyemb.h): the optimiser step fused into a grouped weight-gradient launch."""
    _fields_ = [("g_base", c_vp), ("p", c_vp), ("m", c_vp), ("v", c_vp), ("p_lp", c_vp), ("hyper", c_vp), ("n_decay", c_i64),
                ("beta1", c_f32), ("beta2", c_f32), ("eps", c_f32), ("weight_decay", c_f32), ("grad_scale", c_f32), ("enabled", c_i32)]


class LnBwdSide(ctypes.Structure):
    """skyemb_ln_bwd_side (include/skyemb.h): a LayerNorm backward riding in a grouped weight-gradient launch."""
    _fields_ = [("dy", c_vp), ("x", c_vp), ("gamma", c_vp), ("mean", c_vp), ("rstd", c_vp), ("g_in", c_vp), ("g_out", c_vp), ("g_lp", c_vp),
                ("part", c_vp), ("M", c_i32), ("D", c_i32)]


class MhaPlan(ctypes.Structure):
    """skyemb_mha_plan_t (include/skyemb.h): the launch skyemb_mha_fwd / skyemb_mha_bwd makes for a shape."""
    _fields_ = [("family", c_i32), ("hd", c_i32), ("waves", c_i32), ("per_wave_floats", c_i32), ("nheads", c_i32),
                ("grid_x", c_i32), ("grid_y", c_i32), ("block", c_i32), ("lds_bytes", c_i64), ("lds_limit", c_i64)]


class PrefilterRequest(ctypes.Structure):
    """skyemb_prefilter_request_t (include/skyemb.h): one call of a two-stage search entry point, without its pointers."""
    _fields_ = [("kind", c_i32), ("bank", c_i32), ("Q", c_i32), ("P", c_i32), ("D", c_i32), ("k", c_i32), ("N", c_i64), ("combine", c_i32),
                ("top_t", c_i32), ("has_thr0", c_i32), ("sel", c_i32), ("n_live", c_i32), ("last_live", c_i32), ("direct_sel", c_i32),
                ("lo", c_i32), ("eps", c_f32)]


class PrefilterSlice(ctypes.Structure):
    _fields_ = [("mode", c_i32), ("t0", c_i32), ("t1", c_i32), ("bucket", c_i32), ("tail", c_i32), ("tail_sel", c_i32), ("tail_pos", c_i32),
                ("final", c_i32)]


class PrefilterPlan(ctypes.Structure):
    """skyemb_prefilter_plan_t (include/skyemb.h): what the entry point serving a request decides and launches."""
    _fields_ = [("use_lo", c_i32), ("cap", c_i32), ("T", c_i32), ("T_tail", c_i32), ("has_tail", c_i32), ("first", c_i32),
                ("first_rows", c_i32), ("direct_end", c_i32), ("ends", c_i32 * 6), ("sel", c_i32), ("bf", c_i32), ("tok", c_i32),
                ("cnt", c_i32), ("tok_word", c_i32), ("lgp", c_i32), ("fold", c_i32), ("top_t", c_i32), ("q_padded", c_i32),
                ("lds_stage1", c_i32), ("lds_close", c_i32), ("lds_rescore", c_i32), ("lds_stage1_limit", c_i32),
                ("lds_close_limit", c_i32), ("eps_a_f32", c_f32), ("gfac", c_f32), ("eps_a", c_f64), ("rows", c_i64), ("n_slices", c_i32),
                ("slice", PrefilterSlice * 6)]


class AdamwGroup(ctypes.Structure):
    """skyemb_adamw_group (include/skyemb.h): the scalars of one parameter group of a segmented AdamW launch."""
    _fields_ = [("lr", c_f32), ("bc1", c_f32), ("bc2", c_f32), ("beta1", c_f32), ("beta2", c_f32), ("eps", c_f32), ("wd", c_f32),
                ("decayed", c_i32)]


class AdamwSegment(ctypes.Structure):
    """skyemb_adamw_segment: elements [offset, offset + n) of a flat buffer and the group that steps them."""
    _fields_ = [("offset", c_i64), ("n", c_i64), ("group", c_i32), ("reserved", c_i32)]


class GemmGroupInfo(ctypes.Structure):
    _fields_ = [("total_blocks", c_i32), ("tile", c_i32), ("class_mask", c_i32), ("reserved", c_i32)]


# name -> (restype, argtypes); must list every symbol include/skyemb.h declares (tests check this)
PROTOTYPES = {
    "skyemb_last_error": (ctypes.c_char_p, []),
    "skyemb_version": (c_i32, []),
    "skyemb_debug_skip": (c_i32, [c_i32]),
    "skyemb_gemm_launch_counts": (c_i32, [c_vp, c_i32, c_i32]),
    "skyemb_gemm": (c_i32, [ctypes.POINTER(GemmArgs), c_vp]),
    "skyemb_gemm_group_blob_bytes": (c_i64, [c_i32]),
    "skyemb_gemm_group_plan": (c_i32, [ctypes.POINTER(GemmArgs), c_i32, c_i32, c_vp, c_i64, ctypes.POINTER(GemmGroupInfo)]),
    "skyemb_set_scalars": (c_i32, [c_vp, c_f32, c_f32, c_f32, c_f32, c_vp]),
    "skyemb_gemm_group_plan_adamw": (c_i32, [ctypes.POINTER(GemmArgs), c_i32, c_i32, ctypes.POINTER(AdamwDesc), c_vp, c_i64,
                                             ctypes.POINTER(GemmGroupInfo)]),
    "skyemb_gemm_group_plan_side_adamw": (c_i32, [ctypes.POINTER(GemmArgs), c_i32, c_i32, ctypes.POINTER(AdamwDesc), c_i32, c_i64, c_i64, c_i32,
                                                  c_vp, c_i64, ctypes.POINTER(GemmGroupInfo)]),
    "skyemb_gemm_group_attach_ln_bwd": (c_i32, [c_vp, c_i64, ctypes.POINTER(GemmGroupInfo), ctypes.POINTER(LnBwdSide)]),
    "skyemb_gemm_group_launch": (c_i32, [c_vp, ctypes.POINTER(GemmGroupInfo), c_vp]),
    "skyemb_colsum": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "skyemb_random_mask_from_noise": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "skyemb_simmim_mask_from_noise": (c_i32, [c_vp, c_vp, ctypes.c_double, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "skyemb_patch_gather": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32,
                                    c_f32, c_vp]),
    "skyemb_patch_gather_bwd_pmv": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32,
                                            c_vp]),
    "skyemb_layernorm_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_f32, c_vp]),
    "skyemb_patch_gather_blend": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_vp]),
    "skyemb_patch_gather_bwd_pmv_blend": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_radec_token_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "skyemb_radec_token_bwd": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp]),
    "skyemb_simmim_pixel_loss": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32,
                                         c_f32, c_f32, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "skyemb_gather_rows_host": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_i32]),
    "skyemb_h5_unchunk_host": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32]),
    "skyemb_fits_decode_tiles_host": (c_i32, [c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_i64, c_i32]),
    "skyemb_fits_dequantise_tiles_host": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32,
                                                  c_vp, c_i64, c_i64, c_i32, c_i32]),
    "skyemb_augment": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_attnpool_q": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "skyemb_attnpool_fwd": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_attnpool_bwd": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_attnpool_fwd_long": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_attnpool_bwd_long": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_attnpool_q_bwd": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "skyemb_tile_cutouts": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_f32, c_f32, c_i32, c_i32, c_vp, c_vp]),
    "skyemb_clip_crop": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_f32, c_f32, c_i32, c_i32, c_vp]),
    "skyemb_layernorm_bwd_blocks": (c_i32, [c_i32]),
    "skyemb_layernorm_bwd_reduce_batch": (c_i32, [c_vp, c_vp, c_i32, c_vp]),
    "skyemb_layernorm_bwd": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                     c_i32, c_i32, c_vp]),
    "skyemb_mha_fwd": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_mha_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    # read-only query of the attention launch plan: additive to ABI version 111
    "skyemb_mha_plan": (c_i32, [c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(MhaPlan)]),
    "skyemb_fill_mask_tokens": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_gather_rows": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "skyemb_rowsum_select": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "skyemb_masked_patch_loss": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_i32,
                                         c_i32, c_i32, c_f32, c_f32, c_i32, c_i32, c_f32, c_vp]),
    "skyemb_adamw": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_f32, c_f32, c_f32, c_f32,
                             c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_vp]),
    "skyemb_cast": (c_i32, [c_vp, c_vp, c_i32, c_i64, c_vp]),
    # overflow guard of a dynamically scaled optimiser step: additive to ABI version 111
    "skyemb_grad_probe": (c_i32, [c_vp, c_i32, c_i64, c_vp, c_vp]),
    "skyemb_adamw_guarded": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_f32, c_f32, c_f32, c_f32,
                                     c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_vp, c_vp]),
    # multi-tensor AdamW over segments of a flat buffer (csrc/adamw_segments.hip): additive again
    "skyemb_adamw_segments_limits": (c_i32, [c_vp, c_vp, c_vp]),
    "skyemb_adamw_segments_plan": (c_i32, [c_vp, c_i32, c_i32, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "skyemb_adamw_segments": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_f32, c_vp, c_vp]),
    "skyemb_standardise": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp]),
    "skyemb_weighted_norms": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp]),
    "skyemb_cosine_topk_chunks": (c_i32, [c_i64, c_i32, c_i32, c_i32]),
    "skyemb_cosine_topk": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_i32, c_f32, c_i64, c_i32, c_vp, c_vp,
                                   c_vp, c_vp]),
    "skyemb_kth_largest_floor": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "skyemb_cosine_sample_floor": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp]),
    "skyemb_cosine_sample_floor_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32]),
    "skyemb_topk_merge": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_topk_prefilter_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32]),
    "skyemb_topk_prefilter_ws_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "skyemb_topk_prefilter_ws_layout": (c_i32, [c_i32, c_i32, c_i32, c_vp, c_i32]),     # test / diagnostic hook: additive
    "skyemb_bank16_bytes": (c_i64, [c_i64, c_i32]),
    "skyemb_bank16_rowp_rows": (c_i64, [c_i64]),
    "skyemb_bank16_prepare": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_prefiltered": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_f32, c_i64, c_vp,
                                               c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    # the two-stage search over a resident fp16 bank: additive to ABI version 111
    "skyemb_bank16_rowp_lp": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_prefiltered_lp": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_f32, c_i64, c_vp,
                                                  c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_topk_prefilter_eps_a": (c_f64, [c_i32, c_i32, c_i32]),
    # the two-stage search under a selection of the bank's rows: additive again
    "skyemb_prefilter_select_prepare": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_prefiltered_sel": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_i32,
                                                   c_f32, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_prefiltered_lp_sel": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_i32,
                                                      c_f32, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    # the two-stage search over a resident 16-bit bank of either format (a dtype code: fp16 or bf16): additive again
    "skyemb_resident_rowp": (c_i32, [c_vp, c_i32, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_prefiltered_resident": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_f32, c_i64,
                                                        c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_prefiltered_resident_sel": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i64,
                                                            c_i32, c_i32, c_f32, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_topk_prefilter_eps_a_resident": (c_f64, [c_i32, c_i32, c_i32]),
    # the two-stage search over a resident 16-bit patch-token bank (min | max): additive again
    "skyemb_token_prefilter_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32, c_i32]),
    "skyemb_token_prefilter_ws_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "skyemb_cosine_topk_tokens_prefiltered": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32,
                                                      c_f32, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    # ... and under a selection of the bank's images: additive again
    "skyemb_token_prefilter_select_prepare": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_tokens_prefiltered_sel": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32,
                                                          c_i64, c_i32, c_i32, c_i32, c_i32, c_f32, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp,
                                                          c_vp, c_vp]),
    # ... and under top_t (min: the count of passing rows; max: the plain call): additive again
    "skyemb_token_topt_prefilter_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32]),
    "skyemb_cosine_topk_tokens_prefiltered_top": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32,
                                                          c_i32, c_i32, c_f32, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_tokens_prefiltered_top_sel": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32,
                                                              c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_i64, c_vp, c_vp, c_i64,
                                                              c_vp, c_vp, c_vp, c_vp]),
    # ... and with combine mean, over the pooled image of the bank: additive again
    "skyemb_token_mean_pool": (c_i32, [c_vp, c_i32, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    # read-only query of the two-stage searches' launch plan: additive to ABI version 111
    "skyemb_prefilter_plan": (c_i32, [ctypes.POINTER(PrefilterRequest), ctypes.POINTER(PrefilterPlan)]),
    "skyemb_token_mean_prefilter_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32, c_i32]),
    "skyemb_token_mean_prefilter_ws_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "skyemb_token_mean_prefilter_eps_m": (c_f64, [c_i32, c_i32, c_i32]),
    "skyemb_cosine_topk_tokens_mean_prefiltered": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32,
                                                           c_i32, c_f32, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    # ... and mean under a selection of images, over the compacted pooled image: additive again
    "skyemb_token_mean_select_gather": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_cosine_topk_tokens_mean_prefiltered_sel": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_i32,
                                                               c_i32, c_i32, c_i32, c_f32, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp,
                                                               c_vp]),
    # weighted MSE (min | max) over a resident 16-bit token bank in the same two stages: additive again
    "skyemb_token_mse_prefilter_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32, c_i32]),
    "skyemb_token_mse_prefilter_eps": (c_f64, [c_i32, c_i32, c_i32]),
    "skyemb_token_mse_prefilter_gamma": (c_f64, [c_i32]),
    "skyemb_token_mse_rowp": (c_i32, [c_vp, c_i32, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "skyemb_distance_topk_tokens_prefiltered": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i64,
                                                        c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    # ... under top_t and under a selection of images: the cosine _top / _sel lists with c, t in place of tw, qn, xn, eps
    "skyemb_token_mse_topt_prefilter_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32]),
    "skyemb_distance_topk_tokens_prefiltered_top": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32,
                                                            c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_distance_topk_tokens_prefiltered_sel": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i64, c_i32,
                                                            c_i32, c_i32, c_i32, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_distance_topk_tokens_prefiltered_top_sel": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i64,
                                                                c_i32, c_i32, c_i32, c_i32, c_i32, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp,
                                                                c_vp]),
    # ... with per-query weights c [Q, D]: a second 16-bit image [x ; x o x] of the bank, additive again
    "skyemb_token_mse_pq_prefilter_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32, c_i32]),
    "skyemb_token_mse_pq_prefilter_eps": (c_f64, [c_i32, c_i32, c_i32]),
    "skyemb_token_mse_pq_image": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "skyemb_distance_topk_tokens_prefiltered_pq": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i64,
                                                           c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    # ... under combine mean: a pooled 16-bit image [N, D] of the bank and its constants, additive again
    "skyemb_token_mse_mean_prefilter_applicable": (c_i32, [c_i32, c_i64, c_i32, c_i32, c_i32]),
    "skyemb_token_mse_mean_prefilter_eps": (c_f64, [c_i32, c_i32, c_i32]),
    "skyemb_token_mse_mean_prefilter_gamma": (c_f64, [c_i32, c_i32]),
    "skyemb_token_mse_mean_pool": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_token_mse_mean_rowp": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "skyemb_distance_topk_tokens_mean_prefiltered": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i64,
                                                             c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_cosine_scores": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_f32, c_vp, c_vp]),
    "skyemb_cosine_token_applicable": (c_i32, [c_i32, c_i32, c_i32, c_i32]),
    "skyemb_cosine_token_topk_chunks": (c_i32, [c_i64, c_i32, c_i32, c_i32, c_i32]),
    "skyemb_cosine_token_scores": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp]),
    "skyemb_cosine_token_topk": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_f32, c_i64, c_i32, c_vp,
                                         c_vp, c_vp, c_vp]),
    # half-precision resident banks: additive to ABI version 111 (nothing above changed, so the version did not)
    "skyemb_cosine_token_scores_lp": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp]),
    "skyemb_cosine_token_topk_lp": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_f32, c_i64, c_i32,
                                            c_vp, c_vp, c_vp, c_vp]),
    "skyemb_weighted_norms_lp": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i64, c_i32, c_vp]),
    "skyemb_standardise_lp": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_vp]),
    # top-t combine (n_top_sims): additive again
    "skyemb_cosine_token_scores_top": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp,
                                               c_vp]),
    "skyemb_cosine_token_topk_top": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32,
                                             c_i64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    # selection of images (a packed bitmask): additive again
    "skyemb_cosine_token_scores_sel": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp,
                                               c_vp, c_vp]),
    "skyemb_cosine_token_topk_sel": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32,
                                             c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_pack_select": (c_i32, [c_vp, c_i64, c_vp, c_vp]),
    # weighted MSE / MAE over a token bank: additive again
    "skyemb_distance_token_scores": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "skyemb_distance_token_topk": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i64, c_i32,
                                           c_vp, c_vp, c_vp, c_vp, c_vp]),
    # per-query feature weights (w / c [Q, D]): additive again
    "skyemb_cosine_token_pq_applicable": (c_i32, [c_i32, c_i32, c_i32, c_i32]),
    "skyemb_cosine_token_scores_pq": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp,
                                              c_vp, c_vp]),
    "skyemb_cosine_token_topk_pq": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32,
                                            c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_distance_token_scores_pq": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp,
                                                c_vp]),
    "skyemb_distance_token_topk_pq": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i64,
                                              c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    # linear-probe fits on the device (csrc/probe.hip): additive again
    "skyemb_probe_colstats": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_probe_scale": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "skyemb_probe_softmax_ws_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "skyemb_probe_softmax_loss_grad": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_f64, c_vp, c_vp, c_vp, c_vp, c_i64,
                                               c_vp]),
    "skyemb_probe_gram": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "skyemb_probe_enet_cd": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_f64, c_f64, c_i32, c_f64, c_vp, c_vp, c_vp, c_vp]),
}

_LIB = None


def build(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into sky_embeddings_amd/libskyemb.so (hipcc, no GPU needed)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    return SO_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise SkyembLibraryError(
                f"{SO_PATH} is missing: the HIP hot-path library has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C sky_embeddings_amd/csrc`). "
                "There is no CPU fallback.")
        try:
            L = ctypes.CDLL(SO_PATH)
        except OSError as e:  # pragma: no cover
            raise SkyembLibraryError(f"cannot load {SO_PATH}: {e}") from e
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise SkyembLibraryError(f"{SO_PATH} does not export {name}") from e
            fn.restype, fn.argtypes = res, args
        if L.skyemb_version() != ABI_VERSION:    # struct layouts / argument lists changed between versions: never call across them
            raise SkyembLibraryError(f"{SO_PATH} reports ABI version {L.skyemb_version()}, this binding is written against "
                                     f"{ABI_VERSION}: rebuild the library (make -C sky_embeddings_amd/csrc)")
        _LIB = L
    return _LIB


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().skyemb_last_error()
        raise SkyembError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
