"""ctypes binding of libtokensgen_hip.so (include/tokensgen_hip.h).  Fails loudly if the library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TG_LIB_PATH") or os.path.join(_HERE, "libtokensgen_hip.so")   # override: A/B builds in tools/
TG_MAX_GROUPS = 16

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU, EPI_BIAS_GATE_RES = 0, 1, 2, 3
EPI_BIAS_KEEP_GELU, EPI_BIAS_MUL_GELU_GRAD = 4, 5      # training step; 4-wave GEMM shapes only (kernels.gemm_act_supported)


class GroupTable(C.Structure):
    """struct tg_group_table"""
    _fields_ = [("mod", C.c_void_p), ("mod_ld", C.c_long), ("mod_batch_stride", C.c_long),
                ("tok_group", C.c_void_p), ("row", C.c_int32 * TG_MAX_GROUPS),
                ("shift_col", C.c_int32 * TG_MAX_GROUPS), ("scale_col", C.c_int32 * TG_MAX_GROUPS),
                ("gate_col", C.c_int32 * TG_MAX_GROUPS)]


_vp, _l, _i, _f, _d = C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_double
# name -> argtypes, exactly the prototypes of include/tokensgen_hip.h
PROTOTYPES = {
    "tg_gemm_bf16": [_vp, _l, _l, _vp, _l, _vp, _vp, _l, _l, _i, _i, _i, _i, _i, _vp, _l, _l, C.POINTER(GroupTable), _vp],
    "tg_gemm_bf16_pair": [_vp, _l, _vp, _vp, _vp, _l, _i, _vp, _l, _vp, _vp, _vp, _l, _i, _l, _l, _l, _i, _i, _i, _i, _vp],
    "tg_gemm_bf16_qkv": [_vp, _l, _vp, _vp, _vp, _l, _i, _vp, _l, _vp, _l, _vp, _vp, _vp, _l, _i, _vp, _l, _l, _l, _l, _i, _i, _i, _i, _vp],
    "tg_gemm_bf16_lora": [_vp, _l, _l, _vp, _l, _vp, _vp, _l, _l, _vp, _l, _f, _vp, _l, _l, _i, _i, _i, _i, _i, _vp],
    "tg_adaln_modulate": [_vp, _l, _l, _vp, _l, _l, _vp, _vp, _f, _i, _i, _i, _i, C.POINTER(GroupTable), _vp],
    "tg_qk_layernorm_rope": [_vp, _l, _l, _i, _i, _i, _vp, _vp, _f, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _f, _vp],
    "tg_qk_layernorm_rope_pair": [_vp, _vp, _l, _l, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _f, _f, _vp],
    "tg_qk_layernorm_rope_pair_kmax": [_vp, _vp, _l, _l, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _vp],
    "tg_qk_layernorm_rope_pair_out": [_vp, _vp, _l, _l, _vp, _vp, _l, _l, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _vp],
    "tg_transpose_v": [_vp, _l, _l, _i, _i, _i, _i, _vp, _l, _vp],
    "tg_attention_fwd": [_vp, _l, _l, _vp, _l, _l, _vp, _l, _i, _vp, _l, _l, _vp, _l, _l, _vp, _l, _i, _f, _vp, _l, _l,
                         _i, _i, _i, _f, _i, _vp],
    "tg_attention_fwd_multi": [_vp, _i, _i, _i, _f, _i, _vp, _vp],
    "tg_attention_bwd": [_vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l,
                         _i, _i, _i, _i, _f, _i, _vp, _vp, _vp],
    "tg_attention_bwd_ex": [_vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l,
                            _i, _i, _i, _i, _f, _i, _vp, _vp, _i, _vp, _vp],
    "tg_attention_bwd_multi": [_vp, _i, _i, _i, _i, _vp, _vp],
    "tg_attention_bwd_probe": [_vp, _l, _vp],
    "tg_attention_bwd_probe_verdict": [_vp, _l],
    "tg_attention_fwd_lse": [_vp, _l, _l, _vp, _l, _l, _vp, _l, _i, _vp, _l, _l, _i, _i, _i, _f, _vp, _vp],
    "tg_attention_fwd_lse_ex": [_vp, _l, _l, _vp, _l, _l, _vp, _l, _i, _vp, _l, _l, _i, _i, _i, _f, _i, _vp, _vp, _l, _vp, _vp],
    "tg_qk_layernorm_rope_bwd": [_vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _i, _i, _i, _vp, _f, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _f, _vp, _vp],
    "tg_transpose_2d": [_vp, _l, _i, _i, _vp, _l, _i, _vp],
    "tg_colsum": [_vp, _l, _i, _i, _vp, _vp],
    "tg_adaln_modulate_bwd": [_vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _vp, _f, _i, _i, _i, _i, C.POINTER(GroupTable), _vp, _vp, _vp, _vp, _l, _l, _vp],
    "tg_gate_residual_bwd": [_vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _i, _i, _i, C.POINTER(GroupTable), _vp, _i, _vp],
    "tg_act": [_vp, _vp, _vp, _l, _i, _vp],
    "tg_colsum_f32": [_vp, _l, _i, _i, _vp, _vp],
    "tg_colsum_multi": [_vp, _i, _i, _vp, _vp],
    "tg_grad_accumulate_multi": [_vp, _i, _f, _vp],
    "tg_grad_accumulate": [_vp, _i, _vp, _l, _f, _i, _vp],
    "tg_grad_clip_coef": [_vp, _l, _f, _vp, _vp, _vp],
    "tg_adamw_step": [_vp, _vp, _vp, _vp, _l, _i, _f, _f, _f, _f, _f, _vp, _i, _vp],
    "tg_adamw8bit_step": [_vp] * 11 + [_i, _l, _i, _i, _f, _f, _f, _f, _f, _vp, _i, _vp],
    "tg_adamw_step_sr": [_vp, _vp, _vp, _vp, _l, _i, _f, _f, _f, _f, _f, _vp, _i, _l, C.c_ulonglong, _vp],
    "tg_adamw8bit_step_sr": [_vp] * 11 + [_i, _l, _i, _i, _f, _f, _f, _f, _f, _vp, _i, C.c_ulonglong, _vp],
    "tg_prodigy_step": [_vp] * 9 + [_l, _l, _i] + [_d] * 9 + [_i, _i, _i, _vp, _i, _vp],
    "tg_lora_wgrad": [_vp, _l, _l, _vp, _l, _l, _i, _i, _i, _i, _vp, _l, _l, _f, _f, _vp, _vp],
    "tg_lora_merge": [_vp, _l, _vp, _l, _vp, _l, _vp, _l, _i, _i, _i, _f, _vp],
    "tg_vpred_loss_grad": [_vp, _vp, _vp, _vp, _i, _l, _f, _vp, _vp, _vp],
    "tg_vpred_loss_grad_masked": [_vp, _vp, _vp, _vp, _vp, _i, _i, _l, _vp, _vp, _vp],
    "tg_timestep_sinusoid": [_vp, _i, _i, _vp, _vp],
    "tg_rope_table_3d": [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp],
    "tg_patchify": [_vp, _vp, _l, _i, _i, _i, _i, _i, _vp],
    "tg_unpatchify": [_vp, _l, _vp, _i, _i, _i, _i, _i, _vp],
    "tg_cfg_dpm_step": [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _l, _vp],
    "tg_cfg_dpm_step_f32": [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _l, _vp],
    "tg_cfg_dpm_step_ex": [_vp, _i, _vp, _vp, _vp, _vp, _f, _f, _vp, _i, _i, _i, _vp, _vp, _i, _l, _vp],
    "tg_pca_inverse": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "tg_pca_lowrank_filter": [_vp, _l, _vp, _vp, _vp, _l, _i, _i, _i, _vp],
    "tg_pca_project16": [_vp, _l, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp],
    "tg_gram_accumulate": [_vp, _l, _l, _i, _vp, _vp, _vp],
    "tg_pca_coef_stats": [_vp, _l, _l, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "tg_video_resample": [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp],
    "tg_video_to_uint8": [_vp, _l, _l, _l, _i, _i, _i, _i, _vp, _i, _i, _vp],
    "tg_image_metrics_window": [_vp],
    "tg_image_metrics": [_vp, _l, _l, _l, _l, _l, _vp, _l, _l, _l, _l, _l, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp],
    "tg_lpips_conv_in": [_vp, _l, _l, _l, _l, _l, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "tg_relu_cl": [_vp, _l, _vp],
    "tg_relu_maxpool2_cl": [_vp, _i, _i, _i, _i, _vp, _vp],
    "tg_lpips_head": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp],
    "tg_rmsnorm": [_vp, _l, _vp, _vp, _l, _l, _i, _f, _vp],
    "tg_t5_attention": [_vp, _vp, _vp, _l, _l, _vp, _vp, _i, _i, _i, _vp],
    "tg_gated_gelu": [_vp, _l, _vp, _l, _l, _i, _vp],
    "tg_residual_add": [_vp, _vp, _vp, _l, _vp],
    "tg_vit_patch_rows": [_vp, _i, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp, _i, _vp],
    "tg_vit_assemble": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "tg_layernorm": [_vp, _l, _vp, _vp, _vp, _l, _l, _i, _f, _vp],
    "tg_vit_act": [_vp, _vp, _l, _i, _vp],
    "tg_feature_consistency": [_vp, _l, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "tg_text_embed": [_vp, _l, _i, _vp, _i, _vp, _vp, _l, _i, _vp, _vp],
    "tg_text_alignment": [_vp, _l, _i, _vp, _l, _i, _i, _vp, _vp],
    "tg_luma_u8": [_vp, _l, _l, _l, _l, _l, _i, _i, _i, _i, _vp, _vp],
    "tg_block_motion": [_vp, _l, _l, _vp, _l, _l, _i, _i, _i, _i, _l, _i, _i, _vp, _vp, _vp, _vp],
    "tg_block_warp_sse": [_vp, _l, _l, _l, _l, _l, _vp, _l, _l, _l, _l, _l, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "tg_mci_select": [_vp, _l, _l, _vp, _l, _l, _vp, _vp, _i, _i, _i, _i, _l, _i, _i, _vp, _vp, _vp],
    "tg_mci_render": [_vp, _l, _l, _l, _l, _l, _vp, _l, _l, _l, _l, _l, _vp, _i, _i, _i, _i, _i, _i, _vp, _l, _l, _vp],
    "tg_color_hist_u8": [_vp, _i, _i, _i, _vp, _vp],
    "tg_color_match_lut": [_vp, _i, _vp, _i, _vp, _i, _d, _i, _d, _vp, _vp, _vp],
    "tg_color_apply_lut": [_vp, _vp, _i, _i, _i, _vp, _vp],
    "tg_lab_metrics": [_vp, _l, _l, _l, _l, _l, _vp, _l, _l, _l, _l, _l, _i, _i, _i, _i, _i, _vp, _vp, _vp],
    "tg_jpeg_coeffs": [_vp, _i, _i, _i, _i, _i, _vp, _vp],
    "tg_jpeg_segment_bytes": [_vp, _i, _i, _i, _i, _i, _vp, _vp],
    "tg_jpeg_write": [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _l, _vp],
    "tg_jpeg_huff_table": [_vp, _vp, _i, _vp],
    "tg_jpeg_find_segments": [_vp, _l, _vp, _vp, _i, _l, _vp, _vp, _vp, _vp],
    "tg_jpeg_decode_coeffs": [_vp, _l, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp],
    "tg_jpeg_decode_coeffs_sync": [_vp, _l, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _l, _vp, _vp, _vp, _vp],
    "tg_jpeg_idct_rgb": [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _l, _vp, _l, _vp],
    "tg_png_filter": [_vp, _i, _i, _i, _i, _i, _vp, _vp],
    "tg_png_band_plan": [_vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "tg_png_write": [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _l, _vp],
    "tg_png_inflate": [_vp, _l, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "tg_png_unfilter": [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "tg_conv3d_cl": [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _l, _i, _i, _i, _vp, _vp, _vp, _vp],
    "tg_conv3d_up2_subpixel": [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _l, _i, _vp, _vp, _vp],
    "tg_groupnorm_finalize": [_vp, _l, _i, _f, _vp, _vp],
    "tg_groupnorm_stats": [_vp, _l, _i, _f, _vp, _vp, _vp],
    "tg_groupnorm_silu": [_vp, _l, _i, _vp, _vp, _vp, _vp, _i, _vp],
    "tg_spatialnorm_silu": [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _vp, _i, _vp],
    "tg_groupnorm_reduce": [_vp, _l, _vp, _vp],
    "tg_groupnorm_silu_ex": [_vp, _l, _i, _vp, _vp, _l, _i, _f, _vp, _vp, _vp, _i, _vp],
    "tg_spatialnorm_silu_ex": [_vp, _i, _i, _i, _i, _vp, _vp, _l, _i, _f, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _vp, _i, _vp],
    "tg_avgpool_time": [_vp, _i, _l, _i, _vp, _vp],
    "tg_ncdhw_to_cl": [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp],
    "tg_cl_to_ncdhw": [_vp, _l, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tg_tile_blend": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
}

# name -> argtypes of the `long tg_*(...)` pure host queries (workspace sizes, which kernel a shape gets)
QUERIES = {
    "tg_gemm_kernel": [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long],
    "tg_groupnorm_partial_floats": [C.c_long, C.c_int],
    "tg_conv3d_gn_partial_floats": [C.c_int, C.c_int, C.c_int],
    "tg_conv3d_up2_subpixel_gn_floats": [C.c_int, C.c_int, C.c_int],
    "tg_conv3d_up2_subpixel_ok": [C.c_int] * 5,
    "tg_groupnorm_reduce_rows": [C.c_long],
    "tg_conv3d_splitk_floats": [C.c_int] * 9,
    "tg_conv3d_kernel": [C.c_int] * 18,
    "tg_conv3d_splitk_plan": [C.c_int] * 18,
    "tg_attention_bwd_ws_floats": [C.c_int, C.c_int, C.c_int, C.c_int],
    "tg_attention_bwd_probe_bytes": [],
    "tg_attention_retry_ints": [C.c_int, C.c_int, C.c_int, C.c_int],
    "tg_attention_split_floats": [C.c_int, C.c_int, C.c_int, C.c_int],
    "tg_qk_kmax_ws_floats": [C.c_int, C.c_int, C.c_int],
    "tg_qk_layernorm_rope_bwd_partial_floats": [C.c_int, C.c_int, C.c_int],
    "tg_colsum_partial_floats": [C.c_int, C.c_int],
    "tg_vpred_loss_partial_floats": [C.c_int, C.c_long],
    "tg_grad_norm_ws_floats": [],
    "tg_prodigy_ws_doubles": [],
    "tg_lora_wgrad_ws_floats": [C.c_int, C.c_int, C.c_int],
    "tg_gram_fold_rows": [],
    "tg_pca_coef_stats_ws_floats": [C.c_long, C.c_int],
    "tg_image_metrics_tile": [C.c_int],
    "tg_image_metrics_ws_doubles": [C.c_long, C.c_int, C.c_int],
    "tg_lpips_head_ws_doubles": [C.c_int, C.c_int, C.c_int],
    "tg_luma_pitch": [C.c_int],
    "tg_color_strip_bytes": [C.c_int],
    "tg_lab_metrics_tile": [C.c_int],
    "tg_lab_metrics_ws_doubles": [C.c_long, C.c_int, C.c_int, C.c_int],
    "tg_jpeg_header_bytes": [],
    "tg_jpeg_geometry": [C.c_int] * 5,
    "tg_jpeg_huff_table_bytes": [],
    "tg_jpeg_decode_segments": [C.c_int] * 4,
    "tg_jpeg_idct_ws_bytes": [C.c_int] * 4,
    "tg_jpeg_sync_ws_bytes": [C.c_int] * 5,
    "tg_png_geometry": [C.c_int] * 4,
    "tg_png_decode_geometry": [C.c_int] * 4,
}

TG_BWD_ONE_KERNEL = 1
# declared in the header besides PROTOTYPES and QUERIES (bound by hand in load())
OTHER_EXPORTS = ("tg_version", "tg_last_error_string", "tg_debug_set", "tg_debug_get", "tg_debug_knob_name")

_lib = None


def load():
    """Load the shared library once; raise (never fall back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(make -C tokensgen_amd/csrc). tokensgen_amd has no CPU/PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.argtypes = argtypes
        fn.restype = C.c_int
    for name, argtypes in QUERIES.items():   # pure host functions returning a long (mostly a count of floats)
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_long
    lib.tg_version.restype = C.c_char_p
    lib.tg_last_error_string.restype = C.c_char_p
    lib.tg_debug_set.argtypes, lib.tg_debug_set.restype = [C.c_char_p, C.c_long], C.c_int
    lib.tg_debug_get.argtypes, lib.tg_debug_get.restype = [C.c_char_p, C.POINTER(C.c_long)], C.c_int
    lib.tg_debug_knob_name.argtypes, lib.tg_debug_knob_name.restype = [C.c_int], C.c_char_p
    _lib = lib
    # The library itself reads no environment variable.  The cross-check tests select between two product kernels of one operator per child process:
    # same-named environment variables are forwarded to tg_debug_set here, once, at load time (header: "Dispatch overrides for the cross-check tests").
    i = 0
    while True:
        name = lib.tg_debug_knob_name(i)
        if name is None:
            break
        if os.environ.get(name.decode()) not in (None, ""):
            check(lib.tg_debug_set(name, int(os.environ[name.decode()])), f"tg_debug_set({name.decode()})")
        i += 1
    return lib


def debug_set(knob, value):
    """tg_debug_set: dispatch override for a cross-check test (see the header); returns the previous value."""
    lib = load()
    old = C.c_long(0)
    check(lib.tg_debug_get(knob.encode(), C.byref(old)), f"tg_debug_get({knob})")
    check(lib.tg_debug_set(knob.encode(), int(value)), f"tg_debug_set({knob})")
    return old.value


def gemm_kernel(M, N, K, lda=0, ldw=0):
    """tg_gemm_kernel: what the library launches for this shape NOW (csrc/gemm_plan.h, the TG_GEMM_W4 knob included): 0 the 128x128 tile, 1 the 8-wave 256x256
    kernel, 2 the 4-wave one, < 0 a refused shape.  A leading dimension left at 0 means contiguous rows (K)."""
    return load().tg_gemm_kernel(M, N, K, lda or K, ldw or K)


# tg_conv3d_kernel's answers (enum ConvKernel, csrc/conv_plan.h)
CONV_IN8, CONV_HALO_NARROW, CONV_N16, CONV_HALO2, CONV_W4_256, CONV_W4_128, CONV_128, CONV_128_SPLITK = range(8)


def _conv_query_args(T, H, W, Cin, cout, cout_pad, kt, kh, kw, stride, pad, up, out_dims, t_map, residual, gn_partial):
    To, Ho, Wo = out_dims if out_dims is not None else (T, H, W)
    return (T, H, W, Cin, cout, cout_pad, kt, kh, kw, stride, pad, up, To, Ho, Wo, int(bool(t_map)), int(bool(residual)), int(bool(gn_partial)))


def conv3d_kernel(T, H, W, Cin, cout, cout_pad, kt, kh, kw, stride=1, pad=1, up=1, out_dims=None, t_map=False, residual=False, gn_partial=False):
    """tg_conv3d_kernel: which kernel tg_conv3d_cl launches for this shape NOW (csrc/conv_plan.h with the live TG_CONV_* knobs): one of the CONV_* values above, < 0 a
    refused shape.  out_dims left at None means (T, H, W); t_map / residual / gn_partial: whether the call would pass that optional argument."""
    return load().tg_conv3d_kernel(*_conv_query_args(T, H, W, Cin, cout, cout_pad, kt, kh, kw, stride, pad, up, out_dims, t_map, residual, gn_partial))


def conv3d_splitk_plan(T, H, W, Cin, cout, cout_pad, kt, kh, kw, stride=1, pad=1, up=1, out_dims=None, t_map=False, residual=False, gn_partial=False):
    """tg_conv3d_splitk_plan: (ksplit, template case of the reduce kernel: 2, 4, 8, or 0 for its generic loop) of a CONV_128_SPLITK launch, (1, 0) for every other kernel."""
    v = load().tg_conv3d_splitk_plan(*_conv_query_args(T, H, W, Cin, cout, cout_pad, kt, kh, kw, stride, pad, up, out_dims, t_map, residual, gn_partial))
    if v < 0:
        raise RuntimeError(f"tg_conv3d_splitk_plan: tg_conv3d_cl refuses this shape ({v})")
    return (v >> 4, v & 15) if v else (1, 0)


def check(code, what):
    if code != 0:
        raise RuntimeError(f"{what} failed ({code}): {load().tg_last_error_string().decode()}")


class AttnBwdProblem(C.Structure):
    """tg_attn_bwd_problem (include/tokensgen_hip.h)"""
    _fields_ = ([(n, t) for base in ("q", "k", "v", "o") for n, t in ((base, C.c_void_p), (base + "_ld", C.c_long), (base + "_sb", C.c_long))] +
                [("dout", C.c_void_p), ("do_ld", C.c_long), ("do_sb", C.c_long)] +
                [(n, t) for base in ("dq", "dk", "dv") for n, t in ((base, C.c_void_p), (base + "_ld", C.c_long), (base + "_sb", C.c_long))] +
                [("nq", C.c_int), ("nk", C.c_int), ("scale", C.c_float), ("accumulate", C.c_int), ("lse", C.c_void_p), ("ws", C.c_void_p),
                 ("dv_bf16", C.c_void_p), ("dv_bf16_ld", C.c_long), ("dv_bf16_sb", C.c_long)])


class AccumItem(C.Structure):
    """tg_accum_item (include/tokensgen_hip.h)"""
    _fields_ = [("grad", C.c_void_p), ("acc", C.c_void_p), ("n", C.c_long), ("grad_is_bf16", C.c_int)]


class ColsumItem(C.Structure):
    """tg_colsum_item (include/tokensgen_hip.h)"""
    _fields_ = [("src", C.c_void_p), ("ld", C.c_long), ("rows", C.c_int), ("cols", C.c_int), ("src_is_f32", C.c_int)]


TG_ACCUM_MAX, TG_COLSUM_MAX = 48, 16


class Adamw8bitRow(C.Structure):
    """tg_adamw8bit_row (include/tokensgen_hip.h)"""
    _fields_ = [("offset", C.c_long), ("numel", C.c_long), ("state", C.c_long), ("first_block", C.c_long), ("kind", C.c_int), ("clipped", C.c_int)]


ADAMW8BIT_FP32, ADAMW8BIT_BLOCKWISE = 0, 1
PRODIGY_STATE_DOUBLES = 8          # TG_PRODIGY_STATE_DOUBLES: d, d_max, d_numerator, d_hat, d_denom, dlr, skipped, reserved


class AttnSegment(C.Structure):
    """tg_attn_segment (include/tokensgen_hip.h)"""
    _fields_ = [("q", C.c_void_p), ("q_ld", C.c_long), ("q_strideB", C.c_long),
                ("k", C.c_void_p), ("k_ld", C.c_long), ("k_strideB", C.c_long),
                ("vt", C.c_void_p), ("vt_ld", C.c_long), ("nk", C.c_int), ("k_norm2_max", C.c_void_p)]


class AttnProblem(C.Structure):
    """tg_attn_problem (include/tokensgen_hip.h)"""
    _fields_ = [("seg", AttnSegment * 2), ("nseg", C.c_int), ("seg2_scale", C.c_float),
                ("out", C.c_void_p), ("out_ld", C.c_long), ("out_strideB", C.c_long), ("nq", C.c_int),
                ("seg2_scale_batch", C.POINTER(C.c_float))]


class AttnWorkspace(C.Structure):
    """tg_attn_workspace (include/tokensgen_hip.h)"""
    _fields_ = [("retry", C.c_void_p), ("retry_ints", C.c_long), ("split", C.c_void_p), ("split_floats", C.c_long)]
