"""ctypes binding of libwm2f.so (C ABI declared in include/wm2f.h).

There is NO fallback: if the library is missing or a call fails, the op raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libwm2f.so")
PROF_LIB_PATH = os.path.join(HERE, "libwm2f_prof.so")  # profiling build (include/wm2f_prof.h): tools/ only
if os.environ.get("WM2F_PROF_LIB"):  # tools only: another profiling build (compile-time A/B variants)
    PROF_LIB_PATH = os.environ["WM2F_PROF_LIB"]

WM2F_F32 = 0
WM2F_BF16 = 1
WM2F_I32 = 2
WM2F_U8 = 3
WM2F_U16 = 4
WM2F_I64 = 5
WM2F_CCL_VALUE, WM2F_CCL_BINARY, WM2F_CCL_RGB = 0, 1, 2
WM2F_CCL_MAX_COLORS = 16
WM2F_POLY_MAX_SIDE = 16384
WM2F_POLY_MAX_COORD = 1 << 24
WM2F_RLE_MAX_IDS = 1024
WM2F_AUG_MAX_VIRTUAL = 65536
WM2F_TILE_MAX_SIDE, WM2F_TILE_MAX_IDS, WM2F_TILE_MAX_TILES, WM2F_TILE_MAX_PAIRS = 16384, 256, 1024, 16384
WM2F_AUG_PRE_DESC_LEN, WM2F_AUG_LAB_DESC_LEN = 16, 12
WM2F_PHOTO_BRIGHTNESS, WM2F_PHOTO_CONTRAST, WM2F_PHOTO_SATURATION, WM2F_PHOTO_HUE = 0, 1, 2, 3
WM2F_PHOTO_DESC_LEN = 12
WM2F_ORIENT_DESC_LEN = 22
WM2F_COPY_PASTE_DESC_LEN = 5
WM2F_CLEAN_KEEP_ALL, WM2F_CLEAN_KEEP_LARGEST = 0, 1
WM2F_CLEAN_ALL, WM2F_CLEAN_PIECES, WM2F_CLEAN_CHOOSE, WM2F_CLEAN_HOLES, WM2F_CLEAN_PAINT = range(5)
WM2F_PRE_MAX_IMAGES, WM2F_PRE_MAX_SIDE = 32, 16384
WM2F_COLOR_COLUMNS, WM2F_COLOR_MAX_WEIGHT, WM2F_COLOR_MAX_HUE_BINS = 14, 32, 36
# route[0] of wm2f_masked_xattn_route
(WM2F_K2_UNSUPPORTED, WM2F_K2_FWD_GENERAL, WM2F_K2_FWD_FULL, WM2F_K2_BF16_FWD, WM2F_K2_BWD_GENERAL, WM2F_K2_BWD_FULL,
 WM2F_K2_BF16_BWD) = range(7)
# return codes of include/wm2f.h
WM2F_OK, WM2F_EINVAL, WM2F_EUNSUPPORTED, WM2F_ELAUNCH = 0, -1, -2, -3

_P = c_void_p
_I = c_int
_HOST_I32 = POINTER(c_int32)

# name -> (restype, argtypes); mirrors include/wm2f.h one to one
SIGNATURES = {
    "wm2f_version": (c_int, []),
    "wm2f_last_error": (c_char_p, []),
    "wm2f_msdeform_fwd": (c_int, [_P, _P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_msdeform_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_msdeform_rows_fwd": (c_int, [_P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_msdeform_rows_bwd": (c_int, [_P, _P, _P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_msdeform_bwd_det_workspace": (c_int64, [_HOST_I32, _I, _I, _I, _I, _I]),
    "wm2f_msdeform_bwd_det": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_msdeform_fused_fwd": (c_int, [_P, _P, _P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_msdeform_fused_packed_fwd": (c_int, [_P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_msdeform_fused_lanes_fwd": (c_int, [_P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_msdeform_fwd_v": (c_int, [_P, _P, _P, _P, _P, _HOST_I32, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_select_top_points": (c_int, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_point_sample_levels_fwd": (c_int, [POINTER(c_void_p), _I, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_point_sample_levels_bwd": (c_int, [_P, _P, _P, POINTER(c_void_p), _I, _I, _I, _I, _I, _P]),
    "wm2f_point_sample_levels_bwd_unique": (c_int, [_P, _P, _P, POINTER(c_void_p), _I, _I, _I, _I, _I, _P]),
    "wm2f_mask_loss_rows_fwd": (c_int, [_P, _P, _P, _P, _P, _I, _I, _P]),
    "wm2f_mask_loss_rows_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "wm2f_labelmap_to_masks": (c_int, [_P, _P, _P, c_int64, _I, _P]),
    "wm2f_instance_scores": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_instance_any": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_instance_segmentation": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_instance_maps": (c_int, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_semantic_scores": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_semantic_resize_argmax": (c_int, [_P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_panoptic_probs": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_panoptic_segments": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, c_float, _P]),
    "wm2f_panoptic_relabel": (c_int, [_P, _P, _P, _I, _I, c_int64, _P]),
    "wm2f_mask_einsum_bf16_fwd": (c_int, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_nchw_to_pixel_major_bf16": (c_int, [_P, _P, _I, _I, _I, _P]),
    "wm2f_mask_einsum_fwd": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_mask_einsum_attn_mask_fwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_mask_einsum_bf16_bwd_workspace": (c_int64, [_I, _I, _I, _I]),
    "wm2f_mask_einsum_bf16_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_mask_einsum_bwd_workspace": (c_int64, [_I, _I, _I, _I]),
    "wm2f_mask_einsum_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_attn_mask_build": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_masked_xattn_workspace": (c_int64, [_I, _I, _I, _I, _I]),
    "wm2f_masked_xattn_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_masked_xattn_route": (c_int, [_I, _I, _I, _I, _I, _I, _I, _I, _HOST_I32]),
    "wm2f_masked_xattn_bf16_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_masked_xattn_bf16_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_masked_xattn_bwd_workspace": (c_int64, [_I, _I, _I, _I, _I]),
    "wm2f_masked_xattn_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_swin_window_attn_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_swin_window_attn_train_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_swin_window_attn_bwd_workspace": (c_int64, [_I, _I, _I, _I, _I, _I]),
    "wm2f_swin_window_attn_bwd": (c_int, [_P] * 15 + [_I] * 8 + [_P]),
    "wm2f_matcher_workspace": (c_int64, [_I, _I, _I, _I, _I]),
    "wm2f_matcher_cost": (c_int, [_P, _P, _P, _I, _HOST_I32, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                                  c_float, c_float, c_float, _P]),
    "wm2f_matcher_cost_levels": (c_int, [POINTER(c_void_p), _P, _P, _I, _HOST_I32, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I,
                                         _I, _I, _I, c_float, c_float, c_float, _P]),
    "wm2f_lsa_batched": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_add_broadcast": (c_int, [_P, _P, _P, _I, c_int64, _P]),
    "wm2f_bias_act": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_add_layernorm": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int64, _I, c_int64, c_float, _P]),
    "wm2f_add_layernorm_train_workspace": (c_int64, [c_int64]),
    "wm2f_add_layernorm_train_fwd": (c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, c_int64, _I, c_int64, c_float, c_float, _P]),
    "wm2f_add_layernorm_train_bwd": (c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, c_int64, _I, _P]),
    "wm2f_token_linear_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _I, _I, _I, c_int64, c_float, _I, _P]),
    "wm2f_token_linear_split_weight": (c_int, [_P, _P, _I, _I, _P]),
    "wm2f_token_linear_split_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _I, _I, _I, c_int64, c_float, _I, _P]),
    "wm2f_token_linear_split_weight_rows": (c_int, [_P, _P, _I, _I, _I, _P]),
    "wm2f_token_ffn_row": (c_int, [_I]),
    "wm2f_token_ffn_split_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _I, _I, _I, c_int64, c_float, _P]),
    "wm2f_conv1x1_split_config": (c_int, [_I, _I, _I, _I]),
    "wm2f_conv1x1_split_fwd": (c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv3x3_split_config": (c_int, [_I, _I, _I, _I]),
    "wm2f_conv3x3_split_fwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv1x1_split_gn_fwd": (c_int, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _I, c_float, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv3x3_split_stats_fwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_group_norm_act_apply": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, c_float, _I, _P]),
    "wm2f_group_norm_tokens_apply": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, c_float, _P]),
    "wm2f_stem7x7_pool_fwd":(c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    # the same entry points with a trailing `pieces` before the stream
    "wm2f_token_linear_split_fwd_p": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _I, _I, _I, c_int64, c_float, _I, _I, _P]),
    "wm2f_token_ffn_split_fwd_p": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _I, _I, _I, c_int64, c_float, _I, _P]),
    "wm2f_conv1x1_split_fwd_p": (c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv1x1_split_gn_fwd_p": (c_int, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _I, c_float, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv1x1_split_dual_fwd_p": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv3x3_split_fwd_p": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv3x3_split_stats_fwd_p": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_stem7x7_pool_fwd_p": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    # the 3x3 entry points with `route` before the stream, and the host's rule
    "wm2f_conv3x3_split_fwd_r": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv3x3_split_stats_fwd_r": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_conv3x3_split_route": (c_int, [_I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_swin_linear_split_fwd_p": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int64, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_swin_linear_split_config": (c_int, [c_int64, _I, _I, _I]),
    "wm2f_swin_linear_split_configs": (c_int, []),
    "wm2f_token_wgrad_workspace": (c_int64, [c_int64, _I, _I]),
    "wm2f_token_wgrad_bf16": (c_int, [_P, _P, _P, _P, _P, c_int64, _I, _I, _P]),
    "wm2f_token_wgrad_f32": (c_int, [_P, _P, _P, _P, _P, c_int64, _I, _I, _P]),
    "wm2f_tokens_to_nchw": (c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_group_norm_tokens": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, c_float, _P]),
    "wm2f_resize_bilinear": (c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_resize_pyramid": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "wm2f_bias_relu_maxpool": (c_int, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_group_norm_act": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, c_float, _I, _P]),
    "wm2f_point_sample_fwd": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_point_sample_bwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_pair_counts": (c_int, [_P, _I, _P, _I, _P, _P, _P, _I, c_int64, _I, _I, _P]),
    "wm2f_mask_pair_counts_workspace": (c_int64, [_I, _I, c_int64]),
    "wm2f_mask_pair_counts": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, c_int64, _P]),
    "wm2f_coco_match": (c_int, [_P] * 14 + [_I, _I, _I, _I, _I, _I, _P]),
    "wm2f_coco_match_min": (c_int, [_P] * 17 + [_I, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_boundary_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_labelmap_boundary": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_instance_stats": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_distance_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_labelmap_distance": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_aim_points_workspace": (c_int64, [_I, _I]),
    "wm2f_labelmap_aim_points": (c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_nearest_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_labelmap_nearest": (c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_cell_counts": (c_int, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_panoptic_match": (c_int, [_P] * 8 + [_I, _I, _I, _I, _P]),
    "wm2f_semantic_confusion": (c_int, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, c_int64, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_overlay": (c_int, [_P, _P, _I, _P, _P, _P, _P, ctypes.c_uint32, _I, _I, _P, _I, _I, _I, _I, _P]),
    "wm2f_resize_normalize_u8": (c_int, [_P, c_int64, POINTER(c_int64), _P, c_int64, _P, _P, c_int64, _P, _P, _I, _I, _I,
                                         _P]),
    "wm2f_resize_nearest_labels": (c_int, [_P, _I, c_int64, POINTER(c_int64), _P, c_int64, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_augment_resize_normalize_u8": (c_int, [_P, c_int64, POINTER(c_int64), _P, c_int64, _P, _P, _P, _I, _I, _I, _P]),
    "wm2f_augment_nearest_labels": (c_int, [_P, _I, c_int64, POINTER(c_int64), _P, c_int64, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_photometric_workspace": (c_int64, [_I]),
    "wm2f_photometric_u8": (c_int, [_P, c_int64, POINTER(c_int64), _P, _I, _P]),
    "wm2f_orient_u8": (c_int, [_P, c_int64, _P, c_int64, POINTER(c_int64), _I, _P]),
    "wm2f_orient_labels_u8": (c_int, [_P, c_int64, _P, c_int64, POINTER(c_int64), _I, _P]),
    "wm2f_orient_labels_i32": (c_int, [_P, c_int64, _P, c_int64, POINTER(c_int64), _I, _P]),
    "wm2f_copy_paste_select": (c_int, [_P, _P, _P, _P, _P, POINTER(c_int64), _I, _I, _I, c_int64, c_int64, _P]),
    "wm2f_copy_paste": (c_int, [_P, _P, _P, _P, _P, _P, POINTER(c_int64), _I, _I, _I, _I, _P]),
    "wm2f_copy_paste_prune": (c_int, [_P, _P, _I, _I, _I, c_int64, c_int64, _I, _P]),
    "wm2f_ccl_workspace": (c_int64, [_I, _I]),
    "wm2f_ccl_label": (c_int, [_P, _I, _I, _I, _I, _P, _P, POINTER(ctypes.c_uint8), _I, _I, _I, _P, _P, _P]),
    "wm2f_ccl_keys": (c_int, [_P, _I, _I, _I, _P, _P]),
    "wm2f_ccl_paint": (c_int, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "wm2f_resize_nearest": (c_int, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _P]),
    "wm2f_poly_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_poly_fill": (c_int, [_P, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P]),
    "wm2f_rle_workspace": (c_int64, [_I, _I, _I, _I, _I]),
    "wm2f_labelmap_toggle_counts": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_toggles": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_rle_paint_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_rle_paint": (c_int, [_P, _P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_trace_workspace": (c_int64, [_I, _I, _I, _I]),
    "wm2f_trace_edge_workspace": (c_int64, [c_int64]),
    "wm2f_trace_rounds": (c_int, [c_int64]),
    "wm2f_trace_count": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_trace_link": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_trace_rank": (c_int, [_P, _I, _P]),
    "wm2f_trace_flags": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_trace_loops": (c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_trace_scatter": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_trace_emit": (c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_tile_merge_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_tile_pair_counts": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_tile_owned_counts": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_tile_link": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "wm2f_tile_compose": (c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_tile_blend": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_clean_workspace": (c_int64, [_I, _I, _I, _I]),
    "wm2f_labelmap_clean": (c_int, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, c_int64, _I, c_int64, _I, _I, _P]),
    "wm2f_labelmap_split_workspace": (c_int64, [_I, _I, _I, _I]),
    "wm2f_labelmap_split": (c_int, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_shape_stats": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_hull_workspace": (c_int64, [_I, _I, c_int64]),
    "wm2f_labelmap_hull": (c_int, [_P, _I, _P, _P, _P, _P, _P, c_int64, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_hull_vertices": (c_int, [_P, _P, _P, c_int64, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_row_votes": (c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_row_bands": (c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_skeleton_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_labelmap_skeleton": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_skeleton_stats": (c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_skeleton_prune_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_labelmap_skeleton_prune": (c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_skeleton_graph_workspace": (c_int64, [_I, _I, _I]),
    "wm2f_labelmap_skeleton_graph": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_labelmap_color_stats": (c_int, [_P, _P, _I, _P, _P, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P]),
    "wm2f_image_index_hist": (c_int, [_P, _I, _I, _I, _P, _I, _I, _I, _P]),
    "wm2f_image_index_mask": (c_int, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P]),
}

# additions of the profiling library (include/wm2f_prof.h)
PROF_SIGNATURES = {"wm2f_debug_stamps": (c_int, [_P, c_int64])}

_lib = None


class Wm2fError(RuntimeError):
    pass


def use_profiling_library() -> ctypes.CDLL:
    """tools/ only: make `load()` return libwm2f_prof.so (timing ablations, stamped kernels, environment knobs).  Must be
    called before the first `load()`; raises when that library has not been built
    (`python -m weed_instance_segmentation_amd._build --prof`)."""
    global _lib
    if _lib is not None:
        raise Wm2fError("use_profiling_library() must come before the first kernel call")
    if not os.path.exists(PROF_LIB_PATH):
        raise Wm2fError(f"{PROF_LIB_PATH} not found: python -m weed_instance_segmentation_amd._build --prof")
    lib = ctypes.CDLL(PROF_LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **PROF_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def load() -> ctypes.CDLL:
    """Load libwm2f.so once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Wm2fError(
                f"{LIB_PATH} not found: build it with `python -m weed_instance_segmentation_amd._build` "
                "(hipcc, gfx950). There is no CPU or PyTorch fallback for the hot path.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().wm2f_last_error()
        raise Wm2fError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def host_i32(values) -> ctypes.Array:
    flat = [int(v) for v in values]
    return (c_int32 * len(flat))(*flat)
