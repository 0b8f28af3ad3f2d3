"""Python face of the libwm2f kernels: argument checking, pointer plumbing, autograd glue.

PyTorch is used for device memory, streams and autograd bookkeeping only.  Every function here launches hand-written HIP
through the C ABI (include/wm2f.h) on the caller's current stream and RAISES if the tensors are not on a GPU or the library
is missing -- there is no eager fallback.  One module per kernel family; each launch goes through `_core._launch`.  This
package re-exports them all and owns the switches below: callers assign and read them as `ops.<FLAG>`.
"""
from __future__ import annotations

import os as _os

# K1 backward flavour: None = follow torch.are_deterministic_algorithms_enabled(); True / False force it.
K1_BWD_DETERMINISTIC: bool | None = None

# The inference routes of the 1x1 convolutions (ResNet bottlenecks, pixel-decoder projections) take the split kernel while
# this is True; False sends them through conv1x1(..., split=False), the library convolution plus bias_act_ (the accuracy
# reference of the tests).
CONV1X1_SPLIT = True

# The inference routes of the 3x3 convolutions (ResNet conv2, the pixel decoder's FPN layer_1) take the split kernel while
# this is True; False sends them through conv3x3(..., split=False), the library convolution plus bias_act_ (the accuracy
# reference of the tests).
CONV3X3_SPLIT = True

# The split 3x3 kernel's route: True lets the host's rule send a launch to the staged kernel (the x tile split
# once per channel block in LDS) where it measured faster; False keeps every launch on the direct kernel.  The same bits.
CONV3X3_STAGED = True

# The pixel decoder's inference forward folds GroupNorm into the convolutions around it while this is True: the
# group statistics come out of the convolution epilogues (conv1x1_gn, conv3x3_stats) and mask_projection normalises
# layer_1's raw output in its operand load.  False keeps the separate statistics and apply passes (the reference of the tests).
CONV_GN_FUSED = True

# The inference forward of a ResNet bottleneck with a projection shortcut runs conv3 and the shortcut as ONE split GEMM over
# the concatenated K while this is True and conv1x1_dual_applies: the shortcut's full-width output never reaches
# memory.  False keeps the raw shortcut launch and conv3's residual epilogue (the reference of the tests).
SHORTCUT_FOLD = True

# The inference forward of a pixel-decoder encoder layer runs fc1 + ReLU and fc2 + LayerNorm (+ pos) as ONE kernel while this
# is True and token_ffn_applies: the (tokens, 1024) intermediate never reaches memory.  False keeps the two
# token_linear launches (the reference of the tests: the fused kernel gives their bits).
TOKEN_FFN_FUSED = True

# The inference forward of a Swin layer runs its Linears and MLP (merged q | k | v, o_proj + residual, fc1 + GELU, fc2 +
# residual) and patch merging's reduction on swin_linear while this is on and swin_linear_applies.  True: at
# every level of SPLIT_PRECISION; False: never, the stock F.linear route (the reference of the tests and of tools/);
# a tuple of level names: at those levels only -- the default, set by §45's measurements level by level.
SWIN_LINEAR_SPLIT: bool | tuple = ("highest", "high", "medium")

# The precision of the split-bf16 GEMMs and convolutions (token_linear, conv1x1, conv1x1_gn, conv3x3, conv3x3_stats,
# stem_conv_pool on their split kernels), read at every call: "highest" (or None) = three bf16 pieces per operand
# and six products, fp32 accuracy; "high" = two pieces, three products (error floor 2^-14 of sum |x w|); "medium" = one
# piece, one product (both operands rounded to bf16, fp32 accumulation: floor 2^-6).  Any other value raises ValueError at
# the first call that reads it.  The environment variable WM2F_SPLIT_PRECISION, when set, gives the initial value.
# split=False, training and autocast never reach these kernels and are unaffected.  The package's
# set_inference_precision / get_inference_precision / inference_precision assign and read this flag.
SPLIT_PRECISION: str | None = _os.environ.get("WM2F_SPLIT_PRECISION") or "highest"

# The flags come first: k1 reads K1_BWD_DETERMINISTIC off this package.
from .._lib import check
from ._core import KernelTimer, _p, _stream, set_kernel_timer
from .ccl import label_components, resize_nearest_tables
from .clean import labelmap_clean
from .color import image_index_hist, image_index_mask, index_coefficients, index_range, labelmap_color_stats
from .copy_paste import copy_paste
from .fused import (add_broadcast, bias_act_, bias_relu_maxpool, group_norm_act_, group_norm_act_from_stats_, group_norm_tokens_,
                    group_norm_tokens_from_stats_, resize_bilinear, resize_pyramid, tokens_to_nchw)
from .gemm import (conv1x1, conv1x1_applies, conv1x1_dual, conv1x1_dual_applies, conv1x1_gn, conv3x3, conv3x3_applies, conv3x3_route, conv3x3_stats, conv3x3_stats_route, conv_group_stats_applies,
                   ROWS_FFN, ROWS_NATURAL, ffn_row_order, linear_tokens, split_weight, split_weight_3x3,
                   split_weight_cached, split_weight_rows, split_weight_rows_cached, split_weight_stem, stem_conv_pool,
                   stem_conv_pool_applies, stem_weight_columns, stem_weight_matrix, swin_linear, swin_linear_applies,
                   token_ffn, token_ffn_applies,
                   token_linear, token_linear_applies, token_wgrad, token_wgrad_applies)
from .k1 import (k1_bwd_deterministic, k1_lane_order, k1_lane_rows, k1_lanes_applies, k1_rows_applies, ms_deform_attn,
                 ms_deform_attn_bwd, ms_deform_attn_fused, ms_deform_attn_fused_lanes, ms_deform_attn_fused_packed,
                 ms_deform_attn_rows, ms_deform_attn_variant)
from .k2 import masked_xattn, masked_xattn_bf16_applies
from .k3 import (attn_mask_build, mask_einsum, mask_einsum_attn_mask, mask_einsum_bf16, mask_einsum_bf16_bwd,
                 mask_einsum_bf16_bwd_applies, mask_einsum_bwd, mask_einsum_bwd_applies, nchw_to_pixel_major_bf16)
from .labelmaps import (cell_grid_shape, coco_match, coco_match_min, labelmap_aim_points, labelmap_boundary,
                        labelmap_cell_counts, labelmap_distance, labelmap_hull, labelmap_instance_stats, labelmap_nearest,
                        labelmap_pair_counts, labelmap_shape_stats, labelmap_to_masks, mask_pair_counts, panoptic_match,
                        semantic_confusion_)
from .layernorm import add_layernorm, add_layernorm_train, add_layernorm_train_applies
from .loss import mask_loss_rows, point_sample, point_sample_levels, select_top_points
from .matcher import lsa_batched, matcher_cost
from .overlay import labelmap_overlay
from .polygons import fill_polygons
from .postprocess import (_GRID, instance_any, instance_maps, instance_scores, instance_segmentation, panoptic_probs,
                          panoptic_relabel_, panoptic_segments, semantic_resize_argmax, semantic_scores)
from .rle import labelmap_toggle_counts, labelmap_toggles, rle_paint_
from .rows import labelmap_row_bands, labelmap_row_votes, row_angle_table, row_bins, row_offset
from .skeleton import labelmap_skeleton, labelmap_skeleton_graph, labelmap_skeleton_prune, labelmap_skeleton_stats
from .split import labelmap_split
from .trace import labelmap_trace
from .tiles import tile_blend, tile_compose, tile_link, tile_owned_counts, tile_pair_counts
from .preprocess import (augment_nearest_labels, augment_resize_normalize_u8, orient_labels, orient_u8, photometric_u8,
                         resize_nearest_labels, resize_normalize_u8)
from .swin import (SWIN_HEAD_DIMS, SWIN_WINDOW_SIZES, swin_window_attention, swin_window_attention_applies,
                   swin_window_attention_train)
