"""MI355X-native Mask2Former hot path for marco-conciatori-public/weed_instance_segmentation.

    from weed_instance_segmentation_amd import Mask2FormerForUniversalSegmentation, Mask2FormerConfig

is the drop-in for `transformers.Mask2FormerForUniversalSegmentation` at the reference's call sites
(models/mask2former/train.py:7, :167-172; models/model_utils.py:5, :14).  The kernels live in
libwm2f.so (C ABI: include/wm2f.h); build it with `python -m weed_instance_segmentation_amd._build`.
"""
from .configuration import Mask2FormerConfig  # noqa: F401
from .modeling import Mask2FormerForUniversalSegmentation, Mask2FormerForUniversalSegmentationOutput  # noqa: F401

__version__ = "0.1.0"
from .postprocess import Mask2FormerInstancePostProcessor  # noqa: F401
from .metrics import MeanAveragePrecision  # noqa: F401
from .instances import (CleanOptions, SplitOptions, aim_points, boundary_dilation, boundary_maps,  # noqa: F401
                        clean_label_maps, distance_maps, grow_label_maps, instance_statistics, nearest_instance_maps,
                        shape_from_sums, shape_statistics, split_label_maps)
from .treatment import TreatmentOptions, load_treatment_grid, save_treatment_grid, treatment_grid  # noqa: F401
from .rows import RowOptions, annotate_rows, crop_rows  # noqa: F401
from .skeleton import (SKELETON_GRAPH_TRAITS, SKELETON_TRAITS, PruneOptions, SkeletonOptions, annotate_skeletons,  # noqa: F401
                       prune_skeleton_maps, skeleton_branch_maps, skeleton_from_sums, skeleton_graph_statistics,
                       skeleton_maps, skeleton_statistics)
from .color import (COLOR_TRAITS, ColorOptions, annotate_colors, color_from_sums, color_statistics,  # noqa: F401
                    otsu_threshold, vegetation_masks, vegetation_threshold)
from .rle import (coco_results, decode_rle, encode_label_maps, rle_from_string, rle_to_string,  # noqa: F401
                  save_coco_results)
from .contours import (instance_polygons, save_via_annotations, trace_label_maps, via_annotations)  # noqa: F401
from .preprocess import Mask2FormerImageProcessor  # noqa: F401
from .augment import (AugmentParams, CopyPaste, CopyPasteParams, PhotometricParams, RotateParams,  # noqa: F401
                      TrainAugmentation, adjust_colors, allocate_paste_ids, rotate_images, rotate_maps)
from .data import CopyPasteBatcher, copy_paste  # noqa: F401
from .visualize import (build_overlay_tables, convert_gt_map_to_result, render_label_overlay,  # noqa: F401
                        render_segmentation, render_segmentations, save_comparison)
from .derived import drop_derived  # noqa: F401
from .precision import get_inference_precision, inference_precision, set_inference_precision  # noqa: F401
from .tiling import (TileGrid, blend_tile_scores, merge_tile_results, segment_tiled, segment_tiled_semantic,  # noqa: F401
                     tile_windows)
