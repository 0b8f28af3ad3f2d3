"""Device-side `post_process_instance_segmentation`, and the semantic and panoptic
post-processing of the same processor (see their docstrings).

Mirrors `Mask2FormerImageProcessor.post_process_instance_segmentation` of transformers 5.15.0
(models/mask2former/image_processing_mask2former.py:627-746) -- same arguments, same return structure -- for the
reference's call sites `models/metrics.py:58-63` and `models/mask2former/inference.py:30`:

    processor = Mask2FormerInstancePostProcessor()
    preds = processor.post_process_instance_segmentation(outputs, threshold=0.5, mask_threshold=0.5,
                                                         target_sizes=batch["target_sizes"])

What changes is where the work runs.  The dependency resizes all Q masks to 384 x 384, then loops over the queries in
Python with one `.item()` sync each.  Here the (query, class) selection of :695-701 -- a top-k over Q * C numbers --
runs on the host with the same torch routine the reference's CPU path uses (`topk(sorted=False)`: its order decides
which instance is painted last, and only the same routine reproduces it), everything that touches pixels runs in
the HIP kernels of csrc/postprocess.hip, and ONE device-to-host copy of (B, Q) scores / labels / flags builds the
`segments_info` dictionaries.  `mask_threshold` and `overlap_mask_area_threshold` are accepted and unused, exactly
as in the dependency's instance path.
"""
from __future__ import annotations

import logging

import torch

from . import ops

logger = logging.getLogger(__name__)


def binary_mask_to_rle(mask: torch.Tensor) -> list[int]:
    """COCO-style run lengths of a binary (H, W) mask, row-major (image_processing_mask2former.py:77-97)."""
    pixels = mask.flatten()
    zero = torch.zeros(1, device=pixels.device, dtype=pixels.dtype)
    pixels = torch.cat([zero, pixels, zero])
    runs = torch.where(pixels[1:] != pixels[:-1])[0] + 1
    runs[1::2] -= runs[::2]
    return runs.tolist()


def convert_segmentation_to_rle(segmentation: torch.Tensor) -> list[list[int]]:
    """One run-length list per distinct id of the map, background (-1) included (:100-118)."""
    return [binary_mask_to_rle(torch.where(segmentation == idx, 1, 0)) for idx in torch.unique(segmentation)]


class SemanticSegmentationPostProcessorOutput(dict):
    """One image of `post_process_semantic_segmentation(..., return_segmentation_scores=True)`: `segmentation` (H, W)
    int64 class ids and `segmentation_scores` (C, H, W) fp32, by key or by attribute (the dependency's class of this
    name, without importing it)."""

    def __init__(self, segmentation: torch.Tensor, segmentation_scores: torch.Tensor):
        super().__init__(segmentation=segmentation, segmentation_scores=segmentation_scores)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def assign_segment_ids(labels, scores, above, owned, overlap_mask_area_threshold: float, label_ids_to_fuse):
    """The host half of the dependency's compute_segments (image_processing_mask2former.py:167-224) for ONE image, from
    per-query pixel counts instead of masks.  labels / scores: the kept queries' class and score (host numbers, query
    order); above[k]: pixels whose score-weighted probability is >= mask_threshold (`original_area`); owned[k]: pixels
    whose argmax is k (`mask_k_area`).  Returns (ids, segments_info): ids[k] = segment id painted for query k, 0 if
    the query is rejected.

    The dependency's rules, kept as they are:
    - a query survives if owned > 0, above > 0 and float32(owned / above) > overlap_mask_area_threshold -- a float32
      torch division, so an exact 4 / 5 passes at 0.8 (float32(0.8) > 0.8);
    - ids start at 1; a label in label_ids_to_fuse remembers its first id, and a later query of that label reuses it
      AND resets the running counter to it, so the next new segment repeats an id (labels [A, B, A, C] with A fused
      give ids [1, 2, 1, 2]);
    - was_fused is True for every segment of a fused label; score = round(float(score), 6)."""
    n = len(labels)
    ratio = (torch.tensor(list(owned), dtype=torch.int64) / torch.tensor(list(above), dtype=torch.int64)).tolist() if n else []
    ids = [0] * n
    segments = []
    current, memory = 0, {}
    for k in range(n):
        label = int(labels[k])
        fuse = label in label_ids_to_fuse
        if not (owned[k] > 0 and above[k] > 0 and ratio[k] > overlap_mask_area_threshold):
            continue
        if label in memory:
            current = memory[label]
        else:
            current += 1
        ids[k] = current
        segments.append({"id": current, "label_id": label, "was_fused": fuse, "score": round(float(scores[k]), 6)})
        if fuse:
            memory[label] = current
    return ids, segments


def _device_logits(outputs):
    logits = outputs.masks_queries_logits
    if not logits.is_cuda:
        from ._lib import Wm2fError
        raise Wm2fError(f"masks_queries_logits is on {logits.device}: the wm2f kernels run on a GPU only (no CPU fallback)")
    return logits.float().contiguous()


class Mask2FormerInstancePostProcessor:
    """Stands where the reference holds its `AutoImageProcessor` for post-processing."""

    def post_process_instance_segmentation(self, outputs, threshold: float = 0.5, mask_threshold: float = 0.5,
                                           overlap_mask_area_threshold: float = 0.8, target_sizes=None,
                                           return_coco_annotation: bool = False, return_binary_maps: bool = False,
                                           return_instance_stats: bool = False, return_polygons: bool = False,
                                           clean=None, return_aim_points: bool = False, split=None,
                                           return_shape_stats: bool = False):
        """`clean=CleanOptions(...)` (not an argument of the dependency; `instances.CleanOptions`) repairs every id map on
        the device before anything is taken from it: pieces below `min_area` dropped, with
        keep="largest" one connected piece per instance, with fill_holes=True enclosed background painted.  Entries of
        `segments_info` whose instance owns no pixel afterwards are dropped and the rest renumbered 0 .. n'-1 ("id" is
        the value in the returned map; order, labels and scores unchanged); statistics, the `return_coco_annotation`
        encoding and polygons all describe the cleaned map.  With `return_binary_maps=True` the stack is then cut from
        the cleaned map (`map == id`, fp32, one map per remaining entry) and not from the logits -- otherwise stack and
        `segments_info` would disagree.  clean=None changes nothing.
        `return_polygons=True` (not an argument of the dependency) adds "polygons" to every `segments_info` entry that
        still owns a pixel of the returned id map: its boundary loops `{"points": (P, 2) int32 x, y, "hole": bool}` in
        pixel coordinates, as `contours.trace_label_maps` gives them, from one trace per distinct target size (DESIGN
        section 27).
        `return_instance_stats=True` (not an argument of the dependency) adds to every `segments_info` entry
        "area" (int), "bbox" ([x, y, w, h] ints, COCO) and "centroid" ((cx, cy) floats, None when the area is 0) of the
        instance's pixels in the returned id map -- after later instances have painted over earlier ones, whatever
        form `segmentation` is returned in -- from one more launch per distinct target size and one more
        device-to-host copy.
        `return_aim_points=True` (not an argument of the dependency) adds "aim_point" ((x, y) ints: the instance's pixel
        farthest from everything that is not the instance, None for an instance without a pixel) and "clearance" (float:
        the distance there) to every `segments_info` entry, computed on the returned id map -- after painting, after
        `clean=`, at the target size -- once per distinct target size, with one more device-to-host copy (DESIGN
        section 36).  Independent of `return_instance_stats`.
        `split=SplitOptions(...)` (not an argument of the dependency; `instances.SplitOptions`) parts touching plants that
        one instance covers, after `clean=` and before everything that is taken from the map: the
        part with the highest peak of the interior distance keeps the instance's id, every part split off gets the next
        free id and a new `segments_info` entry after the existing ones -- a copy of its parent's (label, score) with its
        own "id" and "split_from": the parent's id.  Statistics, aim points, the encoding, polygons and, with
        `return_binary_maps=True`, the stack (cut from the map, as with `clean=`) describe the split map.  split=None
        changes nothing.
        `return_shape_stats=True` (not an argument of the dependency) adds the shape traits of `instances.SHAPE_TRAITS`
        -- "orientation", "axis_major_length", "axis_minor_length", "eccentricity", "perimeter", "crack_length" (an int),
        "equivalent_diameter", "extent", "circularity", "area_convex", "solidity", "feret_diameter_max", "hull_perimeter",
        "convexity"; floats, NaN for an instance without a pixel -- to every `segments_info` entry, as
        `shape_statistics` gives them for the returned id map -- after painting, after `clean=` and `split=`, at the
        target size -- once per distinct target size, with one more device-to-host copy."""
        if return_coco_annotation and return_binary_maps:
            raise ValueError("return_coco_annotation and return_binary_maps can not be both set to True.")
        if clean is not None:
            from .instances import CleanOptions, cleaned_segments_info
            if not isinstance(clean, CleanOptions):
                raise TypeError(f"clean must be a CleanOptions or None, got {type(clean).__name__}")
        if split is not None:
            from .instances import SplitOptions, split_rows, split_segments_info
            if not isinstance(split, SplitOptions):
                raise TypeError(f"split must be a SplitOptions or None, got {type(split).__name__}")
        cls = outputs.class_queries_logits
        logits = outputs.masks_queries_logits
        if not logits.is_cuda:
            from ._lib import Wm2fError
            raise Wm2fError(f"masks_queries_logits is on {logits.device}: the wm2f kernels run on a GPU only (no CPU fallback)")
        logits = logits.float().contiguous()
        B, Q = cls.shape[0], cls.shape[1]
        C = cls.shape[-1] - 1
        if target_sizes is not None and len(target_sizes) != B:
            raise ValueError("Make sure that you pass in as many target sizes as the batch dimension of the logits")

        # ---- (query, class) selection, :695-701, on the host (see the module docstring)
        cls_cpu = cls.detach().float().cpu()
        sel_scores, sel_labels, sel_q = [], [], []
        for i in range(B):
            scores = torch.nn.functional.softmax(cls_cpu[i], dim=-1)[:, :-1]
            s, idx = scores.flatten(0, 1).topk(Q, sorted=False)
            sel_scores.append(s)
            sel_labels.append(idx % C)
            sel_q.append(torch.div(idx, C, rounding_mode="floor"))
        dev = logits.device
        sel_scores = torch.stack(sel_scores).to(dev)
        labels_cpu = torch.stack(sel_labels)
        qidx = torch.stack(sel_q).to(torch.int32).to(dev)

        # ---- mask quality on the 384 x 384 grid, :703-709
        sum_sig, cnt = ops.instance_scores(logits, qidx)
        pred_scores = sel_scores * (sum_sig / (cnt + 1e-6))
        cand = pred_scores >= threshold

        sizes = [tuple(int(v) for v in t) for t in target_sizes] if target_sizes is not None else [ops._GRID] * B
        seg_out: list = [None] * B
        rle_out: list = [None] * B
        keep_all = torch.zeros(B, Q, dtype=torch.bool, device=dev)
        kept_q_all = torch.zeros(B, Q, dtype=torch.int32, device=dev)
        n_ids = Q if split is None else split.id_space(Q)  # the id space of the returned maps
        stats_all = torch.zeros(B, n_ids, 8, dtype=torch.int64, device=dev) if return_instance_stats else None
        new_id_all = torch.full((B, Q), -1, dtype=torch.int64, device=dev) if clean is not None else None
        aim_all = torch.zeros(B, n_ids, 4, dtype=torch.int32, device=dev) if return_aim_points else None
        split_all = torch.zeros(B, n_ids + 1, dtype=torch.int64, device=dev) if split is not None else None
        if return_shape_stats:
            from .instances import SHAPE_TRAITS, add_shape_traits, shape_trait_rows
            shape_all = torch.zeros(B, n_ids, len(SHAPE_TRAITS), dtype=torch.float64, device=dev)
        for size in dict.fromkeys(sizes):  # one launch group per distinct target size
            rows = [i for i in range(B) if sizes[i] == size]
            ridx = torch.tensor(rows, device=dev)
            lg, qi = logits[ridx], qidx[ridx]
            if size[0] >= ops._GRID[0] and size[1] >= ops._GRID[1]:
                nonempty = cnt[ridx] > 0  # `nearest` up-sampling keeps every grid pixel
            else:
                nonempty = ops.instance_any(lg, qi, cand[ridx].to(torch.uint8), size) > 0
            keep = cand[ridx] & nonempty  # :724
            # kept instances in query order -> ids 0 .. n-1 (:725-735)
            order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)
            kept_q = torch.gather(qi, 1, order).contiguous()
            n_kept = keep.sum(1).to(torch.int32)
            seg = ops.instance_segmentation(lg, kept_q, n_kept, size)
            if clean is not None:  # in the map's own dtype, ids renumbered: everything below describes the cleaned map
                seg, clean_stats, n_kept = ops.labelmap_clean(seg, Q, relabel=True, out_dtype=seg.dtype, **clean.kernel_arguments())
                new_id_all[ridx] = clean_stats[:, :, 7]
            if split is not None:  # the kernel numbers the parts split off from Q; they continue each image's own ids
                parted, info, status = split_rows(seg, Q, split)
                shift = (Q - n_kept).view(-1, 1, 1)
                seg = torch.where(parted >= Q, parted - shift, parted).to(seg.dtype)
                split_all[ridx, :n_ids] = info[:, :, 0].to(torch.int64)
                split_all[ridx, n_ids] = status[:, 0].clamp(max=n_ids).to(torch.int64)
            keep_all[ridx] = keep
            kept_q_all[ridx] = kept_q
            if return_instance_stats:
                stats_all[ridx] = ops.labelmap_instance_stats(seg, N=n_ids)
            if return_aim_points:
                from .instances import aim_point_rows
                aim_all[ridx] = aim_point_rows(seg, n_ids)
            if return_shape_stats:
                shape_all[ridx] = shape_trait_rows(seg, n_ids)
            if return_coco_annotation:  # one encode per distinct target size, whatever the number of instances
                from .rle import encode_label_maps
                for i, rles in zip(rows, encode_label_maps(seg, n=n_ids, format="hf")):
                    rle_out[i] = list(rles.values())  # ascending ids, -1 first, only ids that still own a pixel
            for j, i in enumerate(rows):
                seg_out[i] = seg[j]

        # ---- the one device-to-host copy
        if clean is None:
            keep_cpu, score_cpu = keep_all.cpu(), pred_scores.cpu()
        else:  # the new ids travel with the flags
            flags = torch.cat([keep_all.to(torch.int64), new_id_all], 1).cpu()
            keep_cpu, new_id_cpu, score_cpu = flags[:, :Q].bool(), flags[:, Q:].numpy(), pred_scores.cpu()
        if split is not None:
            split_cpu = split_all.cpu().numpy()
        if return_instance_stats:
            from .instances import stats_to_boxes
            area, bbox, centroid = (t.tolist() for t in stats_to_boxes(stats_all.cpu()))
        if return_aim_points:
            from .instances import add_aim_points
            aim_cpu = aim_all.cpu().numpy()
        if return_shape_stats:
            shape_cpu = shape_all.cpu().numpy()
        results = []
        for i in range(B):
            ks = torch.nonzero(keep_cpu[i]).flatten().tolist()
            segments = [{"id": r, "label_id": int(labels_cpu[i, j]), "was_fused": False, "score": round(float(score_cpu[i, j]), 6)}
                        for r, j in enumerate(ks)]
            if clean is not None:  # the survivors are numbered 0 .. n'-1 in this order
                segments = cleaned_segments_info(segments, new_id_cpu[i])
            if split is not None:  # kernel ids Q, Q + 1, ... are the map's ids n, n + 1, ...
                n = len(segments)
                extras = int(split_cpu[i, n_ids]) - Q
                segments = split_segments_info(segments, [[p] for p in split_cpu[i, :n]] + [[p] for p in split_cpu[i, Q:Q + extras]],
                                               n + extras)
            if return_instance_stats:
                for r, seg_info in enumerate(segments):
                    seg_info["area"] = area[i][r]
                    seg_info["bbox"] = bbox[i][r]
                    seg_info["centroid"] = tuple(centroid[i][r]) if area[i][r] > 0 else None
            if return_aim_points:
                add_aim_points(segments, aim_cpu[i])
            if return_shape_stats:
                add_shape_traits(segments, shape_cpu[i])
            segmentation = seg_out[i]
            if return_coco_annotation:
                segmentation = rle_out[i]
            if return_binary_maps and ks and clean is None and split is None:
                segmentation = ops.instance_maps(logits[i], kept_q_all[i], len(ks), sizes[i])
            elif return_binary_maps and segments:
                ids = torch.arange(len(segments), device=dev, dtype=seg_out[i].dtype).view(-1, 1, 1)
                segmentation = (seg_out[i].unsqueeze(0) == ids).to(torch.float32)
            results.append({"segmentation": segmentation, "segments_info": segments})
        if return_polygons:
            from .contours import _add_polygons
            _add_polygons(results, maps=seg_out)
        return results

    def post_process_semantic_segmentation(self, outputs, target_sizes=None, return_segmentation_scores: bool = False):
        """`Mask2FormerImageProcessor.post_process_semantic_segmentation` (image_processing_mask2former.py:550-625):
        same arguments, same return structure, on the GPU.

        S = einsum("bqc,bqhw->bchw", softmax(class logits)[..., :-1], sigmoid(bilinear_384(mask logits))) (bilinear,
        align_corners=False, to the dependency's fixed 384 x 384 grid); with target sizes S is resized bilinearly to
        each one; the map is the argmax over classes, the first class winning ties.  Returns per image an (H, W) int64
        map ((384, 384) without target sizes), or with return_segmentation_scores=True a
        SemanticSegmentationPostProcessorOutput whose segmentation_scores are the (C, H, W) fp32 scores the map was
        taken from.  The (B, Q, C + 1) softmax is torch on the device; the einsum, the resize and the argmax run in
        csrc/postprocess_sp.hip; nothing is copied to the host."""
        logits = _device_logits(outputs)
        cls = outputs.class_queries_logits
        B = cls.shape[0]
        if target_sizes is not None and len(target_sizes) != B:
            raise ValueError("Make sure that you pass in as many target sizes as the batch dimension of the logits")
        dev = logits.device
        probs = torch.softmax(cls.detach().to(dev).float(), dim=-1)[..., :-1].contiguous()
        S = ops.semantic_scores(logits, probs)
        results: list = [None] * B
        if target_sizes is None:
            seg, _ = ops.semantic_resize_argmax(S, torch.arange(B, device=dev, dtype=torch.int32), ops._GRID)
            for i in range(B):
                results[i] = (seg[i], S[i])
        else:
            sizes = [tuple(int(v) for v in t) for t in target_sizes]
            for size in dict.fromkeys(sizes):  # one launch per distinct target size
                rows = [i for i in range(B) if sizes[i] == size]
                seg, sc = ops.semantic_resize_argmax(S, torch.tensor(rows, device=dev, dtype=torch.int32), size,
                                                     want_scores=return_segmentation_scores)
                for j, i in enumerate(rows):
                    results[i] = (seg[j], sc[j] if sc is not None else None)
        if not return_segmentation_scores:
            return [m for m, _ in results]
        return [SemanticSegmentationPostProcessorOutput(m, sc) for m, sc in results]

    def post_process_panoptic_segmentation(self, outputs, threshold: float = 0.5, mask_threshold: float = 0.5,
                                           overlap_mask_area_threshold: float = 0.8, label_ids_to_fuse=None,
                                           target_sizes=None):
        """`Mask2FormerImageProcessor.post_process_panoptic_segmentation` (image_processing_mask2former.py:748-841,
        compute_segments :167-224): same arguments, same return structure, on the GPU.

        - Selection, on the host with torch as the dependency's CPU path: scores, labels = softmax(class logits).max(-1);
          a query is kept if label != num_labels and score > threshold (strict, unlike the instance path's >=), in
          query order.
        - Map values: p_k = sigmoid(bilinear_384(logits_k)), resized bilinearly to the target size if one is given (the
          384 x 384 grid itself otherwise), then multiplied by score_k; every pixel goes to the first kept query of
          maximal value.
        - original_area = pixels with that score-weighted value >= mask_threshold; mask_k_area = pixels owned by k;
          segment ids, fusion and the area test as in `assign_segment_ids` (duplicate ids included).
        - The map is int32, 0 where no segment was painted.  An image without a kept query gets a float32 map of -1
          (at the target size, 384 x 384 without one) and no segments.
        label_ids_to_fuse=None logs the dependency's warning and fuses nothing.

        Kernels (csrc/postprocess_sp.hip) compute the kept queries' 384 x 384 probabilities, then per target pixel
        the argmax and the two per-query counts; ONE device-to-host copy of the (B, K, 2) counts feeds the host
        id assignment, and a last kernel relabels the map through the k -> id table."""
        if label_ids_to_fuse is None:
            logger.warning("`label_ids_to_fuse` unset. No instance will be fused.")
            label_ids_to_fuse = set()
        logits = _device_logits(outputs)
        cls = outputs.class_queries_logits
        B = cls.shape[0]
        num_labels = cls.shape[-1] - 1
        if target_sizes is not None and len(target_sizes) != B:
            raise ValueError("Make sure that you pass in as many target sizes as the batch dimension of the logits")
        dev = logits.device
        sizes = [tuple(int(v) for v in t) for t in target_sizes] if target_sizes is not None else [ops._GRID] * B

        # ---- query selection on the host (remove_low_and_no_objects, :121-146)
        cls_cpu = cls.detach().float().cpu()
        pred_scores, pred_labels = torch.nn.functional.softmax(cls_cpu, dim=-1).max(-1)
        keep = pred_labels.ne(num_labels) & (pred_scores > threshold)
        kept = [torch.nonzero(keep[i]).flatten() for i in range(B)]
        n_kept = [int(k.numel()) for k in kept]
        K = max(1, max(n_kept))
        kept_q = torch.zeros(B, K, dtype=torch.int32)
        kept_s = torch.zeros(B, K, dtype=torch.float32)
        for i in range(B):
            kept_q[i, :n_kept[i]] = kept[i].to(torch.int32)
            kept_s[i, :n_kept[i]] = pred_scores[i, kept[i]]

        results: list = [None] * B
        groups = []
        if any(n_kept):
            kept_q_d, kept_s_d = kept_q.to(dev), kept_s.to(dev)
            n_kept_d = torch.tensor(n_kept, dtype=torch.int32).to(dev)
            G = ops.panoptic_probs(logits, kept_q_d, n_kept_d)
            counts = torch.zeros(B, K, 2, dtype=torch.int32, device=dev)
            live = [i for i in range(B) if n_kept[i]]
            for size in dict.fromkeys(sizes[i] for i in live):  # one launch per distinct target size
                rows = [i for i in live if sizes[i] == size]
                rows_d = torch.tensor(rows, dtype=torch.int32).to(dev)
                groups.append((rows, rows_d, ops.panoptic_segments(G, rows_d, n_kept_d, kept_s_d, counts, size, mask_threshold)))
            # ---- the one device-to-host copy of the call's pixel results
            counts_cpu = counts.cpu()
            table = torch.zeros(B, K, dtype=torch.int32)
            segments = [[] for _ in range(B)]
            for i in live:
                n = n_kept[i]
                ids, segments[i] = assign_segment_ids(pred_labels[i, kept[i]].tolist(), kept_s[i, :n].tolist(),
                                                      counts_cpu[i, :n, 0].tolist(), counts_cpu[i, :n, 1].tolist(),
                                                      overlap_mask_area_threshold, label_ids_to_fuse)
                table[i, :n] = torch.tensor(ids, dtype=torch.int32)
            table_d = table.to(dev)
            for rows, rows_d, seg in groups:
                ops.panoptic_relabel_(seg, rows_d, table_d)
                for j, i in enumerate(rows):
                    results[i] = {"segmentation": seg[j], "segments_info": segments[i]}
        for i in range(B):
            if not n_kept[i]:
                results[i] = {"segmentation": torch.full(sizes[i], -1.0, dtype=torch.float32, device=dev), "segments_info": []}
        return results
