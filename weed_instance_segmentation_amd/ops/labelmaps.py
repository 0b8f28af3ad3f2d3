"""Label-map metrics: label expansion, pair counts and COCO matching, per-instance statistics
(section 21), panoptic matching and the semantic confusion matrix (section 22), boundary bands and the matching on the
smaller of two IoUs (section 25)."""
from __future__ import annotations

import torch

from .._lib import load
from ._core import _dtype_code, _id_maps, _id_maps_d2, _id_rows, _launch, _p, _req, _workspace


def labelmap_to_masks(label_map: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """(H, W) int32 id map, (T,) int32 ids -> (T, H, W) uint8 masks `label_map == ids[t]` on the device."""
    label_map, ids = _req(label_map, "label_map", torch.int32), _req(ids, "ids", torch.int32)
    H, W = label_map.shape
    T = int(ids.shape[0])
    out = torch.empty(T, H, W, device=label_map.device, dtype=torch.uint8)
    if T == 0:
        return out
    if (H * W) % 4:
        raise ValueError("labelmap_to_masks: H * W must be divisible by 4")
    _launch("wm2f_labelmap_to_masks", label_map, _p(label_map), _p(ids), _p(out), H * W, T)
    return out


def labelmap_pair_counts(pred_maps: torch.Tensor, gt_maps: torch.Tensor, gt_ids: torch.Tensor, n_ids: torch.Tensor,
                         P: int) -> torch.Tensor:
    """(B, H, W) prediction id maps (fp32 with -1 background, or int32), (B, H, W) GT raw-id maps (uint8 or int32),
    (B, G) ascending accepted GT ids with n_ids (B) valid -> (B, P+1, G+1) int32 joint histogram (row 0: no prediction,
    column 0: no accepted GT id)."""
    if not isinstance(pred_maps, torch.Tensor) or not isinstance(gt_maps, torch.Tensor):
        raise TypeError("labelmap_pair_counts: expected tensors")
    pred_maps = _req(pred_maps, "pred_maps", pred_maps.dtype)
    gt_maps = _req(gt_maps, "gt_maps", gt_maps.dtype)
    gt_ids, n_ids = _req(gt_ids, "gt_ids", torch.int32), _req(n_ids, "n_ids", torch.int32)
    error = f"labelmap_pair_counts: prediction maps fp32 / int32 and GT maps uint8 / int32, got {pred_maps.dtype} / {gt_maps.dtype}"
    pdt = _dtype_code(pred_maps, (torch.float32, torch.int32), error)
    gdt = _dtype_code(gt_maps, (torch.uint8, torch.int32), error)
    B = pred_maps.shape[0]
    if gt_maps.shape != pred_maps.shape or gt_ids.dim() != 2 or gt_ids.shape[0] != B or n_ids.shape != (B,):
        raise ValueError("labelmap_pair_counts: shapes disagree")
    n = pred_maps[0].numel()
    G = int(gt_ids.shape[1])
    hist = torch.empty(B, P + 1, G + 1, device=pred_maps.device, dtype=torch.int32)
    _launch("wm2f_labelmap_pair_counts", pred_maps, _p(pred_maps), pdt, _p(gt_maps), gdt, _p(gt_ids), _p(n_ids), _p(hist), B, n,
            P, G, tag="labelmap_pair_counts")
    return hist


def mask_pair_counts(det_masks: torch.Tensor, gt_masks: torch.Tensor):
    """(D, H, W) and (G, H, W) bool / uint8 mask stacks (may overlap) -> inter (D, G), det_area (D), gt_area (G) int32."""
    det_masks = _req(det_masks, "det_masks", det_masks.dtype if det_masks.dtype in (torch.bool, torch.uint8) else torch.uint8)
    gt_masks = _req(gt_masks, "gt_masks", gt_masks.dtype if gt_masks.dtype in (torch.bool, torch.uint8) else torch.uint8)
    if det_masks.shape[1:] != gt_masks.shape[1:]:
        raise ValueError(f"mask_pair_counts: mask sizes differ: {tuple(det_masks.shape)} vs {tuple(gt_masks.shape)}")
    D, G = int(det_masks.shape[0]), int(gt_masks.shape[0])
    n = det_masks[0].numel() if D else gt_masks[0].numel()
    dev = det_masks.device
    inter = torch.zeros(D, G, device=dev, dtype=torch.int32)
    det_area = torch.zeros(D, device=dev, dtype=torch.int32)
    gt_area = torch.zeros(G, device=dev, dtype=torch.int32)
    if D + G == 0 or n == 0:
        return inter, det_area, gt_area
    ws = torch.empty(int(load().wm2f_mask_pair_counts_workspace(D, G, n)), device=dev, dtype=torch.uint8)
    a, g = det_masks.view(torch.uint8), gt_masks.view(torch.uint8)
    _launch("wm2f_mask_pair_counts", a, _p(a) if D else None, _p(g) if G else None, _p(inter), _p(det_area), _p(gt_area), _p(ws),
            D, G, n, tag="mask_pair_counts")
    return inter, det_area, gt_area


def _match_args(name, inter, det_area, gt_area, det_label, gt_label, det_order, n_det, n_gt, iou_thresholds, area_ranges):
    """The checked arguments and sizes the two matching entry points share."""
    i32 = torch.int32
    inter, det_area, gt_area = _req(inter, "inter", i32), _req(det_area, "det_area", i32), _req(gt_area, "gt_area", i32)
    det_label, gt_label = _req(det_label, "det_label", i32), _req(gt_label, "gt_label", i32)
    det_order, n_det, n_gt = _req(det_order, "det_order", i32), _req(n_det, "n_det", i32), _req(n_gt, "n_gt", i32)
    thr, rng = _req(iou_thresholds, "iou_thresholds", torch.float64), _req(area_ranges, "area_ranges", torch.float64)
    if inter.dim() != 3:
        raise ValueError(f"{name}: inter must be (B, D, G)")
    B, D, G = (int(v) for v in inter.shape)
    T, A = int(thr.shape[0]), int(rng.shape[0])
    if (det_area.shape != (B, D) or det_label.shape != (B, D) or det_order.shape != (B, D) or gt_area.shape != (B, G)
            or gt_label.shape != (B, G) or n_det.shape != (B,) or n_gt.shape != (B,) or rng.shape != (A, 2)):
        raise ValueError(f"{name}: shapes disagree")
    return (inter, det_area, gt_area, det_label, gt_label, det_order, n_det, n_gt, thr, rng), (B, D, G, T, A)


def coco_match(inter, det_area, gt_area, det_label, gt_label, det_order, n_det, n_gt, iou_thresholds, area_ranges,
               max_det: int):
    """Greedy COCO matching of B images (wm2f_coco_match): inter (B, D, G), det_* (B, D), gt_* (B, G), n_det / n_gt (B)
    int32; iou_thresholds (T), area_ranges (A, 2) fp64.  Returns det_rank (B, D) int32, det_matched / det_ignored
    (B, A, T, D) uint8, gt_ignored (B, A, G) uint8."""
    (inter, det_area, gt_area, det_label, gt_label, det_order, n_det, n_gt, thr, rng), (B, D, G, T, A) = _match_args(
        "coco_match", inter, det_area, gt_area, det_label, gt_label, det_order, n_det, n_gt, iou_thresholds, area_ranges)
    i32 = torch.int32
    dev = inter.device
    det_rank = torch.empty(B, D, device=dev, dtype=i32)
    det_matched = torch.empty(B, A, T, D, device=dev, dtype=torch.uint8)
    det_ignored = torch.empty(B, A, T, D, device=dev, dtype=torch.uint8)
    gt_ignored = torch.empty(B, A, G, device=dev, dtype=torch.uint8)
    _launch("wm2f_coco_match", inter, _p(inter), _p(det_area), _p(gt_area), _p(det_label), _p(gt_label), _p(det_order), _p(n_det),
            _p(n_gt), _p(thr), _p(rng), _p(det_rank), _p(det_matched), _p(det_ignored), _p(gt_ignored), B, D, G, T, A,
            int(max_det), tag="coco_match")
    return det_rank, det_matched, det_ignored, gt_ignored


def coco_match_min(inter, det_area, gt_area, inter2, det_area2, gt_area2, det_label, gt_label, det_order, n_det, n_gt,
                   iou_thresholds, area_ranges, max_det: int):
    """`coco_match` on the smaller of two IoUs (wm2f_coco_match_min): the second triple inter2 (B, D, G), det_area2 (B, D),
    gt_area2 (B, G) int32 next to the first; a pair's IoU is min(inter / union, inter2 / union2).  Area ranges, labels,
    order, ranks and the four results are `coco_match`'s, taken from the first triple."""
    (inter, det_area, gt_area, det_label, gt_label, det_order, n_det, n_gt, thr, rng), (B, D, G, T, A) = _match_args(
        "coco_match_min", inter, det_area, gt_area, det_label, gt_label, det_order, n_det, n_gt, iou_thresholds, area_ranges)
    i32 = torch.int32
    inter2, det_area2, gt_area2 = _req(inter2, "inter2", i32), _req(det_area2, "det_area2", i32), _req(gt_area2, "gt_area2", i32)
    if inter2.shape != (B, D, G) or det_area2.shape != (B, D) or gt_area2.shape != (B, G):
        raise ValueError("coco_match_min: the second triple must have the shapes of the first")
    dev = inter.device
    det_rank = torch.empty(B, D, device=dev, dtype=i32)
    det_matched = torch.empty(B, A, T, D, device=dev, dtype=torch.uint8)
    det_ignored = torch.empty(B, A, T, D, device=dev, dtype=torch.uint8)
    gt_ignored = torch.empty(B, A, G, device=dev, dtype=torch.uint8)
    _launch("wm2f_coco_match_min", inter, _p(inter), _p(det_area), _p(gt_area), _p(inter2), _p(det_area2), _p(gt_area2),
            _p(det_label), _p(gt_label), _p(det_order), _p(n_det), _p(n_gt), _p(thr), _p(rng), _p(det_rank), _p(det_matched),
            _p(det_ignored), _p(gt_ignored), B, D, G, T, A, int(max_det), tag="coco_match_min")
    return det_rank, det_matched, det_ignored, gt_ignored


def labelmap_boundary(maps: torch.Tensor, d: int) -> torch.Tensor:
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8) -> (B, H, W) int32 band maps
    (wm2f_labelmap_boundary): a pixel keeps its id where the (2d+1) x (2d+1) square around it leaves the image or meets
    another id -- the boundary band of its instance -- and is -1 where it is interior or has no id."""
    d = int(d)
    maps, dt, B, H, W = _id_maps(maps, "labelmap_boundary", detail=f", d = {d}", bad=d < 1)
    out = torch.empty(B, H, W, device=maps.device, dtype=torch.int32)
    ws = _workspace(load().wm2f_labelmap_boundary_workspace(B, H, W), maps.device)
    _launch("wm2f_labelmap_boundary", maps, _p(maps), dt, _p(out), _p(ws), B, H, W, d, tag="labelmap_boundary")
    return out


def labelmap_instance_stats(maps: torch.Tensor, ids: torch.Tensor | None = None, n_ids: torch.Tensor | None = None,
                            N: int | None = None) -> torch.Tensor:
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8) -> (B, N, 8) int64
    [area, xmin, ymin, xmax, ymax, sum_x, sum_y, 0] per id (wm2f_labelmap_instance_stats), xmax / ymax inclusive, an id
    without a pixel [0, W, H, -1, -1, 0, 0, 0].  Without `ids`, row r is id r of [0, N).  With `ids` (B, N) int32
    ascending and `n_ids` (B) of them valid, row r is the raw id ids[b][r]."""
    maps, dt, B, H, W = _id_maps(maps, "labelmap_instance_stats", "tensors")
    ids, n_ids, N = _id_rows("labelmap_instance_stats", B, ids, n_ids, N)
    stats = torch.empty(B, N, 8, device=maps.device, dtype=torch.int64)
    if N == 0:
        return stats
    _launch("wm2f_labelmap_instance_stats", maps, _p(maps), dt, _p(ids), _p(n_ids), _p(stats), B, H, W, N, tag="instance_stats")
    return stats


def labelmap_distance(maps: torch.Tensor, border_outside: bool = True) -> torch.Tensor:
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8) -> (B, H, W) int32 squared Euclidean distance of every
    pixel to the nearest position that does not carry its id (wm2f_labelmap_distance), 0 for a pixel without an id.
    `border_outside`: the positions just beyond the image count as not carrying the id; without it only real pixels do,
    and a pixel whose id fills its whole image gets INT32_MAX."""
    maps, dt, B, H, W = _id_maps(maps, "labelmap_distance", detail="")
    d2 = torch.empty(B, H, W, device=maps.device, dtype=torch.int32)
    ws = _workspace(load().wm2f_labelmap_distance_workspace(B, H, W), maps.device)
    _launch("wm2f_labelmap_distance", maps, _p(maps), dt, _p(d2), _p(ws), B, H, W, int(bool(border_outside)),
            tag="labelmap_distance")
    return d2


def labelmap_aim_points(maps: torch.Tensor, d2: torch.Tensor, ids: torch.Tensor | None = None,
                        n_ids: torch.Tensor | None = None, N: int | None = None,
                        stats: torch.Tensor | None = None) -> torch.Tensor:
    """(B, H, W) id maps and their `labelmap_distance` -> (B, N, 4) int32 [x, y, d2max, 0] per id
    (wm2f_labelmap_aim_points): a pixel of the instance where d2 is largest -- among equals the one nearest the rounded
    centroid of `stats` (`labelmap_instance_stats` of the same maps and rows; without it this term is 0), then the first
    in raster order; [-1, -1, 0, 0] for an id without a pixel.  `ids` / `n_ids` / `N` as in `labelmap_instance_stats`."""
    maps, dt, d2, B, H, W = _id_maps_d2(maps, d2, "labelmap_aim_points")
    ids, n_ids, N = _id_rows("labelmap_aim_points", B, ids, n_ids, N)
    if stats is not None:
        stats = _req(stats, "stats", torch.int64)
        if stats.shape != (B, N, 8):
            raise ValueError(f"labelmap_aim_points: stats must be ({B}, {N}, 8), got {tuple(stats.shape)}")
    points = torch.empty(B, N, 4, device=maps.device, dtype=torch.int32)
    if N == 0:
        return points
    ws = _workspace(load().wm2f_labelmap_aim_points_workspace(B, N), maps.device, 8)
    _launch("wm2f_labelmap_aim_points", maps, _p(maps), dt, _p(d2), _p(ids), _p(n_ids), _p(stats), _p(points), _p(ws),
            B, H, W, N, tag="labelmap_aim_points")
    return points


SHAPE_COLUMNS = 10
SHAPE_LDS_MAX_IDS = 1024          # wm2f_labelmap_shape_stats: accumulators in LDS up to this N, in the result above
HULL_BOUND_ROWS = 4 * 1024 * 1024  # labelmap_hull: a row table of B N H rows is allocated as it is up to this size (96 MiB)


def labelmap_shape_stats(maps: torch.Tensor, ids: torch.Tensor | None = None, n_ids: torch.Tensor | None = None,
                         N: int | None = None) -> torch.Tensor:
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8) -> (B, N, 10) int64
    [area, sum_x, sum_y, sum_xx, sum_yy, sum_xy, sides, p_straight, p_diag, p_mixed] per id
    (wm2f_labelmap_shape_stats): the raw moments of the pixel indices, the pixel sides between the instance and anything
    else (the outside of the image included) and the three border-pixel counts of the 4-neighbourhood perimeter; an id
    without a pixel has an all-zero row.  `ids` / `n_ids` / `N` as in `labelmap_instance_stats`."""
    maps, dt, B, H, W = _id_maps(maps, "labelmap_shape_stats", "tensors")
    ids, n_ids, N = _id_rows("labelmap_shape_stats", B, ids, n_ids, N)
    shape = torch.empty(B, N, SHAPE_COLUMNS, device=maps.device, dtype=torch.int64)
    if N == 0:
        return shape
    _launch("wm2f_labelmap_shape_stats", maps, _p(maps), dt, _p(ids), _p(n_ids), _p(shape), B, H, W, N, tag="shape_stats")
    return shape


def labelmap_hull(maps: torch.Tensor, ids: torch.Tensor | None = None, n_ids: torch.Tensor | None = None,
                  N: int | None = None, stats: torch.Tensor | None = None, vertices: bool = False):
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8) -> hull (B, N, 3) int64
    [n_vertices, area2, feret2] per id (wm2f_labelmap_hull): the convex hull of the instance's pixel squares on the
    corner lattice [0, W] x [0, H] -- its number of vertices, twice its area (exact) and the largest squared distance
    between two vertices; [0, 0, 0] for an id without a pixel.  `ids` / `n_ids` / `N` as in `labelmap_instance_stats`;
    `stats`: that op's result for the same maps and rows (computed here when None).

    vertices=True returns (hull, points): points (B, N, K, 2) int32, a padded block with K = the largest n_vertices (at
    least 1), row [b, r, k] the k-th vertex (x, y) of the instance and (-1, -1) past its n_vertices.  The vertices are
    strictly convex, start at the smallest (y, then x) and go on towards increasing x (clockwise on the screen: with y
    down every consecutive cross product is positive).

    Host copies: none while the row table's bound B N H is at most HULL_BOUND_ROWS rows; above it copy 1, the sum of the
    box heights (one int64), sizes the table.  vertices=True adds copy 2, the largest n_vertices (one int64), which
    sizes the block.  The three scalars never need more than copy 1."""
    maps, dt, B, H, W = _id_maps(maps, "labelmap_hull", "tensors")
    ids, n_ids, N = _id_rows("labelmap_hull", B, ids, n_ids, N)
    hull = torch.empty(B, N, 3, device=maps.device, dtype=torch.int64)
    if N == 0:
        return (hull, torch.empty(B, 0, 1, 2, device=maps.device, dtype=torch.int32)) if vertices else hull
    if stats is None:
        stats = labelmap_instance_stats(maps, ids, n_ids, N=N)
    else:
        stats = _req(stats, "stats", torch.int64)
        if stats.shape != (B, N, 8):
            raise ValueError(f"labelmap_hull: stats must be ({B}, {N}, 8), got {tuple(stats.shape)}")
    rows = B * N * H
    if rows > HULL_BOUND_ROWS:
        heights = torch.where(stats[..., 0] > 0, stats[..., 4] - stats[..., 2] + 1, torch.zeros_like(stats[..., 0]))
        rows = int(heights.sum())  # copy 1
    ws = _workspace(load().wm2f_labelmap_hull_workspace(B, N, rows), maps.device, 8)
    _launch("wm2f_labelmap_hull", maps, _p(maps), dt, _p(ids), _p(n_ids), _p(stats), _p(hull), _p(ws), rows, B, H, W, N,
            tag="labelmap_hull")
    if not vertices:
        return hull
    K = max(1, int(hull[..., 0].max()))  # copy 2
    points = torch.empty(B, N, K, 2, device=maps.device, dtype=torch.int32)
    _launch("wm2f_labelmap_hull_vertices", maps, _p(stats), _p(hull), _p(ws), rows, _p(points), B, H, N, K,
            tag="labelmap_hull_vertices")
    return hull, points


# wm2f_labelmap_nearest's bounds and launch shape (include/wm2f.h), for callers and tests
NEAREST_MAX_D2 = 1024 * 1024
NEAREST_MIN_CHUNK_ROWS = 32   # columns pass: rows of a chunk, at least (exactly, for a small map taller than this)
NEAREST_ROW_PIXELS = 1024     # rows pass: shorter rows share a workgroup
NEAREST_WIDE_ROW = 4096       # rows pass: a longer row gets 1024 threads
CELL_MAX_GROUPS = 8
INT32_MAX = 2 ** 31 - 1


def labelmap_nearest(maps: torch.Tensor, N: int, max_d2: int, source: torch.Tensor | None = None, blocked: bool = True,
                     walk_all: bool = False):
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8) whose instances are the ids 0 .. N-1 -> (nearest, d2),
    both (B, H, W) int32 (wm2f_labelmap_nearest): per pixel the nearest source instance within squared distance `max_d2`
    (the smallest id among equally near ones) and that squared distance; -1 and INT32_MAX where there is none.  `source`
    (B, N) uint8 / bool: which instances are sources (None: all).  `blocked`: a pixel of an instance that is no source is
    written as its own id with d2 = 0; otherwise it is a query like a free pixel.  `walk_all` switches the rows pass's
    early "none" off (same results; for measurements)."""
    N, max_d2 = int(N), int(max_d2)
    maps, dt, B, H, W = _id_maps(maps, "labelmap_nearest", detail=f", N = {N}, max_d2 = {max_d2}", bad=N < 1 or max_d2 < 0)
    if source is not None:
        source = _req(source, "source", source.dtype if source.dtype in (torch.bool, torch.uint8) else torch.uint8)
        if source.shape != (B, N):
            raise ValueError(f"labelmap_nearest: source must be ({B}, {N}), got {tuple(source.shape)}")
        source = source.view(torch.uint8)
    nearest = torch.empty(B, H, W, device=maps.device, dtype=torch.int32)
    d2 = torch.empty(B, H, W, device=maps.device, dtype=torch.int32)
    ws = _workspace(load().wm2f_labelmap_nearest_workspace(B, H, W), maps.device)
    flags = (1 if blocked else 0) | (2 if walk_all else 0)
    _launch("wm2f_labelmap_nearest", maps, _p(maps), dt, _p(source), _p(nearest), _p(d2), _p(ws), B, H, W, N, max_d2, flags,
            tag="labelmap_nearest")
    return nearest, d2


def cell_grid_shape(H: int, W: int, cell, offset=(0, 0)):
    """(GH, GW) of the grid whose cell (cy, cx) holds the pixels with (y + off_y) // cell_h == cy, (x + off_x) // cell_w == cx."""
    return -(-(int(H) + int(offset[0])) // int(cell[0])), -(-(int(W) + int(offset[1])) // int(cell[1]))


def labelmap_cell_counts(maps: torch.Tensor, group: torch.Tensor, G: int, cell, offset=(0, 0),
                         veto_d2: torch.Tensor | None = None, veto_max: int = 0) -> torch.Tensor:
    """(B, H, W) id maps and group (B, N) uint8 -> counts (B, GH, GW, 2G) int32 (wm2f_labelmap_cell_counts): per cell of
    `cell` = (h, w) pixels, shifted by `offset` = (off_y, off_x) with 0 <= off < cell, the pixels of the instances of
    every group 0 .. G-1 (group value 255: not counted).  Column g counts the pixels with veto_d2 > veto_max (all of them
    without `veto_d2`), column G + g the others."""
    G, (ch, cw), (oy, ox) = int(G), (int(v) for v in cell), (int(v) for v in offset)
    maps, dt, B, H, W = _id_maps(
        maps, "labelmap_cell_counts", detail=f", cell {ch} x {cw}, offset ({oy}, {ox}), G = {G}",
        bad=ch < 1 or cw < 1 or not (0 <= oy < ch and 0 <= ox < cw) or not 1 <= G <= CELL_MAX_GROUPS)
    group = _req(group, "group", torch.uint8)
    if group.dim() != 2 or group.shape[0] != B or group.shape[1] < 1:
        raise ValueError(f"labelmap_cell_counts: group must be ({B}, N), got {tuple(group.shape)}")
    N = int(group.shape[1])
    if veto_d2 is not None:
        veto_d2 = _req(veto_d2, "veto_d2", torch.int32)
        if veto_d2.shape != maps.shape:
            raise ValueError(f"labelmap_cell_counts: veto_d2 must be {tuple(maps.shape)}, got {tuple(veto_d2.shape)}")
    if int(veto_max) < 0:
        raise ValueError(f"labelmap_cell_counts: veto_max must not be negative, got {veto_max}")
    GH, GW = cell_grid_shape(H, W, (ch, cw), (oy, ox))
    counts = torch.empty(B, GH, GW, 2 * G, device=maps.device, dtype=torch.int32)
    _launch("wm2f_labelmap_cell_counts", maps, _p(maps), dt, _p(group), _p(veto_d2), int(veto_max), _p(counts), B, H, W, N, G,
            ch, cw, oy, ox, tag="labelmap_cell_counts")
    return counts


def panoptic_match(hist, pred_label, gt_label, n_pred, n_gt, void_as_background: bool = False):
    """PQ's segment matching of B images (wm2f_panoptic_match): hist (B, P+1, G+1), pred_label (B, P), gt_label (B, G),
    n_pred / n_gt (B) int32.  Returns gt_match (B, G) int32 (matched prediction row, -1 false negative, -2 no such GT),
    gt_iou (B, G) fp64 and pred_state (B, P) uint8 (0 matched, 1 false positive, 2 dropped as mostly void, 3 none)."""
    i32 = torch.int32
    hist, pred_label, gt_label = _req(hist, "hist", i32), _req(pred_label, "pred_label", i32), _req(gt_label, "gt_label", i32)
    n_pred, n_gt = _req(n_pred, "n_pred", i32), _req(n_gt, "n_gt", i32)
    if hist.dim() != 3 or pred_label.dim() != 2 or gt_label.dim() != 2:
        raise ValueError("panoptic_match: hist must be (B, P+1, G+1), the labels (B, P) and (B, G)")
    B, P, G = int(hist.shape[0]), int(pred_label.shape[1]), int(gt_label.shape[1])
    if hist.shape != (B, P + 1, G + 1) or pred_label.shape[0] != B or gt_label.shape[0] != B or n_pred.shape != (B,) or n_gt.shape != (B,):
        raise ValueError("panoptic_match: shapes disagree")
    dev = hist.device
    gt_match = torch.empty(B, G, device=dev, dtype=i32)
    gt_iou = torch.empty(B, G, device=dev, dtype=torch.float64)
    pred_state = torch.empty(B, P, device=dev, dtype=torch.uint8)
    if B == 0:
        return gt_match, gt_iou, pred_state
    _launch("wm2f_panoptic_match", hist, _p(hist), _p(pred_label), _p(gt_label), _p(n_pred), _p(n_gt), _p(gt_match), _p(gt_iou),
            _p(pred_state), B, P, G, int(bool(void_as_background)), tag="panoptic_match")
    return gt_match, gt_iou, pred_state


def semantic_confusion_(conf: torch.Tensor, n_out_of_range: torch.Tensor, pred: torch.Tensor, gt: torch.Tensor,
                        ignore_index: int | None = None, gt_ids: torch.Tensor | None = None,
                        gt_cls: torch.Tensor | None = None, n_ids: torch.Tensor | None = None,
                        background_label: int | None = None) -> None:
    """conf (C, C) int64 += the confusion matrix (rows GT, columns prediction) of pred (B, ...) int64 / int32 / uint8
    against gt (B, ...) uint8 / int32 (wm2f_semantic_confusion); n_out_of_range (1) int64 += the non-ignored pixels whose
    prediction is outside [0, C).  gt holds classes, or raw ids when gt_ids (B, G) ascending, gt_cls (B, G) and n_ids (B)
    int32 are given; an unlisted raw id then has class `background_label`, or is ignored without one.  In place, no
    synchronisation."""
    for name, t in (("conf", conf), ("n_out_of_range", n_out_of_range), ("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"semantic_confusion_: {name} must be a tensor")
    if not conf.is_contiguous() or not n_out_of_range.is_contiguous():
        raise ValueError("semantic_confusion_: conf and n_out_of_range must be contiguous (they are updated in place)")
    conf, n_out = _req(conf, "conf", torch.int64), _req(n_out_of_range, "n_out_of_range", torch.int64)
    pred, gt = _req(pred, "pred", pred.dtype), _req(gt, "gt", gt.dtype)
    error = f"semantic_confusion_: prediction maps int64 / int32 / uint8 and GT maps uint8 / int32, got {pred.dtype} / {gt.dtype}"
    pdt = _dtype_code(pred, (torch.int64, torch.int32, torch.uint8), error)
    gdt = _dtype_code(gt, (torch.uint8, torch.int32), error)
    if conf.dim() != 2 or conf.shape[0] != conf.shape[1] or n_out.numel() != 1:
        raise ValueError("semantic_confusion_: conf must be (C, C) and n_out_of_range one element")
    if pred.shape != gt.shape or pred.dim() < 2:
        raise ValueError(f"semantic_confusion_: maps must be (B, ...) of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    B, C = int(pred.shape[0]), int(conf.shape[0])
    G = 0
    if (gt_ids is None) != (gt_cls is None) or (gt_ids is None) != (n_ids is None):
        raise ValueError("semantic_confusion_: gt_ids, gt_cls and n_ids go together")
    if gt_ids is not None:
        gt_ids, gt_cls, n_ids = _req(gt_ids, "gt_ids", torch.int32), _req(gt_cls, "gt_cls", torch.int32), _req(n_ids, "n_ids", torch.int32)
        G = int(gt_ids.shape[1]) if gt_ids.dim() == 2 else -1
        if gt_ids.shape != (B, G) or gt_cls.shape != (B, G) or n_ids.shape != (B,):
            raise ValueError("semantic_confusion_: shapes disagree")
    if B == 0 or pred[0].numel() == 0 or C == 0:
        return
    n = pred[0].numel()
    ign = -2 ** 31 if ignore_index is None else int(ignore_index)
    bg = -1 if background_label is None else int(background_label)
    _launch("wm2f_semantic_confusion", pred, _p(pred), pdt, _p(gt), gdt, _p(gt_ids), _p(gt_cls), _p(n_ids), _p(conf), _p(n_out),
            B, n, G, C, ign, bg, tag="semantic_confusion")
