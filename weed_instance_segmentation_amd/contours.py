"""Polygons from id maps, and the VIA annotation export: the inverse of `polygons_to_instance_map`.

    from weed_instance_segmentation_amd import instance_polygons, save_via_annotations, trace_label_maps
    loops = trace_label_maps(prediction["segmentation"], n=len(prediction["segments_info"]))  # id -> [{"points", "hole"}]
    save_via_annotations("pre_annotations.json", predictions, file_names, model.config.id2label)

The pixels are read on the device by a fixed chain of launches, whatever the number of segments (csrc/trace.hip: every
pixel side between a segment and something else is a directed edge with one successor, so the boundary is a set of closed
loops that pointer jumping orders).  This module is the host half: it cuts the CSR result of `ops.labelmap_trace` into
per-image dicts and writes the VIA JSON that `SorghumWeedDataset` and `load_ground_truth` read.
- coords="pixel": pixel-index coordinates, what `cv2.fillPoly`, VIA and the loaders use.  `fill_poly` of all loops of an
  id repaints its mask exactly (holes by the even-odd rule).
- coords="crack": vertices of the corner lattice between the pixels; the even-odd interior at pixel centres is the mask.
A loop with "hole": True runs round a hole of its segment (its crack area is negative).
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import ops
from .rle import _as_device_maps

COORDS = {"crack": 0, "pixel": 1}
_MAX_BATCH = 4096  # images per trace call (the kernels' bound)


def loops_from_csr(points, loop_offsets, loop_image, loop_id, twice_area, n_images: int) -> list[dict]:
    """The host half of `trace_label_maps`: the arrays of `ops.labelmap_trace` (on the host) -> per image a dict
    id -> [{"points": (P, 2) int32 array of x, y, "hole": bool}, ...] over the ids that own a pixel, ascending, each id's
    loops in leader order."""
    points = np.asarray(points, dtype=np.int32).reshape(-1, 2)
    offsets, image, ident, area = (np.asarray(a, dtype=np.int64) for a in (loop_offsets, loop_image, loop_id, twice_area))
    out: list[dict] = [{} for _ in range(int(n_images))]
    for l in range(len(image)):
        out[int(image[l])].setdefault(int(ident[l]), []).append(
            {"points": points[int(offsets[l]):int(offsets[l + 1])], "hole": bool(area[l] < 0)})
    return out


def _batch_limit(H: int, W: int) -> int:
    return max(1, min(_MAX_BATCH, (2 ** 31 - 1) // (4 * H * W)))


def trace_label_maps(maps, n: int | None = None, coords: str = "pixel", simplify: bool = True):
    """Trace every id of one (H, W) id map, a (B, H, W) stack or a list of maps of one size -- fp32 with -1 background
    (the post-processor's map), int32 or uint8; a host map is moved to the current GPU.

    The ids are 0 .. n-1 (-1, the background, is not traced); without `n` it is taken from the maps' maximum (one more
    synchronisation); a value outside [-1, n) raises ValueError.  Returns per image a dict id -> list of loops
    `{"points": (P, 2) int32 ndarray of x, y, "hole": bool}` that holds only the ids with at least one pixel, ascending
    (one dict for an (H, W) map, else a list of them).  simplify=True keeps only the points where the outline turns;
    nothing lossy is done."""
    if coords not in COORDS:
        raise ValueError(f"coords must be one of {sorted(COORDS)}, got {coords!r}")
    maps = _as_device_maps(maps, "trace_label_maps")
    single = maps.dim() == 2
    stack = maps.unsqueeze(0) if single else maps
    if n is None:
        n = max(0, int(stack.max()) + 1)
    out = []
    step = _batch_limit(int(stack.shape[1]), int(stack.shape[2])) if stack.shape[1] and stack.shape[2] else 1
    for b0 in range(0, stack.shape[0], step):
        part = stack[b0:b0 + step]
        csr = ops.labelmap_trace(part, int(n), COORDS[coords], simplify)
        out += loops_from_csr(*(t.cpu().numpy() for t in csr[:5]), part.shape[0])
    return out[0] if single else out


def _add_polygons(results, maps=None, coords: str = "pixel", simplify: bool = True) -> None:
    """`polygons` for every segments_info entry of `results` that still owns a pixel of its map (maps[i], or the result's
    own `segmentation`); one trace per distinct map size."""
    if maps is None:
        maps = [r["segmentation"] for r in results]
    groups: dict = {}
    for i, seg in enumerate(maps):
        if not isinstance(seg, torch.Tensor) or seg.dim() != 2:
            raise ValueError("instance_polygons: every result needs its (H, W) id map as `segmentation`")
        groups.setdefault(tuple(seg.shape), []).append(i)
    for rows in groups.values():
        n = max(len(results[i]["segments_info"]) for i in rows)
        traced = trace_label_maps([maps[i] for i in rows], n=n, coords=coords, simplify=simplify)
        for i, loops in zip(rows, traced):
            for info in results[i]["segments_info"]:
                info.pop("polygons", None)
                if info["id"] in loops:  # else painted over entirely
                    info["polygons"] = loops[info["id"]]


def instance_polygons(result: dict, coords: str = "pixel", simplify: bool = True) -> dict:
    """One result of `post_process_instance_segmentation` (its `segmentation` the (H, W) id map) -> the same dict, with
    "polygons" -- the list of loops `{"points", "hole"}` of `trace_label_maps` -- added to every `segments_info` entry
    that still owns a pixel."""
    _add_polygons([result], coords=coords, simplify=simplify)
    return result


# ----------------------------------------------------------------------------------------------------------- VIA export
def _classname(id2label, label_id: int) -> str:
    for key in (label_id, str(label_id)):
        if key in id2label:
            return id2label[key]
    raise KeyError(f"via_annotations: id2label has no name for label id {label_id}")


def via_annotations(results, filenames, id2label, score_threshold: float = 0.0) -> dict:
    """The list `post_process_instance_segmentation` returns -> a VIA (VGG Image Annotator) project dict, the format
    `SorghumWeedDataset` and `load_ground_truth` read: per image `{"filename", "size": -1, "regions": [...],
    "file_attributes": {}}` under the key filename + "-1".  Every OUTER loop of every instance whose score reaches
    `score_threshold` becomes one region `{"shape_attributes": {"name": "polygon", "all_points_x": [...],
    "all_points_y": [...]}, "region_attributes": {"classname": id2label[label_id]}}` in pixel coordinates (plain ints),
    instances in `segments_info` order; a loop of one or two points is written too (the loaders' fillPoly paints a point
    or a line).  Hole loops are NOT exported: a VIA polygon has no holes, so a loader repaints a segment with a hole as
    filled.  A result none of whose entries carries "polygons" yet is traced here (one trace per distinct map size)."""
    results = list(results)
    if len(results) != len(filenames):
        raise ValueError(f"{len(results)} results but {len(filenames)} file names")
    todo = [i for i, r in enumerate(results) if r["segments_info"] and not any("polygons" in s for s in r["segments_info"])]
    traced = {}
    if todo:
        copies = [{"segmentation": results[i]["segmentation"],
                   "segments_info": [{"id": s["id"]} for s in results[i]["segments_info"]]} for i in todo]
        _add_polygons(copies)
        traced = {i: {s["id"]: s.get("polygons", []) for s in c["segments_info"]} for i, c in zip(todo, copies)}
    out = {}
    for i, (r, name) in enumerate(zip(results, filenames)):
        regions = []
        for s in r["segments_info"]:
            if float(s.get("score", 1.0)) < score_threshold:
                continue
            loops = traced[i][s["id"]] if i in traced else s.get("polygons", [])  # none: painted over entirely
            for loop in loops:
                if loop["hole"]:
                    continue
                pts = np.asarray(loop["points"]).reshape(-1, 2)
                regions.append({"shape_attributes": {"name": "polygon", "all_points_x": [int(v) for v in pts[:, 0]],
                                                     "all_points_y": [int(v) for v in pts[:, 1]]},
                                "region_attributes": {"classname": _classname(id2label, int(s["label_id"]))}})
        out[f"{name}-1"] = {"filename": name, "size": -1, "regions": regions, "file_attributes": {}}
    return out


def save_via_annotations(path, results, filenames, id2label, score_threshold: float = 0.0) -> dict:
    """`via_annotations(...)` written to `path` as JSON; returns the dict."""
    project = via_annotations(results, filenames, id2label, score_threshold)
    with open(path, "w") as f:
        json.dump(project, f)
    return project
