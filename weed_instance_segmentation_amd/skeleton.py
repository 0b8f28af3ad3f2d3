"""Plant skeletons on the GPU: the thinned id map of a segmentation result and, per plant, the length
of its skeleton, the number of its ends and junctions and the width of its parts.

    from weed_instance_segmentation_amd import SkeletonOptions, skeleton_maps, skeleton_statistics, annotate_skeletons
    skel = skeleton_maps(prediction["segmentation"], n)                       # an id map again, -1 off the skeletons
    traits = skeleton_statistics(prediction["segmentation"], n=n)
    traits["skeleton_length"], traits["tips"], traits["mean_width"]
    result = annotate_skeletons(result)                                       # the traits on every segments_info entry

Guo and Hall's two-sub-iteration parallel thinning runs on every instance at once in a fixed chain of launches of
csrc/skeleton.hip (tiles held in LDS for several iterations); a second kernel sums the skeleton per instance, and the
widths come from `distance_maps` of the original map.  The integers are exact; the float traits are a few float64
operations on them (`skeleton_from_sums`).  A long narrow plant with few ends is a grass weed, a plant of the same area
with many ends a broadleaf; the tips are a leaf-count proxy.

Not done here: spurs are not pruned, so the tip counts of ragged masks are raw (`clean_label_maps` first smooths the
worst of it); the skeleton is not traced into ordered polylines; there is no medial-axis transform by distance ridges.
The thinning rule is the paper's, restated in tests/skeleton_reference.py; byte identity with another library's `thin`
or `skeletonize` is not claimed.
"""
from __future__ import annotations

import dataclasses
import math
import warnings

import numpy as np
import torch

from . import _lib, ops
from .instances import _border_outside, _id_maps

SQRT2 = math.sqrt(2.0)
# what `annotate_skeletons` writes into a `segments_info` entry (the two widths only with `widths`)
SKELETON_TRAITS = ("skeleton_pixels", "skeleton_length", "tips", "junction_pixels", "mean_width", "max_width",
                   "length_per_area", "settled")
_INTEGER_TRAITS = ("skeleton_pixels", "tips", "junction_pixels")


@dataclasses.dataclass(frozen=True)
class SkeletonOptions:
    """How `skeleton_maps`, `skeleton_statistics` and `annotate_skeletons` thin.

    - `max_iterations` in [1, 1024]: the thinning iterations.  A solid part settles in about its half-width + 1; a map
      that has not settled is reported (`settled`, `status`) and is still the defined result of that many iterations.
    - `border`: the border mode of the distance map behind the widths, "outside" or "inside" (`distance_maps`).
    - `widths`: compute `mean_width` and `max_width` (one more `labelmap_distance` of the original map)."""
    max_iterations: int = 64
    border: str = "outside"
    widths: bool = True

    def __post_init__(self):
        r = self.max_iterations
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= r <= ops.skeleton.MAX_ROUNDS:
            raise ValueError(f"SkeletonOptions: max_iterations must be an integer in [1, {ops.skeleton.MAX_ROUNDS}], got {r!r}")
        _border_outside(self.border, "SkeletonOptions")
        if not isinstance(self.widths, (bool, np.bool_)):
            raise ValueError(f"SkeletonOptions: widths must be a bool, got {self.widths!r}")


def _options(options, who: str) -> SkeletonOptions:
    if options is None:
        return SkeletonOptions()
    if not isinstance(options, SkeletonOptions):
        raise TypeError(f"{who}: options must be a SkeletonOptions, got {type(options).__name__}")
    return options


def _device_stack(seg: torch.Tensor, who: str) -> torch.Tensor:
    if not torch.cuda.is_available():
        raise _lib.Wm2fError(f"{who} runs on a GPU only (no CPU fallback): no device is visible")
    dev = seg.device if seg.is_cuda else torch.device("cuda", torch.cuda.current_device())
    stack = seg.to(dev)
    return stack.unsqueeze(0) if seg.dim() == 2 else stack


def skeleton_maps(maps, n: int, options: SkeletonOptions | None = None, *, return_status: bool = False):
    """Thin one (H, W) id map or a (B, H, W) stack -- fp32 with -1 background (the post-processor's map), int32 or uint8,
    on the device or the host (a host map is moved to the current GPU).  The instances are the ids 0 .. n-1; every other
    value is background; every instance thins on its own, whatever touches it.

    Returns an int32 device tensor of the input's shape: the skeleton as an id map, -1 elsewhere -- `encode_label_maps`,
    `trace_label_maps` and `render_label_overlay` take it as it is.  `return_status=True` returns (map, status): status
    (..., 4) int32 [skeleton pixels, iterations that deleted something, deletions in the last iteration, iterations]; a
    non-zero third entry says `max_iterations` was too small."""
    options = _options(options, "skeleton_maps")
    seg = _id_maps(maps, "skeleton_maps")
    n = int(n)
    if not 0 <= n <= ops.skeleton.MAX_IDS:
        raise ValueError(f"skeleton_maps: n must be in [0, {ops.skeleton.MAX_IDS}], got {n}")
    out, status = ops.labelmap_skeleton(_device_stack(seg, "skeleton_maps"), n, rounds=int(options.max_iterations))
    if seg.dim() == 2:
        out, status = out[0], status[0]
    return (out, status) if return_status else out


def skeleton_from_sums(rows: torch.Tensor, area: torch.Tensor | None = None) -> dict:
    """(..., N, 8) int64 rows of `ops.labelmap_skeleton_stats` -> a dict of (..., N) tensors: "skeleton_pixels", "tips",
    "junction_pixels", "isolated_pixels" (int64) and in float64, NaN for an id without a skeleton pixel,
    "skeleton_length" = orthogonal links + sqrt(2) diagonal links, "mean_width" = 2 sqrt(sum d2 / pixels) - 1 and
    "max_width" = 2 sqrt(max d2) - 1; with `area` (..., N) "length_per_area" = skeleton_length / area.  Pure torch; works
    on either device."""
    f64 = torch.float64
    px = rows[..., 0]
    some = px > 0
    nan = torch.full(px.shape, float("nan"), dtype=f64, device=rows.device)
    length = rows[..., 1].to(f64) + SQRT2 * rows[..., 2].to(f64)
    out = {"skeleton_pixels": px, "tips": rows[..., 3], "junction_pixels": rows[..., 4], "isolated_pixels": rows[..., 5],
           "skeleton_length": torch.where(some, length, nan),
           "mean_width": torch.where(some, 2.0 * torch.sqrt(rows[..., 6].to(f64) / px.to(f64)) - 1.0, nan),
           "max_width": torch.where(some, 2.0 * torch.sqrt(rows[..., 7].to(f64)) - 1.0, nan)}
    if area is not None:
        a = area.to(f64)
        out["length_per_area"] = torch.where(some & (area > 0), length / a, nan)
    return out


def skeleton_rows(maps: torch.Tensor, N: int, options: SkeletonOptions, ids: torch.Tensor | None = None,
                  n_ids: torch.Tensor | None = None, rows: int | None = None):
    """(B, H, W) device id maps whose instances are the ids 0 .. N-1 -> (skel, status, sums, area): the thinning, the
    distance map when `options.widths`, the skeleton sums and the areas, for the ids 0 .. N-1 or the `rows` listed ids.
    Nothing is copied to the host."""
    skel, status = ops.labelmap_skeleton(maps, int(N), rounds=int(options.max_iterations))
    d2 = ops.labelmap_distance(maps, options.border == "outside") if options.widths else None
    R = int(N) if ids is None else int(rows)
    sums = ops.labelmap_skeleton_stats(skel, ids, n_ids, N=R, d2=d2)
    area = ops.labelmap_instance_stats(maps, ids, n_ids, N=R)[..., 0]
    return skel, status, sums, area


def skeleton_statistics(segmentation, n: int | None = None, ids=None, options: SkeletonOptions | None = None) -> dict:
    """The skeleton traits of every instance of one (H, W) id map or a (B, H, W) stack (maps, `n` and `ids` as for
    `instance_statistics`; listed ids must be below 4096).

    Returns a dict of device tensors, each (..., N) in the caller's order of ids: "skeleton_pixels", "tips" (skeleton
    ends) and "junction_pixels" (int64); "skeleton_length" (orthogonal links + sqrt(2) diagonal links), with
    `options.widths` "mean_width" and "max_width" (2 sqrt(d2) - 1 from the root-mean-square and the largest interior
    distance along the skeleton), "length_per_area" (float64); and "settled" (bool): the image's thinning reached its
    fixed point within `options.max_iterations`.  An id without a pixel has 0 counts and NaN traits.  Spurs are not
    pruned: the tips of a ragged mask are raw counts."""
    if (n is None) == (ids is None):
        raise ValueError("skeleton_statistics: give either n (ids 0 .. n-1) or ids")
    options = _options(options, "skeleton_statistics")
    seg = _id_maps(segmentation, "skeleton_statistics")
    order, back = None, None
    if ids is not None:
        raw = [int(v) for v in ids]
        order = sorted(set(raw))
        if len(order) != len(raw):
            raise ValueError("skeleton_statistics: ids must be distinct")
        if order and not 0 <= order[0] <= order[-1] < ops.skeleton.MAX_IDS:
            raise ValueError(f"skeleton_statistics: ids must be in [0, {ops.skeleton.MAX_IDS})")
        back = [order.index(v) for v in raw]
    elif not 0 <= int(n) <= ops.skeleton.MAX_IDS:
        raise ValueError(f"skeleton_statistics: n must be in [0, {ops.skeleton.MAX_IDS}], got {n}")
    maps = _device_stack(seg, "skeleton_statistics")
    B, dev = maps.shape[0], maps.device
    if ids is None:
        _, status, sums, area = skeleton_rows(maps, int(n), options)
    else:
        R = max(1, len(order))
        ids_t = torch.tensor(order + [0] * (R - len(order)), dtype=torch.int32).expand(B, R).contiguous().to(dev)
        n_ids = torch.full((B,), len(order), dtype=torch.int32).to(dev)
        _, status, sums, area = skeleton_rows(maps, order[-1] + 1 if order else 0, options, ids_t, n_ids, rows=R)
        sel = torch.tensor(back, dtype=torch.int64).to(dev)  # the caller's order
        sums, area = sums[:, sel], area[:, sel]
    out = skeleton_from_sums(sums, area)
    del out["isolated_pixels"]
    if not options.widths:
        del out["mean_width"], out["max_width"]
    out["settled"] = (status[:, 2:3] == 0).expand(sums.shape[:2])
    return {k: v[0] for k, v in out.items()} if seg.dim() == 2 else out


def annotate_skeletons(result, options: SkeletonOptions | None = None):
    """One result of `post_process_instance_segmentation`, `merge_tile_results` or `segment_tiled` (a dict with the
    (H, W) id map as `segmentation`, on the host or the device, and `segments_info`), or a list of them -> a new dict
    (list) whose `segments_info` entries carry SKELETON_TRAITS: ints for the counts, floats (NaN for a segment without a
    pixel) for the rest, `settled` a bool; without `options.widths` the two widths are left out.  One host copy per
    result; the input is not modified.  Warns once when an image did not settle within `options.max_iterations`."""
    options = _options(options, "annotate_skeletons")
    if isinstance(result, (list, tuple)):
        done = [_annotate(r, options) for r in result]
        unsettled = [i for i, (_, ok) in enumerate(done) if not ok]
        out = [r for r, _ in done]
    else:
        out, ok = _annotate(result, options)
        unsettled = [] if ok else [0]
    if unsettled:
        warnings.warn(f"annotate_skeletons: {len(unsettled)} image(s) did not settle within {options.max_iterations} "
                      "iterations; their traits are those of that many iterations (raise SkeletonOptions.max_iterations)",
                      RuntimeWarning, stacklevel=2)
    return out


def _annotate(result, options: SkeletonOptions):
    if not isinstance(result, dict) or "segmentation" not in result or "segments_info" not in result:
        raise ValueError("annotate_skeletons: result must be a dict with 'segmentation' and 'segments_info'")
    seg = _id_maps(result["segmentation"], "annotate_skeletons")
    if seg.dim() != 2:
        raise ValueError(f"annotate_skeletons: the segmentation must be (H, W), got {tuple(seg.shape)}")
    wanted = [int(s["id"]) for s in result["segments_info"]]
    if any(i < 0 for i in wanted) or len(set(wanted)) != len(wanted):
        raise ValueError("annotate_skeletons: segment ids must be distinct and not negative")
    out = dict(result)
    if not wanted:
        out["segments_info"] = []
        return out, True
    traits = skeleton_statistics(seg, ids=wanted, options=options)
    names = [k for k in SKELETON_TRAITS if k in traits]
    host = torch.stack([traits[k].to(torch.float64) for k in names], -1).cpu().numpy()  # the one host copy
    infos = []
    for info, row in zip(result["segments_info"], host):
        extra = {}
        for k, v in zip(names, row):
            extra[k] = bool(v) if k == "settled" else (int(v) if k in _INTEGER_TRAITS else float(v))
        infos.append({**info, **extra})
    out["segments_info"] = infos
    return out, bool(host[0, names.index("settled")])
