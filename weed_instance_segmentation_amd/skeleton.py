"""Plant skeletons on the GPU (DESIGN sections 44 and 46): the thinned id map of a segmentation result and, per plant,
the length of its skeleton, the number of its ends and junctions and the width of its parts; the pruning of the spurs
that a ragged mask boundary grows, and the skeleton as a graph of branches and node clusters.

    from weed_instance_segmentation_amd import SkeletonOptions, skeleton_maps, skeleton_statistics, annotate_skeletons
    skel = skeleton_maps(prediction["segmentation"], n)                       # an id map again, -1 off the skeletons
    traits = skeleton_statistics(prediction["segmentation"], n=n)
    traits["skeleton_length"], traits["tips"], traits["mean_width"]
    result = annotate_skeletons(result)                                       # the traits on every segments_info entry
    pruned = SkeletonOptions(prune=PruneOptions())                            # the same three on the pruned skeleton
    graph = skeleton_graph_statistics(prediction["segmentation"], n=n)        # + branches, end_branches, nodes, ...
    graph["tips"]                                                             # the leaf count of a ragged mask

Guo and Hall's two-sub-iteration parallel thinning runs on every instance at once in a fixed chain of launches of
csrc/skeleton.hip (tiles held in LDS for several iterations); a second kernel sums the skeleton per instance, and the
widths come from `distance_maps` of the original map.  The integers are exact; the float traits are a few float64
operations on them (`skeleton_from_sums`).  A long narrow plant with few ends is a grass weed, a plant of the same area
with many ends a broadleaf; the tips are a leaf-count proxy.  The tips of a raw skeleton count every bump of the mask's
boundary; with `SkeletonOptions.prune` the spurs -- end branches no longer than `ratio` half-widths of the part they grow
out of -- are deleted on the device first (csrc/skeleton_graph.hip), and the tips of the pruned skeleton are the leaves.

Not done here: the skeleton is not traced into ordered polylines; there is no medial-axis transform by distance ridges;
the pruning defaults (`ratio` 1.0, `min_pixels` 2) were chosen on synthetic masks and have not been measured on real
predictions.
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
# what it adds with `SkeletonOptions.prune`, and what `skeleton_graph_statistics` adds to `skeleton_statistics`
SKELETON_GRAPH_TRAITS = ("branches", "end_branches", "nodes", "longest_end_branch", "longest_branch", "closed_branches",
                         "pruned_pixels", "prune_settled")
_INTEGER_TRAITS = ("skeleton_pixels", "tips", "junction_pixels") + SKELETON_GRAPH_TRAITS[:7]
_BOOL_TRAITS = ("settled", "prune_settled")
_GRAPH_COLUMNS = {"branches": 0, "end_branches": 1, "nodes": 2, "longest_end_branch": 5, "longest_branch": 6,
                  "closed_branches": 7}


def _integer(v, lo: int, hi: int, what: str) -> None:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}], got {v!r}")


@dataclasses.dataclass(frozen=True)
class PruneOptions:
    """How spurs are pruned from a skeleton.

    - `min_pixels` in [0, 2^20]: an end branch of at most this many pixels is a spur.
    - `ratio` in [0, 64]: an end branch no longer (in pixels) than `ratio` times the half-width of the part it grows out
      of is a spur; the kernel takes it in sixteenths (`ratio_q` = round(16 ratio)).
    - `max_rounds` in [1, 64]: the rounds of delete-then-rethin; ragged masks settle in two or three.
    - `rethin` in [1, 16]: the thinning iterations after every round's deletions.
    The defaults were chosen on synthetic plants; nobody has measured them on real predictions."""
    min_pixels: int = 2
    ratio: float = 1.0
    max_rounds: int = 8
    rethin: int = 4

    def __post_init__(self):
        _integer(self.min_pixels, 0, ops.skeleton.MAX_MIN_PIXELS, "PruneOptions: min_pixels")
        r = self.ratio
        if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, float, np.integer, np.floating)) or not 0 <= r <= 64:
            raise ValueError(f"PruneOptions: ratio must be a number in [0, 64], got {r!r}")  # NaN fails the comparison
        _integer(self.max_rounds, 1, ops.skeleton.MAX_PRUNE_ROUNDS, "PruneOptions: max_rounds")
        _integer(self.rethin, 1, ops.skeleton.MAX_RETHIN, "PruneOptions: rethin")

    @property
    def ratio_q(self) -> int:
        return int(round(16.0 * float(self.ratio)))


@dataclasses.dataclass(frozen=True)
class SkeletonOptions:
    """How `skeleton_maps`, `skeleton_statistics` and `annotate_skeletons` thin.

    - `max_iterations` in [1, 1024]: the thinning iterations.  A solid part settles in about its half-width + 1; a map
      that has not settled is reported (`settled`, `status`) and is still the defined result of that many iterations.
    - `border`: the border mode of the distance map behind the widths, "outside" or "inside" (`distance_maps`).
    - `widths`: compute `mean_width` and `max_width` (one more `labelmap_distance` of the original map).
    - `prune`: a `PruneOptions` prunes the spurs of the thinned map first, and the three work on the pruned skeleton
      (`annotate_skeletons` then also writes SKELETON_GRAPH_TRAITS); None: the raw skeleton."""
    max_iterations: int = 64
    border: str = "outside"
    widths: bool = True
    prune: PruneOptions | None = None

    def __post_init__(self):
        r = self.max_iterations
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= r <= ops.skeleton.MAX_ROUNDS:
            raise ValueError(f"SkeletonOptions: max_iterations must be an integer in [1, {ops.skeleton.MAX_ROUNDS}], got {r!r}")
        _border_outside(self.border, "SkeletonOptions")
        if not isinstance(self.widths, (bool, np.bool_)):
            raise ValueError(f"SkeletonOptions: widths must be a bool, got {self.widths!r}")
        if self.prune is not None and not isinstance(self.prune, PruneOptions):
            raise ValueError(f"SkeletonOptions: prune must be a PruneOptions or None, got {self.prune!r}")


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
    non-zero third entry says `max_iterations` was too small.  With `options.prune` the map is the pruned skeleton; the
    status is still the thinning's (`prune_skeleton_maps` returns the pruning's)."""
    options = _options(options, "skeleton_maps")
    seg = _id_maps(maps, "skeleton_maps")
    n = int(n)
    if not 0 <= n <= ops.skeleton.MAX_IDS:
        raise ValueError(f"skeleton_maps: n must be in [0, {ops.skeleton.MAX_IDS}], got {n}")
    stack = _device_stack(seg, "skeleton_maps")
    out, status = ops.labelmap_skeleton(stack, n, rounds=int(options.max_iterations))
    if options.prune is not None:
        out, _ = _prune(out, ops.labelmap_distance(stack, options.border == "outside"), n, options.prune)
    if seg.dim() == 2:
        out, status = out[0], status[0]
    return (out, status) if return_status else out


def _prune(skel: torch.Tensor, d2: torch.Tensor, N: int, prune: PruneOptions):
    return ops.labelmap_skeleton_prune(skel, d2, int(N), min_pixels=int(prune.min_pixels), ratio_q=prune.ratio_q,
                                       rounds=int(prune.max_rounds), rethin=int(prune.rethin))


def _prune_options(options, who: str) -> PruneOptions:
    if options is None:
        return PruneOptions()
    if not isinstance(options, PruneOptions):
        raise TypeError(f"{who}: options must be a PruneOptions, got {type(options).__name__}")
    return options


def _skeleton_stack(skeletons, who: str) -> torch.Tensor:
    skel = torch.from_numpy(np.ascontiguousarray(skeletons)) if isinstance(skeletons, np.ndarray) else skeletons
    if not isinstance(skel, torch.Tensor) or skel.dtype != torch.int32 or skel.dim() not in (2, 3):
        raise TypeError(f"{who}: skeletons must be an int32 (H, W) or (B, H, W) map (what skeleton_maps returns)")
    return skel


def prune_skeleton_maps(skeletons, maps, n: int, options: PruneOptions | None = None, *, border: str = "outside",
                        return_status: bool = False):
    """Prune the spurs of skeleton maps (`skeleton_maps`' int32 output, (H, W) or (B, H, W)) of the id maps `maps` they
    were thinned from (as for `skeleton_maps`; their interior distance is the half-width a branch is compared with;
    `border` as for `distance_maps`).  Returns the pruned skeleton, an int32 device tensor of the input's shape;
    `return_status=True` returns (map, status): status (..., 4) int32 [pixels left, rounds that removed something,
    pixels removed in the last round, pixels removed in all]; a non-zero third entry says `max_rounds` was too few."""
    options = _prune_options(options, "prune_skeleton_maps")
    outside = _border_outside(border, "prune_skeleton_maps")
    skel = _skeleton_stack(skeletons, "prune_skeleton_maps")
    seg = _id_maps(maps, "prune_skeleton_maps")
    if seg.shape != skel.shape:
        raise ValueError(f"prune_skeleton_maps: skeletons and maps must agree, got {tuple(skel.shape)} and {tuple(seg.shape)}")
    n = int(n)
    if not 0 <= n <= ops.skeleton.MAX_IDS:
        raise ValueError(f"prune_skeleton_maps: n must be in [0, {ops.skeleton.MAX_IDS}], got {n}")
    stack = _device_stack(seg, "prune_skeleton_maps")
    sk = skel.to(stack.device)
    out, status = _prune(sk.unsqueeze(0) if sk.dim() == 2 else sk, ops.labelmap_distance(stack, outside), n, options)
    if seg.dim() == 2:
        out, status = out[0], status[0]
    return (out, status) if return_status else out


def skeleton_branch_maps(skeletons, n: int) -> torch.Tensor:
    """The branches and node clusters of skeleton maps ((H, W) or (B, H, W) int32, ids 0 .. n-1): an int32 device tensor
    of the input's shape, -1 off the skeleton, at a path pixel (at most two same-id neighbours) the label of its branch,
    at a node pixel -2 - the label of its node cluster; a label is the smallest linear index y W + x of the component."""
    skel = _skeleton_stack(skeletons, "skeleton_branch_maps")
    n = int(n)
    if not 0 <= n <= ops.skeleton.MAX_IDS:
        raise ValueError(f"skeleton_branch_maps: n must be in [0, {ops.skeleton.MAX_IDS}], got {n}")
    stack = _device_stack(skel, "skeleton_branch_maps")
    labels, _ = ops.labelmap_skeleton_graph(stack, N=n)
    return labels[0] if skel.dim() == 2 else labels


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
    With `options.prune` the skeleton is pruned before it is summed.  Nothing is copied to the host."""
    return _rows(maps, N, options, ids, n_ids, rows, False)[:4]


def _rows(maps, N, options, ids, n_ids, rows, graph: bool):
    """`skeleton_rows` and, behind its four, the pruning's status (None without `options.prune`) and with `graph` the
    (B, rows, 8) sums of `ops.labelmap_skeleton_graph` (None without)."""
    skel, status = ops.labelmap_skeleton(maps, int(N), rounds=int(options.max_iterations))
    d2 = ops.labelmap_distance(maps, options.border == "outside") if options.widths or options.prune is not None else None
    pruned = None
    if options.prune is not None:
        skel, pruned = _prune(skel, d2, N, options.prune)
    R = int(N) if ids is None else int(rows)
    sums = ops.labelmap_skeleton_stats(skel, ids, n_ids, N=R, d2=d2 if options.widths else None)
    area = ops.labelmap_instance_stats(maps, ids, n_ids, N=R)[..., 0]
    gsums = ops.labelmap_skeleton_graph(skel, ids, n_ids, N=R)[1] if graph else None
    return skel, status, sums, area, pruned, gsums


def skeleton_statistics(segmentation, n: int | None = None, ids=None, options: SkeletonOptions | None = None) -> dict:
    """The skeleton traits of every instance of one (H, W) id map or a (B, H, W) stack (maps, `n` and `ids` as for
    `instance_statistics`; listed ids must be below 4096).

    Returns a dict of device tensors, each (..., N) in the caller's order of ids: "skeleton_pixels", "tips" (skeleton
    ends) and "junction_pixels" (int64); "skeleton_length" (orthogonal links + sqrt(2) diagonal links), with
    `options.widths` "mean_width" and "max_width" (2 sqrt(d2) - 1 from the root-mean-square and the largest interior
    distance along the skeleton), "length_per_area" (float64); and "settled" (bool): the image's thinning reached its
    fixed point within `options.max_iterations`.  An id without a pixel has 0 counts and NaN traits.  Without
    `options.prune` the tips of a ragged mask are raw counts; with it everything is computed on the pruned skeleton."""
    return _statistics(segmentation, n, ids, _options(options, "skeleton_statistics"), "skeleton_statistics", False)


def skeleton_graph_statistics(segmentation, n: int | None = None, ids=None, options: SkeletonOptions | None = None) -> dict:
    """Everything `skeleton_statistics` returns, computed on the PRUNED skeleton (`options.prune`, or `PruneOptions()`
    when that is None), and the skeleton as a graph, each (..., N): "branches", "end_branches" (branches with a free end
    that hang on a node cluster: the leaves of a plant with a junction), "nodes" (node clusters), "longest_end_branch"
    and "longest_branch" (pixels), "closed_branches" (rings), "pruned_pixels" (what the pruning removed from the
    image's skeletons) (int64) and "prune_settled" (bool): the image's pruning reached its fixed point within
    `max_rounds`."""
    options = _options(options, "skeleton_graph_statistics")
    if options.prune is None:
        options = dataclasses.replace(options, prune=PruneOptions())
    return _statistics(segmentation, n, ids, options, "skeleton_graph_statistics", True)


def _statistics(segmentation, n, ids, options: SkeletonOptions, who: str, graph: bool) -> dict:
    if (n is None) == (ids is None):
        raise ValueError(f"{who}: give either n (ids 0 .. n-1) or ids")
    seg = _id_maps(segmentation, who)
    order, back = None, None
    if ids is not None:
        raw = [int(v) for v in ids]
        order = sorted(set(raw))
        if len(order) != len(raw):
            raise ValueError(f"{who}: ids must be distinct")
        if order and not 0 <= order[0] <= order[-1] < ops.skeleton.MAX_IDS:
            raise ValueError(f"{who}: ids must be in [0, {ops.skeleton.MAX_IDS})")
        back = [order.index(v) for v in raw]
    elif not 0 <= int(n) <= ops.skeleton.MAX_IDS:
        raise ValueError(f"{who}: n must be in [0, {ops.skeleton.MAX_IDS}], got {n}")
    maps = _device_stack(seg, who)
    B, dev = maps.shape[0], maps.device
    if ids is None:
        _, status, sums, area, pruned, gsums = _rows(maps, int(n), options, None, None, None, graph)
    else:
        R = max(1, len(order))
        ids_t = torch.tensor(order + [0] * (R - len(order)), dtype=torch.int32).expand(B, R).contiguous().to(dev)
        n_ids = torch.full((B,), len(order), dtype=torch.int32).to(dev)
        _, status, sums, area, pruned, gsums = _rows(maps, order[-1] + 1 if order else 0, options, ids_t, n_ids, R, graph)
        sel = torch.tensor(back, dtype=torch.int64).to(dev)  # the caller's order
        sums, area = sums[:, sel], area[:, sel]
        gsums = gsums[:, sel] if graph else None
    out = skeleton_from_sums(sums, area)
    del out["isolated_pixels"]
    if not options.widths:
        del out["mean_width"], out["max_width"]
    out["settled"] = (status[:, 2:3] == 0).expand(sums.shape[:2])
    if graph:
        for k, col in _GRAPH_COLUMNS.items():
            out[k] = gsums[..., col]
        out["pruned_pixels"] = pruned[:, 3:4].to(torch.int64).expand(sums.shape[:2])
        out["prune_settled"] = (pruned[:, 2:3] == 0).expand(sums.shape[:2])
    return {k: v[0] for k, v in out.items()} if seg.dim() == 2 else out


def annotate_skeletons(result, options: SkeletonOptions | None = None):
    """One result of `post_process_instance_segmentation`, `merge_tile_results` or `segment_tiled` (a dict with the
    (H, W) id map as `segmentation`, on the host or the device, and `segments_info`), or a list of them -> a new dict
    (list) whose `segments_info` entries carry SKELETON_TRAITS: ints for the counts, floats (NaN for a segment without a
    pixel) for the rest, `settled` a bool; without `options.widths` the two widths are left out.  One host copy per
    result; the input is not modified.  Warns once when an image did not settle within `options.max_iterations`.  With
    `options.prune` the traits are those of the pruned skeleton and the entries also carry SKELETON_GRAPH_TRAITS."""
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
    traits = _statistics(seg, None, wanted, options, "annotate_skeletons", options.prune is not None)
    names = [k for k in SKELETON_TRAITS + SKELETON_GRAPH_TRAITS if k in traits]
    host = torch.stack([traits[k].to(torch.float64) for k in names], -1).cpu().numpy()  # the one host copy
    infos = []
    for info, row in zip(result["segments_info"], host):
        extra = {}
        for k, v in zip(names, row):
            extra[k] = bool(v) if k in _BOOL_TRAITS else (int(v) if k in _INTEGER_TRAITS else float(v))
        infos.append({**info, **extra})
    out["segments_info"] = infos
    return out, bool(host[0, names.index("settled")])
