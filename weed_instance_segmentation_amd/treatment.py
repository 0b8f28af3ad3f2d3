"""Treatment maps on the GPU: from a segmentation result to the grid of cells a spot sprayer opens.

    from weed_instance_segmentation_amd import TreatmentOptions, treatment_grid, save_treatment_grid
    grid = treatment_grid(result, TreatmentOptions(cell=(32, 32), margin=8, protect=12, target_labels=[1], protect_labels=[0]))
    save_treatment_grid("field_0001.json", grid, transform=(0.002, 0, 431200.0, 0, -0.002, 5032110.0))

`result` is what the post-processor, `merge_tile_results` or `segment_tiled` return: `segmentation` (an id map with -1
background, ids 0 .. n-1) and `segments_info` with `id` and `label_id`.  The target instances are grown by `margin`
(`grow_label_maps`: Euclidean, never into another plant), every pixel's distance to the protected instances is measured
within `protect` (`nearest_instance_maps`), and the grown target pixels are counted per cell -- kept, or vetoed where they
lie within `protect` of a protected plant (`ops.labelmap_cell_counts`).  A cell is on when it keeps at least `min_pixels`.
Two launches of csrc/nearest.hip per distance map and one for the counts; the maps stay on the device, only the
per-cell and per-instance tables are copied to the host.
"""
from __future__ import annotations

import dataclasses
import json
import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib, ops
from .instances import _id_maps, nearest_rows, squared_cap
from .rows import ZONES, row_zone

FORMAT = "wm2f-treatment-grid"
VERSION = 1


def _pair(v, name: str, low: int):
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError(f"TreatmentOptions: {name} must be a pair (y, x), got {v!r}") from None
    for x in (a, b):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < low:
            raise ValueError(f"TreatmentOptions: {name} must be two integers >= {low}, got {v!r}")
    return int(a), int(b)


def _labels(v, name: str):
    if v is None:
        return None
    try:
        out = tuple(v)
    except TypeError:
        raise ValueError(f"TreatmentOptions: {name} must be an iterable of label ids, got {v!r}") from None
    for x in out:
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise ValueError(f"TreatmentOptions: {name} must hold integer label ids, got {x!r}")
    return tuple(int(x) for x in out)


@dataclasses.dataclass(frozen=True)
class TreatmentOptions:
    """What `treatment_grid` does.

    - `cell` = (h, w): the size of a cell of the sprayer's grid in pixels; `offset` = (off_y, off_x) with 0 <= off < cell
      shifts the grid: pixel (x, y) lies in cell ((y + off_y) // h, (x + off_x) // w).
    - `margin` in [0, 1024] pixels: the target instances are grown by it before they are counted (localisation and
      latency are never pixel-exact).
    - `protect` in [0, 1024] pixels: a grown target pixel within this distance of a protected instance is vetoed -- it
      does not count towards switching its cell on.
    - `target_labels`: the `label_id`s that are treated; None: every label that is not protected.
    - `protect_labels`: the `label_id`s that are protected (the crop).
    - `min_pixels` >= 1: a cell is on when it keeps at least this many target pixels."""
    cell: tuple = (32, 32)
    offset: tuple = (0, 0)
    margin: float = 0.0
    protect: float = 0.0
    target_labels: tuple | None = None
    protect_labels: tuple = ()
    min_pixels: int = 1

    def __post_init__(self):
        object.__setattr__(self, "cell", _pair(self.cell, "cell", 1))
        object.__setattr__(self, "offset", _pair(self.offset, "offset", 0))
        if self.cell[0] > 16384 or self.cell[1] > 16384:
            raise ValueError(f"TreatmentOptions: a cell is at most 16384 pixels a side, got {self.cell!r}")
        if not (self.offset[0] < self.cell[0] and self.offset[1] < self.cell[1]):
            raise ValueError(f"TreatmentOptions: offset must be below cell, got {self.offset!r} for {self.cell!r}")
        for name in ("margin", "protect"):
            squared_cap(getattr(self, name), f"TreatmentOptions: {name}")
        object.__setattr__(self, "target_labels", _labels(self.target_labels, "target_labels"))
        protect = _labels(self.protect_labels, "protect_labels")
        if protect is None:
            raise ValueError("TreatmentOptions: protect_labels must be an iterable (empty for none)")
        object.__setattr__(self, "protect_labels", protect)
        if self.target_labels is not None and set(self.target_labels) & set(protect):
            raise ValueError(f"TreatmentOptions: a label cannot be both treated and protected: "
                             f"{sorted(set(self.target_labels) & set(protect))}")
        if isinstance(self.min_pixels, bool) or not isinstance(self.min_pixels, (int, np.integer)) or self.min_pixels < 1:
            raise ValueError(f"TreatmentOptions: min_pixels must be an integer >= 1, got {self.min_pixels!r}")

    def is_target(self, label_id: int) -> bool:
        if self.target_labels is None:
            return int(label_id) not in self.protect_labels
        return int(label_id) in self.target_labels

    def is_protected(self, label_id: int) -> bool:
        return int(label_id) in self.protect_labels


def on_cell_area(cells, H: int, W: int, cell, offset) -> int:
    """The pixels of an (H, W) image that lie in the on-cells of the host bool grid `cells`."""
    ys = (np.arange(H) + offset[0]) // cell[0]
    xs = (np.arange(W) + offset[1]) // cell[1]
    rows = np.bincount(ys, minlength=cells.shape[0])  # pixel rows per row of cells, clipped to the image
    cols = np.bincount(xs, minlength=cells.shape[1])
    return int((np.asarray(cells, np.int64) * rows[:, None] * cols[None, :]).sum())


def treatment_grid(result: dict, options: TreatmentOptions, rows: dict | None = None, zone: str | None = None) -> dict:
    """The sprayer grid of one segmentation result (see the module's text).  `result["segmentation"]` is an (H, W) id
    map, host or device, whose instances are the `id`s of `result["segments_info"]`; an id of the map that has no entry
    is a plant of no class: it keeps its pixels and is neither treated nor protected.

    Returns a dict: `cells` (GH, GW) bool, `coverage` and `vetoed` (GH, GW) int32 -- the grown target pixels a cell
    keeps, and those the protection zone took away -- `treated_fraction` (the on-cells' area inside the image over H * W,
    a float) and `treated_fraction_exact` (the same as a Fraction), `instances` (per target instance `id`, `label_id`,
    `treated`: the fraction of its own pixels that lie in on-cells, and `vetoed_fraction`: the fraction within the
    protection distance; NaN for an instance without a pixel), and the geometry: `cell`, `offset`, `image_size` (H, W),
    `grid_size` (GH, GW).  The arrays are host numpy arrays.

    `zone` restricts the treatment to one side of the crop rows `rows` (`crop_rows` of the same result, DESIGN section
    41): "inter_row" keeps a grown target pixel only outside the row bands (a hoe between the rows), "intra_row" only
    inside them (an in-row tool).  The grown map is masked before the cells are counted; `treated` keeps its meaning.
    With `zone` None nothing changes, whatever `rows` is."""
    if not isinstance(options, TreatmentOptions):
        raise TypeError(f"treatment_grid: options must be a TreatmentOptions, got {type(options).__name__}")
    if zone is not None:
        if zone not in ZONES:
            raise ValueError(f"treatment_grid: zone must be one of {ZONES} or None, got {zone!r}")
        if not isinstance(rows, dict) or not rows.get("found"):
            raise ValueError("treatment_grid: zone needs rows that were found (crop_rows(...)['found'] is True)")
    if not isinstance(result, dict) or "segmentation" not in result or "segments_info" not in result:
        raise ValueError("treatment_grid: result must be a dict with 'segmentation' and 'segments_info'")
    seg = _id_maps(result["segmentation"], "treatment_grid")
    if seg.dim() != 2:
        raise ValueError(f"treatment_grid: the segmentation must be (H, W), got {tuple(seg.shape)}")
    infos = [(int(s["id"]), int(s["label_id"])) for s in result["segments_info"]]
    if any(i < 0 for i, _ in infos) or len(set(i for i, _ in infos)) != len(infos):
        raise ValueError("treatment_grid: segment ids must be distinct and not negative")
    n = max((i for i, _ in infos), default=-1) + 1
    if n > 4096:
        raise ValueError(f"treatment_grid: at most 4096 instances, got ids up to {n - 1}")
    target = np.zeros(max(n, 1), np.bool_)
    protected = np.zeros(max(n, 1), np.bool_)
    for i, label in infos:
        target[i] = options.is_target(label)
        protected[i] = options.is_protected(label)
    if not torch.cuda.is_available():
        raise _lib.Wm2fError("treatment_grid runs on a GPU only (no CPU fallback): no device is visible")
    dev = seg.device if seg.is_cuda else torch.device("cuda", torch.cuda.current_device())
    maps = seg.to(dev).unsqueeze(0)
    H, W = int(seg.shape[0]), int(seg.shape[1])
    N = max(n, 1)

    grown, _ = nearest_rows(maps, N, squared_cap(options.margin, "treatment_grid"), target[:N], True)
    veto_d2, veto_max = None, squared_cap(options.protect, "treatment_grid")
    if protected.any():
        _, veto_d2 = nearest_rows(maps, N, veto_max, protected[:N], False)
    if zone is not None:
        in_band = row_zone(maps, rows) != 0
        grown = torch.where((in_band if zone == "intra_row" else ~in_band).unsqueeze(0), grown, torch.full_like(grown, -1))
    group = torch.from_numpy(np.where(target, 0, 255).astype(np.uint8)).to(dev).unsqueeze(0)
    counts = ops.labelmap_cell_counts(grown, group, 1, options.cell, options.offset, veto_d2, veto_max)[0]
    cells_dev = counts[..., 0] >= int(options.min_pixels)

    # per instance: its own pixels that lie in on-cells, and those within the protection distance, over its area
    cy = (torch.arange(H, device=dev) + options.offset[0]) // options.cell[0]
    cx = (torch.arange(W, device=dev) + options.offset[1]) // options.cell[1]
    own = maps[0].to(torch.int32) if maps.dtype == torch.uint8 else maps[0]
    minus = torch.full_like(own, -1)
    stack = [own, torch.where(cells_dev[cy][:, cx], own, minus)]
    if veto_d2 is not None:
        stack.append(torch.where(veto_d2[0] <= veto_max, own, minus))
    area = ops.labelmap_instance_stats(torch.stack(stack).contiguous(), N=N)[..., 0].cpu().numpy()
    counts_h = counts.cpu().numpy()

    cells = counts_h[..., 0] >= int(options.min_pixels)
    exact = Fraction(on_cell_area(cells, H, W, options.cell, options.offset), H * W)
    rows = []
    for i, label in infos:
        if not target[i]:
            continue
        a = int(area[0, i])
        rows.append({"id": i, "label_id": label,
                     "treated": int(area[1, i]) / a if a else float("nan"),
                     "vetoed_fraction": (int(area[2, i]) / a if veto_d2 is not None else 0.0) if a else float("nan")})
    return {"cells": cells, "coverage": counts_h[..., 0].copy(), "vetoed": counts_h[..., 1].copy(),
            "treated_fraction": float(exact), "treated_fraction_exact": exact, "instances": rows,
            "cell": tuple(options.cell), "offset": tuple(options.offset), "image_size": (H, W),
            "grid_size": (int(cells.shape[0]), int(cells.shape[1]))}


def save_treatment_grid(path, grid: dict, transform=None) -> None:
    """Write a `treatment_grid` as JSON: the cell size, the offset, the image size, the on-cells as rows of 0 / 1, the
    treated fraction, the per-instance table and, passed through as given, `transform`: the six numbers (a, b, c, d, e, f)
    of the pixel -> world affine X = a x + b y + c, Y = d x + e y + f."""
    if transform is not None:
        transform = [float(v) for v in transform]
        if len(transform) != 6 or not all(math.isfinite(v) for v in transform):
            raise ValueError(f"save_treatment_grid: transform must be six finite numbers, got {transform!r}")
    exact = grid["treated_fraction_exact"]
    doc = {"format": FORMAT, "version": VERSION,
           "cell": [int(v) for v in grid["cell"]], "offset": [int(v) for v in grid["offset"]],
           "image_size": [int(v) for v in grid["image_size"]], "grid_size": [int(v) for v in grid["grid_size"]],
           "cells": [[int(v) for v in row] for row in np.asarray(grid["cells"])],
           "treated_fraction": [int(exact.numerator), int(exact.denominator)],
           "instances": [{"id": int(r["id"]), "label_id": int(r["label_id"]),
                          "treated": None if math.isnan(r["treated"]) else float(r["treated"]),
                          "vetoed_fraction": None if math.isnan(r["vetoed_fraction"]) else float(r["vetoed_fraction"])}
                         for r in grid["instances"]],
           "transform": transform}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def load_treatment_grid(path) -> dict:
    """Read a file of `save_treatment_grid` back: the keys of `treatment_grid` that the file holds (no `coverage`, no
    `vetoed`), plus `transform` (a tuple of six floats, or None)."""
    with open(path) as f:
        doc = json.load(f)
    if doc.get("format") != FORMAT or doc.get("version") != VERSION:
        raise ValueError(f"load_treatment_grid: {path} is not a version {VERSION} {FORMAT} file")
    cells = np.asarray(doc["cells"], np.bool_).reshape(tuple(doc["grid_size"]))
    exact = Fraction(int(doc["treated_fraction"][0]), int(doc["treated_fraction"][1]))
    nan = float("nan")
    rows = [{"id": int(r["id"]), "label_id": int(r["label_id"]),
             "treated": nan if r["treated"] is None else float(r["treated"]),
             "vetoed_fraction": nan if r["vetoed_fraction"] is None else float(r["vetoed_fraction"])}
            for r in doc["instances"]]
    return {"cells": cells, "treated_fraction": float(exact), "treated_fraction_exact": exact, "instances": rows,
            "cell": tuple(doc["cell"]), "offset": tuple(doc["offset"]), "image_size": tuple(doc["image_size"]),
            "grid_size": tuple(doc["grid_size"]),
            "transform": None if doc["transform"] is None else tuple(float(v) for v in doc["transform"])}
