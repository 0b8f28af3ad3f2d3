"""Tiled inference for images larger than the model's input.

    from weed_instance_segmentation_amd import segment_tiled
    result = segment_tiled(image, model, processor, tile=1024, overlap=256)      # a 6000 x 4000 field photograph
    result["segmentation"]     # (H, W) int32 on the device, -1 background
    result["segments_info"]    # one entry per plant, with the (tile, id) views it was merged from

The image is cut into overlapping tiles at native resolution, every tile goes through the processor, the model and
`post_process_instance_segmentation` as a single image would, and `merge_tile_results` decides which instances of
neighbouring tiles are the same object, gives them one id and writes one id map -- four calls into csrc/tiles.hip that
read each tile once, whatever the number of tiles, pairs and instances.  The contract of the merge is written out in
include/wm2f.h.  Two instances of one tile may end up merged when a neighbour's instance links both.

The semantic task takes the same tiles but blends class scores, not ids:

    result = segment_tiled_semantic(image, model, processor, flips=("none", "h"))
    result["segmentation"]     # (H, W) int32 class ids on the device

Every tile's (C, 384, 384) scores from `post_process_semantic_segmentation` are kept as they are; one kernel
(csrc/tile_blend.hip) samples, per output pixel, every tile that covers it, weights the samples by a feathering window and
takes the argmax.  Views computed on flipped tiles (horizontal / vertical flip test-time augmentation) are further
covering views, read at the mirrored pixel.

Not covered: rescaling before tiling (resize first), panoptic tiling, multi-scale test-time augmentation, and test-time
augmentation for the instance route.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import ops

MAX_MERGED_IDS = 4096  # what the consumers of an id map take (statistics, RLE, overlays, AP)


@dataclass(frozen=True)
class TileGrid:
    """The tiles of one image: all of size (th, tw), numbered row-major over `ys` x `xs` (their origins).  `cuts_y` /
    `cuts_x` bound the cells: output pixel (y, x) belongs to the tile whose row cell [cuts_y[r], cuts_y[r+1]) and column
    cell [cuts_x[c], cuts_x[c+1]) contain it.  `windows[t]` = (y0, x0, y1, x1); `pairs` lists every a < b whose windows
    intersect as (a, b, ay, ax, by, bx, h, w): the (h, w) intersection at (ay, ax) of tile a and (by, bx) of tile b."""
    height: int
    width: int
    th: int
    tw: int
    ys: list = field(default_factory=list)
    xs: list = field(default_factory=list)
    cuts_y: list = field(default_factory=list)
    cuts_x: list = field(default_factory=list)
    windows: list = field(default_factory=list)
    pairs: list = field(default_factory=list)

    @property
    def n_tiles(self) -> int:
        return len(self.windows)

    def owner_cell(self, t: int):
        """(cy0, cy1, cx0, cx1): the output pixels tile t owns."""
        r, c = divmod(t, len(self.xs))
        return self.cuts_y[r], self.cuts_y[r + 1], self.cuts_x[c], self.cuts_x[c + 1]

    def geom_table(self) -> np.ndarray:
        """(T, 6) int32 rows (oy, ox, cy0, cy1, cx0, cx1) of include/wm2f.h."""
        rows = [(w[0], w[1], *self.owner_cell(t)) for t, w in enumerate(self.windows)]
        return np.asarray(rows, dtype=np.int32).reshape(len(rows), 6)

    def pair_table(self) -> np.ndarray:
        """(P, 8) int32 rows (a, b, ay, ax, by, bx, h, w) of include/wm2f.h."""
        return np.asarray(self.pairs, dtype=np.int32).reshape(len(self.pairs), 8)


def _axis(L: int, tile: int, overlap: int):
    """Tile side, origins and cuts of one axis of length L."""
    t = min(tile, L)
    n = 1 if L <= tile else 1 + -(-(L - tile) // (tile - overlap))
    o = [0] if n == 1 else [(i * (L - tile)) // (n - 1) for i in range(n)]
    cuts = [0] + [(o[i] + t + o[i + 1]) // 2 for i in range(n - 1)] + [L]
    return t, o, cuts


def tile_windows(height: int, width: int, tile: int = 1024, overlap: int = 256) -> TileGrid:
    """The tiles of a (height, width) image.  Per axis of length L: side t = min(tile, L); n = 1 tiles when L <= tile,
    else 1 + ceil((L - tile) / (tile - overlap)); origins o[i] = (i * (L - tile)) // (n - 1) -- the first tile starts at
    0, the last ends at L, neighbours overlap by at least `overlap`.  The cut between two neighbours is the midpoint of
    their overlap, (o[i] + t + o[i+1]) // 2."""
    height, width, tile, overlap = int(height), int(width), int(tile), int(overlap)
    if height < 1 or width < 1:
        raise ValueError(f"tile_windows: bad image size {height} x {width}")
    if tile < 1 or not 0 <= overlap <= tile // 2:
        raise ValueError(f"tile_windows: need tile >= 1 and 0 <= overlap <= tile // 2, got tile {tile}, overlap {overlap}")
    th, ys, cuts_y = _axis(height, tile, overlap)
    tw, xs, cuts_x = _axis(width, tile, overlap)
    R, C = len(ys), len(xs)
    windows = [(y, x, y + th, x + tw) for y in ys for x in xs]
    # separable: every row / column whose extent meets r's / c's (itself included); b <= a is dropped below
    row_meets = [[r2 for r2 in range(R) if abs(ys[r2] - ys[r]) < th] for r in range(R)]
    col_meets = [[c2 for c2 in range(C) if abs(xs[c2] - xs[c]) < tw] for c in range(C)]
    pairs = []
    for a in range(R * C):
        ra, ca = divmod(a, C)
        for rb in row_meets[ra]:
            for cb in col_meets[ca]:
                b = rb * C + cb
                if b <= a:
                    continue
                y0, y1 = max(ys[ra], ys[rb]), min(ys[ra], ys[rb]) + th
                x0, x1 = max(xs[ca], xs[cb]), min(xs[ca], xs[cb]) + tw
                pairs.append((a, b, y0 - ys[ra], x0 - xs[ca], y0 - ys[rb], x0 - xs[cb], y1 - y0, x1 - x0))
    return TileGrid(height, width, th, tw, ys, xs, cuts_y, cuts_x, windows, pairs)


def merged_segments_info(remap, n_merged: int, results) -> list:
    """The host half of `merge_tile_results`: remap (T, N) integers (-1: not reported), the number of merged ids and the
    per-tile results -> one entry per merged id: `id`, `label_id` (its members share it), `score` (the maximum over
    members), `was_fused` False, `members` [(tile, id), ...] ascending."""
    n_merged = int(n_merged)
    if n_merged > MAX_MERGED_IDS:
        raise ValueError(f"merge_tile_results: {n_merged} merged instances, but an id map takes at most {MAX_MERGED_IDS} "
                         "downstream (statistics, RLE, overlays, AP): raise `threshold` or split the image")
    remap = np.asarray(remap)
    merged = [{"id": k, "label_id": None, "score": None, "was_fused": False, "members": []} for k in range(n_merged)]
    for t, res in enumerate(results):
        for info in res["segments_info"]:
            i = int(info["id"])
            k = int(remap[t, i])
            if k < 0:
                continue
            if not k < n_merged:
                raise ValueError(f"merge_tile_results: remap[{t}][{i}] = {k} with {n_merged} merged ids")
            m = merged[k]
            m["members"].append((t, i))
            if m["label_id"] is None:
                m["label_id"] = int(info["label_id"])
            m["score"] = info["score"] if m["score"] is None else max(m["score"], info["score"])
    return merged


def _tile_tables(results, T: int):
    """n_ids (T) and labels (T, N) int32 from the tiles' segments_info, whose ids must be 0 .. n-1 (the post-processor's)."""
    n_ids = np.zeros(T, dtype=np.int32)
    for t, res in enumerate(results):
        ids = [int(s["id"]) for s in res["segments_info"]]
        if ids != list(range(len(ids))):
            raise ValueError(f"merge_tile_results: tile {t}: segments_info ids must be 0 .. n-1 in order, got {ids[:8]} ...")
        n_ids[t] = len(ids)
    N = int(n_ids.max()) if T else 0
    labels = np.full((T, N), -1, dtype=np.int32)
    for t, res in enumerate(results):
        labels[t, :n_ids[t]] = [int(s["label_id"]) for s in res["segments_info"]]
    return n_ids, labels


def merge_tile_results(results, grid: TileGrid, merge_threshold=(1, 2), return_instance_stats: bool = False,
                       clean=None, return_aim_points: bool = False, split=None,
                       return_shape_stats: bool = False) -> dict:
    """Merge the per-tile results of `post_process_instance_segmentation(target_sizes=[(grid.th, grid.tw)] * T)` (tiles in
    `grid` order) into one image's result: {"segmentation": (H, W) int32 on the device with -1 background,
    "segments_info": [...]}, entries as `merged_segments_info` gives them.

    Two instances of neighbouring tiles with the same label are one object when their intersection inside the tiles'
    overlap is at least `merge_threshold` = (num, den) of the smaller of their two areas inside that overlap; links are
    transitive.  Every output pixel shows the prediction of the tile that owns it (`grid.cuts_y`, `grid.cuts_x`),
    relabelled; an instance with no pixel in any owning cell is not reported.  `return_instance_stats=True` adds "area",
    "bbox" and "centroid" of the merged map's instances, as the post-processor does.  Four kernel calls, one host-to-device
    and one device-to-host copy.

    `clean=CleanOptions(...)` repairs the composed map as the post-processor's `clean=` does -- a
    plant cut at a cell border can leave slivers that survive as pieces of the merged id: entries whose instance owns
    no pixel afterwards are dropped, the rest renumbered 0 .. n'-1 in order, and the statistics are taken from the
    cleaned map.  The new ids travel in the same device-to-host copy.

    `return_aim_points=True` adds "aim_point" and "clearance" of the merged (and cleaned) map's instances, as the
    post-processor does: the point of the field map a tool would be driven from.  They travel in the
    same copy too.

    `split=SplitOptions(...)` parts touching plants of the merged (and cleaned) field map as the post-processor's
    `split=` does -- the tile merge can only join instances, this parts them: a part split off gets
    the next free id and an entry after the merged ones, a copy of its parent's with its own "id" and "split_from";
    statistics and aim points describe the split map.

    `return_shape_stats=True` adds the shape traits of the merged (cleaned, split) map's instances, as the post-processor
    does; they travel in a device-to-host copy of their own, being float64."""
    results = list(results)
    T = grid.n_tiles
    if len(results) != T:
        raise ValueError(f"merge_tile_results: {len(results)} results for {T} tiles")
    maps = [r["segmentation"] for r in results]
    if not all(isinstance(m, torch.Tensor) for m in maps):
        raise TypeError("merge_tile_results: every result needs a `segmentation` tensor (not RLE or binary maps)")
    for m in maps:
        ops._core._on_gpu(m, "segmentation")
        if tuple(m.shape) != (grid.th, grid.tw):
            raise ValueError(f"merge_tile_results: a tile map of {tuple(m.shape)}, the grid's tiles are {(grid.th, grid.tw)}")
    num, den = (int(v) for v in merge_threshold)
    if num < 0 or den < 1:
        raise ValueError(f"merge_tile_results: merge_threshold (num, den) needs num >= 0 and den >= 1, got {(num, den)}")
    if clean is not None:
        from .instances import CleanOptions, cleaned_segments_info
        if not isinstance(clean, CleanOptions):
            raise TypeError(f"merge_tile_results: clean must be a CleanOptions or None, got {type(clean).__name__}")
    if split is not None:
        from .instances import SplitOptions, split_rows, split_segments_info
        if not isinstance(split, SplitOptions):
            raise TypeError(f"merge_tile_results: split must be a SplitOptions or None, got {type(split).__name__}")
    n_ids_h, labels_h = _tile_tables(results, T)
    N = int(labels_h.shape[1])
    tiles = torch.stack(maps)
    dev = tiles.device
    geom_h, pairs_h = grid.geom_table(), grid.pair_table()
    packed = np.concatenate([n_ids_h, labels_h.reshape(-1), geom_h.reshape(-1), pairs_h.reshape(-1)])
    d = torch.from_numpy(packed).pin_memory().to(dev, non_blocking=True)
    o = np.cumsum([0, T, T * N, T * 6, pairs_h.size])
    n_ids, labels = d[o[0]:o[1]], d[o[1]:o[2]].view(T, N)
    geom, pairs = d[o[2]:o[3]].view(T, 6), d[o[3]:o[4]].view(-1, 8)

    hist = ops.tile_pair_counts(tiles, n_ids, pairs, N)
    owned = ops.tile_owned_counts(tiles, n_ids, geom, N)
    remap, n_merged = ops.tile_link(hist, pairs, labels, n_ids, owned, (num, den))
    out = ops.tile_compose(tiles, n_ids, geom, remap, (grid.height, grid.width))

    back = [remap.reshape(-1).to(torch.int64), n_merged.to(torch.int64)]
    n_stats = min(int(n_ids_h.sum()), MAX_MERGED_IDS)  # an upper bound of n_merged known without a copy
    cleaning = clean is not None and n_stats > 0
    if cleaning:  # merged ids beyond n_stats (then merged_segments_info raises below) would count as background
        cleaned, clean_stats, n_merged = ops.labelmap_clean(out.unsqueeze(0), n_stats, relabel=True, **clean.kernel_arguments())
        out = cleaned[0]
        back.append(clean_stats[0, :, 7])
    splitting = split is not None and n_stats > 0
    n_rows = split.id_space(n_stats) if splitting else n_stats  # the id space of the returned map
    if splitting:  # the kernel numbers the parts split off from n_stats; they continue the map's own ids
        parted, info, status = split_rows(out.unsqueeze(0), n_stats, split)
        out = torch.where(parted[0] >= n_stats, parted[0] - (n_stats - n_merged.view(())).to(torch.int32), parted[0])
        back += [info[0, :, 0].to(torch.int64), status[0, :1].clamp(max=n_rows).to(torch.int64)]
    if return_instance_stats and n_stats:
        back.append(ops.labelmap_instance_stats(out.unsqueeze(0), N=n_rows).reshape(-1))
    if return_aim_points and n_stats:
        from .instances import add_aim_points, aim_point_rows
        back.append(aim_point_rows(out.unsqueeze(0), n_rows).reshape(-1).to(torch.int64))
    shape_dev = None
    if return_shape_stats and n_stats:
        from .instances import add_shape_traits, shape_trait_rows
        shape_dev = shape_trait_rows(out.unsqueeze(0), n_rows)[0]
    host = torch.cat(back).cpu()  # the one device-to-host copy
    segments = merged_segments_info(host[:T * N].view(T, N).numpy(), int(host[T * N]), results)
    rest = host[T * N + 1:]
    if cleaning:
        segments = cleaned_segments_info(segments, rest[:n_stats].numpy())
        rest = rest[n_stats:]
    if splitting:
        parents, extras = rest[:n_rows].numpy(), int(rest[n_rows]) - n_stats
        n = len(segments)
        segments = split_segments_info(segments, [[p] for p in parents[:n]] + [[p] for p in parents[n_stats:n_stats + extras]],
                                       n + extras)
        rest = rest[n_rows + 1:]
    if return_instance_stats and segments:
        from .instances import stats_to_boxes
        stats = rest[:n_rows * 8].view(-1, 8)[:len(segments)]
        area, bbox, centroid = (v.tolist() for v in stats_to_boxes(stats))
        for k, info in enumerate(segments):
            info["area"] = area[k]
            info["bbox"] = bbox[k]
            info["centroid"] = tuple(centroid[k]) if area[k] > 0 else None
    if return_instance_stats and n_stats:
        rest = rest[n_rows * 8:]
    if return_aim_points and segments:
        add_aim_points(segments, rest[:n_rows * 4].view(-1, 4).numpy())
    if shape_dev is not None and segments:
        add_shape_traits(segments, shape_dev.cpu().numpy())
    return {"segmentation": out, "segments_info": segments}


def _device_image(image) -> torch.Tensor:
    """A PIL RGB image, a numpy or torch (H, W, 3) uint8 array -> a uint8 (H, W, 3) tensor on the GPU."""
    from ._lib import Wm2fError
    from .preprocess import _image_hwc_u8
    img = _image_hwc_u8(image, 0)
    if not torch.cuda.is_available():
        raise Wm2fError("segment_tiled runs on a GPU only (no CPU fallback): no device is visible")
    if isinstance(img, torch.Tensor):
        return img if img.is_cuda else img.cuda()
    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


def segment_tiled(image, model, processor, tile: int = 1024, overlap: int = 256, batch_size: int = 4,
                  threshold: float = 0.5, mask_threshold: float = 0.5, overlap_mask_area_threshold: float = 0.8,
                  merge_threshold=(1, 2), return_instance_stats: bool = False, clean=None,
                  return_aim_points: bool = False, split=None, *, colors=None, return_shape_stats: bool = False) -> dict:
    """Instance segmentation of an image of any size at native resolution: overlapping tiles (`tile_windows`), `batch_size`
    of them at a time through `processor(images=...)`, `model(pixel_values=...)` under no_grad and
    `processor.post_process_instance_segmentation(target_sizes=tile size)`, then `merge_tile_results`.  The image (PIL
    RGB, numpy or torch (H, W, 3) uint8) is moved to the device once and the tiles are slices of it.  An image no larger
    than one tile takes the same route with one tile.  `processor` is this package's `Mask2FormerImageProcessor` (or
    anything that takes a list of device uint8 (h, w, 3) tensors and post-processes into id maps on the device); it is
    called with `images=` alone, so its own size settings decide how a tile is fed.  `clean=CleanOptions(...)` repairs
    the merged map (`merge_tile_results`); the tiles themselves are merged as predicted; `return_aim_points=True` adds the
    merged map's aim points and clearances there; `split=SplitOptions(...)` parts touching plants of the merged map
    there; `return_shape_stats=True` adds the merged map's shape traits there.  Returns `merge_tile_results`'s dictionary.
    `colors=ColorOptions(...)` adds the colour traits of the merged map's instances under the full-size picture, which is
    on the device already (`annotate_colors`); None: the result is what it is without.  `colors` and
    `return_shape_stats` are keyword-only: a further option can join them without moving anyone's positional slot."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"segment_tiled: batch_size must be at least 1, got {batch_size}")
    if colors is not None:
        from .color import ColorOptions, annotate_colors
        if not isinstance(colors, ColorOptions):
            raise TypeError(f"segment_tiled: colors must be a ColorOptions or None, got {type(colors).__name__}")
    img = _device_image(image)
    grid = tile_windows(int(img.shape[0]), int(img.shape[1]), tile, overlap)
    crops = [img[y0:y1, x0:x1] for y0, x0, y1, x1 in grid.windows]
    results = []
    with torch.no_grad(), torch.cuda.device(img.device):
        for s in range(0, len(crops), batch_size):
            batch = crops[s:s + batch_size]
            inputs = processor(images=batch)  # the crops are on the device already
            outputs = model(pixel_values=inputs["pixel_values"])
            results += processor.post_process_instance_segmentation(
                outputs, threshold=threshold, mask_threshold=mask_threshold,
                overlap_mask_area_threshold=overlap_mask_area_threshold, target_sizes=[(grid.th, grid.tw)] * len(batch))
    merged = merge_tile_results(results, grid, merge_threshold=merge_threshold, return_instance_stats=return_instance_stats,
                                clean=clean, return_aim_points=return_aim_points, split=split,
                                return_shape_stats=return_shape_stats)
    return merged if colors is None else annotate_colors(merged, img, colors)


# ---------------------------------------------------------------------------------------------- the semantic route
FLIP_CODES = {"none": 0, "h": 1, "v": 2, "hv": 3}  # bit 0: horizontal flip, bit 1: vertical flip (include/wm2f.h)


def _flip_codes(flips, who: str) -> list:
    flips = [flips] if isinstance(flips, str) else list(flips)
    if not flips:
        raise ValueError(f"{who}: flips must name at least one view")
    bad = [f for f in flips if f not in FLIP_CODES]
    if bad:
        raise ValueError(f"{who}: unknown flip {bad[0]!r}, expected one of {tuple(FLIP_CODES)}")
    return [FLIP_CODES[f] for f in flips]


def _axis_ramp(origins, side: int) -> int:
    """The default ramp of one axis: the smallest overlap of two neighbouring tiles, at least 1 (1 with one tile)."""
    gaps = [origins[i] + side - origins[i + 1] for i in range(len(origins) - 1)]
    return max(1, min(gaps)) if gaps else 1


def _check_cover(origins, side: int, length: int, axis: str) -> None:
    o = [int(v) for v in origins]
    if not o or o[0] != 0 or o[-1] + side < length or any(b <= a or b > a + side for a, b in zip(o, o[1:])):
        raise ValueError(f"blend_tile_scores: the grid's {axis} origins {o[:8]} with side {side} do not cover [0, {length}) "
                         "in ascending order without a gap")


def blend_tile_scores(scores, grid: TileGrid, flips=("none",), ramp=None, return_scores: bool = False) -> dict:
    """Blend per-tile class scores into one image's semantic result: {"segmentation": (H, W) int32 class ids on the
    device, "scores": (C, H, W) fp32 with return_scores}.

    `scores` is (F, T, C, gh, gw) fp32 on the device, or (T, C, gh, gw) for one view: for every view in `flips` (names out
    of "none", "h", "v", "hv") and every tile in `grid` order, the (C, gh, gw) scores `post_process_semantic_segmentation(
    target_sizes=None, return_segmentation_scores=True)` gave for that tile -- for a flipped view, computed on the flipped
    tile and stored as they came out; the kernel reads them at the mirrored pixel.

    Per output pixel every covering view is resized bilinearly (align_corners=False, as the post-processor resizes) to the
    tile size on demand, weighted by a tent that rises by 1 per pixel from each tile border and is capped at `ramp`, and
    summed in a fixed order; the map is the first-max argmax of the sums, the scores their weighted mean.  A pixel that one
    view alone covers gets that tile's own result bit for bit.  `ramp` is an integer or (ramp_y, ramp_x); the default per
    axis is the smallest overlap of two neighbouring tiles of `grid` (`TileGrid` does not record the overlap it was asked
    for; `tile_windows` squeezes the origins, so the actual overlaps are at least that), and at least 1: the window then
    reaches its plateau exactly where the narrowest overlap ends, and no seam is visible where tiles disagree.  The
    contract is written out in include/wm2f.h (wm2f_tile_blend).  One kernel call; the (R + Cn + F) origins and flip codes
    are the only host-to-device copy."""
    who = "blend_tile_scores"
    codes = _flip_codes(flips, who)
    if not isinstance(scores, torch.Tensor):
        raise TypeError(f"{who}: scores must be a tensor")
    if scores.dim() == 4:
        scores = scores.unsqueeze(0)
    if scores.dim() != 5:
        raise ValueError(f"{who}: scores must be (F, T, C, gh, gw) or (T, C, gh, gw), got {tuple(scores.shape)}")
    if scores.shape[0] != len(codes) or scores.shape[1] != grid.n_tiles:
        raise ValueError(f"{who}: scores hold {scores.shape[0]} views of {scores.shape[1]} tiles, expected {len(codes)} "
                         f"views ({', '.join(flips) if not isinstance(flips, str) else flips}) of {grid.n_tiles} tiles")
    _check_cover(grid.ys, grid.th, grid.height, "row")
    _check_cover(grid.xs, grid.tw, grid.width, "column")
    if ramp is None:
        ramp = (_axis_ramp(grid.ys, grid.th), _axis_ramp(grid.xs, grid.tw))
    elif isinstance(ramp, (int, np.integer)):
        ramp = (int(ramp), int(ramp))
    ramp = tuple(int(v) for v in ramp)
    if len(ramp) != 2 or min(ramp) < 1:
        raise ValueError(f"{who}: ramp must be an integer or (ramp_y, ramp_x), each at least 1, got {ramp}")
    ops._core._on_gpu(scores, "scores")
    R, Cn = len(grid.ys), len(grid.xs)
    packed = np.asarray([*grid.ys, *grid.xs, *codes], dtype=np.int32)
    d = torch.from_numpy(packed).pin_memory().to(scores.device, non_blocking=True)
    seg, out = ops.tile_blend(scores, d[:R], d[R:R + Cn], d[R + Cn:], (grid.height, grid.width), (grid.th, grid.tw), ramp,
                              want_scores=return_scores)
    result = {"segmentation": seg}
    if return_scores:
        result["scores"] = out
    return result


def segment_tiled_semantic(image, model, processor, tile: int = 1024, overlap: int = 256, batch_size: int = 4,
                           flips=("none",), return_scores: bool = False) -> dict:
    """Semantic segmentation of an image of any size at native resolution: overlapping tiles (`tile_windows`), and per view
    in `flips` (names out of "none", "h", "v", "hv": the tiles as they are, flipped horizontally, vertically, both)
    `batch_size` tiles at a time -- flipped on the device with `torch.flip` -- through `processor(images=...)`,
    `model(pixel_values=...)` under no_grad and `processor.post_process_semantic_segmentation(target_sizes=None,
    return_segmentation_scores=True)`, whose (C, gh, gw) scores go straight into one preallocated (F, T, C, gh, gw) fp32
    buffer of F * T * C * gh * gw * 4 bytes (6000 x 4000 at tile 1024, overlap 256: T = 40 tiles on the 384 x 384 grid,
    71 MB per view at C = 3); then one `blend_tile_scores` call with the default ramp.  Image and processor as for
    `segment_tiled`.  Returns {"segmentation": (H, W) int32 class ids, "scores": (C, H, W) fp32 with return_scores}, on
    the device; nothing is copied to the host."""
    who = "segment_tiled_semantic"
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"{who}: batch_size must be at least 1, got {batch_size}")
    codes = _flip_codes(flips, who)
    img = _device_image(image)
    grid = tile_windows(int(img.shape[0]), int(img.shape[1]), tile, overlap)
    crops = [img[y0:y1, x0:x1] for y0, x0, y1, x1 in grid.windows]
    buf = None
    with torch.no_grad(), torch.cuda.device(img.device):
        for v, code in enumerate(codes):
            dims = [d for bit, d in ((2, 0), (1, 1)) if code & bit]
            for s in range(0, len(crops), batch_size):
                batch = crops[s:s + batch_size]
                if dims:
                    batch = [torch.flip(c, dims) for c in batch]
                inputs = processor(images=batch)
                outputs = model(pixel_values=inputs["pixel_values"])
                res = processor.post_process_semantic_segmentation(outputs, target_sizes=None, return_segmentation_scores=True)
                for j, r in enumerate(res):
                    S = r["segmentation_scores"]
                    if buf is None:
                        buf = torch.empty(len(codes), len(crops), *S.shape, device=S.device, dtype=torch.float32)
                    buf[v, s + j].copy_(S)
    return blend_tile_scores(buf, grid, flips=flips, return_scores=return_scores)
