"""Merging the instances of overlapping tiles (the contract is in include/wm2f.h)."""
from __future__ import annotations

import torch

from .._lib import load
from ._core import _dtype_code, _launch, _p, _req, _workspace


def _tiles(tiles: torch.Tensor, n_ids: torch.Tensor, who: str):
    if not isinstance(tiles, torch.Tensor):
        raise TypeError(f"{who}: expected tensors")
    tiles = _req(tiles, "tiles", tiles.dtype)
    dt = _dtype_code(tiles, (torch.float32, torch.int32), f"{who}: tiles fp32 / int32, got {tiles.dtype}")
    n_ids = _req(n_ids, "n_ids", torch.int32)
    if tiles.dim() != 3 or 0 in tiles.shape or n_ids.shape != (tiles.shape[0],):
        raise ValueError(f"{who}: tiles must be a non-empty (T, th, tw) stack and n_ids (T), got {tuple(tiles.shape)} and "
                         f"{tuple(n_ids.shape)}")
    return tiles, dt, n_ids, tuple(int(v) for v in tiles.shape)


def _table(t: torch.Tensor, name: str, rows: int | None, cols: int, who: str) -> torch.Tensor:
    t = _req(t, name, torch.int32)
    if t.dim() != 2 or t.shape[1] != cols or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{who}: {name} must be ({'P' if rows is None else rows}, {cols}) int32, got {tuple(t.shape)}")
    return t


def tile_blend(scores: torch.Tensor, ys: torch.Tensor, xs: torch.Tensor, flips: torch.Tensor, size, tile_size, ramp,
               want_scores: bool = False):
    """scores (F, R * Cn, C, gh, gw) fp32 -- the score grid of every class of every tile of every view --, ys (R) and xs
    (Cn) int32 tile origins, flips (F) int32 (bit 0: the view was computed on the horizontally flipped tile, bit 1: on the
    vertically flipped one), size (H, W), tile_size (th, tw), ramp (ramp_y, ramp_x) -> seg (H, W) int32 and, with
    want_scores, the blended scores (C, H, W) fp32, else None (wm2f_tile_blend): per output pixel the bilinear samples of
    the covering views under a tent window capped at the ramp, summed in a fixed order, first-max argmax; -1 and zero
    scores where no tile covers."""
    scores = _req(scores, "scores", torch.float32)
    ys, xs, flips = _req(ys, "ys", torch.int32), _req(xs, "xs", torch.int32), _req(flips, "flips", torch.int32)
    if scores.dim() != 5 or 0 in scores.shape or ys.dim() != 1 or xs.dim() != 1 or flips.dim() != 1:
        raise ValueError(f"tile_blend: scores must be a non-empty (F, T, C, gh, gw) stack and ys, xs, flips vectors, got "
                         f"{tuple(scores.shape)}, {tuple(ys.shape)}, {tuple(xs.shape)}, {tuple(flips.shape)}")
    F, T, C, gh, gw = (int(v) for v in scores.shape)
    R, Cn = int(ys.shape[0]), int(xs.shape[0])
    if R * Cn != T or int(flips.shape[0]) != F:
        raise ValueError(f"tile_blend: {T} tiles and {F} views in scores, but {R} x {Cn} origins and {int(flips.shape[0])} flips")
    for t, name in ((ys, "ys"), (xs, "xs"), (flips, "flips")):
        if t.device != scores.device:
            raise ValueError(f"tile_blend: {name} is on {t.device}, scores on {scores.device}")
    (H, W), (th, tw), (ramp_y, ramp_x) = ((int(v[0]), int(v[1])) for v in (size, tile_size, ramp))
    if H <= 0 or W <= 0 or th <= 0 or tw <= 0:
        raise ValueError(f"tile_blend: bad size {(H, W)} or tile size {(th, tw)}")
    if ramp_y < 1 or ramp_x < 1:
        raise ValueError(f"tile_blend: the ramps must be at least 1, got {(ramp_y, ramp_x)}")
    seg = torch.empty(H, W, device=scores.device, dtype=torch.int32)
    out = torch.empty(C, H, W, device=scores.device, dtype=torch.float32) if want_scores else None
    _launch("wm2f_tile_blend", scores, _p(scores), _p(ys), _p(xs), _p(flips), _p(seg), _p(out), F, R, Cn, C, gh, gw, th, tw,
            ramp_y, ramp_x, H, W, tag="tile_blend")
    return seg, out


def tile_pair_counts(tiles: torch.Tensor, n_ids: torch.Tensor, pairs: torch.Tensor, N: int) -> torch.Tensor:
    """(T, th, tw) id maps (fp32 with -1 background, or int32), n_ids (T) int32, pairs (P, 8) int32 rows
    (a, b, ay, ax, by, bx, h, w) -> hist (P, N+1, N+1) int32, the joint histogram of tiles a and b over the rectangle they
    share (wm2f_tile_pair_counts); bin 0 on either side is "no id"."""
    tiles, dt, n_ids, (T, th, tw) = _tiles(tiles, n_ids, "tile_pair_counts")
    pairs = _table(pairs, "pairs", None, 8, "tile_pair_counts")
    N, P = int(N), int(pairs.shape[0])
    if N < 0:
        raise ValueError("tile_pair_counts: N must not be negative")
    hist = torch.empty(P, N + 1, N + 1, device=tiles.device, dtype=torch.int32)
    _launch("wm2f_tile_pair_counts", tiles, _p(tiles), dt, _p(n_ids), _p(pairs), _p(hist), T, th, tw, N, P,
            tag="tile_pair_counts")
    return hist


def tile_owned_counts(tiles: torch.Tensor, n_ids: torch.Tensor, geom: torch.Tensor, N: int) -> torch.Tensor:
    """tiles, n_ids as above, geom (T, 6) int32 rows (oy, ox, cy0, cy1, cx0, cx1) -> owned (T, N) int32, the pixels of
    every id inside its tile's own cell (wm2f_tile_owned_counts)."""
    tiles, dt, n_ids, (T, th, tw) = _tiles(tiles, n_ids, "tile_owned_counts")
    geom = _table(geom, "geom", T, 6, "tile_owned_counts")
    N = int(N)
    if N < 0:
        raise ValueError("tile_owned_counts: N must not be negative")
    owned = torch.empty(T, N, device=tiles.device, dtype=torch.int32)
    _launch("wm2f_tile_owned_counts", tiles, _p(tiles), dt, _p(n_ids), _p(geom), _p(owned), T, th, tw, N,
            tag="tile_owned_counts")
    return owned


def tile_link(hist: torch.Tensor, pairs: torch.Tensor, labels: torch.Tensor, n_ids: torch.Tensor, owned: torch.Tensor,
              merge_threshold=(1, 2)):
    """hist (P, N+1, N+1), pairs (P, 8), labels (T, N), n_ids (T), owned (T, N) int32 -> remap (T, N) int32 and n_merged
    (1) int32 (wm2f_tile_link): instances linked by the rule `inter * den >= num * min(area_a, area_b)` with equal labels
    share a merged id; sets that own a pixel are numbered in ascending order of their smallest node, every other node
    maps to -1.  merge_threshold = (num, den)."""
    labels, n_ids = _req(labels, "labels", torch.int32), _req(n_ids, "n_ids", torch.int32)
    hist, owned = _req(hist, "hist", torch.int32), _req(owned, "owned", torch.int32)
    pairs = _table(pairs, "pairs", None, 8, "tile_link")
    if labels.dim() != 2 or labels.shape[0] == 0:
        raise ValueError(f"tile_link: labels must be (T, N), got {tuple(labels.shape)}")
    T, N, P = int(labels.shape[0]), int(labels.shape[1]), int(pairs.shape[0])
    if owned.shape != (T, N) or n_ids.shape != (T,) or hist.shape != (P, N + 1, N + 1):
        raise ValueError("tile_link: shapes disagree")
    num, den = (int(v) for v in merge_threshold)
    dev = labels.device
    remap = torch.empty(T, N, device=dev, dtype=torch.int32)
    n_merged = torch.empty(1, device=dev, dtype=torch.int32)
    ws = _workspace(load().wm2f_tile_merge_workspace(T, N, P), dev, 16)
    _launch("wm2f_tile_link", labels, _p(hist), _p(pairs), _p(labels), _p(n_ids), _p(owned), _p(remap), _p(n_merged), _p(ws),
            T, N, P, num, den, tag="tile_link")
    return remap, n_merged


def tile_compose(tiles: torch.Tensor, n_ids: torch.Tensor, geom: torch.Tensor, remap: torch.Tensor, size) -> torch.Tensor:
    """tiles, n_ids, geom as above, remap (T, N) int32, size (H, W) -> out (H, W) int32 (wm2f_tile_compose): every
    output pixel is its owner tile's value relabelled through remap, -1 where that value is no id.  The cells of geom must
    partition (H, W), as `tiling.tile_windows`' do: the output is written once, inside the cells only, so a pixel that no
    cell covers is left uninitialised."""
    tiles, dt, n_ids, (T, th, tw) = _tiles(tiles, n_ids, "tile_compose")
    geom = _table(geom, "geom", T, 6, "tile_compose")
    remap = _req(remap, "remap", torch.int32)
    if remap.dim() != 2 or remap.shape[0] != T:
        raise ValueError(f"tile_compose: remap must be ({T}, N), got {tuple(remap.shape)}")
    H, W = int(size[0]), int(size[1])
    if H <= 0 or W <= 0:
        raise ValueError(f"tile_compose: bad size {(H, W)}")
    out = torch.empty(H, W, device=tiles.device, dtype=torch.int32)
    _launch("wm2f_tile_compose", tiles, _p(tiles), dt, _p(n_ids), _p(geom), _p(remap), _p(out), T, th, tw,
            int(remap.shape[1]), H, W, tag="tile_compose")
    return out
