"""Skeletons of id maps: Guo-Hall thinning of every instance at once and per-instance skeleton sums
-- csrc/skeleton.hip, a fixed chain of launches over a whole (B, H, W) stack; spur pruning and the decomposition into
branches and node clusters -- csrc/skeleton_graph.hip."""
from __future__ import annotations

import torch

from .._lib import load
from ._core import _id_maps, _id_rows, _launch, _p, _req, _workspace

MAX_IDS, MAX_ROUNDS, PER_LAUNCH, DEFAULT_PER_LAUNCH = 4096, 1024, (0, 1, 2, 4, 8), 4
STAT_COLUMNS = 8


def labelmap_skeleton(maps: torch.Tensor, N: int, rounds: int = 64, per_launch: int = 0):
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8), instances 0 .. N-1 -> (out, status)
    (wm2f_labelmap_skeleton).  `rounds` iterations of Guo and Hall's two-sub-iteration parallel thinning, every instance
    on its own (another id counts as background).  out (B, H, W) int32: the skeleton as an id map, -1 elsewhere; status
    (B, 4) int32 [skeleton pixels, iterations that deleted something, deletions in the last of the `rounds` iterations,
    rounds]: a non-zero third entry says `rounds` was too small, and out is then the result of exactly `rounds`
    iterations.  `per_launch`: the iterations a launch runs on a tile held in LDS, 1, 2, 4 or 8 (0: the default); every
    value gives the same bits.  2 + ceil(rounds / per_launch) launches; everything stays on the device."""
    N, rounds, per_launch = int(N), int(rounds), int(per_launch)
    maps, dt, B, H, W = _id_maps(maps, "labelmap_skeleton", detail=f", N = {N}", bad=N < 0)
    if not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError(f"labelmap_skeleton: 1 <= rounds <= {MAX_ROUNDS}, got {rounds}")
    if per_launch not in PER_LAUNCH:
        raise ValueError(f"labelmap_skeleton: per_launch must be one of {PER_LAUNCH}, got {per_launch}")
    dev = maps.device
    out = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    status = torch.empty(B, 4, device=dev, dtype=torch.int32)
    ws = _workspace(load().wm2f_labelmap_skeleton_workspace(B, H, W), dev, 16)
    _launch("wm2f_labelmap_skeleton", maps, _p(maps), dt, _p(out), _p(status), _p(ws), B, H, W, N, rounds, per_launch,
            tag="labelmap_skeleton")
    return out, status


def labelmap_skeleton_stats(skel: torch.Tensor, ids: torch.Tensor | None = None, n_ids: torch.Tensor | None = None,
                            N: int | None = None, d2: torch.Tensor | None = None) -> torch.Tensor:
    """(B, H, W) int32 skeleton maps of `labelmap_skeleton` -> (B, N, 8) int64 per id
    [pixels, orthogonal links, diagonal links, tips, junction pixels, isolated pixels, sum d2, max d2]
    (wm2f_labelmap_skeleton_stats): a pair of 4-adjacent skeleton pixels is an orthogonal link, a diagonally adjacent pair
    a diagonal link unless one of the two pixels 4-adjacent to both belongs to the skeleton too; with b the same-id
    neighbours of a skeleton pixel and X its crossing number, a tip has X = 1 and b <= 2, a junction pixel X >= 3, an
    isolated pixel b = 0.  `d2`: the `labelmap_distance` of the ORIGINAL maps (without it the last two columns are 0).
    `ids` / `n_ids` / `N` as in `labelmap_instance_stats`; an id without a skeleton pixel has an all-zero row."""
    if not isinstance(skel, torch.Tensor):
        raise TypeError("labelmap_skeleton_stats: expected tensors")
    skel = _req(skel, "skel", torch.int32)
    skel, _, B, H, W = _id_maps(skel, "labelmap_skeleton_stats", "tensors")
    ids, n_ids, N = _id_rows("labelmap_skeleton_stats", B, ids, n_ids, N)
    if d2 is not None:
        d2 = _req(d2, "d2", torch.int32)
        if d2.shape != skel.shape:
            raise ValueError(f"labelmap_skeleton_stats: skel and d2 must agree, got {tuple(skel.shape)} and {tuple(d2.shape)}")
    stats = torch.empty(B, N, STAT_COLUMNS, device=skel.device, dtype=torch.int64)
    if N == 0:
        return stats
    _launch("wm2f_labelmap_skeleton_stats", skel, _p(skel), _p(d2), _p(ids), _p(n_ids), _p(stats), B, H, W, N,
            tag="skeleton_stats")
    return stats


GRAPH_COLUMNS = 8
MAX_PRUNE_ROUNDS, MAX_RETHIN, MAX_MIN_PIXELS, MAX_RATIO_Q = 64, 16, 1 << 20, 1024


def labelmap_skeleton_prune(skel: torch.Tensor, d2: torch.Tensor, N: int, min_pixels: int = 2, ratio_q: int = 16,
                            rounds: int = 8, rethin: int = 4):
    """(B, H, W) int32 skeleton maps of `labelmap_skeleton` and the `labelmap_distance` of the ORIGINAL maps -> (out,
    status) (wm2f_labelmap_skeleton_prune).  `rounds` rounds of: delete every spur -- a branch with a
    free end that hangs on one node cluster and has at most `min_pixels` pixels, or is no longer than `ratio_q` / 16 times
    the half-width of the part it grows out of -- then `rethin` thinning iterations.  out (B, H, W) int32: the pruned
    skeleton as an id map; status (B, 4) int32 [pixels left, rounds that removed something, pixels removed in the last
    of the `rounds` rounds, pixels removed in all]: a non-zero third entry says `rounds` was too few.  A fixed number of
    launches; everything stays on the device."""
    N, min_pixels, ratio_q, rounds, rethin = int(N), int(min_pixels), int(ratio_q), int(rounds), int(rethin)
    if not isinstance(skel, torch.Tensor) or not isinstance(d2, torch.Tensor):
        raise TypeError("labelmap_skeleton_prune: expected tensors")
    skel = _req(skel, "skel", torch.int32)
    skel, _, B, H, W = _id_maps(skel, "labelmap_skeleton_prune", "tensors", detail=f", N = {N}", bad=N < 0)
    d2 = _req(d2, "d2", torch.int32)
    if d2.shape != skel.shape:
        raise ValueError(f"labelmap_skeleton_prune: skel and d2 must agree, got {tuple(skel.shape)} and {tuple(d2.shape)}")
    for name, v, lo, hi in (("min_pixels", min_pixels, 0, MAX_MIN_PIXELS), ("ratio_q", ratio_q, 0, MAX_RATIO_Q),
                            ("rounds", rounds, 1, MAX_PRUNE_ROUNDS), ("rethin", rethin, 1, MAX_RETHIN)):
        if not lo <= v <= hi:
            raise ValueError(f"labelmap_skeleton_prune: {lo} <= {name} <= {hi}, got {v}")
    dev = skel.device
    out = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    status = torch.empty(B, 4, device=dev, dtype=torch.int32)
    ws = _workspace(load().wm2f_labelmap_skeleton_prune_workspace(B, H, W), dev, 16)
    _launch("wm2f_labelmap_skeleton_prune", skel, _p(skel), _p(d2), _p(out), _p(status), _p(ws), B, H, W, N, min_pixels,
            ratio_q, rounds, rethin, tag="labelmap_skeleton_prune")
    return out, status


def labelmap_skeleton_graph(skel: torch.Tensor, ids: torch.Tensor | None = None, n_ids: torch.Tensor | None = None,
                            N: int | None = None):
    """(B, H, W) int32 skeleton maps -> (labels, sums) (wm2f_labelmap_skeleton_graph): the skeleton's
    branches (8-connected sets of pixels with at most two same-id neighbours) and node clusters (of pixels with three or
    more).  labels (B, H, W) int32: -1 off the skeleton, a path pixel's branch label (the smallest linear index of the
    branch), -2 - (cluster label) for a node pixel.  sums (B, N, 8) int64 per id [branches, end branches, node clusters,
    node pixels, free ends, pixels of the longest end branch, pixels of the longest branch, closed branches].  `ids` /
    `n_ids` / `N` as in `labelmap_skeleton_stats`; with a list, a pixel whose value is not listed is off the skeleton."""
    if not isinstance(skel, torch.Tensor):
        raise TypeError("labelmap_skeleton_graph: expected tensors")
    skel = _req(skel, "skel", torch.int32)
    skel, _, B, H, W = _id_maps(skel, "labelmap_skeleton_graph", "tensors")
    ids, n_ids, N = _id_rows("labelmap_skeleton_graph", B, ids, n_ids, N)
    dev = skel.device
    labels = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    sums = torch.empty(B, N, GRAPH_COLUMNS, device=dev, dtype=torch.int64)
    ws = _workspace(load().wm2f_labelmap_skeleton_graph_workspace(B, H, W), dev, 16)
    _launch("wm2f_labelmap_skeleton_graph", skel, _p(skel), _p(ids), _p(n_ids), _p(labels), _p(sums) if N else _p(None),
            _p(ws), B, H, W, N, tag="labelmap_skeleton_graph")
    return labels, sums
