"""Skeletons of id maps: Guo-Hall thinning of every instance at once and per-instance skeleton sums
-- csrc/skeleton.hip, a fixed chain of launches over a whole (B, H, W) stack."""
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
