"""Splitting touching instances of id maps: a watershed of the interior distance -- csrc/split.hip,
a fixed chain of launches over a whole (B, H, W) stack."""
from __future__ import annotations

import torch

from .._lib import load
from ._core import _id_maps_d2, _launch, _p, _workspace

MAX_IDS, MAX_ROUNDS, MAX_DEN = 4096, 32, 1024


def labelmap_split(maps: torch.Tensor, d2: torch.Tensor, N: int, M: int, num: int, den: int, min_peak_d2: int = 0,
                   rounds: int = 8):
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8), instances 0 .. N-1, and their `labelmap_distance`
    -> (out, info, status) (wm2f_labelmap_split).  Every pixel ascends d2 to a peak; the basins of one id are merged, in
    `rounds` synchronous rounds, into the higher neighbour across their highest pass when the pass's d2 is at least
    (num / den)^2 of the part's own peak d2, or when that peak d2 is below `min_peak_d2`.  Per id the part with the highest
    peak keeps the id; the others get N, N+1, ... in raster order of their peaks, those past `M` stay with their id.
    out (B, H, W) int32 with -1 background; info (B, M, 4) int32 [parent_id, peak_x, peak_y, peak_d2] per output id,
    [-1, -1, -1, 0] for an id without a pixel; status (B, 4) int32 [ids wanted, basins, links made in the last round,
    rounds].  Everything stays on the device."""
    if not isinstance(d2, torch.Tensor):
        raise TypeError("labelmap_split: expected tensors")
    N, M, num, den, min_peak_d2, rounds = int(N), int(M), int(num), int(den), int(min_peak_d2), int(rounds)
    maps, dt, d2, B, H, W = _id_maps_d2(maps, d2, "labelmap_split", detail=f", N = {N}, M = {M}", bad=N < 0 or M < N)
    if not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError(f"labelmap_split: 1 <= rounds <= {MAX_ROUNDS}, got {rounds}")
    if not (1 <= den <= MAX_DEN and 0 <= num <= den):
        raise ValueError(f"labelmap_split: 0 <= num <= den and 1 <= den <= {MAX_DEN}, got {num} / {den}")
    if not 0 <= min_peak_d2 < 2 ** 31:
        raise ValueError(f"labelmap_split: min_peak_d2 must be in [0, 2^31), got {min_peak_d2}")
    dev = maps.device
    out = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    info = torch.empty(B, max(M, 1), 4, device=dev, dtype=torch.int32)[:, :M]  # M = 0: a pointer all the same
    status = torch.empty(B, 4, device=dev, dtype=torch.int32)
    ws = _workspace(load().wm2f_labelmap_split_workspace(B, H, W, M), dev, 16)
    _launch("wm2f_labelmap_split", maps, _p(maps), dt, _p(d2), _p(out), _p(info) if M else None, _p(status), _p(ws), B, H, W,
            N, M, num, den, min_peak_d2, rounds, tag="labelmap_split")
    return out, info, status
