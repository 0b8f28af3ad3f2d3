"""Splitting touching instances of id maps: a watershed of the interior distance -- csrc/split.hip,
a fixed chain of launches over a whole (B, H, W) stack."""
from __future__ import annotations

import torch

from .._lib import load
from ._core import _dtype_code, _launch, _p, _req

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
    if not isinstance(maps, torch.Tensor) or not isinstance(d2, torch.Tensor):
        raise TypeError("labelmap_split: expected tensors")
    maps = _req(maps, "maps", maps.dtype)
    dt = _dtype_code(maps, (torch.float32, torch.int32, torch.uint8),
                     f"labelmap_split: maps fp32 / int32 / uint8, got {maps.dtype}")
    d2 = _req(d2, "d2", torch.int32)
    if maps.dim() != 3 or d2.shape != maps.shape:
        raise ValueError(f"labelmap_split: maps and d2 must be (B, H, W), got {tuple(maps.shape)} and {tuple(d2.shape)}")
    B, H, W = (int(v) for v in maps.shape)
    N, M, num, den, min_peak_d2, rounds = int(N), int(M), int(num), int(den), int(min_peak_d2), int(rounds)
    if B == 0 or H == 0 or W == 0 or N < 0 or M < N:
        raise ValueError(f"labelmap_split: bad size {tuple(maps.shape)}, N = {N}, M = {M}")
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
    nbytes = int(load().wm2f_labelmap_split_workspace(B, H, W, M))
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)  # an unsupported size: the launch reports it
    _launch("wm2f_labelmap_split", maps, _p(maps), dt, _p(d2), _p(out), _p(info) if M else None, _p(status), _p(ws), B, H, W,
            N, M, num, den, min_peak_d2, rounds, tag="labelmap_split")
    return out, info, status
