"""Crop rows: the Hough accumulator of the voting pixels of id maps with its energies, and every
instance's relation to a set of parallel lines (csrc/rows.hip)."""
from __future__ import annotations

import numpy as np
import torch

from ._core import _id_maps, _id_rows, _launch, _p, _req

ROW_FIXED_BITS = 14          # positions along a direction are integers in units of 2^-14 pixel
ROW_MIN_SHIFT, ROW_MAX_SHIFT = 14, 20
ROW_MAX_ANGLES = 1024
ROW_MAX_ROWS = 1024
ROW_ANGLE_BAND = 16          # wm2f_labelmap_row_votes: directions per LDS histogram band
ROW_LDS_MAX_IDS = 1024       # wm2f_labelmap_row_bands: accumulators in LDS up to this N, in the result above
ROW_COLUMNS = 3


def row_angle_table(T: int) -> np.ndarray:
    """The (T, 2) int32 table [c_t, s_t] = [rint(cos th_t 2^14), rint(sin th_t 2^14)] of th_t = pi t / T, the directions
    of the row normal; s_t >= 0."""
    T = int(T)
    if T < 1:
        raise ValueError(f"row_angle_table: T must be at least 1, got {T}")
    th = np.pi * np.arange(T, dtype=np.float64) / T
    return np.stack([np.rint(np.cos(th) * (1 << ROW_FIXED_BITS)), np.rint(np.sin(th) * (1 << ROW_FIXED_BITS))], 1).astype(np.int32)


def row_bins(H: int, W: int, shift: int) -> int:
    """R, the bins per direction of an (H, W) image: (((W + H - 2) << 14) >> shift) + 1."""
    return (((int(W) + int(H) - 2) << ROW_FIXED_BITS) >> int(shift)) + 1


def row_offset(c: int, W: int) -> int:
    """off = -min(0, c) (W - 1): what makes x c + y s + off >= 0 over the image."""
    return -min(0, int(c)) * (int(W) - 1)


def labelmap_row_votes(maps: torch.Tensor, vote: torch.Tensor, cs: torch.Tensor, shift: int = ROW_MIN_SHIFT):
    """(B, H, W) id maps (fp32, int32 or uint8; a value that is no id of [0, N) belongs to nothing), vote (B, N) uint8 /
    bool and the direction table cs (T, 2) int32 (`row_angle_table`, on the maps' device) -> (acc, energy)
    (wm2f_labelmap_row_votes): acc (B, T, R) int32, the pixels of the voting ids per bin
    (x c_t + y s_t + off_t) >> shift of every direction, R = `row_bins(H, W, shift)`; energy (B, T) int64, the sum of
    acc^2 over the bins."""
    shift = int(shift)
    maps, dt, B, H, W = _id_maps(maps, "labelmap_row_votes", "tensors")
    vote = _req(vote, "vote", vote.dtype if isinstance(vote, torch.Tensor) and vote.dtype in (torch.bool, torch.uint8) else torch.uint8)
    cs = _req(cs, "cs", torch.int32)
    if vote.dim() != 2 or vote.shape[0] != B:
        raise ValueError(f"labelmap_row_votes: vote must be ({B}, N), got {tuple(vote.shape)}")
    if cs.dim() != 2 or cs.shape[1] != 2:
        raise ValueError(f"labelmap_row_votes: cs must be (T, 2), got {tuple(cs.shape)}")
    if vote.device != maps.device or cs.device != maps.device:
        raise ValueError("labelmap_row_votes: maps, vote and cs must be on one device")
    N, T = int(vote.shape[1]), int(cs.shape[0])
    R = max(1, row_bins(H, W, min(max(shift, ROW_MIN_SHIFT), ROW_MAX_SHIFT)))
    ok = 1 <= T <= ROW_MAX_ANGLES  # the call refuses what is not; the results then only have to exist
    acc = torch.empty(B, T if ok else 0, R, device=maps.device, dtype=torch.int32)
    energy = torch.empty(B, T if ok else 0, device=maps.device, dtype=torch.int64)
    _launch("wm2f_labelmap_row_votes", maps, _p(maps), dt, _p(vote.view(torch.uint8)), _p(cs), _p(acc), _p(energy), B, H, W, N,
            T, shift, tag="row_votes")
    return acc, energy


def labelmap_row_bands(maps: torch.Tensor, line: torch.Tensor, rho: torch.Tensor, band: int,
                       ids: torch.Tensor | None = None, n_ids: torch.Tensor | None = None, N: int | None = None,
                       zone: bool = False):
    """(B, H, W) id maps, line (B, 4) int32 [c, s, off, K] and rho (B, Kmax) int32 ascending row positions (K of them
    valid) in units of 2^-14 pixel -> counts (B, N, 3) int64 per id (wm2f_labelmap_row_bands): its pixels, those with
    |x c + y s + off - nearest rho_k| <= band, and the sum of x c + y s + off over its pixels.  zone=True returns
    (counts, zone): zone (B, H, W) uint8, 1 for a pixel in a band whatever its id.  `ids` / `n_ids` / `N` as in
    `labelmap_instance_stats`."""
    band = int(band)
    maps, dt, B, H, W = _id_maps(maps, "labelmap_row_bands", "tensors")
    ids, n_ids, N = _id_rows("labelmap_row_bands", B, ids, n_ids, N)
    line, rho = _req(line, "line", torch.int32), _req(rho, "rho", torch.int32)
    if line.shape != (B, 4) or rho.dim() != 2 or rho.shape[0] != B:
        raise ValueError(f"labelmap_row_bands: line must be ({B}, 4) and rho ({B}, Kmax), got {tuple(line.shape)} and {tuple(rho.shape)}")
    if line.device != maps.device or rho.device != maps.device:
        raise ValueError("labelmap_row_bands: maps, line and rho must be on one device")
    if band < 0 or band > 2 ** 31 - 1:
        raise ValueError(f"labelmap_row_bands: band must be in [0, 2^31), got {band}")
    Kmax = int(rho.shape[1])
    counts = torch.empty(B, N, ROW_COLUMNS, device=maps.device, dtype=torch.int64)
    z = torch.empty(B, H, W, device=maps.device, dtype=torch.uint8) if zone else None
    if N == 0:
        if zone:
            raise ValueError("labelmap_row_bands: the zone needs N >= 1")
        return counts
    _launch("wm2f_labelmap_row_bands", maps, _p(maps), dt, _p(ids), _p(n_ids), _p(line), _p(rho) if Kmax else _p(None), _p(counts),
            _p(z), B, H, W, N, Kmax, band, tag="row_bands")
    return (counts, z) if zone else counts
