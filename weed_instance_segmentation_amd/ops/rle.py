"""Run-length encoding and decoding of id maps: toggle counts, toggle positions in CSR layout, and
painting runs back into a map."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .._lib import Wm2fError, load
from ._core import _id_maps, _launch, _p, _req


def _toggle_args(maps, N, order, who):
    maps, dt, B, H, W = _id_maps(maps, who, "tensors")
    N, order = int(N), int(order)
    if order not in (0, 1):
        raise ValueError(f"{who}: order is 0 (row-major) or 1 (column-major), got {order}")
    if N < 0 or N > _lib.WM2F_RLE_MAX_IDS:
        raise ValueError(f"{who}: N must be in [0, {_lib.WM2F_RLE_MAX_IDS}], got {N}")
    return maps, dt, B, H, W, N, order


def _toggle_counts(maps, dt, B, H, W, N, order):
    size = int(load().wm2f_rle_workspace(B, H, W, N, order))
    if size < 0:
        raise ValueError(f"labelmap_toggle_counts: unsupported size {B} x {H} x {W}, N = {N}")
    ws = torch.empty(size, device=maps.device, dtype=torch.uint8)
    counts = torch.empty(B, N + 1, device=maps.device, dtype=torch.int32)
    out_of_range = torch.empty(B, device=maps.device, dtype=torch.int32)
    _launch("wm2f_labelmap_toggle_counts", maps, _p(maps), dt, _p(counts), _p(out_of_range), _p(ws), B, H, W, N, order,
            tag="labelmap_toggle_counts")
    return counts, out_of_range, ws


def labelmap_toggle_counts(maps: torch.Tensor, N: int, order: int = 0):
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8), ids in [-1, N) -> counts (B, N + 1) int32, the
    length of every slot's toggle list (slot 0 is id -1, slot k + 1 id k) in scan order `order` (0 row-major, 1
    column-major), and out_of_range (B) int32, the pixels whose value is outside [-1, N).  On the device, no
    synchronisation (wm2f_labelmap_toggle_counts)."""
    maps, dt, B, H, W, N, order = _toggle_args(maps, N, order, "labelmap_toggle_counts")
    counts, out_of_range, _ = _toggle_counts(maps, dt, B, H, W, N, order)
    return counts, out_of_range


def labelmap_toggles(maps: torch.Tensor, N: int, order: int = 0):
    """The toggle lists of every slot of (B, H, W) id maps: (counts, positions, offsets).  counts (B, N + 1) int64 numpy
    on the host; positions (total) int32 on the device, slot s of image b at offsets[b * (N + 1) + s] (CSR, image-major
    then slot), ascending; offsets (B * (N + 1) + 1) int64 numpy.  Two launches with ONE device-to-host copy of the
    counts between them, which sizes `positions` exactly.  Raises ValueError when a map holds a value outside [-1, N)."""
    maps, dt, B, H, W, N, order = _toggle_args(maps, N, order, "labelmap_toggles")
    counts_d, out_d, ws = _toggle_counts(maps, dt, B, H, W, N, order)
    host = torch.cat([counts_d.flatten(), out_d]).cpu().numpy().astype(np.int64)  # the one copy
    counts, bad = host[:B * (N + 1)].reshape(B, N + 1), host[B * (N + 1):]
    if bad.any():
        b = int(np.nonzero(bad)[0][0])
        raise ValueError(f"labelmap_toggles: image {b} holds {int(bad[b])} pixels whose value is outside [-1, {N})")
    offsets = np.zeros(B * (N + 1) + 1, np.int64)
    np.cumsum(counts.reshape(-1), out=offsets[1:])
    total = int(offsets[-1])
    if total >= 2 ** 31:
        raise ValueError(f"labelmap_toggles: {total} toggles do not fit int32 offsets; encode fewer images per call")
    positions = torch.empty(total, device=maps.device, dtype=torch.int32)
    offsets_d = torch.from_numpy(offsets.astype(np.int32)).to(maps.device)
    _launch("wm2f_labelmap_toggles", maps, _p(maps), dt, _p(offsets_d), _p(positions), _p(ws), B, H, W, N, order,
            tag="labelmap_toggles")
    return counts, positions, offsets


def rle_paint_(out: torch.Tensor, runs: torch.Tensor, order: int = 0) -> torch.Tensor:
    """Paint runs (R, 4) int32 (image, start, length, value), positions in scan order `order`, into out (B, H, W) int32
    in place (wm2f_rle_paint): a later run over an earlier one; pixels no run covers keep their value.  A run outside its
    image (start + length > H * W, a negative start or length, a bad image index) is not clipped: the whole call is
    refused, nothing is painted and Wm2fError is raised.  Reads one status word back from the device."""
    if not isinstance(out, torch.Tensor) or not isinstance(runs, torch.Tensor):
        raise TypeError("rle_paint_: expected tensors")
    if not out.is_contiguous():
        raise ValueError("rle_paint_: out must be contiguous (it is painted in place)")
    out, runs = _req(out, "out", torch.int32), _req(runs, "runs", torch.int32)
    if out.dim() != 3 or runs.dim() != 2 or runs.shape[1] != 4:
        raise ValueError(f"rle_paint_: out must be (B, H, W) and runs (R, 4), got {tuple(out.shape)} and {tuple(runs.shape)}")
    if int(order) not in (0, 1):
        raise ValueError(f"rle_paint_: order is 0 (row-major) or 1 (column-major), got {order}")
    B, H, W = (int(v) for v in out.shape)
    R = int(runs.shape[0])
    if R == 0:
        return out
    size = int(load().wm2f_rle_paint_workspace(B, H, W))
    if size < 0:
        raise ValueError(f"rle_paint_: unsupported size {B} x {H} x {W}")
    ws = torch.empty(size, device=out.device, dtype=torch.uint8)
    status = torch.empty(1, device=out.device, dtype=torch.int32)
    _launch("wm2f_rle_paint", out, _p(out), _p(runs), R, _p(status), _p(ws), B, H, W, int(order), tag="rle_paint")
    bad = int(status.item())
    if bad != 2 ** 31 - 1:
        raise Wm2fError(f"wm2f_rle_paint failed (code {_lib.WM2F_EINVAL}): run {bad} does not lie inside its image "
                        f"({H} x {W}); nothing was painted")
    return out
