"""Repair of id maps: small pieces dropped, the largest piece kept, enclosed holes filled, ids
renumbered -- csrc/clean.hip, a fixed chain of launches over a whole (B, H, W) stack."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import load
from ._core import _dtype_code, _id_maps, _launch, _p, _workspace

_KEEP = {"all": _lib.WM2F_CLEAN_KEEP_ALL, "largest": _lib.WM2F_CLEAN_KEEP_LARGEST}
# the parts of the chain in order, each its own tagged launch so that a kernel timer sees them
_PHASES = ((_lib.WM2F_CLEAN_PIECES, "clean_pieces"), (_lib.WM2F_CLEAN_CHOOSE, "clean_choose"),
           (_lib.WM2F_CLEAN_HOLES, "clean_holes"), (_lib.WM2F_CLEAN_PAINT, "clean_paint"))


def labelmap_clean(maps: torch.Tensor, N: int, keep: str = "all", min_area: int = 0, fill_holes: bool = False,
                   max_hole_area: int | None = None, relabel: bool = False, out_dtype: torch.dtype = torch.int32):
    """(B, H, W) id maps (fp32 with -1 background, int32 or uint8), instances 0 .. N-1 -> (out, stats, n_out)
    (wm2f_labelmap_clean): per id the 8-connected pieces, of which `keep` = "all" or only the "largest" stay, those
    below `min_area` pixels dropped; with `fill_holes` the free 4-connected components enclosed by one id (of at most
    `max_hole_area` pixels, None: any) painted with it; with `relabel` the surviving ids renumbered 0 .. n'-1.
    out (B, H, W) `out_dtype` (int32 or fp32) with -1 where free; stats (B, N, 8) int64
    [area_in, pieces_in, pieces_kept, area_kept, holes_filled, pixels_filled, area_out, new_id]; n_out (B) int32.
    Everything stays on the device."""
    N, min_area = int(N), int(min_area)
    maps, dt, B, H, W = _id_maps(maps, "labelmap_clean", detail=f", N = {N}, or min_area = {min_area}",
                                 bad=N < 0 or min_area < 0)
    if out_dtype not in (torch.int32, torch.float32):
        raise TypeError(f"labelmap_clean: out_dtype int32 or fp32, got {out_dtype}")
    if keep not in _KEEP:
        raise ValueError(f"labelmap_clean: keep must be 'all' or 'largest', got {keep!r}")
    limit = -1 if max_hole_area is None else int(max_hole_area)
    if limit < 0 and max_hole_area is not None:
        raise ValueError(f"labelmap_clean: max_hole_area must not be negative, got {max_hole_area}")
    dev = maps.device
    out = torch.empty(B, H, W, device=dev, dtype=out_dtype)
    stats = torch.empty(B, N, 8, device=dev, dtype=torch.int64)
    n_out = torch.empty(B, device=dev, dtype=torch.int32)
    ws = _workspace(load().wm2f_labelmap_clean_workspace(B, H, W, N), dev, 8)
    odt = _dtype_code(out, (torch.int32, torch.float32), "labelmap_clean: out_dtype")
    for phase, tag in _PHASES:
        if phase == _lib.WM2F_CLEAN_HOLES and not fill_holes:
            continue
        _launch("wm2f_labelmap_clean", maps, _p(maps), dt, _p(out), odt, _p(stats) if N else None, _p(n_out), _p(ws), B, H, W, N,
                _KEEP[keep], min_area, int(bool(fill_holes)), limit, int(bool(relabel)), phase, tag=tag)
    return out, stats, n_out
