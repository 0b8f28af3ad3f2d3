"""Polygon rasterisation."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import load
from ._core import _launch, _on_gpu, _p


def _i32_array(a, name: str, ndim: int) -> "np.ndarray":
    import numpy as np
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.size == 0:
        a = a.reshape((0,) * (ndim - 1) + ((2,) if ndim == 2 else (0,)))
    if a.ndim != ndim or (ndim == 2 and a.shape[1] != 2):
        raise ValueError(f"{name}: expected {'(N, 2)' if ndim == 2 else 'a 1-D'} integer array, got shape {a.shape}")
    if a.size and a.dtype.kind not in "iub":
        raise ValueError(f"{name}: expected integers, got {a.dtype}")
    return a.astype(np.int64)


def fill_polygons(out: torch.Tensor, verts, contour_offsets, call_offsets, values) -> torch.Tensor:
    """A chain of `cv2.fillPoly(out, contours, value)` calls on the device, in place and in order (include/wm2f.h,
    wm2f_poly_fill): `out` is (H, W) int32 on the GPU; `verts` (V, 2) host integers x, y; `contour_offsets` (C + 1)
    vertex ranges of the contours; `call_offsets` (K + 1) contour ranges of the calls; `values` (K) the value each call
    paints.  A later call overwrites an earlier one.  One host-to-device copy of the packed tables, no read-back."""
    _on_gpu(out, "out")
    if out.dtype != torch.int32 or out.dim() != 2 or not out.is_contiguous():
        raise TypeError(f"out: expected a contiguous (H, W) int32 map, got {tuple(out.shape)} {out.dtype}")
    H, W = int(out.shape[0]), int(out.shape[1])
    packed, counts = _poly_tables(H, W, verts, contour_offsets, call_offsets, values)
    V, C, K, n_items = counts
    if K == 0:
        return out
    dev = out.device
    ws_bytes = int(load().wm2f_poly_workspace(H, W, V))
    if ws_bytes < 0:
        raise ValueError(f"size {(H, W)} outside the built bounds")
    d = torch.from_numpy(packed).pin_memory().to(dev, non_blocking=True)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    o = [0, 2 * V]
    for n in (C + 1, K + 1, K, K, K + 1):
        o.append(o[-1] + n)
    part = [d[o[i]:o[i + 1]] for i in range(6)]
    _launch("wm2f_poly_fill", out, _p(out), H, W, _p(part[0]), V, _p(part[1]), C, _p(part[2]), _p(part[3]), _p(part[4]),
            _p(part[5]), K, n_items, _p(ws), tag="poly_fill")
    return out


def _poly_tables(H: int, W: int, verts, contour_offsets, call_offsets, values):
    """Validated host tables of wm2f_poly_fill packed into one int32 array: verts, contour_offsets, call_offsets,
    values, call_row0, item_offsets.  Returns (packed, (V, C, K, n_items))."""
    import numpy as np
    if H <= 0 or W <= 0:
        raise ValueError(f"out: empty map {(H, W)}")
    if H > _lib.WM2F_POLY_MAX_SIDE or W > _lib.WM2F_POLY_MAX_SIDE:
        raise ValueError(f"out: sides must be <= {_lib.WM2F_POLY_MAX_SIDE}, got {(H, W)}")
    v = _i32_array(verts, "verts", 2)
    co = _i32_array(contour_offsets, "contour_offsets", 1)
    ko = _i32_array(call_offsets, "call_offsets", 1)
    val = _i32_array(values, "values", 1)
    V, C, K = len(v), len(co) - 1, len(ko) - 1
    if C < 0 or K < 0 or co[0] != 0 or co[-1] != V or ko[0] != 0 or ko[-1] != C:
        raise ValueError("offsets must run from 0 to the number of vertices / contours")
    if np.any(np.diff(co) <= 0):
        raise ValueError("every contour needs at least one point")
    if np.any(np.diff(ko) < 0):
        raise ValueError("call_offsets must be non-decreasing")
    if len(val) != K:
        raise ValueError(f"values: expected {K} values, got {len(val)}")
    if V and int(np.abs(v).max()) > _lib.WM2F_POLY_MAX_COORD:
        raise ValueError(f"coordinates must lie within +-{_lib.WM2F_POLY_MAX_COORD}")
    if val.size and (val.min() < -2 ** 31 or val.max() >= 2 ** 31):
        raise ValueError("values must fit int32")
    if V >= 2 ** 31 - 1:
        raise ValueError(f"{V} vertices: at most 2^31 - 2")
    if K == 0:
        return np.zeros(0, dtype=np.int32), (V, C, K, 0)
    # scan-fill rows of each call: [max(0, min y), min(H, max y) - 1] (a row at the bottom vertex is no edge's)
    row0 = np.zeros(K, dtype=np.int64)
    nrow = np.zeros(K, dtype=np.int64)
    vstart = co[ko[:-1]]
    has = co[ko[1:]] > vstart
    if has.any():
        ys = v[:, 1]
        row0[has] = np.maximum(np.minimum.reduceat(ys, vstart[has]), 0)
        top = np.minimum(np.maximum.reduceat(ys, vstart[has]), H)
        nrow[has] = np.maximum(top - row0[has], 0)
    item_offsets = np.concatenate([[0], np.cumsum(nrow)])
    if item_offsets[-1] >= 2 ** 31:
        raise ValueError(f"{int(item_offsets[-1])} (call, row) items: at most 2^31 - 1")
    packed = np.concatenate([v.reshape(-1), co, ko, val, row0, item_offsets]).astype(np.int32)
    return packed, (V, C, K, int(item_offsets[-1]))
