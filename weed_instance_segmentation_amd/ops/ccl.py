"""Connected components of class maps and the table-driven nearest resize."""
from __future__ import annotations

import ctypes

import torch

from .. import _lib
from .._lib import load
from ._core import _dtype_code, _launch, _on_gpu, _p

_CCL_DTYPES = (torch.uint8, torch.bool, torch.uint16, torch.int32)


def _index_table(t, n: int, name: str, dev) -> torch.Tensor:
    t = torch.as_tensor(t, dtype=torch.int32)
    if t.shape != (n,):
        raise ValueError(f"{name}: expected {n} source indices, got shape {tuple(t.shape)}")
    return t.to(dev).contiguous()


def label_components(src: torch.Tensor, mode: int, size=None, ty=None, tx=None, colors=None, skip_255: bool = True,
                     background: int = 255):
    """Connected components (8-connectivity, same nonzero class) of a class map on the device, numbered by
    (class, first 2 x 2 block) as OpenCV numbers them (include/wm2f.h, wm2f_ccl_*).

    `src` is (H, W) uint8 / bool / uint16 / int32 (mode WM2F_CCL_VALUE or WM2F_CCL_BINARY) or (H, W, 3) uint8
    (WM2F_CCL_RGB with `colors`, a sequence of rgb triples).  `size` = (h, w) of the output, read from the source
    through the int32 index tables `ty` (h) and `tx` (w); without them the source size.  Returns
    (out (h, w) int32 ids with `background` outside every component, comp_class (n) int32 device tensor of the
    classes in id order, n)."""
    _on_gpu(src, "src")
    rgb = mode == _lib.WM2F_CCL_RGB
    if rgb:
        if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
            raise TypeError(f"RGB maps are (H, W, 3) uint8, got {tuple(src.shape)} {src.dtype}")
        dt = _lib.WM2F_U8
    else:
        error = f"class maps are (H, W) uint8, bool, uint16 or int32, got {tuple(src.shape)} {src.dtype}"
        if src.dim() != 2:
            raise TypeError(error)
        dt = _dtype_code(src, _CCL_DTYPES, error)
    src = src.contiguous()
    sh, sw = int(src.shape[0]), int(src.shape[1])
    h, w = (sh, sw) if size is None else (int(size[0]), int(size[1]))
    if min(sh, sw, h, w) <= 0:
        raise ValueError(f"empty map: source {(sh, sw)}, output {(h, w)}")
    dev = src.device
    if (ty is None) != (tx is None):
        raise ValueError("give both index tables or neither")
    if ty is None and (h, w) != (sh, sw):
        raise ValueError(f"output size {(h, w)} differs from the source {(sh, sw)}: index tables needed")
    if ty is not None:
        ty, tx = _index_table(ty, h, "ty", dev), _index_table(tx, w, "tx", dev)
    col = None
    n_col = 0
    if rgb:
        flat = [int(c) for rgb3 in colors for c in rgb3]
        n_col = len(flat) // 3
        if n_col == 0 or len(flat) != 3 * n_col or any(not 0 <= c <= 255 for c in flat):
            raise ValueError(f"colors: expected rgb triples of 0..255, got {colors!r}")
        col = (ctypes.c_uint8 * len(flat))(*flat)
    ws_bytes = int(load().wm2f_ccl_workspace(h, w))
    if ws_bytes < 0:
        raise ValueError(f"size {(h, w)} outside the built bounds")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    _launch("wm2f_ccl_label", src, _p(src), int(mode), dt, sh, sw, _p(ty), _p(tx), col, n_col, h, w, _p(ws), _p(count),
            tag="ccl_label")
    n = int(count.item())
    keys = torch.empty(n, device=dev, dtype=torch.int64)
    _launch("wm2f_ccl_keys", src, _p(ws), n, h, w, _p(keys))
    order = torch.sort(keys).indices
    out = torch.empty(h, w, device=dev, dtype=torch.int32)
    comp_class = torch.empty(n, device=dev, dtype=torch.int32)
    _launch("wm2f_ccl_paint", src, _p(ws), _p(order), n, h, w, int(bool(skip_255)), int(background), _p(out), _p(comp_class),
            tag="ccl_paint")
    return out, comp_class, n


def resize_nearest_tables(src: torch.Tensor, ty, tx) -> torch.Tensor:
    """dst[y, x] = src[ty[y], tx[x]] for an (H, W) or (H, W, 3) map of 1-, 2- or 4-byte elements (3-byte pixels for
    (H, W, 3) uint8) on the device; ty / tx int32 index tables (host or device)."""
    _on_gpu(src, "src")
    if src.dim() == 3 and src.shape[2] == 3 and src.dtype == torch.uint8:
        elem = 3
    elif src.dim() == 2 and src.element_size() in (1, 2, 4):
        elem = src.element_size()
    else:
        raise TypeError(f"expected an (H, W) map of 1-, 2- or 4-byte elements or (H, W, 3) uint8, got "
                        f"{tuple(src.shape)} {src.dtype}")
    src = src.contiguous()
    sh, sw = int(src.shape[0]), int(src.shape[1])
    h, w = len(ty), len(tx)
    dev = src.device
    ty, tx = _index_table(ty, h, "ty", dev), _index_table(tx, w, "tx", dev)
    dst = torch.empty((h, w) + tuple(src.shape[2:]), device=dev, dtype=src.dtype)
    if h == 0 or w == 0:
        return dst
    _launch("wm2f_resize_nearest", src, _p(src), elem, sh, sw, _p(ty), _p(tx), _p(dst), h, w)
    return dst
