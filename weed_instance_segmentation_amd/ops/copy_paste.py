"""Simple Copy-Paste on a compact batch: select, paste, prune -- three launches, no host round trip."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ._core import _host_desc, _launch, _p, _req


def _rows(v, name: str, B: int, n: int) -> np.ndarray:
    a = np.asarray(v)
    if a.shape != (B, n) or a.dtype.kind not in "iu":
        raise ValueError(f"{name}: expected {B} rows of {n} integers, got shape {a.shape} {a.dtype}")
    return a.astype(np.int64)


def copy_paste(pixel_values: torch.Tensor, maps: torch.Tensor, source, lut, shift, window=None, min_visible=(0, 1),
               ignore_index: int = 255):
    """Pastes instances between the images of one batch (wm2f_copy_paste_select, wm2f_copy_paste, wm2f_copy_paste_prune;
    the rule is the contract comment of include/wm2f.h).  `pixel_values` (B, C, H, W) float32 and `maps` (B, H, W) int32
    on the device; `source` B integers (-1: the image takes nothing, else another image of the batch); `lut` (B, 256)
    integers, lut[b][source id] = the id it is pasted as or -1 (a host array, or an int32 device tensor); `shift` B pairs
    (dy, dx); `window` B pairs (h, w), the destination's un-padded part (None: the whole frame); `min_visible` the
    integers (num, den), 0 <= num <= den <= 1024.  Returns new tensors (pixels, maps, lut_final (B, 256) int32,
    areas (B, 3, 256) int32 = before, after, original); the batch is never written.  Shifts that leave the frame are
    clamped to (+-H, +-W): nothing lands either way.  With num == 0 the prune step has nothing to do and is not launched."""
    pv, m = _req(pixel_values, "pixel_values", torch.float32), _req(maps, "maps", torch.int32)
    if pv.ndim != 4 or m.ndim != 3 or pv.shape[0] != m.shape[0] or pv.shape[2:] != m.shape[1:] or pv.numel() == 0:
        raise ValueError(f"expected pixel_values (B, C, H, W) and maps (B, H, W), got {tuple(pv.shape)} and {tuple(m.shape)}")
    if pv.device != m.device:
        raise ValueError(f"pixel_values is on {pv.device}, maps on {m.device}")
    B, C, H, W = (int(v) for v in pv.shape)
    num, den = (int(v) for v in min_visible)
    if not 0 <= num <= den <= 1024 or den < 1:
        raise ValueError(f"min_visible: expected integers 0 <= num <= den <= 1024, got {min_visible!r}")
    if 0 <= int(ignore_index) <= 254:
        raise ValueError(f"ignore_index = {ignore_index} is an instance id (ids are 0 .. 254)")
    desc = np.zeros((B, _lib.WM2F_COPY_PASTE_DESC_LEN), dtype=np.int64)
    desc[:, 0] = _rows(np.asarray(source).reshape(-1, 1), "source", B, 1)[:, 0]
    desc[:, 1:3] = np.clip(_rows(shift, "shift", B, 2), [-H, -W], [H, W])
    desc[:, 3:5] = (H, W) if window is None else _rows(window, "window", B, 2)
    dev = pv.device
    if isinstance(lut, torch.Tensor) and lut.is_cuda:
        lut_in = _req(lut, "lut", torch.int32)
        if tuple(lut_in.shape) != (B, 256) or lut_in.device != dev:
            raise ValueError(f"lut: expected (B, 256) on {dev}, got {tuple(lut_in.shape)} on {lut_in.device}")
    else:
        host = torch.from_numpy(_rows(lut.numpy() if isinstance(lut, torch.Tensor) else lut, "lut", B, 256).astype(np.int32))
        lut_in = host.pin_memory().to(dev, non_blocking=True)
    d, d_ptr = _host_desc(desc)
    lut_out = torch.empty(B, 256, device=dev, dtype=torch.int32)
    areas = torch.empty(B, 3, 256, device=dev, dtype=torch.int32)
    ws = torch.empty(B, 256, device=dev, dtype=torch.int32)
    out_pv, out_m = torch.empty_like(pv), torch.empty_like(m)
    _launch("wm2f_copy_paste_select", m, _p(m), _p(lut_in), _p(lut_out), _p(areas), _p(ws), d_ptr, B, H, W, num, den,
            tag="copy_paste_select")
    _launch("wm2f_copy_paste", m, _p(pv), _p(m), _p(lut_out), _p(out_pv), _p(out_m), _p(areas), d_ptr, B, C, H, W,
            tag="copy_paste")
    if num > 0:
        _launch("wm2f_copy_paste_prune", m, _p(out_m), _p(areas), B, H, W, num, den, int(ignore_index),
                tag="copy_paste_prune")
    return out_pv, out_m, lut_out, areas
