"""Image and label-map preprocessing, and the training augmentation (DESIGN sections 20 and 29)."""
from __future__ import annotations

import torch

from .. import _lib
from ._core import _dtype_code, _host_desc, _launch, _on_gpu, _p, _req


def resize_normalize_u8(images: torch.Tensor, desc, tables: torch.Tensor, lut: torch.Tensor, Hp: int, Wp: int):
    """Packed uint8 HWC images (flat, on the device) -> (pixel_values (B, 3, Hp, Wp) float32, pixel_mask (B, Hp, Wp)
    int64) through Pillow's fixed-point bilinear resample and a (3, 256) float32 lookup table (include/wm2f.h).
    `desc` is a host int64 array (B, 12): in_off, ws_off, H, W, h, w, tx, cx, kx, ty, cy, ky; `tables` int32 on the
    device.  The uint8 intermediate lives in a workspace of sum(H * w * 3) bytes allocated here."""
    images, tables, lut = _req(images, "images", torch.uint8), _req(tables, "tables", torch.int32), _req(lut, "lut", torch.float32)
    d, d_ptr = _host_desc(desc)
    B = int(d.shape[0])
    ws_bytes = int((d[:, 2] * d[:, 5] * 3).sum())
    dev = images.device
    ws = torch.empty(max(ws_bytes, 1), device=dev, dtype=torch.uint8)
    pv = torch.empty(B, 3, Hp, Wp, device=dev, dtype=torch.float32)
    pm = torch.empty(B, Hp, Wp, device=dev, dtype=torch.int64)
    _launch("wm2f_resize_normalize_u8", images, _p(images), images.numel(), d_ptr,
            _p(tables), tables.numel(), _p(lut), _p(ws), ws.numel(), _p(pv), _p(pm), B, Hp, Wp)
    return pv, pm


def resize_nearest_labels(maps: torch.Tensor, desc, tables: torch.Tensor, Hp: int, Wp: int, ignore_index: int):
    """Packed uint8 or int32 id maps (flat, on the device) -> (maps (B, Hp, Wp) int32 padded with `ignore_index`,
    present (B, 256) uint8 flags of the id values inside each image) through host-built nearest index tables.
    `desc` is a host int64 array (B, 7): in_off, H, W, h, w, xi, yi."""
    _on_gpu(maps, "maps")
    dtype = _dtype_code(maps, (torch.uint8, torch.int32), f"maps must be uint8 or int32, got {maps.dtype}")
    tables = _req(tables, "tables", torch.int32)
    d, d_ptr = _host_desc(desc)
    B = int(d.shape[0])
    out = torch.empty(B, Hp, Wp, device=maps.device, dtype=torch.int32)
    present = torch.empty(B, 256, device=maps.device, dtype=torch.uint8)
    _launch("wm2f_resize_nearest_labels", maps, _p(maps.contiguous()), dtype, maps.numel(),
            d_ptr, _p(tables), tables.numel(), _p(out), _p(present), B, Hp, Wp,
            int(ignore_index))
    return out, present


def augment_resize_normalize_u8(images: torch.Tensor, desc, tables: torch.Tensor, lut: torch.Tensor, Hp: int, Wp: int):
    """Flip, resize and crop of packed uint8 HWC images (flat, on the device) in one launch
    (wm2f_augment_resize_normalize_u8): (pixel_values (B, 3, Hp, Wp) float32, pixel_mask (B, Hp, Wp) int64), bit for bit
    what `resize_normalize_u8` makes of the mirrored image, cut to the window and padded.  `desc` is a host int64 array
    (B, 16): in_off, H, W, h, w, tx, cx, kx, ty, cy, ky, flip, y0, x0, ch, cw; `tables` holds the whole tables of the
    (H, W) -> (h, w) resize.  No workspace: the (h, w) frame is never stored."""
    images, tables, lut = _req(images, "images", torch.uint8), _req(tables, "tables", torch.int32), _req(lut, "lut", torch.float32)
    d, d_ptr = _host_desc(desc)
    if d.ndim != 2 or d.shape[1] != _lib.WM2F_AUG_PRE_DESC_LEN:
        raise ValueError(f"desc: expected (B, {_lib.WM2F_AUG_PRE_DESC_LEN}), got {d.shape}")
    B = int(d.shape[0])
    dev = images.device
    pv = torch.empty(B, 3, Hp, Wp, device=dev, dtype=torch.float32)
    pm = torch.empty(B, Hp, Wp, device=dev, dtype=torch.int64)
    _launch("wm2f_augment_resize_normalize_u8", images, _p(images), images.numel(),
            d_ptr, _p(tables), tables.numel(), _p(lut), _p(pv), _p(pm), B, Hp, Wp)
    return pv, pm


def augment_nearest_labels(maps: torch.Tensor, desc, tables: torch.Tensor, Hp: int, Wp: int, ignore_index: int):
    """Flip, nearest resize and crop of packed uint8 or int32 id maps (wm2f_augment_nearest_labels): (maps (B, Hp, Wp)
    int32 padded with `ignore_index`, present (B, 256) uint8 flags of the id values inside each window).  `desc` is a
    host int64 array (B, 12): in_off, H, W, h, w, xi, yi, flip, y0, x0, ch, cw."""
    _on_gpu(maps, "maps")
    dtype = _dtype_code(maps, (torch.uint8, torch.int32), f"maps must be uint8 or int32, got {maps.dtype}")
    tables = _req(tables, "tables", torch.int32)
    d, d_ptr = _host_desc(desc)
    if d.ndim != 2 or d.shape[1] != _lib.WM2F_AUG_LAB_DESC_LEN:
        raise ValueError(f"desc: expected (B, {_lib.WM2F_AUG_LAB_DESC_LEN}), got {d.shape}")
    B = int(d.shape[0])
    out = torch.empty(B, Hp, Wp, device=maps.device, dtype=torch.int32)
    present = torch.empty(B, 256, device=maps.device, dtype=torch.uint8)
    _launch("wm2f_augment_nearest_labels", maps, _p(maps.contiguous()), dtype, maps.numel(),
            d_ptr, _p(tables), tables.numel(), _p(out), _p(present), B, Hp, Wp,
            int(ignore_index))
    return out, present


def photometric_u8(images: torch.Tensor, desc) -> torch.Tensor:
    """Colour jitter of packed uint8 HWC images (flat, on the device) IN PLACE (wm2f_photometric_u8):
    per image a chain of at most four of brightness, contrast, saturation and hue, byte for byte what Pillow's
    ImageEnhance and HSV conversions give.  `desc` is a host int64 array (B, 12): in_off, H, W, n_ops, then four (kind,
    parameter) pairs, the parameter being the float32 factor's bit pattern or the hue byte dh.  Returns `images`.  The
    (B,) int64 workspace of the contrast sums is allocated here; nothing synchronises with the host."""
    _on_gpu(images, "images")
    if images.dtype != torch.uint8 or not images.is_contiguous():
        raise TypeError(f"images: expected a contiguous uint8 tensor (it is written in place), got {images.dtype}")
    d, d_ptr = _host_desc(desc)
    if d.ndim != 2 or d.shape[1] != _lib.WM2F_PHOTO_DESC_LEN:
        raise ValueError(f"desc: expected (B, {_lib.WM2F_PHOTO_DESC_LEN}), got {d.shape}")
    B = int(d.shape[0])
    ws = torch.empty(max(B, 1), device=images.device, dtype=torch.int64)
    _launch("wm2f_photometric_u8", images, _p(images), images.numel(), d_ptr, _p(ws), B)
    return images


def _orient_desc(desc):
    d, d_ptr = _host_desc(desc)
    if d.ndim != 2 or d.shape[1] != _lib.WM2F_ORIENT_DESC_LEN:
        raise ValueError(f"desc: expected (B, {_lib.WM2F_ORIENT_DESC_LEN}), got {d.shape}")
    return d, d_ptr


def orient_u8(src: torch.Tensor, dst: torch.Tensor, desc) -> torch.Tensor:
    """Vertical flip, quarter turns and rotation of packed uint8 HWC images (flat, on the device) from `src` into `dst`
    (wm2f_orient_u8), byte for byte what Pillow's transpose and rotate(BILINEAR) give.  `desc` is a
    host int64 array (B, 22): in_off, H, W, out_off (bytes), vflip, turns, affine, six float64 bit patterns of the
    matrix, six fixed-point terms, the fill bytes r, g, b (`RotateParams.desc_row`).  One launch; `src` and `dst` must
    not overlap.  Returns `dst`."""
    _on_gpu(src, "src"), _on_gpu(dst, "dst")
    if src.dtype != torch.uint8 or dst.dtype != torch.uint8 or not src.is_contiguous() or not dst.is_contiguous():
        raise TypeError(f"src, dst: expected contiguous uint8 tensors, got {src.dtype}, {dst.dtype}")
    if src.device != dst.device:
        raise ValueError(f"src is on {src.device}, dst on {dst.device}")
    d, d_ptr = _orient_desc(desc)
    _launch("wm2f_orient_u8", src, _p(src), src.numel(), _p(dst), dst.numel(), d_ptr, int(d.shape[0]))
    return dst


def orient_labels(src: torch.Tensor, dst: torch.Tensor, desc) -> torch.Tensor:
    """The same for packed uint8 or int32 id maps (wm2f_orient_labels_u8 / _i32): Pillow's transpose and
    rotate(NEAREST).  Offsets count elements; the fill is the id in column 19.  Returns `dst`."""
    _on_gpu(src, "src"), _on_gpu(dst, "dst")
    _dtype_code(src, (torch.uint8, torch.int32), f"src must be uint8 or int32, got {src.dtype}")
    if dst.dtype != src.dtype or not src.is_contiguous() or not dst.is_contiguous():
        raise TypeError(f"src, dst: expected contiguous tensors of one dtype, got {src.dtype}, {dst.dtype}")
    if src.device != dst.device:
        raise ValueError(f"src is on {src.device}, dst on {dst.device}")
    d, d_ptr = _orient_desc(desc)
    symbol = "wm2f_orient_labels_u8" if src.dtype == torch.uint8 else "wm2f_orient_labels_i32"
    _launch(symbol, src, _p(src), src.numel(), _p(dst), dst.numel(), d_ptr, int(d.shape[0]))
    return dst
