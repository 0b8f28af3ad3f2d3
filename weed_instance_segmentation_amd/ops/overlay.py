"""Overlays and contours."""
from __future__ import annotations

import torch

from ._core import _id_maps_dtype, _id_maps_size, _launch, _on_gpu, _p, _req


def labelmap_overlay(image: torch.Tensor, maps: torch.Tensor, ids: torch.Tensor | None, n_ids: torch.Tensor | None,
                     rgba: torch.Tensor | None, order: torch.Tensor | None, default_rgba=(0, 0, 0, 0), inner: int = 1,
                     outer: int = 1) -> torch.Tensor:
    """(B, H, W, 3) uint8 pictures and their (B, H, W) id maps (fp32, int32 or uint8) -> the pictures with every listed
    id filled at its alpha and outlined at full colour (wm2f_labelmap_overlay), a new (B, H, W, 3) uint8 tensor.
    `ids` (B, N) int32 ascending with `n_ids` (B) of them valid, `rgba` (B, N, 4) uint8 and `order` (B, N) int32 per
    listed entry (a negative order: fill only); all four None (or N == 0): every pixel takes `default_rgba`."""
    image = _req(image, "image", torch.uint8)
    _on_gpu(maps, "maps")
    maps, dt = _id_maps_dtype(maps, "labelmap_overlay")
    if image.dim() != 4 or image.shape[3] != 3 or maps.shape != image.shape[:3]:
        raise ValueError(f"labelmap_overlay: image (B, H, W, 3) and maps (B, H, W), got {tuple(image.shape)} and {tuple(maps.shape)}")
    B, H, W = _id_maps_size(maps, "labelmap_overlay")
    tables = (ids, n_ids, rgba, order)
    if any(t is None for t in tables) != all(t is None for t in tables):
        raise ValueError("labelmap_overlay: ids, n_ids, rgba and order go together")
    N = 0
    if ids is not None:
        ids, n_ids, order = _req(ids, "ids", torch.int32), _req(n_ids, "n_ids", torch.int32), _req(order, "order", torch.int32)
        rgba = _req(rgba, "rgba", torch.uint8)
        N = int(ids.shape[1]) if ids.dim() == 2 else -1
        if N < 0 or ids.shape[0] != B or n_ids.shape != (B,) or rgba.shape != (B, N, 4) or order.shape != (B, N):
            raise ValueError("labelmap_overlay: ids (B, N), n_ids (B), rgba (B, N, 4) and order (B, N) disagree")
    r, g, b, a = (int(v) for v in default_rgba)
    if not all(0 <= v <= 255 for v in (r, g, b, a)):
        raise ValueError("labelmap_overlay: default_rgba is four bytes")
    out = torch.empty_like(image)
    _launch("wm2f_labelmap_overlay", image, _p(image), _p(maps), dt, _p(ids if N else None), _p(n_ids if N else None),
            _p(rgba if N else None), _p(order if N else None), r | g << 8 | b << 16 | a << 24, int(inner), int(outer), _p(out), B,
            H, W, N, tag="labelmap_overlay")
    return out
