"""Colour under id maps and vegetation indices of pictures: per-instance colour sums and hue
histograms, the histogram of a linear index over a picture, and its thresholded mask."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ._core import _id_maps_dtype, _id_maps_size, _id_rows, _launch, _p, _req

COLOR_COLUMNS = _lib.WM2F_COLOR_COLUMNS
COLOR_LDS_MAX_IDS = 240        # wm2f_labelmap_color_stats: accumulators in LDS up to this N, in the result above
MAX_IDS = 4096                 # kMapMaxIds of csrc/labelmap.h: the result rows of one call, and the listed ids lie below it
INDEX_MAX_WEIGHT = _lib.WM2F_COLOR_MAX_WEIGHT
MAX_HUE_BINS = _lib.WM2F_COLOR_MAX_HUE_BINS
# the named indices: Woebbecke's excess green, 5 x excess red (1.4 R - G), 5 x (ExG - ExR)
INDEX_PRESETS = {"exg": (-1, 2, -1), "exr5": (7, -5, 0), "exgr5": (-12, 15, -5)}


def index_coefficients(index, who: str = "index_coefficients") -> tuple:
    """A preset name or three integers -> (a, b, c) of I = a R + b G + c B: not all zero, |a| + |b| + |c| <= 32."""
    if isinstance(index, str):
        if index not in INDEX_PRESETS:
            raise ValueError(f"{who}: unknown index {index!r}, expected one of {tuple(INDEX_PRESETS)} or three integers")
        return INDEX_PRESETS[index]
    try:
        coef = tuple(index)
    except TypeError:
        raise ValueError(f"{who}: an index is a preset name or three integers, got {index!r}") from None
    if len(coef) != 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in coef):
        raise ValueError(f"{who}: an index is a preset name or three integers, got {index!r}")
    coef = tuple(int(v) for v in coef)
    weight = sum(abs(v) for v in coef)
    if not 1 <= weight <= INDEX_MAX_WEIGHT:
        raise ValueError(f"{who}: the coefficients must not all be zero and |a| + |b| + |c| <= {INDEX_MAX_WEIGHT}, got {coef}")
    return coef


def index_range(index) -> tuple:
    """(bins, Imin) of an index: it takes the bins values Imin .. Imin + bins - 1, and a pixel's bin is I - Imin."""
    coef = index_coefficients(index, "index_range")
    return 255 * sum(abs(v) for v in coef) + 1, -255 * sum(-v for v in coef if v < 0)


def _typed(t, name: str, dtypes, who: str) -> None:
    """The refusals of this module are Wm2fError (not on a GPU) or ValueError, a wrong dtype included."""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        got = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: {name} must be a tensor of {' / '.join(str(d) for d in dtypes)}, got {got}")


def _pictures(images, who: str) -> torch.Tensor:
    _typed(images, "images", (torch.uint8,), who)
    images = _req(images, "images", torch.uint8)
    if images.dim() != 4 or images.shape[3] != 3 or 0 in images.shape:
        raise ValueError(f"{who}: images must be (B, H, W, 3) and not empty, got {tuple(images.shape)}")
    return images


def _thresholds(thresholds, B: int, device, who: str) -> torch.Tensor:
    _typed(thresholds, "thresholds", (torch.int32,), who)
    thresholds = _req(thresholds, "thresholds", torch.int32)
    if thresholds.shape != (B,) or thresholds.device != device:
        raise ValueError(f"{who}: thresholds must be ({B},) int32 on the pictures' device, got {tuple(thresholds.shape)} "
                         f"on {thresholds.device}")
    return thresholds


def labelmap_color_stats(images: torch.Tensor, maps: torch.Tensor, thresholds: torch.Tensor,
                         ids: torch.Tensor | None = None, n_ids: torch.Tensor | None = None, N: int | None = None,
                         index="exg", dark: int = 32, bright: int = 250, hue_bins: int | None = 12, min_chroma: int = 16):
    """(B, H, W, 3) uint8 pictures and their (B, H, W) id maps (fp32 with -1 background, int32 or uint8) -> (sums, hue)
    (wm2f_labelmap_color_stats): sums (B, N, 14) int64 per id over the pixels that carry it
    [area, sum R, G, B, sum R^2, G^2, B^2, sum RG, RB, GB, n_on, sum q, n_dark, n_bright] with I = a R + b G + c B the
    `index`, n_on the pixels with I > thresholds[b] (`thresholds` (B) int32 on the device),
    q = floor(4096 I / (R + G + B)), n_dark those with max(R, G, B) < dark and n_bright those with max(R, G, B) >= bright;
    hue (B, N, hue_bins) int64, the pixels with chroma >= min_chroma per bin of the integer hue (None with
    hue_bins=None).  An id without a pixel has all-zero rows.  `ids` / `n_ids` / `N` as in `labelmap_instance_stats`."""
    who = "labelmap_color_stats"
    images = _pictures(images, who)
    _typed(maps, "maps", (torch.float32, torch.int32, torch.uint8), who)
    maps, dt = _id_maps_dtype(maps, who, "tensors")
    if maps.shape != images.shape[:3] or maps.device != images.device:
        raise ValueError(f"{who}: images (B, H, W, 3) and maps (B, H, W) on one device, got {tuple(images.shape)} and "
                         f"{tuple(maps.shape)}")
    B, H, W = _id_maps_size(maps, who)
    ids, n_ids, N = _id_rows(who, B, ids, n_ids, N)
    a, b, c = index_coefficients(index, who)
    thresholds = _thresholds(thresholds, B, images.device, who)
    dark, bright = int(dark), int(bright)
    if not (0 <= dark <= 255 and 0 <= bright <= 255):
        raise ValueError(f"{who}: dark and bright are bytes, got {dark} and {bright}")
    K = 0
    if hue_bins is not None:
        K, min_chroma = int(hue_bins), int(min_chroma)
        if not 1 <= K <= MAX_HUE_BINS or 360 % K:
            raise ValueError(f"{who}: hue_bins must divide 360 and be in [1, {MAX_HUE_BINS}], got {hue_bins}")
        if not 1 <= min_chroma <= 255:
            raise ValueError(f"{who}: min_chroma must be in [1, 255], got {min_chroma}")
    sums = torch.empty(B, N, COLOR_COLUMNS, device=images.device, dtype=torch.int64)
    hue = torch.empty(B, N, K, device=images.device, dtype=torch.int64) if K else None
    if N == 0:
        return sums, hue
    _launch("wm2f_labelmap_color_stats", images, _p(images), _p(maps), dt, _p(ids), _p(n_ids), a, b, c, _p(thresholds), dark,
            bright, K, int(min_chroma) if K else 0, _p(sums), _p(hue), B, H, W, N, tag="color_stats")
    return sums, hue


def image_index_hist(images: torch.Tensor, index="exg") -> torch.Tensor:
    """(B, H, W, 3) uint8 pictures -> (B, bins) int64 (wm2f_image_index_hist): how many pixels take every value of the
    index I = a R + b G + c B; column j is the value Imin + j (`index_range`)."""
    images = _pictures(images, "image_index_hist")
    a, b, c = index_coefficients(index, "image_index_hist")
    B, H, W = (int(v) for v in images.shape[:3])
    hist = torch.empty(B, index_range((a, b, c))[0], device=images.device, dtype=torch.int64)
    _launch("wm2f_image_index_hist", images, _p(images), a, b, c, _p(hist), B, H, W, tag="index_hist")
    return hist


def image_index_mask(images: torch.Tensor, thresholds: torch.Tensor, index="exg"):
    """(B, H, W, 3) uint8 pictures and `thresholds` (B) int32 on the device -> (mask, counts) (wm2f_image_index_mask):
    mask (B, H, W) uint8, 1 where I > thresholds[b], and counts (B) int64, the on-pixels of every picture."""
    images = _pictures(images, "image_index_mask")
    a, b, c = index_coefficients(index, "image_index_mask")
    B, H, W = (int(v) for v in images.shape[:3])
    thresholds = _thresholds(thresholds, B, images.device, "image_index_mask")
    mask = torch.empty(B, H, W, device=images.device, dtype=torch.uint8)
    counts = torch.empty(B, device=images.device, dtype=torch.int64)
    _launch("wm2f_image_index_mask", images, _p(images), a, b, c, _p(thresholds), _p(mask), _p(counts), B, H, W, tag="index_mask")
    return mask, counts
