"""Colour on the GPU: per-plant colour traits of a segmentation result, read from the picture under
its id map, and the classical label-free vegetation mask -- a linear vegetation index, Otsu's threshold, a mask.

    from weed_instance_segmentation_amd import ColorOptions, color_statistics, annotate_colors, vegetation_masks
    traits = color_statistics(prediction["segmentation"], image, n=n)         # image: (H, W, 3) uint8
    traits["mean_rgb"], traits["vegetation_fraction"], traits["dominant_hue"]
    result = annotate_colors(result, image)                                    # the traits on every segments_info entry

    masks, cover = vegetation_masks(images, ColorOptions(index="exg"), return_cover=True)   # (B, H, W) uint8, (B) float64
    num_labels, labels = connected_components(masks[0])                        # the mask as an instance map, cv2's numbering
    # labels feeds clean_label_maps, MeanIoU and treatment_grid as any id map does

An index is I = a R + b G + c B with small integer coefficients ("exg": 2G - R - B, Woebbecke's excess green; "exr5":
7R - 5G, five times the excess red 1.4R - G; "exgr5": 5 (ExG - ExR); or any three integers with |a| + |b| + |c| <= 32).
csrc/color.hip sums, per instance and in one read of map and picture, the ten first and second moments of R, G, B --
which give the mean and the variance of ANY linear index exactly --, the pixels above the threshold, the Q12 normalised
index, the dark and the bright pixels and a histogram of an integer hue.  The integers are exact and bit-identical from
run to run; the float traits are a few float64 operations on them (`color_from_sums`).  A "plant" whose pixels are
soil-coloured (vegetation_fraction near 0) is a false positive no shape trait sees.

Otsu's threshold is exact: the index histogram comes from the device (one small copy), the maximisation runs on the host
in Python integers, fractions compared by cross-multiplication.

Not done here: no illumination correction, no CIELab, no per-instance medians or index histograms, no NIR channel; the
hue is the project's own integer hue, not Pillow's float HSV (`adjust_colors`); Otsu looks at the whole picture, never at
a region.
"""
from __future__ import annotations

import dataclasses
import warnings

import numpy as np
import torch

from . import _lib, ops
from .instances import _id_maps
from .ops.color import INDEX_PRESETS, index_coefficients, index_range  # noqa: F401

# what `annotate_colors` writes into a `segments_info` entry
COLOR_TRAITS = ("mean_rgb", "std_rgb", "index_mean", "index_std", "index_normalised_mean", "vegetation_fraction",
                "dark_fraction", "bright_fraction", "dominant_hue", "hue_histogram")
_SCALAR_TRAITS = COLOR_TRAITS[2:9]


def _integer(v, lo: int, hi: int, what: str) -> None:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}], got {v!r}")


@dataclasses.dataclass(frozen=True)
class ColorOptions:
    """How `color_statistics`, `annotate_colors`, `vegetation_threshold` and `vegetation_masks` read a picture.

    - `index`: "exg", "exr5", "exgr5" or three integers (a, b, c), not all zero, |a| + |b| + |c| <= 32.
    - `threshold`: "otsu" (per picture, exact, one small host copy) or an integer in index units; a pixel is vegetation
      when its index is ABOVE the threshold.
    - `hue_bins` in [1, 36], a divisor of 360: the bins of the hue histogram.
    - `min_chroma` in [1, 255]: a pixel with max - min of R, G, B below it has no hue.
    - `dark`, `bright` in [0, 255]: a pixel is dark when max(R, G, B) < dark, bright when max(R, G, B) >= bright."""
    index: object = "exg"
    threshold: object = "otsu"
    hue_bins: int = 12
    min_chroma: int = 16
    dark: int = 32
    bright: int = 250

    def __post_init__(self):
        index_coefficients(self.index, "ColorOptions")
        t = self.threshold
        is_int = isinstance(t, (int, np.integer)) and not isinstance(t, (bool, np.bool_))
        if not (t == "otsu" if isinstance(t, str) else is_int and -2 ** 31 <= t < 2 ** 31):
            raise ValueError(f"ColorOptions: threshold must be 'otsu' or an int32, got {t!r}")
        _integer(self.hue_bins, 1, ops.color.MAX_HUE_BINS, "ColorOptions: hue_bins")
        if 360 % self.hue_bins:
            raise ValueError(f"ColorOptions: hue_bins must divide 360, got {self.hue_bins}")
        _integer(self.min_chroma, 1, 255, "ColorOptions: min_chroma")
        _integer(self.dark, 0, 255, "ColorOptions: dark")
        _integer(self.bright, 0, 255, "ColorOptions: bright")

    @property
    def coefficients(self) -> tuple:
        return index_coefficients(self.index, "ColorOptions")

    @property
    def bins(self) -> int:
        return index_range(self.coefficients)[0]

    @property
    def index_min(self) -> int:
        return index_range(self.coefficients)[1]


def _options(options, who: str) -> ColorOptions:
    if options is None:
        return ColorOptions()
    if not isinstance(options, ColorOptions):
        raise TypeError(f"{who}: options must be a ColorOptions, got {type(options).__name__}")
    return options


def otsu_threshold(hist, index_min: int = 0):
    """Otsu's threshold of one histogram (a sequence of bin counts), exact: the smallest bin t in [0, bins - 2] with both
    classes non-empty that maximises (S n0 - s0 n)^2 / (n0 (n - n0)) -- n0 and s0 the count and the bin-sum of the bins
    <= t, n and S the totals --, fractions compared by cross-multiplication in Python integers.  Returns t + index_min, in
    index units, or None when no t separates two classes (a picture of one value, or an empty histogram)."""
    h = [int(v) for v in hist]
    n = sum(h)
    S = sum(t * v for t, v in enumerate(h))
    best, best_num, best_den = None, 0, 1
    n0 = s0 = 0
    for t in range(len(h) - 1):
        n0 += h[t]
        s0 += t * h[t]
        if n0 == 0:
            continue
        if n0 == n:
            break
        num, den = (S * n0 - s0 * n) ** 2, n0 * (n - n0)
        if best is None or num * best_den > best_num * den:
            best, best_num, best_den = t, num, den
    return None if best is None else best + int(index_min)


def _device():
    if not torch.cuda.is_available():
        raise _lib.Wm2fError("the colour kernels run on a GPU only (no CPU fallback): no device is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _picture_stack(images, who: str):
    """One (H, W, 3) picture or a (B, H, W, 3) stack, uint8, numpy or torch, host or device -> (tensor, single), not yet
    moved."""
    t = torch.from_numpy(np.ascontiguousarray(images)) if isinstance(images, np.ndarray) else images
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3 or 0 in t.shape:
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: pictures are uint8 (H, W, 3) or (B, H, W, 3), got {got}")
    return t, t.dim() == 3


def _thresholds(stack: torch.Tensor, options: ColorOptions):
    """((B) int32 on the device, flat): the option's integer, or Otsu's threshold of every picture (the one host copy);
    flat lists the pictures of one index value, which have no Otsu threshold.  The public caller warns (`_warn_flat`), so
    that the warning points at the user's line."""
    B = int(stack.shape[0])
    if not isinstance(options.threshold, str):
        return torch.full((B,), int(options.threshold), dtype=torch.int32, device=stack.device), []
    coef = options.coefficients
    bins, imin = index_range(coef)
    hist = ops.image_index_hist(stack, coef).cpu().numpy()  # the host copy
    out, flat = [], []
    for i in range(B):
        t = otsu_threshold(hist[i].tolist(), imin)
        if t is None:
            flat.append(i)
            t = imin - 1 + bins  # the largest value: nothing is above it
        out.append(t)
    return torch.tensor(out, dtype=torch.int32).to(stack.device), flat


def _warn_flat(flat, who: str) -> None:
    """Called by a public function directly: stacklevel 3 is that function's caller."""
    if flat:
        warnings.warn(f"{who}: image(s) {flat} hold one value of the index; Otsu has no threshold there and nothing is "
                      "vegetation in them", RuntimeWarning, stacklevel=3)


def vegetation_threshold(images, options: ColorOptions | None = None) -> torch.Tensor:
    """The threshold of every picture of a (B, H, W, 3) uint8 stack (or of one (H, W, 3) picture: a 0-d tensor), in index
    units, int32 on the device: `options.threshold` itself, or with "otsu" Otsu's exact threshold of the picture's index
    histogram -- one launch, one host copy of B x bins counts, the maximisation in Python integers.  A picture of one
    value has no Otsu threshold: it gets the index's largest value, so nothing is vegetation, and a RuntimeWarning names it."""
    options = _options(options, "vegetation_threshold")
    t, single = _picture_stack(images, "vegetation_threshold")
    stack = t.to(t.device if t.is_cuda else _device())
    thr, flat = _thresholds(stack.unsqueeze(0) if single else stack, options)
    _warn_flat(flat, "vegetation_threshold")
    return thr[0] if single else thr


def vegetation_masks(images, options: ColorOptions | None = None, return_cover: bool = False):
    """The vegetation mask of every picture of a (B, H, W, 3) uint8 stack (or of one (H, W, 3) picture): uint8 on the
    device, 1 where the index is above the picture's threshold (`vegetation_threshold`).  `return_cover=True` returns
    (masks, cover): cover float64, the on-pixels over H W -- the canopy cover.

        num_labels, labels = connected_components(vegetation_masks(image))    # plants without a model
    """
    options = _options(options, "vegetation_masks")
    t, single = _picture_stack(images, "vegetation_masks")
    stack = t.to(t.device if t.is_cuda else _device())
    stack = stack.unsqueeze(0) if single else stack
    thr, flat = _thresholds(stack, options)
    _warn_flat(flat, "vegetation_masks")
    mask, counts = ops.image_index_mask(stack, thr, options.coefficients)
    on = counts.to(torch.float64)
    cover = on / torch.full_like(on, float(stack.shape[1] * stack.shape[2]))  # a tensor: a true division, no reciprocal
    if single:
        mask, cover = mask[0], cover[0]
    return (mask, cover) if return_cover else mask


def _centre(s1, area):
    """sum x and the area -> (c, d): the centre c = round(mean) as an integer and d = mean - c in float64."""
    c = torch.div(2 * s1 + area, 2 * area, rounding_mode="floor")
    return c, (s1 - c * area).to(torch.float64) / area.to(torch.float64)


def color_from_sums(sums: torch.Tensor, coef="exg") -> dict:
    """(..., N, 14) int64 rows of `ops.labelmap_color_stats` and the index they were summed under -> a dict of float64
    tensors, NaN for an id without a pixel: "mean_rgb" and "std_rgb" (..., N, 3) (the population standard deviation),
    "index_mean" and "index_std" (of I = a R + b G + c B, from the means and the covariance matrix),
    "index_normalised_mean" = sum q / (4096 area), "vegetation_fraction" = n_on / area, "dark_fraction" and
    "bright_fraction"; and "area" (int64).  Pure torch; works on either device.

    Variances do not cancel: with c = round(sum R / area) as an integer, M = sum R^2 - 2 c sum R + c^2 area is exact in
    int64 and var = M / area - ((sum R - c area) / area)^2; the covariances likewise.  A one-colour instance has std 0.0."""
    a3 = index_coefficients(coef, "color_from_sums")
    if sums.dtype != torch.int64 or sums.shape[-1] != ops.color.COLOR_COLUMNS:
        raise ValueError(f"color_from_sums: sums must be (..., {ops.color.COLOR_COLUMNS}) int64, got {sums.dtype} {tuple(sums.shape)}")
    f64 = torch.float64
    area = sums[..., 0]
    some = area > 0
    A = torch.where(some, area, torch.ones_like(area))  # an empty row divides by 1 and is masked below
    Af = A.to(f64)
    s1 = [sums[..., 1 + i] for i in range(3)]
    cd = [_centre(s, A) for s in s1]
    c, d = [v[0] for v in cd], [v[1] for v in cd]
    second = {(0, 0): 4, (1, 1): 5, (2, 2): 6, (0, 1): 7, (0, 2): 8, (1, 2): 9}
    cov = {}
    for (i, j), col in second.items():
        m = sums[..., col] - c[i] * s1[j] - c[j] * s1[i] + c[i] * c[j] * A  # sum (x_i - c_i)(x_j - c_j), exact
        cov[i, j] = cov[j, i] = m.to(f64) / Af - d[i] * d[j]
    nan = torch.full(area.shape, float("nan"), dtype=f64, device=sums.device)
    zero = torch.zeros_like(nan)

    def masked(v):
        return torch.where(some, v, nan)

    mean = [masked(s.to(f64) / Af) for s in s1]
    std = [masked(torch.sqrt(torch.maximum(cov[i, i], zero))) for i in range(3)]
    ivar = sum(a3[i] * a3[j] * cov[i, j] for i in range(3) for j in range(3))
    isum = a3[0] * s1[0] + a3[1] * s1[1] + a3[2] * s1[2]
    return {"area": area, "mean_rgb": torch.stack(mean, -1), "std_rgb": torch.stack(std, -1),
            "index_mean": masked(isum.to(f64) / Af), "index_std": masked(torch.sqrt(torch.maximum(ivar, zero))),
            "index_normalised_mean": masked(sums[..., 11].to(f64) / (4096.0 * Af)),
            "vegetation_fraction": masked(sums[..., 10].to(f64) / Af),
            "dark_fraction": masked(sums[..., 12].to(f64) / Af), "bright_fraction": masked(sums[..., 13].to(f64) / Af)}


def dominant_hue(hue: torch.Tensor) -> torch.Tensor:
    """(..., K) int64 hue histograms -> (...) float64: the centre in degrees of the first largest bin, NaN when the
    histogram is empty."""
    K = int(hue.shape[-1])
    top = hue.max(-1, keepdim=True).values
    first = torch.where(hue == top, torch.arange(K, device=hue.device), K).min(-1).values
    centre = (first.to(torch.float64) + 0.5) * (360.0 / K)
    return torch.where(top[..., 0] > 0, centre, torch.full_like(centre, float("nan")))


def color_statistics(segmentation, images, n: int | None = None, ids=None, options: ColorOptions | None = None) -> dict:
    """The colour traits of every instance of one (H, W) id map under its (H, W, 3) uint8 picture, or of a (B, H, W) stack
    under a (B, H, W, 3) stack (maps, `n` and `ids` as for `instance_statistics`; listed ids must be below 4096; maps and
    pictures on the host are moved to the current GPU).

    Returns a dict of device tensors in the caller's order of ids: what `color_from_sums` returns, each (..., N) or
    (..., N, 3), "hue_histogram" (..., N, hue_bins) int64 and "dominant_hue" (..., N) float64, the centre in degrees of
    the first largest hue bin (NaN when no pixel of the instance reached `min_chroma`).  With `options.threshold` "otsu"
    the pictures' thresholds cost one small host copy (`vegetation_threshold`); with an integer nothing is copied."""
    out, flat = _statistics(segmentation, images, n, ids, _options(options, "color_statistics"), "color_statistics")
    _warn_flat(flat, "color_statistics")
    return out


def _statistics(segmentation, images, n, ids, options: ColorOptions, who: str):
    """(the dict of traits, the pictures without an Otsu threshold)."""
    if (n is None) == (ids is None):
        raise ValueError(f"{who}: give either n (ids 0 .. n-1) or ids")
    seg = _id_maps(segmentation, who)
    pic, single = _picture_stack(images, who)
    if single != (seg.dim() == 2) or tuple(pic.shape[:-1]) != tuple(seg.shape):
        raise ValueError(f"{who}: the pictures {tuple(pic.shape)} do not fit the maps {tuple(seg.shape)}")
    limit = ops.color.MAX_IDS
    order, back = None, None
    if ids is not None:
        raw = [int(v) for v in ids]
        order = sorted(set(raw))
        if len(order) != len(raw):
            raise ValueError(f"{who}: ids must be distinct")
        if order and not 0 <= order[0] <= order[-1] < limit:
            raise ValueError(f"{who}: ids must be in [0, {limit})")
        back = [order.index(v) for v in raw]
    elif not 0 <= int(n) <= limit:
        raise ValueError(f"{who}: n must be in [0, {limit}], got {n}")
    dev = seg.device if seg.is_cuda else (pic.device if pic.is_cuda else _device())
    maps, stack = seg.to(dev), pic.to(dev)
    if single:
        maps, stack = maps.unsqueeze(0), stack.unsqueeze(0)
    B = int(maps.shape[0])
    thr, flat = _thresholds(stack, options)
    kw = dict(index=options.coefficients, dark=int(options.dark), bright=int(options.bright), hue_bins=int(options.hue_bins),
              min_chroma=int(options.min_chroma))
    if ids is None:
        sums, hue = ops.labelmap_color_stats(stack, maps, thr, N=int(n), **kw)
    else:
        R = max(1, len(order))
        ids_t = torch.tensor(order + [0] * (R - len(order)), dtype=torch.int32).expand(B, R).contiguous().to(dev)
        n_ids = torch.full((B,), len(order), dtype=torch.int32).to(dev)
        sums, hue = ops.labelmap_color_stats(stack, maps, thr, ids_t, n_ids, **kw)
        sel = torch.tensor(back, dtype=torch.int64).to(dev)  # the caller's order
        sums, hue = sums[:, sel], hue[:, sel]
    out = color_from_sums(sums, options.coefficients)
    out["hue_histogram"] = hue
    out["dominant_hue"] = dominant_hue(hue)
    return ({k: v[0] for k, v in out.items()} if single else out), flat


def annotate_colors(result, image, options: ColorOptions | None = None):
    """One result of `post_process_instance_segmentation`, `merge_tile_results` or `segment_tiled` (a dict with the
    (H, W) id map as `segmentation`, on the host or the device, and `segments_info`) and its picture (PIL RGB, numpy or
    torch (H, W, 3) uint8, as the renderers take it), or a list of results and a list of as many pictures -> a new dict
    (list) whose `segments_info` entries carry COLOR_TRAITS: floats (NaN for a segment without a pixel), `mean_rgb` and
    `std_rgb` lists of three floats, `hue_histogram` a list of ints.  A picture whose size is not the map's raises.  One
    device-to-host copy per result for the traits (with `options.threshold` "otsu" the histogram behind the threshold is
    a second, small one); the input is not modified."""
    options = _options(options, "annotate_colors")
    if isinstance(result, (list, tuple)):
        if not isinstance(image, (list, tuple)) or len(image) != len(result):
            raise ValueError("annotate_colors: a list of results needs a list of as many pictures")
        done = [_annotate(r, im, options) for r, im in zip(result, image)]
        _warn_flat([i for i, (_, flat) in enumerate(done) if flat], "annotate_colors")
        return [r for r, _ in done]
    out, flat = _annotate(result, image, options)
    _warn_flat(flat, "annotate_colors")
    return out


def _annotate(result, image, options: ColorOptions):
    from .visualize import _picture
    if not isinstance(result, dict) or "segmentation" not in result or "segments_info" not in result:
        raise ValueError("annotate_colors: result must be a dict with 'segmentation' and 'segments_info'")
    seg = _id_maps(result["segmentation"], "annotate_colors")
    if seg.dim() != 2:
        raise ValueError(f"annotate_colors: the segmentation must be (H, W), got {tuple(seg.shape)}")
    pic = _picture(image, image.device if isinstance(image, torch.Tensor) else "cpu")  # coerced and checked, not yet moved
    if tuple(pic.shape[:2]) != tuple(seg.shape):
        raise ValueError(f"annotate_colors: a picture of {tuple(pic.shape[:2])} for a map of {tuple(seg.shape)}")
    wanted = [int(s["id"]) for s in result["segments_info"]]
    if any(i < 0 for i in wanted) or len(set(wanted)) != len(wanted):
        raise ValueError("annotate_colors: segment ids must be distinct and not negative")
    out = dict(result)
    if not wanted:
        out["segments_info"] = []
        return out, []
    traits, flat = _statistics(seg, pic, None, wanted, options, "annotate_colors")
    f64 = torch.float64
    packed = torch.cat([traits["mean_rgb"], traits["std_rgb"], torch.stack([traits[k] for k in _SCALAR_TRAITS], -1),
                        traits["hue_histogram"].to(f64)], -1)  # counts are below 2^53: exact in float64
    host = packed.cpu().numpy()  # the one host copy of the traits
    infos = []
    for info, row in zip(result["segments_info"], host):
        extra = {"mean_rgb": [float(v) for v in row[0:3]], "std_rgb": [float(v) for v in row[3:6]]}
        for k, v in zip(_SCALAR_TRAITS, row[6:6 + len(_SCALAR_TRAITS)]):
            extra[k] = float(v)
        extra["hue_histogram"] = [int(v) for v in row[6 + len(_SCALAR_TRAITS):]]
        infos.append({**info, **{k: extra[k] for k in COLOR_TRAITS}})
    out["segments_info"] = infos
    return out, flat
