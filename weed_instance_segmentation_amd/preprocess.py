"""Device-side Mask2Former preprocessing (the image half).

`Mask2FormerImageProcessor` stands where the reference holds its `AutoImageProcessor`
(`datasets/preprocess.py:13`, `train.py:79`, `test.py:23`, `model_utils.py:13`): the call

    inputs = processor(images=image, segmentation_maps=instance_map, instance_id_to_semantic_id=id_to_semantic)

returns what `Mask2FormerImageProcessorPil._preprocess` of transformers 5.15.0
(models/mask2former/image_processing_pil_mask2former.py:485-585) returns -- `pixel_values`, `pixel_mask`,
`mask_labels`, `class_labels` -- bit for bit, but computed on the GPU, and `post_process_instance_segmentation` is the
one of `Mask2FormerInstancePostProcessor`.

What stays on the host is integer and float64 bookkeeping: the output-size rule, Pillow's tap tables (bilinear: start,
count and 22-bit fixed-point coefficients per output column and row; nearest: one source index per output column and
row) and a (3, 256) float32 table of the rescaled, normalised value of every (channel, byte).  These, the uint8 images
and the uint8 maps travel in ONE pinned host buffer per call.  The pixels are touched only by the HIP kernels of
csrc/preprocess.hip (`wm2f_resize_normalize_u8`, `wm2f_resize_nearest_labels`) and `wm2f_labelmap_to_masks`; the
unique ids of the resized maps come back as (B, 256) presence flags in one device-to-host copy.  A call without
`augment` is described as the identity window of the augmentation (no flip, origin (0, 0), the whole resized frame;
DESIGN section 20), so one set of host rows serves both; only the dispatch tells the two pairs of kernels apart.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from . import ops
from ._lib import Wm2fError
from .postprocess import Mask2FormerInstancePostProcessor

IMAGENET_DEFAULT_MEAN = [0.485, 0.456, 0.406]
IMAGENET_DEFAULT_STD = [0.229, 0.224, 0.225]
NEAREST, BILINEAR = 0, 2  # PIL.Image.Resampling values
PRECISION_BITS = 22  # Pillow Resample.c, 8-bit images
CONFIG_NAME = "preprocessor_config.json"
_SETTINGS = ("do_resize", "size", "size_divisor", "resample", "do_rescale", "rescale_factor", "do_normalize",
             "image_mean", "image_std", "ignore_index", "do_reduce_labels", "pad_size", "num_labels")


# ------------------------------------------------------------------------------------------------ host tables
def bilinear_tables(in_size: int, out_size: int):
    """Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` (Resample.c) for the bilinear filter: (out, 2) int32
    (start, count) and (out, k) int32 fixed-point coefficients.  An unchanged size is the identity (Pillow skips that
    pass)."""
    if in_size == out_size:
        idx = np.arange(out_size, dtype=np.int32)
        return np.stack([idx, np.ones_like(idx)], 1), np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5), in_size).astype(np.int64) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = 1.0 - np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((w > 0) & (x < xmax[:, None]), w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):  # left to right, as the C loop adds them
        ww += w[:, j]
    w = np.where(ww[:, None] != 0, w / np.where(ww == 0, 1.0, ww)[:, None], w)
    k = w * float(1 << PRECISION_BITS)
    coef = np.trunc(np.where(k < 0, k - 0.5, k + 0.5)).astype(np.int32)
    return np.stack([xmin, xmax], 1).astype(np.int32), coef


def nearest_table(in_size: int, out_size: int) -> np.ndarray:
    """Pillow's nearest resize (ImagingScaleAffine): the source coordinate is a float64 accumulator that starts at
    scale / 2 and grows by scale per output, truncated."""
    scale = float(in_size) / out_size
    out = np.empty(out_size, dtype=np.int32)
    xo = scale * 0.5
    for i in range(out_size):
        out[i] = min(int(xo), in_size - 1)
        xo += scale
    return out


def _size_with_aspect_ratio(height: int, width: int, size: int, max_size: int | None):
    """transformers.image_transforms.get_size_with_aspect_ratio."""
    raw_size = None
    if max_size is not None:
        mn, mx = float(min(height, width)), float(max(height, width))
        if mx / mn * size > max_size:
            raw_size = max_size * mn / mx
            size = int(round(raw_size))
    if (height <= width and height == size) or (width <= height and width == size):
        return height, width
    if width < height:
        ow = size
        oh = int(raw_size * height / width) if (max_size is not None and raw_size is not None) else int(size * height / width)
        return oh, ow
    oh = size
    ow = int(raw_size * width / height) if (max_size is not None and raw_size is not None) else int(size * width / height)
    return oh, ow


def output_size(height: int, width: int, size: dict, size_divisor: int = 0):
    """The (h, w) an image is resized to (Mask2FormerImageProcessorPil.resize): shortest / longest edge, max height /
    width or an exact size, then each side rounded UP to a multiple of `size_divisor` (a stretch, not padding)."""
    g = lambda k: size.get(k) or None  # noqa: E731
    if g("shortest_edge") and g("longest_edge"):
        h, w = _size_with_aspect_ratio(height, width, size["shortest_edge"], size["longest_edge"])
    elif g("max_height") and g("max_width"):
        s = min(size["max_height"] / height, size["max_width"] / width)
        h, w = int(height * s), int(width * s)
    elif g("height") and g("width"):
        h, w = size["height"], size["width"]
    else:
        raise ValueError(f"Size must contain 'height' and 'width' keys or 'shortest_edge' and 'longest_edge' keys. Got {size}.")
    if size_divisor and size_divisor > 0:
        h = int(math.ceil(h / size_divisor) * size_divisor)
        w = int(math.ceil(w / size_divisor) * size_divisor)
    return h, w


def normalize_table(do_rescale: bool, rescale_factor: float, do_normalize: bool, mean, std) -> np.ndarray:
    """(3, 256) float32: the value byte v of channel c takes after `rescale` (float64 product, cast to float32) and
    `normalize` ((x - mean) / std in float32) of transformers.image_transforms."""
    x = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    if do_rescale:
        x = (x.astype(np.float64) * rescale_factor).astype(np.float32)
    if do_normalize:
        x = x.astype(np.float32) if not np.issubdtype(x.dtype, np.floating) else x
        m = np.array(mean if isinstance(mean, (list, tuple)) else [mean] * 3, dtype=x.dtype)
        s = np.array(std if isinstance(std, (list, tuple)) else [std] * 3, dtype=x.dtype)
        x = (x - m[:, None]) / s[:, None]
    return np.ascontiguousarray(x, dtype=np.float32)


def _size_dict(size, max_size=None) -> dict:
    """get_size_dict(size, max_size, default_to_square=False) of transformers.image_processing_utils."""
    if isinstance(size, dict):
        return dict(size)
    if isinstance(size, int):
        return {"shortest_edge": size, "longest_edge": max_size} if max_size is not None else {"shortest_edge": size}
    if isinstance(size, (list, tuple)) and len(size) == 2:
        return {"height": int(size[0]), "width": int(size[1])}
    if size is None and max_size is not None:
        return {"longest_edge": max_size}
    raise ValueError(f"size must be a dict, an int or a (height, width) pair, got {size!r}")


# ------------------------------------------------------------------------------------------------ inputs
def _is_pil(x) -> bool:
    return type(x).__module__.startswith("PIL.") and hasattr(x, "mode") and hasattr(x, "size")


def _image_hwc_u8(img, i: int):
    """A PIL RGB image, a numpy (H, W, 3) uint8 array or a uint8 torch tensor (H, W, 3) on host or device."""
    if _is_pil(img):
        img = np.asarray(img)
    if isinstance(img, np.ndarray) or isinstance(img, torch.Tensor):
        if tuple(img.shape[2:]) == (3,) and img.ndim == 3 and img.dtype in (np.uint8, torch.uint8) and min(img.shape[:2]) > 0:
            return img
    raise ValueError(f"images[{i}]: expected a PIL RGB image, a numpy (H, W, 3) uint8 array or a uint8 torch tensor "
                     f"(H, W, 3), got {type(img).__name__} {getattr(img, 'shape', '')} {getattr(img, 'dtype', '')}")


def _map_hw_u8(m, i: int, hw):
    """An (H, W) id map (PIL, numpy or torch) -> uint8 (ids outside 0..255 raise, as the dependency's uint8 PIL
    conversion does)."""
    if _is_pil(m):
        m = np.asarray(m)
    if isinstance(m, np.ndarray):
        if m.ndim == 3 and m.shape[0] == 1:
            m = m[0]
        lo, hi = (int(m.min()), int(m.max())) if m.size else (0, 0)
    elif isinstance(m, torch.Tensor):
        if m.ndim == 3 and m.shape[0] == 1:
            m = m[0]
        lo, hi = (int(m.min()), int(m.max())) if m.numel() else (0, 0)
    else:
        raise ValueError(f"segmentation_maps[{i}]: expected a PIL image, a numpy array or a torch tensor (H, W), "
                         f"got {type(m).__name__}")
    if m.ndim != 2 or tuple(m.shape) != tuple(hw):
        raise ValueError(f"segmentation_maps[{i}]: expected shape {tuple(hw)} (its image's), got {tuple(m.shape)}")
    if lo < 0 or hi > 255:
        raise ValueError(f"The image to be converted to a PIL image contains values outside the range [0, 255], got "
                         f"[{lo}, {hi}] which cannot be converted to uint8.")
    return m.astype(np.uint8) if isinstance(m, np.ndarray) else m.to(torch.uint8)


class BatchFeature(dict):
    """The processor's result: a dict with attribute access and `.to(device)` (inference.py:25 calls it)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as e:
            raise AttributeError(name) from e

    def to(self, *args, **kwargs) -> "BatchFeature":
        def mv(v):
            if isinstance(v, torch.Tensor):
                return v.to(*args, **kwargs)
            if isinstance(v, (list, tuple)):
                return type(v)(mv(x) for x in v)
            return v
        return BatchFeature({k: mv(v) for k, v in self.items()})


def _aligned(n: int) -> int:
    return (n + 63) // 64 * 64


def _descriptors(sizes_in, frames, wins, with_maps: bool):
    """The host rows of include/wm2f.h for (H, W) sources resized to (h, w) `frames` and cut to `wins` = (flip, y0, x0,
    ch, cw): (desc (B, 16) int64, ldesc (B, 12) int64, tables int32), column 0 (the input offsets) left 0.  The tables
    are those of the whole frame; the kernels index them at the window's origin."""
    parts, n_tab = [], 0

    def put(a):
        nonlocal n_tab
        a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        off = n_tab
        parts.append(a)
        n_tab += a.size
        return off

    desc = np.zeros((len(sizes_in), 16), dtype=np.int64)
    ldesc = np.zeros((len(sizes_in), 12), dtype=np.int64)
    for b, ((H, W), (h, w)) in enumerate(zip(sizes_in, frames)):
        bx, cx = bilinear_tables(W, w)
        by, cy = bilinear_tables(H, h)
        desc[b, 1:] = [H, W, h, w, put(bx), put(cx), cx.shape[1], put(by), put(cy), cy.shape[1], *wins[b]]
        if with_maps:
            ldesc[b, 1:] = [H, W, h, w, put(nearest_table(W, w)), put(nearest_table(H, h)), *wins[b]]
    return desc, ldesc, np.concatenate(parts)


def _plain_rows(desc: np.ndarray, ldesc: np.ndarray):
    """The rows of `_descriptors` at the identity window as the plain kernels of csrc/preprocess.hip take them: (B, 12)
    with the running workspace offset of the (H, w, 3) intermediates behind column 0, and (B, 7)."""
    ws_off = np.cumsum(desc[:, 1] * desc[:, 4] * 3) - desc[:, 1] * desc[:, 4] * 3
    return np.column_stack([desc[:, 0], ws_off, desc[:, 1:11]]), ldesc[:, :7]


# ------------------------------------------------------------------------------------------------ processor
class Mask2FormerImageProcessor(Mask2FormerInstancePostProcessor):
    """`Mask2FormerImageProcessorPil` of transformers 5.15.0 on the GPU: same keywords and defaults, same outputs bit
    for bit.  Only BILINEAR image resampling is built; the maps always use NEAREST."""

    def __init__(self, do_resize: bool = True, size=None, size_divisor: int = 32, resample: int = BILINEAR,
                 do_rescale: bool = True, rescale_factor: float = 1 / 255, do_normalize: bool = True,
                 image_mean=None, image_std=None, ignore_index: int | None = None, do_reduce_labels: bool = False,
                 pad_size=None, num_labels: int | None = None, max_size: int | None = None, **kwargs):
        if "size_divisibility" in kwargs:  # legacy keys the dependency's configs carry
            size_divisor = kwargs.pop("size_divisibility")
        if "reduce_labels" in kwargs:
            do_reduce_labels = kwargs.pop("reduce_labels")
        if size is None:
            size = {"shortest_edge": 800, "longest_edge": 1333 if max_size is None else max_size}
        self.do_resize = do_resize
        self.size = _size_dict(size, max_size)
        self.size_divisor = size_divisor
        self.resample = int(resample)
        self.do_rescale = do_rescale
        self.rescale_factor = rescale_factor
        self.do_normalize = do_normalize
        self.image_mean = list(IMAGENET_DEFAULT_MEAN if image_mean is None else image_mean)
        self.image_std = list(IMAGENET_DEFAULT_STD if image_std is None else image_std)
        self.ignore_index = ignore_index
        self.do_reduce_labels = do_reduce_labels
        self.pad_size = pad_size
        self.num_labels = num_labels
        self._check(self.resample)

    @staticmethod
    def _check(resample):
        if int(resample) != BILINEAR:
            raise NotImplementedError(f"resample={resample}: only BILINEAR ({BILINEAR}) image resampling is built")

    # ---- configuration files
    def to_dict(self) -> dict:
        d = {k: getattr(self, k) for k in _SETTINGS}
        d["image_processor_type"] = "Mask2FormerImageProcessor"
        return d

    def save_pretrained(self, save_directory: str) -> str:
        """Writes preprocessor_config.json, which the dependency's `from_pretrained` loads to the same settings."""
        os.makedirs(save_directory, exist_ok=True)
        path = os.path.join(save_directory, CONFIG_NAME)
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2, sort_keys=True)
        return path

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, **kwargs) -> "Mask2FormerImageProcessor":
        """A local directory holding preprocessor_config.json (hub names cannot be fetched: FileNotFoundError)."""
        d = str(pretrained_model_name_or_path)
        if not os.path.isdir(d):
            raise FileNotFoundError(f"{d} is not a local directory: this package loads processor settings from a "
                                    f"directory holding {CONFIG_NAME} (no hub access)")
        path = os.path.join(d, CONFIG_NAME)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"no {CONFIG_NAME} in {d}")
        with open(path) as f:
            cfg = json.load(f)
        known = set(_SETTINGS) | {"max_size", "size_divisibility", "reduce_labels"}
        args = {k: v for k, v in cfg.items() if k in known}
        args.update(kwargs)
        return cls(**args)

    # ---- the call
    def __call__(self, images, segmentation_maps=None, instance_id_to_semantic_id=None, **kwargs) -> BatchFeature:
        return self.preprocess(images, segmentation_maps, instance_id_to_semantic_id, **kwargs)

    def preprocess(self, images, segmentation_maps=None, instance_id_to_semantic_id=None, return_tensors="pt",
                   device="cuda", mask_dtype: torch.dtype = torch.float32, augment=None,
                   return_instance_maps: bool = False, **overrides) -> BatchFeature:
        """`augment`: None, one `AugmentParams` for every image or a list with one per image.  With
        parameters each image is mirrored (flip), resized to the parameters' own (h, w) -- `size` and `size_divisor` do
        not apply -- and cut to the window; `pad_size` defaults to the batch's largest window.  Parameters that carry a
        `photometric` chain have it applied to the source image first, on the call's private device
        copy: the caller's tensors are never written, and maps and labels do not see it.  Parameters that carry a
        `rotate` with something enabled have image and map oriented next (vertical flip, quarter turns, rotation; DESIGN
        section 30), one launch each into a second region of the private buffer; `size`, `origin` and `window` then
        refer to the turned frame, and `map_fill` is a raw id, written as if before `do_reduce_labels`.  The call stays
        deterministic: the draws are `TrainAugmentation.sample`'s.
        `return_instance_maps=True` (with `segmentation_maps`): the result also carries `instance_maps`, the processed
        (B, Hp, Wp) int32 id map `mask_labels` are made from, padded with `ignore_index` -- what a compact sample stores
        and `copy_paste` works on."""
        unknown = set(overrides) - set(_SETTINGS)
        if unknown:
            raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
        s = {k: overrides.get(k, getattr(self, k)) for k in _SETTINGS}
        s["size"] = _size_dict(s["size"])
        self._check(s["resample"])
        if return_tensors not in ("pt", None):
            raise ValueError(f"return_tensors={return_tensors!r}: only 'pt' is supported")
        if mask_dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"mask_dtype must be torch.float32 or torch.uint8, got {mask_dtype}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise Wm2fError(f"device={device}: the wm2f kernels run on a GPU only (no CPU fallback)")
        ims = list(images) if isinstance(images, (list, tuple)) else [images]
        if not ims:
            raise ValueError("images is empty")
        ims = [_image_hwc_u8(im, i) for i, im in enumerate(ims)]
        augs = None
        if augment is not None:
            from .augment import AugmentParams
            augs = list(augment) if isinstance(augment, (list, tuple)) else [augment] * len(ims)
            if len(augs) != len(ims) or not all(isinstance(a, AugmentParams) for a in augs):
                raise ValueError(f"augment: expected one AugmentParams or a list of {len(ims)}, one per image")
            if not s["do_resize"]:
                raise ValueError("augment needs do_resize=True: the parameters carry the resized size")
        maps = None
        if segmentation_maps is not None:
            maps = list(segmentation_maps) if isinstance(segmentation_maps, (list, tuple)) else [segmentation_maps]
            if len(maps) != len(ims):
                raise ValueError("Images and segmentation maps must have the same length.")
            maps = [_map_hw_u8(m, i, im.shape[:2]) for i, (m, im) in enumerate(zip(maps, ims))]
            if s["do_reduce_labels"]:
                if s["ignore_index"] is None:
                    raise ValueError("If `do_reduce_labels` is True, `ignore_index` must be provided.")
                ig = int(s["ignore_index"])
                maps = [np.where(m == 0, ig, m - 1).astype(np.int64) if isinstance(m, np.ndarray)
                        else torch.where(m == 0, ig, m.to(torch.int64) - 1) for m in maps]
                maps = [_map_hw_u8(m, i, m.shape) for i, m in enumerate(maps)]
        B = len(ims)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())

        sizes_src = [tuple(int(v) for v in im.shape[:2]) for im in ims]  # as stored
        # orientation: the resize, the tables and the window see the turned frame
        orient = augs is not None and any(a.rotate is not None and a.rotate.enabled for a in augs)
        sizes_in = [a.rotate.out_size(H, W) if a.rotate is not None else (H, W)
                    for a, (H, W) in zip(augs, sizes_src)] if orient else sizes_src
        if augs is not None:
            frames = [a.size for a in augs]
            sizes_out = [a.window for a in augs]  # what the image occupies in the padded output
            wins = [[a.flip, *a.origin, *a.window] for a in augs]
        else:  # the identity window: no flip, the whole resized frame
            frames = sizes_out = [output_size(H, W, s["size"], s["size_divisor"]) if s["do_resize"] else (H, W)
                                  for H, W in sizes_in]
            wins = [[0, 0, 0, h, w] for h, w in frames]
        if s["pad_size"] is not None:
            ps = s["pad_size"]
            Hp, Wp = (int(ps["height"]), int(ps["width"])) if isinstance(ps, dict) else (int(ps[0]), int(ps[1]))
        else:
            Hp, Wp = max(h for h, _ in sizes_out), max(w for _, w in sizes_out)
        for h, w in sizes_out:
            if h > Hp or w > Wp:
                raise ValueError(f"Padding dimensions are negative. Please make sure that the padded size is larger than "
                                 f"the original size. Got padded size: {(Hp, Wp)}, original size: {(h, w)}.")

        desc, ldesc, tables = _descriptors(sizes_in, frames, wins, maps is not None)
        lut = normalize_table(s["do_rescale"], s["rescale_factor"], s["do_normalize"], s["image_mean"], s["image_std"])

        # one pinned buffer: tables | lut | host images | host maps
        img_bytes = [H * W * 3 for H, W in sizes_in]
        map_bytes = [H * W for H, W in sizes_in] if maps is not None else []
        o_lut = _aligned(tables.nbytes)
        o_img = o_lut + _aligned(lut.nbytes)
        img_off = np.cumsum([0] + img_bytes)
        o_map = o_img + _aligned(int(img_off[-1]))
        map_off = np.cumsum([0] + map_bytes)
        total = o_map + _aligned(int(map_off[-1]) if maps is not None else 0)
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hb = host.numpy()
        hb[:tables.nbytes] = tables.view(np.uint8)
        hb[o_lut:o_lut + lut.nbytes] = lut.reshape(-1).view(np.uint8)
        on_dev = []
        for b, im in enumerate(ims):
            if isinstance(im, torch.Tensor) and im.is_cuda:
                on_dev.append((o_img + int(img_off[b]), im))
            else:
                a = im.numpy() if isinstance(im, torch.Tensor) else im
                hb[o_img + int(img_off[b]):o_img + int(img_off[b + 1])] = np.ascontiguousarray(a).reshape(-1)
        if maps is not None:
            for b, m in enumerate(maps):
                if isinstance(m, torch.Tensor) and m.is_cuda:
                    on_dev.append((o_map + int(map_off[b]), m))
                else:
                    a = m.numpy() if isinstance(m, torch.Tensor) else m
                    hb[o_map + int(map_off[b]):o_map + int(map_off[b + 1])] = np.ascontiguousarray(a).reshape(-1)
        if orient:  # a second region behind the first: oriented images | oriented maps, device only
            o_rimg = total
            o_rmap = o_rimg + _aligned(int(img_off[-1]))
            buf = torch.empty(o_rmap + _aligned(int(map_off[-1]) if maps is not None else 0), dtype=torch.uint8, device=dev)
            buf[:total].copy_(host, non_blocking=True)
        else:
            buf = host.to(dev, non_blocking=True)
        for off, t in on_dev:
            buf[off:off + t.numel()].copy_(t.to(dev).reshape(-1))
        desc[:, 0] = img_off[:-1]
        t_tab = buf[:tables.nbytes].view(torch.int32)
        t_lut = buf[o_lut:o_lut + lut.nbytes].view(torch.float32)
        if augs is not None and any(a.photometric is not None and a.photometric.ops for a in augs):
            # colour jitter: in place on the private copy, before the flip and the resize read it
            from .augment import PhotometricParams
            none = PhotometricParams()
            pdesc = np.array([(a.photometric or none).desc_row(int(img_off[b]), *sizes_src[b]) for b, a in enumerate(augs)],
                             dtype=np.int64)
            ops.photometric_u8(buf[o_img:o_img + int(img_off[-1])], pdesc)
        if orient:
            # one launch from the first region into the second; images with nothing enabled are copied, and every offset
            # stays what it was, so the kernels below only read another region
            from .augment import RotateParams
            rots = [a.rotate or RotateParams() for a in augs]
            odesc = np.array([r.desc_row(int(img_off[b]), *sizes_src[b], int(img_off[b])) for b, r in enumerate(rots)],
                             dtype=np.int64)
            ops.orient_u8(buf[o_img:o_img + int(img_off[-1])], buf[o_rimg:o_rimg + int(img_off[-1])], odesc)
            o_img = o_rimg
        # One descriptor layout up to here.  The plain call keeps kernels of its own only because they measured faster
        # than the identity window of the augmentation kernels at field-image sizes.
        resize_images, resize_labels = ops.augment_resize_normalize_u8, ops.augment_nearest_labels
        if augs is None:
            resize_images, resize_labels = ops.resize_normalize_u8, ops.resize_nearest_labels
            desc, ldesc = _plain_rows(desc, ldesc)
        pv, pm = resize_images(buf[o_img:o_img + int(img_off[-1])], desc, t_tab, t_lut, Hp, Wp)
        out = BatchFeature(pixel_values=pv, pixel_mask=pm)
        if maps is None:
            return out

        # labels: nearest resize + presence flags, one flag copy, masks per image
        ig = s["ignore_index"]
        ldesc[:, 0] = map_off[:-1]
        if orient:
            odesc = np.array([r.desc_row(int(map_off[b]), *sizes_src[b], int(map_off[b]), labels=True)
                              for b, r in enumerate(rots)], dtype=np.int64)
            # map_fill is a raw id: the maps in the buffer are already reduced, so the fill is reduced the same way
            fills = odesc[:, 19]
            if s["do_reduce_labels"]:
                fills = np.where(fills == 0, int(ig), fills - 1)
            if fills.min() < 0 or fills.max() > 255:
                raise ValueError(f"map_fill: the ids {sorted(set(fills.tolist()))} do not all fit the uint8 id maps")
            odesc[:, 19] = fills
            ops.orient_labels(buf[o_map:o_map + int(map_off[-1])], buf[o_rmap:o_rmap + int(map_off[-1])], odesc)
            o_map = o_rmap
        lab, present = resize_labels(buf[o_map:o_map + int(map_off[-1])], ldesc, t_tab, Hp, Wp,
                                     255 if ig is None else int(ig))
        flags = present.cpu().numpy()
        id_maps = instance_id_to_semantic_id
        mask_labels, class_labels = [], []
        n = Hp * Wp
        for b, (h, w) in enumerate(sizes_out):
            ids = np.flatnonzero(flags[b])
            if ig is not None:
                ids = ids[ids != int(ig)]
            if (h, w) != (Hp, Wp) and ig is None:
                raise ValueError("Unsupported format: None (padding mask_labels needs ignore_index, as in the "
                                 "dependency)")
            if ids.size:
                t_ids = torch.from_numpy(ids.astype(np.int32)).to(dev, non_blocking=True)
                m = lab[b].reshape(1, n)
                if n % 4:
                    m = torch.cat([m, m.new_full((1, 4 - n % 4), -1)], 1)
                masks = ops.labelmap_to_masks(m, t_ids)[:, 0, :n].reshape(-1, Hp, Wp)
            else:
                masks = torch.empty(0, Hp, Wp, device=dev, dtype=torch.uint8)
            masks = masks.to(mask_dtype)
            if (h, w) != (Hp, Wp):
                if mask_dtype == torch.uint8 and not 0 <= int(ig) <= 255:
                    raise ValueError(f"ignore_index {ig} does not fit mask_dtype=torch.uint8")
                masks[:, h:, :] = int(ig)
                masks[:, :h, w:] = int(ig)
            im = id_maps[b] if isinstance(id_maps, (list, tuple)) else id_maps
            if im is not None:
                lut_ids = {int(k): int(v) for k, v in im.items()}
                if s["do_reduce_labels"]:
                    cls = [lut_ids[int(i) + 1] - 1 for i in ids]
                else:
                    cls = [lut_ids[int(i)] for i in ids]
            else:
                cls = [int(i) for i in ids]
            mask_labels.append(masks)
            class_labels.append(torch.tensor(cls, dtype=torch.int64).to(dev, non_blocking=True))
        out["mask_labels"] = mask_labels
        out["class_labels"] = class_labels
        if return_instance_maps:
            out["instance_maps"] = lab
        return out
