"""Training augmentation (DESIGN.md sections 20 and 29): random horizontal flip, random scale, fixed-size crop or
short-edge choice, and colour jitter (brightness, contrast, saturation, hue).  Not in the reference, which trains on one
deterministic resize per image.

    from weed_instance_segmentation_amd import TrainAugmentation, AugmentParams

    aug = TrainAugmentation(short_edge=range(640, 801, 32), max_size=1333)        # COCO-style multi-scale
    aug = TrainAugmentation(scale=(0.1, 2.0), crop_size=(1024, 1024))             # large-scale jitter
    params = aug.sample(height, width, generator)                                 # an AugmentParams
    inputs = processor(images=image, segmentation_maps=instance_map, augment=params, pad_size=aug.pad_size, ...)

    aug = TrainAugmentation(scale=(0.1, 2.0), crop_size=(1024, 1024), brightness=0.2, contrast=0.2, saturation=0.2,
                            hue=0.05)                                             # the same, with colour jitter
    out = adjust_colors(image, PhotometricParams((("brightness", 1.2), ("hue", -0.03))))   # outside the processor

`AugmentParams` are explicit and public, so an augmentation can be replayed.  The processor stays deterministic; every
random draw happens in `TrainAugmentation.sample`, from the caller's CPU `torch.Generator`.  The pixels are produced by
csrc/augment.hip, bit for bit what Pillow makes of the flipped, resized, cropped image, and the colours by
csrc/photometric.hip, bit for bit what Pillow's `ImageEnhance` and HSV conversions make of the source image.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass

import torch

from . import _lib

__all__ = ["AugmentParams", "PhotometricParams", "TrainAugmentation", "adjust_colors"]

PHOTOMETRIC_KINDS = ("brightness", "contrast", "saturation", "hue")  # index = the WM2F_PHOTO_* constant
_FLOAT32_MAX = 3.4028234663852886e38


def _pair(v, name: str):
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected a pair of integers, got {v!r}") from None
    for x in (a, b):
        if isinstance(x, bool) or int(x) != x:
            raise ValueError(f"{name}: expected a pair of integers, got {v!r}")
    return int(a), int(b)


def _float32_bits(v: float) -> int:
    return struct.unpack("<I", struct.pack("<f", v))[0]


@dataclass(frozen=True)
class PhotometricParams:
    """One image's colour chain: `ops` = ((kind, value), ...), at most four steps, each kind of "brightness", "contrast",
    "saturation", "hue" at most once, applied left to right to the uint8 source image.  The value of
    the first three is Pillow's enhancement factor f >= 0 (1 leaves the image as it is), used as float32 as Pillow does;
    the value of "hue" is a shift s in [-0.5, 0.5] of the hue circle, applied as the byte `hue_byte()` added to Pillow's
    H channel mod 256.  An empty chain leaves the image untouched."""
    ops: tuple = ()

    def __post_init__(self):
        try:
            steps = [(k, v) for k, v in self.ops]
        except (TypeError, ValueError):
            raise ValueError(f"ops: expected ((kind, value), ...), got {self.ops!r}") from None
        if len(steps) > len(PHOTOMETRIC_KINDS):
            raise ValueError(f"ops: at most {len(PHOTOMETRIC_KINDS)} steps, got {len(steps)}")
        seen, out = set(), []
        for kind, value in steps:
            if kind not in PHOTOMETRIC_KINDS:
                raise ValueError(f"ops: unknown kind {kind!r}, expected one of {PHOTOMETRIC_KINDS}")
            if kind in seen:
                raise ValueError(f"ops: {kind!r} appears more than once")
            seen.add(kind)
            if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
                raise ValueError(f"ops: {kind}: expected a finite number, got {value!r}")
            value = float(value)
            if kind == "hue":
                if not -0.5 <= value <= 0.5:
                    raise ValueError(f"ops: hue shift must lie in [-0.5, 0.5], got {value}")
            elif not 0.0 <= value <= _FLOAT32_MAX:
                raise ValueError(f"ops: {kind} factor must be a float32 >= 0, got {value}")
            out.append((kind, value))
        object.__setattr__(self, "ops", tuple(out))

    def _value(self, kind: str) -> float:
        for k, v in self.ops:
            if k == kind:
                return v
        raise KeyError(f"{kind!r} is not in the chain {tuple(k for k, _ in self.ops)}")

    def factor32(self, kind: str) -> float:
        """The float32 factor the blend of `kind` (brightness, contrast or saturation) uses, as a Python float."""
        if kind == "hue":
            raise ValueError("hue has no blend factor: see hue_byte()")
        return struct.unpack("<f", struct.pack("<f", self._value(kind)))[0]

    def hue_byte(self) -> int:
        """dh = int(shift * 255) mod 256 (Python's int, truncation toward zero): the byte added to H."""
        return int(self._value("hue") * 255) % 256

    def desc_row(self, in_off: int, height: int, width: int) -> list:
        """The image's row of wm2f_photometric_u8's host descriptor (include/wm2f.h)."""
        row = [int(in_off), int(height), int(width), len(self.ops)]
        for kind, value in self.ops:
            row += [PHOTOMETRIC_KINDS.index(kind), self.hue_byte() if kind == "hue" else _float32_bits(value)]
        return row + [0] * (_lib.WM2F_PHOTO_DESC_LEN - len(row))


@dataclass(frozen=True)
class AugmentParams:
    """One image's augmentation: `flip` (0 or 1, a horizontal mirror of the source, applied before the resize), `size` =
    (h, w) of the resized frame, `origin` = (y0, x0) and `window` = (ch, cw) of the crop inside that frame.  The window
    must lie inside the frame: y0 + ch <= h and x0 + cw <= w.  `photometric`, a `PhotometricParams` or None, is the colour
    chain applied to the source image before the flip and the resize."""
    flip: int
    size: tuple
    origin: tuple = (0, 0)
    window: tuple | None = None
    photometric: PhotometricParams | None = None

    def __post_init__(self):
        if self.photometric is not None and not isinstance(self.photometric, PhotometricParams):
            raise ValueError(f"photometric must be a PhotometricParams or None, got {self.photometric!r}")
        if self.flip not in (0, 1, False, True):
            raise ValueError(f"flip must be 0 or 1, got {self.flip!r}")
        h, w = _pair(self.size, "size")
        y0, x0 = _pair(self.origin, "origin")
        ch, cw = (h, w) if self.window is None else _pair(self.window, "window")
        if h <= 0 or w <= 0:
            raise ValueError(f"size must be positive, got {(h, w)}")
        if ch <= 0 or cw <= 0:
            raise ValueError(f"window must be positive, got {(ch, cw)}")
        if y0 < 0 or x0 < 0 or y0 + ch > h or x0 + cw > w:
            raise ValueError(f"window {(ch, cw)} at origin {(y0, x0)} lies outside the {(h, w)} frame")
        object.__setattr__(self, "flip", int(self.flip))
        object.__setattr__(self, "size", (h, w))
        object.__setattr__(self, "origin", (y0, x0))
        object.__setattr__(self, "window", (ch, cw))

    @classmethod
    def identity(cls, height: int, width: int) -> "AugmentParams":
        """No flip and the whole (height, width) frame: equals the processor's size={'height', 'width'} call."""
        return cls(0, (height, width))


class TrainAugmentation:
    """Draws `AugmentParams` for an image of a given size.  Exactly one of the two recipes:

    - `short_edge=(640, 672, ..., 800), max_size=1333`: COCO-style multi-scale.  One entry is chosen uniformly; (h, w)
      is the processor's `output_size` for {'shortest_edge': entry, 'longest_edge': max_size} and `size_divisor` (give it
      the processor's).  No crop: the window is the frame, and `pad_size` is None (the batch's largest window).
    - `scale=(lo, hi), crop_size=(Ch, Cw)`: large-scale jitter.  f is uniform in [lo, hi]; r = min(Ch f / H, Cw f / W);
      (h, w) = (max(1, round(H r)), max(1, round(W r))); the window is (min(Ch, h), min(Cw, w)) at an origin uniform over
      the integer positions that fit; `pad_size` is (Ch, Cw).

    `sample` takes four draws from the generator, always in this order and always all four: the flip (one float32
    uniform, flip when it is below `flip_prob`), then the edge index (randint) or f (one float64 uniform), then y0, then x0
    (randint over the positions that fit, one position when there is no crop).  The same seed gives the same parameters on
    any machine.

    Colour jitter: `brightness`, `contrast`, `saturation` and `hue`, each None (off), a number or a
    (lo, hi) pair.  A number b means the factor range [max(0, 1 - b), 1 + b]; for hue a number h <= 0.5 means the shift
    range [-h, h]; a pair is the range itself (factors >= 0, shifts inside [-0.5, 0.5]).  With all four None `sample`
    takes exactly the four draws above and returns `photometric=None`.  Otherwise it takes, AFTER those four, one
    `torch.randperm(4)` for the order of the chain and then one float64 uniform each for brightness, contrast, saturation
    and hue, in that order of names and always all four, whether or not the kind is switched on.  Kinds left None are
    dropped from the chain; the others appear in the permutation's order (entry k of the permutation names the k-th of
    brightness, contrast, saturation, hue).  So a seed gives the same geometry with and without colour jitter."""

    def __init__(self, short_edge=None, max_size: int = 1333, scale=None, crop_size=None, flip_prob: float = 0.5,
                 size_divisor: int = 32, brightness=None, contrast=None, saturation=None, hue=None):
        if (short_edge is None) == (scale is None):
            raise ValueError("give exactly one of short_edge=(...) and scale=(lo, hi)")
        if not 0.0 <= float(flip_prob) <= 1.0:
            raise ValueError(f"flip_prob must lie in [0, 1], got {flip_prob}")
        self.flip_prob = float(flip_prob)
        self.size_divisor = int(size_divisor)
        self.short_edge = self.scale = self.crop_size = None
        self.max_size = int(max_size)
        if short_edge is not None:
            if crop_size is not None:
                raise ValueError("crop_size belongs to the scale=(lo, hi) recipe")
            edges = [short_edge] if isinstance(short_edge, int) else list(short_edge)
            if not edges or any(isinstance(e, bool) or int(e) != e or int(e) <= 0 for e in edges):
                raise ValueError(f"short_edge: expected positive integers, got {short_edge!r}")
            if self.max_size <= 0:
                raise ValueError(f"max_size must be positive, got {max_size}")
            self.short_edge = tuple(int(e) for e in edges)
        else:
            lo, hi = (float(v) for v in scale)
            if not 0.0 < lo <= hi:
                raise ValueError(f"scale: expected 0 < lo <= hi, got {scale!r}")
            if crop_size is None:
                raise ValueError("scale=(lo, hi) needs crop_size=(Ch, Cw)")
            Ch, Cw = _pair(crop_size, "crop_size")
            if Ch <= 0 or Cw <= 0:
                raise ValueError(f"crop_size must be positive, got {crop_size!r}")
            self.scale, self.crop_size = (lo, hi), (Ch, Cw)
        self.color_ranges = tuple(self._color_range(name, v) for name, v in
                                  zip(PHOTOMETRIC_KINDS, (brightness, contrast, saturation, hue)))

    @staticmethod
    def _color_range(name: str, v):
        """None, or the (lo, hi) range of a colour argument."""
        if v is None:
            return None
        lo_bound, hi_bound = (-0.5, 0.5) if name == "hue" else (0.0, _FLOAT32_MAX)
        try:
            if isinstance(v, (int, float)) and not isinstance(v, bool):
                b = float(v)
                if not b >= 0.0:
                    raise ValueError
                lo, hi = (-b, b) if name == "hue" else (max(0.0, 1.0 - b), 1.0 + b)
            else:
                lo, hi = (float(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: expected None, a number >= 0 or a (lo, hi) pair, got {v!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo_bound <= lo <= hi <= hi_bound):
            raise ValueError(f"{name}: the range {(lo, hi)} must satisfy {lo_bound} <= lo <= hi <= {hi_bound}")
        return lo, hi

    @property
    def pad_size(self):
        """The processor's `pad_size` for this recipe: {'height': Ch, 'width': Cw} for the jitter, None otherwise."""
        if self.crop_size is None:
            return None
        return {"height": self.crop_size[0], "width": self.crop_size[1]}

    def sample(self, height: int, width: int, generator: torch.Generator | None = None) -> AugmentParams:
        H, W = int(height), int(width)
        if H <= 0 or W <= 0:
            raise ValueError(f"image size must be positive, got {(height, width)}")
        if generator is not None and generator.device.type != "cpu":
            raise ValueError("generator must be a CPU torch.Generator")
        flip = int(torch.rand(1, generator=generator).item() < self.flip_prob)
        if self.short_edge is not None:
            from .preprocess import output_size
            edge = self.short_edge[int(torch.randint(len(self.short_edge), (1,), generator=generator).item())]
            h, w = output_size(H, W, {"shortest_edge": edge, "longest_edge": self.max_size}, self.size_divisor)
            ch, cw = h, w
        else:
            lo, hi = self.scale
            f = lo + (hi - lo) * float(torch.rand(1, dtype=torch.float64, generator=generator).item())
            Ch, Cw = self.crop_size
            r = min(Ch * f / H, Cw * f / W)
            h, w = max(1, int(round(H * r))), max(1, int(round(W * r)))
            ch, cw = min(Ch, h), min(Cw, w)
        y0 = int(torch.randint(h - ch + 1, (1,), generator=generator).item())
        x0 = int(torch.randint(w - cw + 1, (1,), generator=generator).item())
        photometric = None
        if any(r is not None for r in self.color_ranges):
            order = torch.randperm(len(PHOTOMETRIC_KINDS), generator=generator).tolist()
            u = [float(torch.rand(1, dtype=torch.float64, generator=generator).item()) for _ in PHOTOMETRIC_KINDS]
            # min(): lo + (hi - lo) u can round one ulp above hi
            photometric = PhotometricParams(tuple(
                (PHOTOMETRIC_KINDS[k], min(self.color_ranges[k][0] + (self.color_ranges[k][1] - self.color_ranges[k][0]) * u[k],
                                           self.color_ranges[k][1]))
                for k in order if self.color_ranges[k] is not None))
        return AugmentParams(flip, (h, w), (y0, x0), (ch, cw), photometric)


def adjust_colors(images, params, device="cuda"):
    """The colour chain(s) `params` on the GPU (csrc/photometric.hip), byte for byte what Pillow gives.
    `images`: one (H, W, 3) uint8 image (torch tensor on host or device, numpy array or PIL RGB image) or a list of them;
    `params`: one `PhotometricParams` for every image or a list with one per image.  Returns new uint8 (H, W, 3) device
    tensors (one tensor for one image, a list for a list); the inputs are never written.  Host images are copied to
    `device`, or to the device of the first image that already lives on a GPU."""
    from . import ops
    from .preprocess import _image_hwc_u8
    single = not isinstance(images, (list, tuple))
    ims = [_image_hwc_u8(im, i) for i, im in enumerate([images] if single else list(images))]
    if not ims:
        raise ValueError("images is empty")
    ps = list(params) if isinstance(params, (list, tuple)) else [params] * len(ims)
    if len(ps) != len(ims) or not all(isinstance(p, PhotometricParams) for p in ps):
        raise ValueError(f"params: expected one PhotometricParams or a list of {len(ims)}, one per image")
    if not torch.cuda.is_available():
        raise _lib.Wm2fError("adjust_colors: the wm2f kernels run on a GPU only (no CPU fallback)")
    _lib.load()
    dev = next((im.device for im in ims if isinstance(im, torch.Tensor) and im.is_cuda), torch.device(device))
    if dev.type != "cuda":
        raise _lib.Wm2fError(f"device={device}: the wm2f kernels run on a GPU only (no CPU fallback)")
    import numpy as np
    sizes = [tuple(int(v) for v in im.shape[:2]) for im in ims]
    off = [0]
    for H, W in sizes:
        off.append(off[-1] + H * W * 3)
    buf = torch.empty(off[-1], dtype=torch.uint8, device=dev)
    for b, im in enumerate(ims):
        t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.array(im))  # a copy: PIL's arrays are read-only
        buf[off[b]:off[b + 1]].copy_(t.reshape(-1), non_blocking=True)
    desc = np.array([p.desc_row(off[b], *sizes[b]) for b, p in enumerate(ps)], dtype=np.int64)
    ops.photometric_u8(buf, desc)
    out = [buf[off[b]:off[b + 1]].view(H, W, 3) for b, (H, W) in enumerate(sizes)]
    if single:
        return out[0]
    return [o.clone() for o in out]  # each result owns its memory, not a slice of the batch buffer
