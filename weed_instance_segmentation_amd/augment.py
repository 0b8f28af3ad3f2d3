"""Training augmentation (DESIGN.md sections 20, 29 and 30): random horizontal flip, random scale, fixed-size crop or
short-edge choice, colour jitter (brightness, contrast, saturation, hue) and orientation (vertical flip, quarter turns,
rotation by any angle).  Not in the reference, which trains on one deterministic resize per image.

    from weed_instance_segmentation_amd import TrainAugmentation, AugmentParams

    aug = TrainAugmentation(short_edge=range(640, 801, 32), max_size=1333)        # COCO-style multi-scale
    aug = TrainAugmentation(scale=(0.1, 2.0), crop_size=(1024, 1024))             # large-scale jitter
    params = aug.sample(height, width, generator)                                 # an AugmentParams
    inputs = processor(images=image, segmentation_maps=instance_map, augment=params, pad_size=aug.pad_size, ...)

    aug = TrainAugmentation(scale=(0.1, 2.0), crop_size=(1024, 1024), brightness=0.2, contrast=0.2, saturation=0.2,
                            hue=0.05)                                             # the same, with colour jitter
    out = adjust_colors(image, PhotometricParams((("brightness", 1.2), ("hue", -0.03))))   # outside the processor

    aug = TrainAugmentation(scale=(0.1, 2.0), crop_size=(1024, 1024), vflip_prob=0.5, quarter_turns=True, rotate=15,
                            fill=(124, 116, 104), map_fill=255)                   # top-down imagery: any orientation
    out = rotate_images(image, RotateParams(vflip=True, turns=1, angle=13.37))    # outside the processor

    recipe = CopyPaste(prob=0.5, select=0.5, classes=(1,), min_visible=0.25)      # Simple Copy-Paste between the images
    batch = CopyPasteBatcher(recipe, generator)(collate_fn(compact_items))        # of a compact batch (data.py, section 31)

`AugmentParams` are explicit and public, so an augmentation can be replayed.  The processor stays deterministic; every
random draw happens in `TrainAugmentation.sample`, from the caller's CPU `torch.Generator`.  The pixels are produced by
csrc/augment.hip, bit for bit what Pillow makes of the flipped, resized, cropped image, and the colours by
csrc/photometric.hip, bit for bit what Pillow's `ImageEnhance` and HSV conversions make of the source image, and the
orientation by csrc/orient.hip, bit for bit what Pillow's `transpose` and `rotate` make of image and id map.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass

import torch

from . import _lib

__all__ = ["AugmentParams", "CopyPaste", "CopyPasteParams", "PhotometricParams", "RotateParams", "TrainAugmentation",
           "adjust_colors", "allocate_paste_ids", "rotate_images", "rotate_maps"]

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


def _float64_bits(v: float) -> int:
    return struct.unpack("<q", struct.pack("<d", v))[0]


def _fix(v: float) -> int:
    """Pillow's FIX: floor(v * 65536.0 + 0.5), as a Python integer."""
    return math.floor(v * 65536.0 + 0.5)


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


@dataclass(frozen=True)
class RotateParams:
    """One image's orientation, applied to the source image and its id map in this order, each step
    only when enabled: `vflip` (Pillow's FLIP_TOP_BOTTOM), `turns` in 0 .. 3 counter-clockwise quarter turns (ROTATE_90,
    ROTATE_180, ROTATE_270; 1 and 3 swap the frame of a non-square image to (W, H)), then `angle` in degrees when
    angle % 360 != 0: `rotate(angle, BILINEAR, expand=False, fillcolor=fill)` for the image and
    `rotate(angle, NEAREST, expand=False, fillcolor=map_fill)` for the map, counter-clockwise, the frame keeping its
    size.  `fill` is three bytes, `map_fill` a raw id (the processor writes it before `do_reduce_labels`)."""
    vflip: bool = False
    turns: int = 0
    angle: float = 0.0
    fill: tuple = (0, 0, 0)
    map_fill: int = 0

    def __post_init__(self):
        if not (isinstance(self.vflip, bool) or (_is_int(self.vflip) and self.vflip in (0, 1))):
            raise ValueError(f"vflip must be a bool, got {self.vflip!r}")
        if not _is_int(self.turns) or not 0 <= self.turns <= 3:
            raise ValueError(f"turns must be an integer in 0 .. 3, got {self.turns!r}")
        if isinstance(self.angle, bool) or not isinstance(self.angle, (int, float)) or not math.isfinite(self.angle):
            raise ValueError(f"angle must be a finite number of degrees, got {self.angle!r}")
        try:
            fill = tuple(self.fill)
        except TypeError:
            fill = ()
        if len(fill) != 3 or not all(_is_int(c) and 0 <= c <= 255 for c in fill):
            raise ValueError(f"fill must be three bytes (r, g, b), got {self.fill!r}")
        if not _is_int(self.map_fill) or not -2 ** 31 <= self.map_fill < 2 ** 31:
            raise ValueError(f"map_fill must be an int32 id, got {self.map_fill!r}")
        object.__setattr__(self, "vflip", bool(self.vflip))
        object.__setattr__(self, "angle", float(self.angle))
        object.__setattr__(self, "fill", fill)

    @property
    def enabled(self) -> bool:
        """Whether any of the three steps changes the image."""
        return self.vflip or self.turns != 0 or self.angle % 360.0 != 0

    def out_size(self, height: int, width: int) -> tuple:
        """The (H, W) of the oriented frame of a stored (height, width) image: swapped by an odd number of turns."""
        return (int(width), int(height)) if self.turns & 1 else (int(height), int(width))

    def matrix(self, height: int, width: int) -> list:
        """The six float64 entries `Image.rotate` hands to the affine transform for a (height, width) frame -- the frame
        the rotation reads, that is the TURNED frame -- computed in Python floats exactly as Pillow does."""
        a = -math.radians(self.angle % 360.0)
        m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
        cx, cy = width / 2.0, height / 2.0
        m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
        m[2] += cx
        m[5] += cy
        return m

    def fixed(self, height: int, width: int) -> list:
        """Pillow's 16.16 terms a0 .. a5 of the nearest-neighbour transform for the same frame, as Python integers."""
        m = self.matrix(height, width)
        return [_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
                _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]

    def folded(self, height: int, width: int) -> tuple:
        """(turns, affine) as the kernels take them for a stored (height, width) image.  Pillow routes angle % 360 of 0 and
        180, and of 90 and 270 on a square frame, to `transpose`; those are folded into the turn and `affine` is False."""
        h, w = self.out_size(height, width)
        a = self.angle % 360.0
        if a == 0:
            return self.turns, False
        if a == 180:
            return (self.turns + 2) % 4, False
        if a in (90, 270) and h == w:
            return (self.turns + (1 if a == 90 else 3)) % 4, False
        return self.turns, True

    def desc_row(self, in_off: int, height: int, width: int, out_off: int, labels: bool = False) -> list:
        """The image's row of wm2f_orient_u8's host descriptor, or with labels=True of wm2f_orient_labels_*'s
        (include/wm2f.h); (height, width) is the stored size."""
        turns, affine = self.folded(height, width)
        h, w = self.out_size(height, width)
        m, fx = (self.matrix(h, w), self.fixed(h, w)) if affine else ([0.0] * 6, [0] * 6)
        fill = [self.map_fill, 0, 0] if labels else list(self.fill)
        return [int(in_off), int(height), int(width), int(out_off), int(self.vflip), turns, int(affine),
                *[_float64_bits(v) for v in m], *fx, *fill]


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
    chain applied to the source image before the flip and the resize.  `rotate`, a `RotateParams` or None, is the
    orientation (vertical flip, quarter turns, rotation) applied after the colour chain and before the flip and the
    resize; `size`, `origin` and `window` then refer to the turned frame."""
    flip: int
    size: tuple
    origin: tuple = (0, 0)
    window: tuple | None = None
    photometric: PhotometricParams | None = None
    rotate: RotateParams | None = None

    def __post_init__(self):
        if self.rotate is not None and not isinstance(self.rotate, RotateParams):
            raise ValueError(f"rotate must be a RotateParams or None, got {self.rotate!r}")
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
    brightness, contrast, saturation, hue).  So a seed gives the same geometry with and without colour jitter.

    Orientation: `vflip_prob` (the probability of a vertical flip), `quarter_turns` (True: a uniform
    number of counter-clockwise quarter turns in 0 .. 3) and `rotate` (None, a number d for an angle uniform in [-d, d]
    degrees, or a (lo, hi) pair); `fill` and `map_fill` are what the rotation writes where it reads outside the image and
    the id map.  With all three off `sample` takes no new draw and returns `rotate=None`.  With any of them on it takes
    three draws BEFORE all the others, always all three and in this order: one float32 uniform (vertical flip when it is
    below `vflip_prob`), one randint(4) (the turns), one float64 uniform (the angle); draws of options that are off are
    discarded.  They come first because the turned frame is the (H, W) that decides (h, w) and the ranges of y0 and x0: a
    recipe with orientation on therefore gives a seed ANOTHER geometry than the same recipe without."""

    def __init__(self, short_edge=None, max_size: int = 1333, scale=None, crop_size=None, flip_prob: float = 0.5,
                 size_divisor: int = 32, brightness=None, contrast=None, saturation=None, hue=None,
                 vflip_prob: float = 0.0, quarter_turns: bool = False, rotate=None, fill=(0, 0, 0), map_fill: int = 0):
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
        if not 0.0 <= float(vflip_prob) <= 1.0:
            raise ValueError(f"vflip_prob must lie in [0, 1], got {vflip_prob}")
        if not isinstance(quarter_turns, bool):
            raise ValueError(f"quarter_turns must be a bool, got {quarter_turns!r}")
        self.vflip_prob, self.quarter_turns = float(vflip_prob), quarter_turns
        self.rotate_range = self._angle_range(rotate)
        self._orient_base = RotateParams(fill=fill, map_fill=map_fill)  # validates the two fills
        self.fill, self.map_fill = self._orient_base.fill, map_fill

    @staticmethod
    def _angle_range(v):
        """None, or the (lo, hi) range of the angle in degrees."""
        if v is None:
            return None
        try:
            if isinstance(v, (int, float)) and not isinstance(v, bool):
                d = float(v)
                if not d >= 0.0:
                    raise ValueError
                lo, hi = -d, d
            else:
                lo, hi = (float(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"rotate: expected None, a number >= 0 or a (lo, hi) pair of degrees, got {v!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            raise ValueError(f"rotate: the range {(lo, hi)} must be finite with lo <= hi")
        return lo, hi

    @property
    def orients(self) -> bool:
        """Whether any of vertical flip, quarter turns and rotation is switched on."""
        return self.vflip_prob > 0.0 or self.quarter_turns or self.rotate_range is not None

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
        rotate = None
        if self.orients:
            u_flip = float(torch.rand(1, generator=generator).item())
            k = int(torch.randint(4, (1,), generator=generator).item())
            u_angle = float(torch.rand(1, dtype=torch.float64, generator=generator).item())
            angle = 0.0
            if self.rotate_range is not None:
                lo, hi = self.rotate_range
                angle = min(lo + (hi - lo) * u_angle, hi)
            rotate = RotateParams(u_flip < self.vflip_prob, k if self.quarter_turns else 0, angle, self.fill, self.map_fill)
            H, W = rotate.out_size(H, W)  # everything below sees the turned frame
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
        return AugmentParams(flip, (h, w), (y0, x0), (ch, cw), photometric, rotate)


def _instance_ids(id_mapping) -> list:
    """The ascending instance ids (0 .. 254) among the keys of one image's id -> class dictionary."""
    return sorted(k for k in (int(k) for k in id_mapping) if 0 <= k <= 254)


def allocate_paste_ids(selected, dest_id_mapping) -> tuple:
    """The ids `selected` (ascending source ids) are pasted as: the k-th gets the k-th smallest value of 0 .. 254 that is
    not a key of the destination's id -> class dictionary.  255 is never handed out.  With more selected ids than free
    values the result is shorter than `selected`: the surplus, the highest source ids, is not pasted."""
    taken = {int(k) for k in dest_id_mapping}
    free = (v for v in range(255) if v not in taken)
    return tuple(v for _, v in zip(selected, free))


@dataclass(frozen=True)
class CopyPasteParams:
    """One batch's copy-paste, explicit so that it can be replayed.  Per destination image b:
    `source[b]` (-1: nothing is pasted, else the index of ANOTHER image of the batch), `selected[b]` (the source ids to
    paste, ascending, each in 0 .. 254; empty without source), `new_ids[b]` (what they are pasted as: entry k belongs to
    selected[b][k]; it may be shorter than `selected[b]`, the surplus is not pasted; its values are distinct and in
    0 .. 254) and `shift[b]` = (dy, dx) in whole pixels.  `min_visible` in [0, 1] is the share of its area an instance must
    keep: a pasted one after the shift has clipped it, a destination one after the paste has covered it.  It is applied
    as the integers `fraction()` = Fraction(min_visible).limit_denominator(1024)."""
    source: tuple
    selected: tuple
    new_ids: tuple
    shift: tuple
    min_visible: float = 0.0

    def __post_init__(self):
        try:
            source = tuple(self.source)
            selected = tuple(tuple(s) for s in self.selected)
            new_ids = tuple(tuple(s) for s in self.new_ids)
            shift = tuple(self.shift)
        except TypeError:
            raise ValueError("source, selected, new_ids and shift must be sequences with one entry per image") from None
        B = len(source)
        if not (len(selected) == len(new_ids) == len(shift) == B):
            raise ValueError(f"source, selected, new_ids and shift must have one entry per image, got lengths "
                             f"{B}, {len(selected)}, {len(new_ids)}, {len(shift)}")
        for b in range(B):
            s = source[b]
            if not _is_int(s) or not -1 <= s < B or s == b:
                raise ValueError(f"source[{b}] = {s!r}: expected -1 or the index of another image of the batch of {B}")
            sel, new = selected[b], new_ids[b]
            if not all(_is_int(i) and 0 <= i <= 254 for i in sel) or list(sel) != sorted(set(sel)):
                raise ValueError(f"selected[{b}] = {sel!r}: expected ascending distinct ids in 0 .. 254")
            if s < 0 and sel:
                raise ValueError(f"selected[{b}] = {sel!r}, but image {b} has no source")
            if not all(_is_int(i) and 0 <= i <= 254 for i in new) or len(set(new)) != len(new):
                raise ValueError(f"new_ids[{b}] = {new!r}: expected distinct ids in 0 .. 254 (255 is never an instance)")
            if len(new) > len(sel):
                raise ValueError(f"new_ids[{b}] has {len(new)} entries for {len(sel)} selected ids")
        shift = tuple(_pair(v, f"shift[{b}]") for b, v in enumerate(shift))
        mv = self.min_visible
        if isinstance(mv, bool) or not isinstance(mv, (int, float)) or not 0.0 <= mv <= 1.0:
            raise ValueError(f"min_visible must be a number in [0, 1], got {mv!r}")
        object.__setattr__(self, "source", tuple(int(s) for s in source))
        object.__setattr__(self, "selected", selected)
        object.__setattr__(self, "new_ids", new_ids)
        object.__setattr__(self, "shift", shift)
        object.__setattr__(self, "min_visible", float(mv))

    def __len__(self) -> int:
        return len(self.source)

    def fraction(self) -> tuple:
        """(num, den): min_visible as the integers the kernels compare with, visible * den >= num * original."""
        from fractions import Fraction
        f = Fraction(self.min_visible).limit_denominator(1024)
        return f.numerator, f.denominator

    def lut(self):
        """The (B, 256) int32 table of `ops.copy_paste`: lut[b][source id] = new id, -1 everywhere else."""
        import numpy as np
        lut = np.full((len(self), 256), -1, dtype=np.int32)
        for b, (sel, new) in enumerate(zip(self.selected, self.new_ids)):
            for i, v in zip(sel, new):
                lut[b, i] = v
        return lut


class CopyPaste:
    """Draws `CopyPasteParams` for a collated compact batch (Simple Copy-Paste, Ghiasi et al., CVPR 2021; DESIGN
    section 31).  `prob`: the probability that an image receives a paste; `select`: the probability that an instance of
    its source is taken; `max_instances`: None or the largest number of instances one paste may carry; `classes`: None or
    the class ids that may be pasted (weeds only, say, for class balance); `shift`: None (instances keep their place),
    a number m (dy and dx uniform over the integers -m .. m) or a pair (my, mx); `min_visible`: see `CopyPasteParams`.

    `sample(id_mappings, generator)` takes the batch's id -> class dictionaries.  With one image nothing is pasted and
    no draw is taken.  Otherwise it takes, per image b in order and always all of them, whether or not b ends up pasting:
    one float32 uniform (paste when it is below `prob`); one randint(B - 1) for the source among the other images (k
    stands for image k when k < b, else k + 1); then, for the ids 0 .. 254 of the source's dictionary whose class is
    allowed, ascending, one float32 uniform each (kept when it is below `select`); with `max_instances` set, one
    randperm(number of candidates), whose order decides which kept ids stay when they are more than `max_instances`;
    then randint(2 my + 1) and randint(2 mx + 1) for the shift.  The same seed gives the same parameters on any
    machine.  New ids come from `allocate_paste_ids`."""

    def __init__(self, prob: float = 0.5, select: float = 0.5, max_instances=None, classes=None, shift=None,
                 min_visible: float = 0.0):
        for name, v in (("prob", prob), ("select", select), ("min_visible", min_visible)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
                raise ValueError(f"{name} must lie in [0, 1], got {v!r}")
        if max_instances is not None and (not _is_int(max_instances) or max_instances < 0):
            raise ValueError(f"max_instances must be None or an integer >= 0, got {max_instances!r}")
        if shift is None:
            my = mx = 0
        elif _is_int(shift):
            my = mx = shift
        else:
            my, mx = _pair(shift, "shift")
        if my < 0 or mx < 0:
            raise ValueError(f"shift: expected None, an integer >= 0 or a pair of them, got {shift!r}")
        self.prob, self.select, self.min_visible = float(prob), float(select), float(min_visible)
        self.max_instances = max_instances
        self.classes = None if classes is None else frozenset(int(c) for c in classes)
        self.shift = (my, mx)

    def sample(self, id_mappings, generator: torch.Generator | None = None) -> CopyPasteParams:
        if generator is not None and generator.device.type != "cpu":
            raise ValueError("generator must be a CPU torch.Generator")
        maps = [{int(k): int(v) for k, v in m.items()} for m in id_mappings]
        B = len(maps)
        source, selected, new_ids, shift = [], [], [], []
        for b in range(B):
            if B == 1:
                source.append(-1), selected.append(()), new_ids.append(()), shift.append((0, 0))
                break
            paste = float(torch.rand(1, generator=generator).item()) < self.prob
            k = int(torch.randint(B - 1, (1,), generator=generator).item())
            s = k if k < b else k + 1
            cand = [i for i in _instance_ids(maps[s]) if self.classes is None or maps[s][i] in self.classes]
            kept = [i for i in cand if float(torch.rand(1, generator=generator).item()) < self.select]
            if self.max_instances is not None:
                order = torch.randperm(len(cand), generator=generator).tolist()
                if len(kept) > self.max_instances:
                    first = [cand[j] for j in order if cand[j] in kept][:self.max_instances]
                    kept = sorted(first)
            dy = int(torch.randint(2 * self.shift[0] + 1, (1,), generator=generator).item()) - self.shift[0]
            dx = int(torch.randint(2 * self.shift[1] + 1, (1,), generator=generator).item()) - self.shift[1]
            new = allocate_paste_ids(kept, maps[b]) if paste else ()
            if not paste or not new:
                source.append(-1), selected.append(()), new_ids.append(()), shift.append((0, 0))
                continue
            source.append(s), selected.append(tuple(kept)), new_ids.append(new), shift.append((dy, dx))
        return CopyPasteParams(tuple(source), tuple(selected), tuple(new_ids), tuple(shift), self.min_visible)


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


def _rotate_on_device(tensors, sizes, params, dev, labels: bool):
    """Pack, one orient call, unpack: what `rotate_images` and `rotate_maps` share.  `tensors` are flat-able host or
    device tensors of one dtype, `sizes` their stored (H, W)."""
    from . import ops
    import numpy as np
    per = 1 if labels else 3
    off = [0]
    for H, W in sizes:
        off.append(off[-1] + H * W * per)
    src = torch.empty(off[-1], dtype=tensors[0].dtype, device=dev)
    dst = torch.empty_like(src)
    for b, t in enumerate(tensors):
        src[off[b]:off[b + 1]].copy_(t.reshape(-1), non_blocking=True)
    desc = np.array([p.desc_row(off[b], *sizes[b], off[b], labels=labels) for b, p in enumerate(params)], dtype=np.int64)
    (ops.orient_labels if labels else ops.orient_u8)(src, dst, desc)
    out = []
    for b, p in enumerate(params):
        h, w = p.out_size(*sizes[b])
        o = dst[off[b]:off[b + 1]]
        out.append((o.view(h, w) if labels else o.view(h, w, 3)).clone())  # each result owns its memory
    return out


def _rotate_args(name, items, params, device):
    single = not isinstance(items, (list, tuple))
    items = [items] if single else list(items)
    if not items:
        raise ValueError(f"{name} is empty")
    ps = list(params) if isinstance(params, (list, tuple)) else [params] * len(items)
    if len(ps) != len(items) or not all(isinstance(p, RotateParams) for p in ps):
        raise ValueError(f"params: expected one RotateParams or a list of {len(items)}, one per entry of {name}")
    if not torch.cuda.is_available():
        raise _lib.Wm2fError(f"rotate_{name}: the wm2f kernels run on a GPU only (no CPU fallback)")
    _lib.load()
    dev = next((x.device for x in items if isinstance(x, torch.Tensor) and x.is_cuda), torch.device(device))
    if dev.type != "cuda":
        raise _lib.Wm2fError(f"device={device}: the wm2f kernels run on a GPU only (no CPU fallback)")
    return single, items, ps, dev


def rotate_images(images, params, device="cuda"):
    """The orientation(s) `params` on the GPU (csrc/orient.hip), byte for byte what Pillow's
    `transpose` and `rotate(angle, BILINEAR, fillcolor=fill)` give.  `images`: one (H, W, 3) uint8 image (torch tensor on
    host or device, numpy array or PIL RGB image) or a list of them; `params`: one `RotateParams` for every image or a
    list with one per image.  Returns new uint8 device tensors of the turned size (one tensor for one image, a list for a
    list); the inputs are never written."""
    import numpy as np
    from .preprocess import _image_hwc_u8
    single, ims, ps, dev = _rotate_args("images", images, params, device)
    ims = [_image_hwc_u8(im, i) for i, im in enumerate(ims)]
    ts = [im if isinstance(im, torch.Tensor) else torch.from_numpy(np.array(im)) for im in ims]
    out = _rotate_on_device(ts, [tuple(int(v) for v in t.shape[:2]) for t in ts], ps, dev, labels=False)
    return out[0] if single else out


def rotate_maps(maps, params, device="cuda"):
    """The same for (H, W) id maps, uint8 or int32 (torch tensor, numpy array, or a PIL image of mode L or I), all of one
    dtype: Pillow's `transpose` and `rotate(angle, NEAREST, fillcolor=map_fill)`.  Returns new device tensors of the
    maps' dtype."""
    import numpy as np
    single, ms, ps, dev = _rotate_args("maps", maps, params, device)
    ts = []
    for i, m in enumerate(ms):
        if not isinstance(m, (torch.Tensor, np.ndarray)):
            m = np.array(m)
        t = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.array(m))
        if t.ndim != 2 or t.dtype not in (torch.uint8, torch.int32) or t.numel() == 0:
            raise ValueError(f"maps[{i}]: expected a non-empty (H, W) uint8 or int32 map, got {tuple(t.shape)} {t.dtype}")
        ts.append(t)
    if len({t.dtype for t in ts}) != 1:
        raise ValueError("maps: all maps of one call must have the same dtype")
    if ts[0].dtype == torch.uint8 and not all(0 <= p.map_fill <= 255 for p in ps):
        raise ValueError("map_fill must lie in 0 .. 255 for uint8 maps")
    out = _rotate_on_device(ts, [tuple(int(v) for v in t.shape) for t in ts], ps, dev, labels=True)
    return out[0] if single else out
