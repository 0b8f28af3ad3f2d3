"""Multi-scale training augmentation: random horizontal flip, random scale, fixed-size crop or
short-edge choice.  Not in the reference, which trains on one deterministic resize per image.

    from weed_instance_segmentation_amd import TrainAugmentation, AugmentParams

    aug = TrainAugmentation(short_edge=range(640, 801, 32), max_size=1333)        # COCO-style multi-scale
    aug = TrainAugmentation(scale=(0.1, 2.0), crop_size=(1024, 1024))             # large-scale jitter
    params = aug.sample(height, width, generator)                                 # an AugmentParams
    inputs = processor(images=image, segmentation_maps=instance_map, augment=params, pad_size=aug.pad_size, ...)

`AugmentParams` are explicit and public, so an augmentation can be replayed.  The processor stays deterministic; every
random draw happens in `TrainAugmentation.sample`, from the caller's CPU `torch.Generator`.  The pixels are produced by
csrc/augment.hip, bit for bit what Pillow makes of the flipped, resized, cropped image.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

__all__ = ["AugmentParams", "TrainAugmentation"]


def _pair(v, name: str):
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected a pair of integers, got {v!r}") from None
    for x in (a, b):
        if isinstance(x, bool) or int(x) != x:
            raise ValueError(f"{name}: expected a pair of integers, got {v!r}")
    return int(a), int(b)


@dataclass(frozen=True)
class AugmentParams:
    """One image's augmentation: `flip` (0 or 1, a horizontal mirror of the source, applied before the resize), `size` =
    (h, w) of the resized frame, `origin` = (y0, x0) and `window` = (ch, cw) of the crop inside that frame.  The window
    must lie inside the frame: y0 + ch <= h and x0 + cw <= w."""
    flip: int
    size: tuple
    origin: tuple = (0, 0)
    window: tuple | None = None

    def __post_init__(self):
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
    any machine."""

    def __init__(self, short_edge=None, max_size: int = 1333, scale=None, crop_size=None, flip_prob: float = 0.5,
                 size_divisor: int = 32):
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
        return AugmentParams(flip, (h, w), (y0, x0), (ch, cw))
