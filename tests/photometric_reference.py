"""The colour-jitter contract of DESIGN section 29 restated in numpy (no GPU): Pillow 12.2's `ImageEnhance.Brightness`,
`Contrast`, `Color` and a hue shift through its HSV conversions, byte for byte.  tests/test_photometric_cpu.py holds it
to Pillow itself; tests/test_photometric_gpu.py holds csrc/photometric.hip to it and to Pillow.

`fused=True` is the blend as a fused multiply-add would compute it (one rounding instead of two): what a device build
gives when the compiler contracts a * b + c.  It exists so that tests can show their inputs tell the two apart."""
from __future__ import annotations

import numpy as np

KINDS = ("brightness", "contrast", "saturation", "hue")
# factors at which the fused blend differs from Pillow's somewhere on the 256 x 256 (d, v) grid
DISCRIMINATING = (0.6, 0.8, 0.85, 1.1, 1.2, 1.6, 1.7, 0.9639175534248352, 0.2928571105003357, 1.830188512802124)


def luma(rgb: np.ndarray) -> np.ndarray:
    """Pillow's L of (..., 3) uint8: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    c = rgb.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(d, v, f, fused: bool = False) -> np.ndarray:
    """Image.blend(degenerate, image, f) per byte: t = fl32(fl32(d) + fl32(a * fl32(v - d))), a = float32(f); 0 when
    t <= 0, 255 when t >= 255, else trunc(t)."""
    a = np.float32(f)
    d = np.asarray(d)
    df = d.astype(np.float32)
    diff = (np.asarray(v).astype(np.int32) - d.astype(np.int32)).astype(np.float32)
    if fused:  # the product (33 bits) and the sum are exact in float64 for the factors in use: one rounding to float32
        t = (df.astype(np.float64) + np.float64(a) * diff.astype(np.float64)).astype(np.float32)
    else:
        t = df + a * diff  # numpy rounds each float32 operation
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def contrast_mean(im: np.ndarray) -> int:
    """int(S / (H W) + 0.5) with S the integer sum of L, the division in float64."""
    L = luma(im)
    return int(int(L.astype(np.int64).sum()) / L.size + 0.5)


def brightness(im, f, fused=False):
    return blend(np.zeros_like(im), im, f, fused)


def contrast(im, f, fused=False):
    return blend(np.full_like(im, contrast_mean(im)), im, f, fused)


def saturation(im, f, fused=False):
    return blend(np.broadcast_to(luma(im)[..., None], im.shape), im, f, fused)


def _clip8(x):
    return np.clip(x, 0, 255).astype(np.uint8)


def rgb_to_hsv(rgb: np.ndarray) -> np.ndarray:
    """Pillow's rgb2hsv (Convert.c) of (..., 3) uint8."""
    c = rgb.astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = c.max(-1), c.min(-1)
    grey = mx == mn
    f32, f64 = np.float32, np.float64
    cr = np.where(grey, 1, mx - mn).astype(f32)
    s = cr / np.where(grey, 1, mx).astype(f32)
    rc, gc, bc = ((mx - r).astype(f32) / cr, (mx - g).astype(f32) / cr, (mx - b).astype(f32) / cr)
    h = np.where(r == mx, bc - gc,
                 np.where(g == mx, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                          (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32))).astype(f32)
    x = h.astype(f64) / 6.0 + 1.0  # in [5/6, 11/6): fmod(x, 1) is x - 1 or x, exactly
    h = np.where(x >= 1.0, x - 1.0, x).astype(f32)
    H = np.where(grey, 0, _clip8(np.trunc(h.astype(f64) * 255.0)))
    S = np.where(grey, 0, _clip8(np.trunc(s.astype(f64) * 255.0)))
    return np.stack([H, S, mx], -1).astype(np.uint8)


def _round_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """Pillow's hsv2rgb (Convert.c) of (..., 3) uint8."""
    f32, f64 = np.float32, np.float64
    H, S, V = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    hf = H.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i).astype(f32)
    fs = (S.astype(f64) / 255.0).astype(f32)
    v = V.astype(f64)
    p = _clip8(_round_away(v * (1.0 - fs.astype(f64))))
    q = _clip8(_round_away(v * (1.0 - (fs * f).astype(f64))))  # fs * f is a float32 product in C
    t = _clip8(_round_away(v * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64)))))
    sel = i.astype(np.int64) % 6
    R = np.choose(sel, [V, q, p, p, t, V])
    G = np.choose(sel, [t, V, V, q, p, p])
    B = np.choose(sel, [p, p, t, V, V, q])
    out = np.stack([R, G, B], -1).astype(np.uint8)
    return np.where((S == 0)[..., None], V[..., None], out).astype(np.uint8)


def hue_dh(shift: float) -> int:
    """The byte added to H for a shift in [-0.5, 0.5]: int(shift * 255) mod 256, Python's int and mod."""
    return int(shift * 255) % 256


def hue(im, dh: int):
    hsv = rgb_to_hsv(im)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(dh)) % 256
    return hsv_to_rgb(hsv)


def apply(im: np.ndarray, ops, fused: bool = False) -> np.ndarray:
    """The chain `ops` = ((kind, value), ...) left to right on an (H, W, 3) uint8 image; each step reads the uint8 image
    the one before it made.  The value of a hue step is the shift, not dh."""
    out = np.ascontiguousarray(im)
    for kind, value in ops:
        if kind == "hue":
            out = hue(out, hue_dh(value))
        else:
            out = {"brightness": brightness, "contrast": contrast, "saturation": saturation}[kind](out, value, fused)
    return out


def pil_apply(im: np.ndarray, ops) -> np.ndarray:
    """The same chain in Pillow itself."""
    from PIL import Image, ImageEnhance
    a = Image.fromarray(im)
    for kind, value in ops:
        if kind == "hue":
            h, s, v = a.convert("HSV").split()
            dh = hue_dh(value)
            h = h.point(lambda x: (x + dh) % 256)
            a = Image.merge("HSV", (h, s, v)).convert("RGB")
        else:
            enh = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast,
                   "saturation": ImageEnhance.Color}[kind]
            a = enh(a).enhance(value)
    return np.asarray(a)
