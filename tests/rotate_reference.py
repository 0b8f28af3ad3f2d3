"""The orientation contract of DESIGN section 30 restated in numpy (no GPU): Pillow 12.2's `transpose(FLIP_TOP_BOTTOM)`,
`transpose(ROTATE_90 / 180 / 270)` and `rotate(angle, BILINEAR or NEAREST, expand=False, fillcolor)`, byte for byte.
tests/test_rotate_cpu.py holds it to Pillow itself; tests/test_rotate_gpu.py holds csrc/orient.hip to it and to Pillow.

`fused=1` or `2` is the bilinear path as a build that contracts a * b + c would compute it (exact product and sum,
rounded once; the two values are the two ways the coordinates can contract); it exists for the search of
test_rotate_cpu.py."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

SIZES = ((1, 1), (5, 7), (33, 130), (96, 64), (64, 64), (257, 31))  # (H, W)
NAMED_ANGLES = (1, -7.5, 13.37, 45, 90, 270, 359.9, 30.000001, 89.99, -180.5, 180, 0, 360, -180, -90, 450, 0.001)


def angles(seed: int = 0):
    """The named angles and twenty random ones."""
    rng = np.random.default_rng(1000 + seed)
    return NAMED_ANGLES + tuple(float(a) for a in rng.uniform(-360, 360, 20))


def matrix(angle: float, H: int, W: int) -> list:
    """Image.rotate's matrix for a (H, W) frame, in Python floats."""
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def fixed(m) -> list:
    """Pillow's 16.16 terms, FIX(v) = floor(v 65536.0 + 0.5), as Python integers."""
    fix = lambda v: math.floor(v * 65536.0 + 0.5)  # noqa: E731
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def shortcut(angle: float, H: int, W: int):
    """The number of quarter turns Pillow's rotate routes this angle to on a (H, W) frame, or None for the transform."""
    a = angle % 360.0
    if a == 0:
        return 0
    if a == 180:
        return 2
    if a in (90, 270) and H == W:
        return 1 if a == 90 else 3
    return None


def turn(a: np.ndarray, turns: int) -> np.ndarray:
    """`turns` counter-clockwise quarter turns of (H, W) or (H, W, C), written as the index maps of include/wm2f.h."""
    H, W = a.shape[:2]
    if turns == 0:
        return a.copy()
    if turns == 2:
        return a[::-1, ::-1].copy()
    y, x = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")  # the (W, H) output frame
    return a[x, W - 1 - y].copy() if turns == 1 else a[H - 1 - x, y].copy()


def vflip(a: np.ndarray) -> np.ndarray:
    return a[::-1].copy()


def fma_exact(a, b, c) -> np.ndarray:
    """a * b + c rounded once, elementwise, through exact rationals: what a fused multiply-add gives.  Slow."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    out = np.empty(a.shape, np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """p + e = a b exactly (Dekker's product on Veltkamp's split; no overflow or underflow at the magnitudes in use)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fma(a, b, c) -> np.ndarray:
    """The same value as `fma_exact`, vectorised: Boldo and Melquiond's emulation.  uh + ul = a b and th + tl = c + uh
    exactly; v = tl + ul rounded TO ODD; the result is th + v rounded to nearest.  test_rotate_cpu.py holds it to
    `fma_exact` on the operands of the search."""
    a, b, c = (np.ascontiguousarray(v, np.float64) for v in np.broadcast_arrays(a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    v, e = _two_sum(tl, ul)
    even = (v.view(np.int64) & 1) == 0
    other = np.nextafter(v, np.where(e > 0, np.inf, -np.inf))  # the other float that encloses the exact sum
    return th + np.where((e != 0) & even, other, v)


def rotate_bilinear(im: np.ndarray, angle: float, fill=(0, 0, 0), fused: bool = False, m=None) -> np.ndarray:
    """rotate(angle, BILINEAR, expand=False, fillcolor=fill) of (H, W, 3) uint8, float64 and unfused.  `m`: the six
    matrix entries from elsewhere (RotateParams.matrix) instead of this module's."""
    H, W = im.shape[:2]
    k = shortcut(angle, H, W)
    if k is not None:
        return turn(im, k)
    m0, m1, m2, m3, m4, m5 = (np.float64(v) for v in (matrix(angle, H, W) if m is None else m))
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xi, yi = x + 0.5, y + 0.5
    if fused == 2:  # (m0 * xi + m1 * yi) + m2 contracted: one product is rounded, the other fused into the sum
        xin = _fma(m1, yi, m0 * xi) + m2
        yin = _fma(m4, yi, m3 * xi) + m5
    elif fused:  # ... or the other way round; the search takes both
        xin = _fma(m0, xi, m1 * yi) + m2
        yin = _fma(m3, xi, m4 * yi) + m5
    else:
        xin = m0 * xi + m1 * yi + m2
        yin = m3 * xi + m4 * yi + m5
    outside = (xin < 0) | (xin >= W) | (yin < 0) | (yin >= H)
    xin, yin = xin - 0.5, yin - 0.5
    X, Y = np.floor(xin), np.floor(yin)
    dx, dy = (xin - X)[..., None], (yin - Y)[..., None]
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    x0, x1, yc = np.clip(X, 0, W - 1), np.clip(X + 1, 0, W - 1), np.clip(Y, 0, H - 1)
    two = ((Y + 1 >= 0) & (Y + 1 < H))[..., None]
    y1 = np.clip(Y + 1, 0, H - 1)
    f = im.astype(np.float64)
    a, b, a2, b2 = f[yc, x0], f[yc, x1], f[y1, x0], f[y1, x1]
    if fused:
        v1 = _fma(b - a, dx, a)
        v2 = np.where(two, _fma(b2 - a2, dx, a2), v1)
        v = _fma(v2 - v1, dy, v1)
    else:
        v1 = a + (b - a) * dx
        v2 = np.where(two, a2 + (b2 - a2) * dx, v1)
        v = v1 + (v2 - v1) * dy
    out = np.trunc(v).astype(np.uint8)
    out[outside] = np.asarray(fill, np.uint8)
    return out


def rotate_nearest(m: np.ndarray, angle: float, fill: int = 0, a=None) -> np.ndarray:
    """rotate(angle, NEAREST, expand=False, fillcolor=fill) of an (H, W) integer map: Pillow's 16.16 fixed point.  `a`:
    the six fixed-point terms from elsewhere (RotateParams.fixed) instead of this module's."""
    H, W = m.shape
    k = shortcut(angle, H, W)
    if k is not None:
        return turn(m, k)
    a0, a1, a2, a3, a4, a5 = fixed(matrix(angle, H, W)) if a is None else a
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    xs, ys = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    out = np.full((H, W), fill, dtype=m.dtype)
    out[inside] = m[ys[inside], xs[inside]]
    return out


def orient_image(im: np.ndarray, vf=False, turns=0, angle=0.0, fill=(0, 0, 0), fused: bool = False) -> np.ndarray:
    """The whole stage on an image: flip, turn, rotation, each only when enabled."""
    out = vflip(im) if vf else im
    out = turn(out, turns) if turns else out
    return rotate_bilinear(out, angle, fill, fused) if angle % 360.0 != 0 else out.copy()


def orient_map(m: np.ndarray, vf=False, turns=0, angle=0.0, fill: int = 0) -> np.ndarray:
    out = vflip(m) if vf else m
    out = turn(out, turns) if turns else out
    return rotate_nearest(out, angle, fill) if angle % 360.0 != 0 else out.copy()


# ------------------------------------------------------------------------------------------------ Pillow itself
def pil_orient_image(im: np.ndarray, vf=False, turns=0, angle=0.0, fill=(0, 0, 0)) -> np.ndarray:
    from PIL import Image
    p = Image.fromarray(im)
    if vf:
        p = p.transpose(Image.FLIP_TOP_BOTTOM)
    if turns:
        p = p.transpose((Image.ROTATE_90, Image.ROTATE_180, Image.ROTATE_270)[turns - 1])
    if angle % 360.0 != 0:
        p = p.rotate(angle, resample=Image.BILINEAR, expand=False, fillcolor=tuple(fill))
    return np.asarray(p).copy()


def pil_orient_map(m: np.ndarray, vf=False, turns=0, angle=0.0, fill: int = 0) -> np.ndarray:
    """uint8 maps go through mode L, int32 maps through mode I."""
    from PIL import Image
    p = Image.fromarray(m)
    assert p.mode == ("L" if m.dtype == np.uint8 else "I"), p.mode
    if vf:
        p = p.transpose(Image.FLIP_TOP_BOTTOM)
    if turns:
        p = p.transpose((Image.ROTATE_90, Image.ROTATE_180, Image.ROTATE_270)[turns - 1])
    if angle % 360.0 != 0:
        p = p.rotate(angle, resample=Image.NEAREST, expand=False, fillcolor=int(fill))
    return np.asarray(p).astype(m.dtype)
