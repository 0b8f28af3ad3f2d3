"""The colour contract of include/wm2f.h restated in numpy, one id at a time: `img[m == i]`, Python's
`//` for both floor divisions, np.bincount for the histogram, fractions.Fraction for Otsu.  Nothing here walks rows, folds
runs or multiplies by reciprocals as csrc/color.hip does."""
from fractions import Fraction

import numpy as np

from shape_reference import ellipse_scene

PRESETS = {"exg": (-1, 2, -1), "exr5": (7, -5, 0), "exgr5": (-12, 15, -5)}
PLANT, SOIL, NOISE = (60, 140, 50), (120, 90, 60), 25


def index_range(coef):
    """(bins, Imin)."""
    return 255 * sum(abs(c) for c in coef) + 1, -255 * sum(-c for c in coef if c < 0)


def index_image(img, coef):
    """(..., 3) uint8 -> (...) int64 values of I = a R + b G + c B."""
    p = img.astype(np.int64)
    return coef[0] * p[..., 0] + coef[1] * p[..., 1] + coef[2] * p[..., 2]


def pixel_q(R, G, B, coef):
    """The Q12 normalised index of one pixel (Python ints, floor division)."""
    s = R + G + B
    return 0 if s == 0 else (4096 * (coef[0] * R + coef[1] * G + coef[2] * B)) // s


def pixel_hue(R, G, B):
    """(h, chroma) of one pixel: the integer hue in [0, 360) (None for a grey pixel) and max - min."""
    mx, mn = max(R, G, B), min(R, G, B)
    cr = mx - mn
    if cr == 0:
        return None, 0
    if mx == R:
        h = (60 * (G - B)) // cr
        h += 360 if h < 0 else 0
    elif mx == G:
        h = 120 + (60 * (B - R)) // cr
    else:
        h = 240 + (60 * (R - G)) // cr
    return h, cr


def _rows(m, ids, N):
    """The map values of the N result rows of one image: 0 .. N-1, or the listed ids (None past the list)."""
    return list(range(N)) if ids is None else [int(v) for v in ids] + [None] * (N - len(ids))


def _members(m, value):
    """Boolean mask of the pixels whose value stands for the integer `value`; a float map's fractions, negatives, NaN and
    values from 2^24 on stand for nothing (-0.0 is 0)."""
    if m.dtype.kind == "f":
        return (m == np.float32(value)) & (value < 2 ** 24)
    return m == value


def color_stats(img, m, N, coef, threshold, dark, bright, K=None, min_chroma=16, ids=None):
    """One image: img (H, W, 3) uint8, m (H, W) map -> (sums (N, 14) int64, hue (N, K) int64 or None)."""
    sums = np.zeros((N, 14), np.int64)
    hue = None if K is None else np.zeros((N, K), np.int64)
    for r, value in enumerate(_rows(m, ids, N)):
        if value is None or value < 0:
            continue
        px = img[_members(m, value)].astype(np.int64)  # (n, 3)
        if len(px) == 0:
            continue
        R, G, B = px[:, 0], px[:, 1], px[:, 2]
        I = coef[0] * R + coef[1] * G + coef[2] * B
        mx = px.max(1)
        q = sum(pixel_q(int(a), int(b), int(c), coef) for a, b, c in px)
        sums[r] = [len(px), R.sum(), G.sum(), B.sum(), (R * R).sum(), (G * G).sum(), (B * B).sum(), (R * G).sum(),
                   (R * B).sum(), (G * B).sum(), (I > threshold).sum(), q, (mx < dark).sum(), (mx >= bright).sum()]
        if K is not None:
            for a, b, c in px:
                h, cr = pixel_hue(int(a), int(b), int(c))
                if cr >= min_chroma:
                    hue[r, h // (360 // K)] += 1
    return sums, hue


def color_stats_batch(imgs, maps, N, coef, thresholds, dark, bright, K=None, min_chroma=16, ids=None, n_ids=None):
    out = [color_stats(imgs[b], maps[b], N, coef, int(thresholds[b]), dark, bright, K, min_chroma,
                       None if ids is None else ids[b][:int(n_ids[b])]) for b in range(len(imgs))]
    return np.stack([s for s, _ in out]), (None if K is None else np.stack([h for _, h in out]))


def index_hist(img, coef):
    """(H, W, 3) uint8 -> (bins) int64."""
    bins, imin = index_range(coef)
    return np.bincount((index_image(img, coef) - imin).ravel(), minlength=bins).astype(np.int64)


def otsu(hist, imin):
    """Otsu's threshold in index units, None when no bin separates two non-empty classes: the smallest t in
    [0, bins - 2] that maximises the between-class term (S n0 - s0 n)^2 / (n0 (n - n0)), as exact fractions."""
    h = [int(v) for v in hist]
    n, S = sum(h), sum(t * v for t, v in enumerate(h))
    best, best_t = None, None
    for t in range(len(h) - 1):
        n0, s0 = sum(h[:t + 1]), sum(k * v for k, v in enumerate(h[:t + 1]))
        if n0 == 0 or n0 == n:
            continue
        score = Fraction((S * n0 - s0 * n) ** 2, n0 * (n - n0))
        if best is None or score > best:
            best, best_t = score, t
    return None if best_t is None else best_t + imin


def otsu_fast(hist, imin):
    """`otsu` with running sums (for the 8161-bin histograms of the tests; test_color_cpu holds the two equal)."""
    h = np.asarray(hist, dtype=object)
    n, S = int(h.sum()), sum(t * int(v) for t, v in enumerate(h))
    best, best_t, n0, s0 = None, None, 0, 0
    for t in range(len(h) - 1):
        n0 += int(h[t])
        s0 += t * int(h[t])
        if n0 == 0 or n0 == n:
            continue
        score = Fraction((S * n0 - s0 * n) ** 2, n0 * (n - n0))
        if best is None or score > best:
            best, best_t = score, t
    return None if best_t is None else best_t + imin


def threshold_of(img, coef):
    """The picture's threshold as the package defines it: Otsu's, or the index's largest value for a one-value picture."""
    bins, imin = index_range(coef)
    t = otsu_fast(index_hist(img, coef), imin)
    return imin - 1 + bins if t is None else t


def index_mask(img, coef, threshold):
    """(mask (H, W) uint8, count)."""
    mask = (index_image(img, coef) > threshold).astype(np.uint8)
    return mask, int(mask.sum())


def scene(rng, shape, N, dtype=np.int32, background=-1):
    """(img (H, W, 3) uint8, map): `ellipse_scene`'s map, plant pixels (60, 140, 50) and soil pixels (120, 90, 60), each
    byte plus uniform noise in [-25, 25], clipped."""
    m = ellipse_scene(rng, shape, N, dtype=np.int64)
    base = np.where((m >= 0)[..., None], np.array(PLANT), np.array(SOIL))
    img = np.clip(base + rng.integers(-NOISE, NOISE + 1, base.shape), 0, 255).astype(np.uint8)
    if background != -1:
        m = np.where(m < 0, background, m)
    return img, m.astype(dtype)
