"""Numpy restatements of the interior distance maps and the aim points, written as the definition
reads.

- `d2_brute`: for every pixel with an id, the smallest squared distance to any position that does not carry that id,
  over all pairs.  Border-outside mode surrounds the map with a ring of positions that carry no id.
- `d2_scipy`: the same through `scipy.ndimage.distance_transform_edt(mask, return_indices=True)` per id; the squared
  distance is taken in integers from the returned indices, so nothing is rounded.
- `d2_two_pass`: the form the kernels take -- the vertical distance g per column, then a walk outwards along the row that
  stops once step^2 reaches the best so far.
- `d2_run_bounded`: the two-pass form as the rows kernel walks it -- h, the horizontal distance to the end of the
  pixel's run, bounds the walk, so the steps read g alone, clamped at the row's ends, and never look at an id.
- `squared_distance`: brute force for small maps, the scipy form otherwise.
- `aim_points`: per id the pixel with the largest d2, nearest the rounded centroid among equals, first in raster order
  among those.
"""
import numpy as np

INT32_MAX = 2 ** 31 - 1
G_NONE = 0xFFFF


def id_keys(id_map):
    """(H, W) int64: the id of every pixel, -1 where the value is no id.  Floats: negative, fractional, not finite or
    >= 2^24 is no id and -0.0 is 0; integers: negative is no id."""
    a = np.asarray(id_map)
    if a.dtype.kind == "f":
        out = np.full(a.shape, -1, np.int64)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(a) & (a >= 0) & (a < 2.0 ** 24)
            ok &= np.where(ok, a, 0) == np.floor(np.where(ok, a, 0))
        out[ok] = a[ok].astype(np.int64)
        return out
    a = a.astype(np.int64)
    return np.where(a >= 0, a, -1)


def _ringed(key, border_outside):
    """The key map with the positions just beyond the image added as positions without an id, and the offset of the
    image inside it."""
    if not border_outside:
        return key, 0
    return np.pad(key, 1, constant_values=-1), 1


def d2_brute(id_map, border_outside=True):
    key = id_keys(id_map)
    H, W = key.shape
    big, o = _ringed(key, border_outside)
    qy, qx = np.mgrid[0:big.shape[0], 0:big.shape[1]]
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            k = key[y, x]
            if k < 0:
                continue
            other = big != k
            if not other.any():
                out[y, x] = INT32_MAX
                continue
            out[y, x] = int((((qy - (y + o)) ** 2 + (qx - (x + o)) ** 2)[other]).min())
    return out.astype(np.int32)


def d2_scipy(id_map, border_outside=True):
    from scipy import ndimage
    key = id_keys(id_map)
    H, W = key.shape
    big, o = _ringed(key, border_outside)
    out = np.zeros((H, W), np.int64)
    for k in np.unique(key[key >= 0]):
        ys, xs = np.nonzero(key == k)
        if border_outside:  # the ring round the instance's box holds no k: nothing beyond it can be nearer
            y0, y1, x0, x1 = ys.min() + o - 1, ys.max() + o + 2, xs.min() + o - 1, xs.max() + o + 2
        else:
            y0, y1, x0, x1 = 0, H, 0, W
        mask = big[y0:y1, x0:x1] == k
        if mask.all():
            out[key == k] = INT32_MAX
            continue
        iy, ix = ndimage.distance_transform_edt(mask, return_distances=False, return_indices=True)
        gy, gx = np.mgrid[0:mask.shape[0], 0:mask.shape[1]]
        d = (iy.astype(np.int64) - gy) ** 2 + (ix.astype(np.int64) - gx) ** 2
        out[ys, xs] = d[ys + o - y0, xs + o - x0]
    return out.astype(np.int32)


def column_distance(id_map, border_outside=True):
    """g (H, W): the vertical distance to the nearest position of the pixel's column that does not carry its id; 0 for a
    pixel without an id, G_NONE where the column has no such position (border-inside mode only)."""
    key = id_keys(id_map)
    H, W = key.shape
    g = np.zeros((H, W), np.int64)
    for x in range(W):
        for y in range(H):
            k = key[y, x]
            if k < 0:
                continue
            best = G_NONE
            for step in range(1, H + 1):
                for yy in (y - step, y + step):
                    if 0 <= yy < H:
                        if key[yy, x] != k:
                            best = min(best, step)
                    elif border_outside and yy in (-1, H):
                        best = min(best, step)
                if best != G_NONE:
                    break
            g[y, x] = best
    return g


def d2_two_pass(id_map, border_outside=True):
    key = id_keys(id_map)
    H, W = key.shape
    g = column_distance(id_map, border_outside)
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            k = key[y, x]
            if k < 0:
                continue
            best = INT32_MAX if g[y, x] == G_NONE else int(g[y, x]) ** 2
            alive = {-1: True, 1: True}
            step = 1
            while (alive[-1] or alive[1]) and step * step < best:
                for side in (-1, 1):
                    if not alive[side]:
                        continue
                    xx = x + side * step
                    if xx < 0 or xx >= W:
                        if border_outside:
                            best = min(best, step * step)
                        alive[side] = False
                    elif key[y, xx] != k:
                        best = min(best, step * step)
                        alive[side] = False
                    elif g[y, xx] != G_NONE:
                        best = min(best, step * step + int(g[y, xx]) ** 2)
                step += 1
            out[y, x] = best
    return out.astype(np.int32)


def row_distance(id_map, border_outside=True):
    """h (H, W): `column_distance` along the rows."""
    return column_distance(np.asarray(id_map).T, border_outside).T


def d2_run_bounded(id_map, border_outside=True):
    H, W = np.asarray(id_map).shape
    g, h = column_distance(id_map, border_outside), row_distance(id_map, border_outside)
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            if g[y, x] == 0:  # a pixel without an id
                continue
            m0 = min(g[y, x], h[y, x])
            best = INT32_MAX if m0 == G_NONE else int(m0) ** 2
            step = 1
            while step <= max(x, W - 1 - x) and step * step < best:
                gm = min(g[y, max(x - step, 0)], g[y, min(x + step, W - 1)])  # whoever's pixels these are
                if gm != G_NONE:
                    best = min(best, step * step + int(gm) ** 2)
                step += 1
            out[y, x] = best
    return out.astype(np.int32)


def squared_distance(id_map, border_outside=True):
    a = np.asarray(id_map)
    return d2_brute(a, border_outside) if a.size <= 400 else d2_scipy(a, border_outside)


def rounded_centroid(key, k):
    """(cx, cy) = (2 sum + area) // (2 area) per coordinate: the centroid rounded half up, in integers."""
    ys, xs = np.nonzero(key == k)
    area = len(ys)
    return (2 * int(xs.sum()) + area) // (2 * area), (2 * int(ys.sum()) + area) // (2 * area)


def aim_points(id_map, d2, ids, centred=True):
    """(len(ids), 4) int32 rows [x, y, d2max, 0], [-1, -1, 0, 0] for an id without a pixel."""
    key = id_keys(id_map)
    W = key.shape[1]
    d2 = np.asarray(d2).astype(np.int64)
    out = np.zeros((len(ids), 4), np.int32)
    for r, k in enumerate(ids):
        ys, xs = np.nonzero(key == int(k)) if int(k) >= 0 else (np.zeros(0, np.int64),) * 2
        if len(ys) == 0:
            out[r] = (-1, -1, 0, 0)
            continue
        d = d2[ys, xs]
        top = d == d.max()
        ys, xs = ys[top], xs[top]
        if centred:
            cx, cy = rounded_centroid(key, int(k))
            c = (xs - cx) ** 2 + (ys - cy) ** 2
        else:
            c = np.zeros(len(ys), np.int64)
        best = min(zip(c.tolist(), (ys * W + xs).tolist()))
        out[r] = (best[1] % W, best[1] // W, int(d.max()), 0)
    return out


def instance_stats(id_map, ids):
    """(len(ids), 8) int64 rows [area, xmin, ymin, xmax, ymax, sum_x, sum_y, 0] as wm2f_labelmap_instance_stats writes
    them."""
    key = id_keys(id_map)
    H, W = key.shape
    out = np.zeros((len(ids), 8), np.int64)
    for r, k in enumerate(ids):
        ys, xs = np.nonzero(key == int(k)) if int(k) >= 0 else (np.zeros(0, np.int64),) * 2
        out[r] = (0, W, H, -1, -1, 0, 0, 0) if len(ys) == 0 else (len(ys), xs.min(), ys.min(), xs.max(), ys.max(),
                                                                    xs.sum(), ys.sum(), 0)
    return out
