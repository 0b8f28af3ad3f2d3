"""Numpy restatements of the nearest-instance maps, the per-cell counts and the treatment grid,
written as the definitions read.

- `nearest_brute`: for every pixel, over all source pixels within the cap, the smallest (squared distance, id).
- `column_nearest` and `nearest_two_pass`: the form the kernels take -- per column the vertical distance g to the nearest
  source pixel within r = floor(sqrt(max_d2)) rows (r + 1: none) and its id, the smaller id on an up / down tie; then per
  pixel the prefix count of its row's window [x - r, x + r] (nothing there: "none" at once) and a walk s = 0, 1, ... <= r
  along the row that goes on while s^2 <= best, clamped at the row's ends as the kernel clamps it.
- `nearest_separable`: the same minimum over (x - x')^2 + g(x', y)^2 with whole-array shifts, for maps too large for the
  loops above.
- `grow`: `grow_label_maps`.
- `cell_counts`: wm2f_labelmap_cell_counts.
- `treatment`: `treatment_grid`.
"""
from fractions import Fraction

import numpy as np

from distance_reference import id_keys

INT32_MAX = 2 ** 31 - 1


def isqrt(v):
    r = 0
    while (r + 1) * (r + 1) <= v:
        r += 1
    return r


def source_mask(id_map, N, source=None):
    """(key, is_source): the id of every pixel (-1: free, which covers every value outside [0, N)) and whether the pixel
    belongs to a source instance."""
    key = id_keys(id_map)
    key = np.where(key < N, key, -1)
    if source is None:
        return key, key >= 0
    source = np.asarray(source).astype(bool)
    return key, (key >= 0) & source[np.maximum(key, 0)]


def _blocked_fix(nearest, d2, key, is_src, blocked):
    if blocked:
        keep = (key >= 0) & ~is_src
        nearest[keep] = key[keep]
        d2[keep] = 0
    return nearest.astype(np.int32), d2.astype(np.int32)


def nearest_brute(id_map, N, max_d2, source=None, blocked=False, ties=None):
    """`ties`: a list that receives 1 for every pixel whose minimum is attained by two different ids."""
    key, is_src = source_mask(id_map, N, source)
    H, W = key.shape
    sy, sx = np.nonzero(is_src)
    sid = key[sy, sx]
    nearest = np.full((H, W), -1, np.int64)
    d2 = np.full((H, W), INT32_MAX, np.int64)
    for y in range(H):
        for x in range(W):
            if len(sy) == 0:
                continue
            d = (sy - y) ** 2 + (sx - x) ** 2
            ok = d <= max_d2
            if ok.any():
                best = min(zip(d[ok].tolist(), sid[ok].tolist()))
                d2[y, x], nearest[y, x] = best
                if ties is not None and len(set(sid[ok][d[ok] == best[0]].tolist())) > 1:
                    ties.append(1)
    return _blocked_fix(nearest, d2, key, is_src, blocked)


def column_nearest(key, is_src, r):
    """g (H, W): rows to the nearest source pixel of the column, r + 1 where none lies within r; gid: its id, the smaller
    one where the pixel above and the pixel below are equally far, -1 for none."""
    H, W = key.shape
    g = np.full((H, W), r + 1, np.int64)
    gid = np.full((H, W), -1, np.int64)
    for x in range(W):
        for y in range(H):
            for dy in range(0, r + 1):
                ids = [int(key[yy, x]) for yy in {y - dy, y + dy} if 0 <= yy < H and is_src[yy, x]]
                if ids:
                    g[y, x], gid[y, x] = dy, min(ids)
                    break
    return g, gid


def nearest_two_pass(id_map, N, max_d2, source=None, blocked=False, use_prefix=True):
    key, is_src = source_mask(id_map, N, source)
    H, W = key.shape
    r = isqrt(max_d2)
    g, gid = column_nearest(key, is_src, r)
    nearest = np.full((H, W), -1, np.int64)
    d2 = np.full((H, W), INT32_MAX, np.int64)
    none = (max_d2 + 1, 0)
    for y in range(H):
        prefix = np.cumsum(g[y] <= r)
        for x in range(W):
            if use_prefix:
                lo, hi = x - r, min(x + r, W - 1)
                if prefix[hi] - (prefix[lo - 1] if lo > 0 else 0) == 0:
                    continue
            best = none
            if g[y, x] ** 2 <= max_d2:
                best = (int(g[y, x]) ** 2, int(gid[y, x]))
            s = 1
            while s <= r and s <= max(x, W - 1 - x) and s * s <= best[0]:
                for xx in (max(x - s, 0), min(x + s, W - 1)):  # the end pixel again where the step leaves the row
                    cand = s * s + int(g[y, xx]) ** 2
                    if cand <= best[0]:
                        best = min(best, (cand, int(gid[y, xx]) & 0xFFFFFFFF))
                s += 1
            if best[0] <= max_d2:
                d2[y, x], nearest[y, x] = best
    return _blocked_fix(nearest, d2, key, is_src, blocked)


def _shift(a, k, axis, fill):
    """a moved by k along the axis: out[i] = a[i - k], `fill` where that leaves the array."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(k) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(0, n - k) if k >= 0 else slice(-k, n)
    dst[axis] = slice(k, n) if k >= 0 else slice(0, n + k)
    out[tuple(dst)] = a[tuple(src)]
    return out


def nearest_separable(id_map, N, max_d2, source=None, blocked=False):
    """The same result from packed keys d2 << 32 | id: the minimum over dy within r per column, then over dx per row."""
    key, is_src = source_mask(id_map, N, source)
    r = isqrt(max_d2)
    BIG = np.int64(1) << 62
    base = np.where(is_src, key.astype(np.int64), BIG)  # distance 0, the id
    col = base.copy()
    for dy in range(1, min(r, key.shape[0] - 1) + 1):
        for k in (dy, -dy):
            sh = _shift(base, k, 0, BIG)
            col = np.minimum(col, np.where(sh < BIG, sh + (np.int64(dy * dy) << 32), BIG))
    best = col.copy()
    for dx in range(1, min(r, key.shape[1] - 1) + 1):
        for k in (dx, -dx):
            sh = _shift(col, k, 1, BIG)
            best = np.minimum(best, np.where(sh < BIG, sh + (np.int64(dx * dx) << 32), BIG))
    d2 = best >> 32
    ok = (best < BIG) & (d2 <= max_d2)
    nearest = np.where(ok, best & 0xFFFFFFFF, -1)
    d2 = np.where(ok, d2, INT32_MAX)
    return _blocked_fix(nearest, d2, key, is_src, blocked)


def grow(id_map, n, margin, sources=None):
    """`grow_label_maps`: sources None, ids or a bool array."""
    max_d2 = int(Fraction(margin) ** 2 // 1)
    src = None
    if sources is not None:
        a = np.asarray(sources)
        src = a if a.dtype == np.bool_ else np.isin(np.arange(n), a)
    if n == 0:
        return np.full(np.asarray(id_map).shape, -1, np.int32)
    f = nearest_brute if np.asarray(id_map).size <= 400 else nearest_separable
    return f(id_map, n, max_d2, src, True)[0]


def grid_shape(H, W, cell, offset):
    return -(-(H + offset[0]) // cell[0]), -(-(W + offset[1]) // cell[1])


def cell_counts(id_map, group, G, cell, offset=(0, 0), veto_d2=None, veto_max=0):
    """(GH, GW, 2G) int32, pixel by pixel."""
    group = np.asarray(group)
    key, _ = source_mask(id_map, len(group))
    H, W = key.shape
    GH, GW = grid_shape(H, W, cell, offset)
    out = np.zeros((GH, GW, 2 * G), np.int32)
    for y in range(H):
        for x in range(W):
            k = key[y, x]
            if k < 0 or group[k] >= G:
                continue
            veto = veto_d2 is not None and veto_d2[y, x] <= veto_max
            out[(y + offset[0]) // cell[0], (x + offset[1]) // cell[1], (G if veto else 0) + group[k]] += 1
    return out


def treatment(id_map, infos, cell, offset=(0, 0), margin=0, protect=0, target_labels=None, protect_labels=(), min_pixels=1):
    """`treatment_grid` for an (H, W) map and infos = [(id, label_id), ...]."""
    id_map = np.asarray(id_map)
    H, W = id_map.shape
    n = max((i for i, _ in infos), default=-1) + 1
    N = max(n, 1)
    target = np.zeros(N, bool)
    protected = np.zeros(N, bool)
    for i, label in infos:
        target[i] = label in target_labels if target_labels is not None else label not in protect_labels
        protected[i] = label in protect_labels
    grown = nearest_separable(id_map, N, int(Fraction(margin) ** 2 // 1), target, True)[0]
    veto_max = int(Fraction(protect) ** 2 // 1)
    veto_d2 = nearest_separable(id_map, N, veto_max, protected, False)[1] if protected.any() else None
    counts = cell_counts(grown, np.where(target, 0, 255), 1, cell, offset, veto_d2, veto_max)
    cells = counts[..., 0] >= min_pixels
    cy = (np.arange(H) + offset[0]) // cell[0]
    cx = (np.arange(W) + offset[1]) // cell[1]
    on = cells[cy][:, cx]
    key, _ = source_mask(id_map, N)
    rows = []
    for i, label in infos:
        if not target[i]:
            continue
        own = key == i
        a = int(own.sum())
        rows.append({"id": i, "label_id": label, "treated": int((own & on).sum()) / a if a else float("nan"),
                     "vetoed_fraction": ((int((own & (veto_d2 <= veto_max)).sum()) / a) if veto_d2 is not None else 0.0)
                     if a else float("nan")})
    return {"cells": cells, "coverage": counts[..., 0], "vetoed": counts[..., 1],
            "treated_fraction_exact": Fraction(int(on.sum()), H * W), "instances": rows, "grid_size": cells.shape}
