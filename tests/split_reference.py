"""A numpy restatement of the watershed split of touching instances (include/wm2f.h), written as the
rule reads: ascent of the squared interior distance to peaks, basins, and synchronous rounds that link a group under the
neighbour across its highest pass.  Pixels are visited by plain array passes; groups live in dicts.

- `split`: (out, info, status) as wm2f_labelmap_split writes them, from an id map and its d2.
- `split_map`: the same from the map alone, the distances from tests/distance_reference.py.
- `pieces`: the number of output ids that own a pixel.
- the hand cases of the tests: `discs`, `two_discs`, `dumbbell_with_bump`, `bar`, `disc_with_bud`, `three_discs`, and
  `ragged`, gaussian-filtered noise thresholded and labelled.
"""
import numpy as np

import distance_reference as D

LOW = 0xFFFFFFFF
_NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
_FORWARD = [(0, 1), (1, -1), (1, 0), (1, 1)]


def instance_ids(id_map, N):
    """(H, W) int64: the id in [0, N) of every pixel, -1 for everything else."""
    key = D.id_keys(id_map)
    return np.where((key >= 0) & (key < N), key, -1)


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` beyond the image."""
    H, W = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    b[yd, xd] = a[ys, xs]
    return b


def pixel_keys(d2):
    H, W = d2.shape
    lin = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    return (d2.astype(np.int64).astype(np.uint64) << np.uint64(32)) | (np.uint64(LOW) - lin)


def ascent(ids, d2):
    """up (H * W) int64: the linear index of the pixel of largest key among p and its 8 neighbours of p's id; p itself
    on background."""
    H, W = ids.shape
    key = pixel_keys(d2)
    best = key.copy()
    up = np.arange(H * W, dtype=np.int64).reshape(H, W).copy()
    lin = up.copy()
    for dy, dx in _NEIGHBOURS:
        same = (_shifted(ids, dy, dx, -2) == ids) & (ids >= 0)
        kq = _shifted(key, dy, dx, np.uint64(0))
        better = same & (kq > best)
        best = np.where(better, kq, best)
        up = np.where(better, _shifted(lin, dy, dx, 0), up)
    return up.reshape(-1)


def basins(ids, d2):
    """(H * W) int64: the peak every pixel ends at, following up; -1 on background."""
    lab = ascent(ids, d2)
    while True:
        nxt = lab[lab]
        if np.array_equal(nxt, lab):
            break
        lab = nxt
    return np.where(ids.reshape(-1) >= 0, lab, -1)


def split(id_map, d2, N, M, num, den, min_peak_d2=0, rounds=8):
    ids = instance_ids(id_map, N)
    H, W = ids.shape
    d2 = np.asarray(d2).astype(np.int64)
    flat_ids, flat_d2 = ids.reshape(-1), d2.reshape(-1)
    basin = basins(ids, d2)
    peaks = [int(p) for p in np.unique(basin[basin >= 0])]
    group = {p: p for p in peaks}  # basin (its peak pixel) -> group (its peak pixel)

    def key(p):
        return (int(flat_d2[p]) << 32) | (LOW - p)

    # the adjacent pairs of equal id in different basins, once: (basin of p, basin of q, pass height)
    pairs = {}
    bmap = basin.reshape(H, W)
    for dy, dx in _FORWARD:
        bq = _shifted(bmap, dy, dx, -1)
        sel = (ids >= 0) & (_shifted(ids, dy, dx, -2) == ids) & (bq != bmap)
        s = np.minimum(d2, _shifted(d2, dy, dx, 0))
        for a, b, h in zip(bmap[sel].tolist(), bq[sel].tolist(), s[sel].tolist()):
            e = (a, b) if a < b else (b, a)
            if pairs.get(e, -1) < h:
                pairs[e] = h

    last_links = 0
    for _ in range(rounds):
        best = {}
        for (a, b), s in pairs.items():
            ga, gb = group[a], group[b]
            if ga == gb:
                continue
            for g, other in ((ga, gb), (gb, ga)):
                cand = (s << 32) | (LOW - other)
                if cand > best.get(g, 0):
                    best[g] = cand
        link = {}
        for g, cand in best.items():
            s, other = cand >> 32, LOW - (cand & LOW)
            peak_d2 = int(flat_d2[g])
            if key(other) > key(g) and (peak_d2 < min_peak_d2 or s * den * den >= num * num * peak_d2):
                link[g] = other
        last_links = len(link)

        def root(g):
            while g in link:
                g = link[g]
            return g
        group = {b: root(g) for b, g in group.items()}

    # numbering
    roots = sorted(set(group.values()))
    keep = {}
    for g in roots:
        k = int(flat_ids[g])
        if k not in keep or key(g) > key(keep[k]):
            keep[k] = g
    new_id, nxt = {}, N
    for g in roots:  # ascending pixel index: raster order
        k = int(flat_ids[g])
        if keep[k] == g:
            new_id[g] = k
        else:
            new_id[g] = nxt
            nxt += 1
    info = np.tile(np.array([-1, -1, -1, 0], np.int32), (M, 1))
    for g, j in new_id.items():
        if j < M:
            info[j] = (int(flat_ids[g]), g % W, g // W, int(flat_d2[g]))
    out = np.full(H * W, -1, np.int32)
    inside = basin >= 0
    if peaks:
        lut = np.zeros(H * W, np.int64)
        for b, g in group.items():
            j = new_id[g]
            lut[b] = j if j < M else int(flat_ids[g])
        out[inside] = lut[basin[inside]]
    status = np.array([nxt, len(peaks), last_links, rounds], np.int32)
    return out.reshape(H, W), info, status


def split_map(id_map, N, M, num, den, min_peak_d2=0, rounds=8, border_outside=True):
    return split(id_map, D.squared_distance(np.asarray(id_map), border_outside), N, M, num, den, min_peak_d2, rounds)


def pieces(out):
    return len(np.unique(out[out >= 0]))


# ---------------------------------------------------------------------------------------------------- the hand cases
def discs(shape, spec, dtype=np.int32):
    """A map of -1 with the discs (cx, cy, radius, id) painted in this order."""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.full(shape, -1, dtype)
    for cx, cy, r, k in spec:
        m[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = k
    return m


def two_discs():
    """Two discs of radius 20 with centres 30 apart: the neck is 0.66 of the radius."""
    return discs((56, 86), [(28, 28, 20, 0), (58, 28, 20, 0)])


def dumbbell_with_bump():
    """Two discs of radius 20 joined by a bar 11 thick, with a disc of radius 9 sitting on the bar's middle: the bar is
    0.27 of the ends' clearance and 0.6 of the bump's."""
    m = discs((64, 130), [(30, 36, 20, 0), (100, 36, 20, 0)])
    m[31:42, 30:101] = 0
    m[discs((64, 130), [(65, 28, 9, 0)]) == 0] = 0
    return m


def bar():
    m = np.full((9, 46), -1, np.int32)
    m[2:7, 3:43] = 0
    return m


def disc():
    return discs((48, 48), [(24, 24, 20, 0)])


def disc_with_bud():
    """A disc of radius 50 with a bud of radius 10 whose centre lies 55 from the disc's."""
    return discs((112, 124), [(55, 55, 50, 0), (110, 55, 10, 0)])


def three_discs():
    """Radii 20 / 18 / 22 in a row, overlapping."""
    return discs((56, 120), [(24, 28, 20, 0), (54, 28, 18, 0), (88, 28, 22, 0)])


def ragged(side, seed, sigma=6.0, level=0.0):
    """Gaussian-filtered noise thresholded and 8-connected-labelled: an int32 id map with -1 background and its number of
    ids."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    field = ndimage.gaussian_filter(rng.standard_normal((side, side)), sigma)
    lab, n = ndimage.label(field > level * field.std(), structure=np.ones((3, 3), int))
    return (lab - 1).astype(np.int32), int(n)
