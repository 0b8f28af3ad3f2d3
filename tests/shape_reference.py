"""The contracts of wm2f_labelmap_shape_stats and wm2f_labelmap_hull (include/wm2f.h) restated in numpy
and scipy: a plain loop over ids, one mask each.  Nothing here shares the kernels' algorithm: sums come from np.nonzero,
the border counts from scipy.ndimage's erosion and convolution (skimage.measure.perimeter's own steps), the sides from
differences of the padded mask, the hull from scipy.spatial.ConvexHull of all four corners of all pixels."""
import numpy as np
from scipy import ndimage
from scipy.spatial import ConvexHull

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
KERNEL = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
STRAIGHT, DIAG, MIXED = (5, 7, 15, 17, 25, 27), (21, 33), (13, 23)


def mask_shape_row(mask):
    """A bool mask -> the 10 integers [area, sx, sy, sxx, syy, sxy, sides, p_straight, p_diag, p_mixed]."""
    mask = np.asarray(mask, bool)
    ys, xs = (v.astype(np.int64) for v in np.nonzero(mask))
    if len(ys) == 0:
        return [0] * 10
    border = mask & ~ndimage.binary_erosion(mask, CROSS, border_value=0)
    codes = np.bincount(ndimage.convolve(border.astype(np.int64), KERNEL, mode="constant", cval=0)[border], minlength=50)
    padded = np.pad(mask, 1).astype(np.int8)
    sides = int(np.abs(np.diff(padded, axis=0)).sum() + np.abs(np.diff(padded, axis=1)).sum())
    return [len(ys), xs.sum(), ys.sum(), (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum(), sides,
            int(codes[list(STRAIGHT)].sum()), int(codes[list(DIAG)].sum()), int(codes[list(MIXED)].sum())]


def mask_hull(mask):
    """A bool mask -> ([n_vertices, area2, feret2], vertices (n, 2) int64 (x, y)): the hull of the corners of the pixel
    squares, strictly convex, from the vertex with the smallest (y, then x) on towards increasing x."""
    ys, xs = np.nonzero(np.asarray(mask, bool))
    if len(ys) == 0:
        return [0, 0, 0], np.zeros((0, 2), np.int64)
    pts = np.unique(np.concatenate([np.stack([xs + dx, ys + dy], 1) for dx in (0, 1) for dy in (0, 1)]), axis=0).astype(np.int64)
    h = ConvexHull(pts)  # Qhull drops collinear points from `vertices`
    v = pts[h.vertices]  # counter-clockwise in a y-up frame
    e, f = np.roll(v, -1, 0) - v, np.roll(v, -2, 0) - np.roll(v, -1, 0)
    cross = e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]  # (b - a) x (c - b) of consecutive vertices a, b, c
    assert (cross != 0).all() and len(set(np.sign(cross))) == 1
    if cross[0] < 0:
        v = v[::-1]
    start = min(range(len(v)), key=lambda i: (v[i, 1], v[i, 0]))
    v = np.roll(v, -start, 0)
    d = v[:, None, :] - v[None, :, :]
    return [len(v), int(round(2 * h.volume)), int((d * d).sum(-1).max())], v


def _ids_of(N, ids):
    return [(r if ids is None else (ids[r] if r < len(ids) else None)) for r in range(N)]


def shape_stats_reference(m, ids=None, N=None):
    """(H, W) map -> (N, 10) int64.  ids None: row r is id r of [0, N); else row r is the raw id ids[r], later rows empty."""
    m = np.asarray(m)
    N = len(ids) if N is None else N
    out = np.zeros((N, 10), np.int64)
    for r, v in enumerate(_ids_of(N, ids)):
        if v is not None:
            out[r] = mask_shape_row(m == v)
    return out


def hull_reference(m, ids=None, N=None):
    """(H, W) map -> (hull (N, 3) int64, [vertices (n_r, 2) int64 per row])."""
    m = np.asarray(m)
    N = len(ids) if N is None else N
    out, verts = np.zeros((N, 3), np.int64), []
    for r, v in enumerate(_ids_of(N, ids)):
        row, pts = mask_hull(m == v) if v is not None else ([0, 0, 0], np.zeros((0, 2), np.int64))
        out[r] = row
        verts.append(pts)
    return out, verts


def ellipse_scene(rng, shape, N, dtype=np.int32, knock=0.08, background=-1):
    """Random rotated ellipses of ids 0 .. N-1 painted over one another (later ids hide earlier ones, some wholly), then
    about `knock` of the pixels set to background: holes, ragged edges, disconnected pieces."""
    H, W = shape
    m = np.full(shape, background, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(N):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        a, b = rng.uniform(2, max(3, 0.45 * min(H, W))), rng.uniform(1, max(2, 0.2 * min(H, W)))
        t = rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)
        w = -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
        m[(u / a) ** 2 + (w / b) ** 2 <= 1] = k
    m[rng.random(shape) < knock] = background
    return m.astype(dtype)
