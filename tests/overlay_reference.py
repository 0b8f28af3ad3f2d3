"""The contract of wm2f_labelmap_overlay (include/wm2f.h) restated in numpy, in two independent forms:

- `overlay_reference`: per pixel, the maximum over the contour candidates (the header's "equivalently" form);
- `overlay_painter`: the structure of models/model_utils.py::plot_segmentation -- fills first, then a loop over the
  segments in painter's order, each painting (s & dilate(~s, inner)) | (~s & dilate(s, outer)) over what is there.

Both take ONE image: image (H, W, 3) uint8, map (H, W) float32 / int32 / uint8, ids (n) ascending, rgba (n, 4) uint8,
order (n) int, default_rgba four bytes.  Nothing here runs on a GPU or imports the package.
"""
import numpy as np


def entries_of(seg, ids):
    """(H, W) int64: the position of every pixel's value in the ascending list `ids`, -1 for a value that is not listed.
    A float value counts as the integer it equals; negative, fractional, non-finite or >= 2^24: not listed."""
    seg = np.asarray(seg)
    ids = np.asarray(ids, np.int64).reshape(-1)
    assert np.all(np.diff(ids) > 0), "ids must be ascending"
    if seg.dtype.kind == "f":
        ok = np.isfinite(seg) & (seg >= 0) & (seg < 2.0 ** 24)
        safe = np.where(ok, seg, 0.0)
        ok &= safe == np.floor(safe)
        val = np.where(ok, safe, -1.0).astype(np.int64)
    else:
        ok = np.ones(seg.shape, bool)
        val = seg.astype(np.int64)
    ent = np.full(seg.shape, -1, np.int64)
    if len(ids):
        pos = np.clip(np.searchsorted(ids, val), 0, len(ids) - 1)
        hit = ok & (ids[pos] == val)
        ent[hit] = pos[hit]
    return ent


def blend_fill(image, ent, rgba, default_rgba):
    """out_c = (image_c * (255 - a) + col_c * a + 127) // 255 with (col, a) of the pixel's entry, or the default."""
    table = np.concatenate([np.asarray(rgba, np.int64).reshape(-1, 4), np.asarray(default_rgba, np.int64).reshape(1, 4)])
    col = table[np.where(ent >= 0, ent, len(table) - 1)]  # (H, W, 4)
    a = col[..., 3:4]
    return ((image.astype(np.int64) * (255 - a) + col[..., :3] * a + 127) // 255).astype(np.uint8)


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` where that lies outside the array."""
    H, W = a.shape
    b = np.full_like(a, fill)
    if abs(dy) >= H or abs(dx) >= W:
        return b
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    b[yd, xd] = a[ys, xs]
    return b


def _diamond(r):
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if 0 < abs(dy) + abs(dx) <= r]


def overlay_reference(image, seg, ids, rgba, order, default_rgba=(0, 0, 0, 0), inner=1, outer=1):
    """Per pixel: the candidates are e(p) when a differing in-image neighbour lies within `inner`, and e(q) of every
    differing neighbour within `outer`; none and negative orders are skipped; the greatest (order, entry) wins."""
    image = np.asarray(image)
    rgba = np.asarray(rgba, np.uint8).reshape(-1, 4)
    order = np.asarray(order, np.int64).reshape(-1)
    ent = entries_of(seg, ids)
    out = blend_fill(image, ent, rgba, default_rgba)
    n = len(order)
    OUTSIDE = -2
    # key of a candidate entry: order * (n + 1) + entry, -1 when it may not draw
    key_ent = np.full(ent.shape, -1, np.int64)
    if n:
        key_of = np.where(order >= 0, order * (n + 1) + np.arange(n), -1)
        key_ent = np.where(ent >= 0, key_of[np.maximum(ent, 0)], -1)
    best = np.full(ent.shape, -1, np.int64)
    differs_inside = np.zeros(ent.shape, bool)
    for dy, dx in _diamond(max(inner, outer)):
        d = abs(dy) + abs(dx)
        q = _shift(ent, dy, dx, OUTSIDE)
        differs = (q != OUTSIDE) & (q != ent)
        if d <= inner:
            differs_inside |= differs
        if d <= outer:
            kq = _shift(key_ent, dy, dx, -1)
            best = np.maximum(best, np.where(differs, kq, -1))
    best = np.maximum(best, np.where(differs_inside, key_ent, -1))
    on = best >= 0
    if n:
        out[on] = rgba[best[on] % (n + 1), :3]
    return out


def _dilate(mask, r):
    """Diamond dilation by array shifts: nothing outside the array is counted.  r == 0 gives nothing (no neighbours)."""
    acc = np.zeros_like(mask)
    for dy, dx in _diamond(r):
        acc |= _shift(mask, dy, dx, False)
    return acc


def overlay_painter(image, seg, ids, rgba, order, default_rgba=(0, 0, 0, 0), inner=1, outer=1):
    """Fills, then every entry of non-negative order in ascending (order, entry) paints its contour over the rest."""
    image = np.asarray(image)
    rgba = np.asarray(rgba, np.uint8).reshape(-1, 4)
    order = np.asarray(order, np.int64).reshape(-1)
    ent = entries_of(seg, ids)
    out = blend_fill(image, ent, rgba, default_rgba)
    for s in sorted(range(len(order)), key=lambda i: (order[i], i)):
        if order[s] < 0:
            continue
        m = ent == s
        ring = (m & _dilate(~m, inner)) | (~m & _dilate(m, outer))
        out[ring] = rgba[s, :3]
    return out


def overlay_batch(fn, images, segs, ids, n_ids, rgba, order, default_rgba, inner, outer):
    """The batched arguments of `ops.labelmap_overlay` (numpy) through a one-image form `fn`."""
    return np.stack([fn(images[b], segs[b], ids[b][:n_ids[b]], rgba[b][:n_ids[b]], order[b][:n_ids[b]], default_rgba,
                        inner, outer) for b in range(len(images))])
