"""The tile merge of DESIGN section 28 (contract: include/wm2f.h, "merging the instances of overlapping tiles") restated in
plain numpy, and the generators of the cases the CPU and GPU tests share.  Nothing here imports the package's kernels.

Tables: geom (T, 6) rows (oy, ox, cy0, cy1, cx0, cx1); pairs (P, 8) rows (a, b, ay, ax, by, bx, h, w)."""
import numpy as np


# ------------------------------------------------------------------------------------------------ the contract
def slots(tile, n):
    """Per pixel 0 for "no id", id + 1 for an id in [0, n).  A float is the integer it equals (+-0 is 0); negative,
    fractional, non-finite and >= 2^24 values are no id."""
    tile = np.asarray(tile)
    if tile.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(tile) & (tile >= 0) & (tile == np.floor(tile)) & (tile < 2.0 ** 24)
        v = np.where(ok, tile, -1).astype(np.int64)
    else:
        v = tile.astype(np.int64)
    n = int(n)
    return np.where((v >= 0) & (v < n), v + 1, 0)


def _n(n_ids, t, N):
    return min(max(int(n_ids[t]), 0), N)


def pair_counts(tiles, n_ids, pairs, N):
    """hist (P, N+1, N+1): the joint histogram of the two tiles' slots over the pair's rectangle."""
    hist = np.zeros((len(pairs), N + 1, N + 1), np.int32)
    for p, (a, b, ay, ax, by, bx, h, w) in enumerate(np.asarray(pairs).reshape(-1, 8).tolist()):
        sa = slots(tiles[a][ay:ay + h, ax:ax + w], _n(n_ids, a, N))
        sb = slots(tiles[b][by:by + h, bx:bx + w], _n(n_ids, b, N))
        hist[p] = np.bincount((sa * (N + 1) + sb).reshape(-1), minlength=(N + 1) ** 2).reshape(N + 1, N + 1)
    return hist


def owned_counts(tiles, n_ids, geom, N):
    """owned (T, N): pixels of every id inside its tile's own cell."""
    owned = np.zeros((len(tiles), N), np.int32)
    for t, (oy, ox, cy0, cy1, cx0, cx1) in enumerate(np.asarray(geom).reshape(-1, 6).tolist()):
        s = slots(tiles[t][cy0 - oy:cy1 - oy, cx0 - ox:cx1 - ox], _n(n_ids, t, N))
        owned[t] = np.bincount(s.reshape(-1), minlength=N + 1)[1:]
    return owned


def link(hist, pairs, labels, n_ids, owned, num=1, den=2, return_roots=False):
    """remap (T, N) int32 and n_merged: the link rule on every inner bin, transitive closure with the smallest node as the
    root, sets that own a pixel numbered in ascending root order."""
    labels = np.asarray(labels)
    T, N = labels.shape
    parent = list(range(T * N))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for p, row in enumerate(np.asarray(pairs).reshape(-1, 8).tolist()):
        a, b = row[0], row[1]
        h = hist[p].astype(np.int64)
        area_a, area_b = h.sum(1), h.sum(0)
        for i1, j1 in zip(*np.nonzero(h[1:, 1:])):
            i, j = int(i1), int(j1)
            if i >= _n(n_ids, a, N) or j >= _n(n_ids, b, N) or labels[a, i] != labels[b, j]:
                continue
            inter = int(h[i + 1, j + 1])
            if inter * int(den) >= int(num) * min(int(area_a[i + 1]), int(area_b[j + 1])):
                ra, rb = find(a * N + i), find(b * N + j)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(g) for g in range(T * N)], np.int64).reshape(T, N)
    valid = np.arange(N)[None, :] < np.array([_n(n_ids, t, N) for t in range(T)])[:, None]
    owning = sorted(set(roots[valid & (np.asarray(owned) > 0)].tolist()))
    number = {r: k for k, r in enumerate(owning)}
    remap = np.full((T, N), -1, np.int32)
    for t in range(T):
        for i in range(N):
            if valid[t, i]:
                remap[t, i] = number.get(int(roots[t, i]), -1)
    return (remap, len(owning), roots) if return_roots else (remap, len(owning))


def compose(tiles, n_ids, geom, remap, H, W):
    """out (H, W) int32: every pixel is its owner tile's value through remap, -1 where that value is no id."""
    out = np.full((H, W), -2, np.int32)
    N = np.asarray(remap).shape[1]
    for t, (oy, ox, cy0, cy1, cx0, cx1) in enumerate(np.asarray(geom).reshape(-1, 6).tolist()):
        s = slots(tiles[t][cy0 - oy:cy1 - oy, cx0 - ox:cx1 - ox], _n(n_ids, t, N))
        table = np.concatenate([[-1], np.asarray(remap[t], np.int32)]).astype(np.int32)
        out[cy0:cy1, cx0:cx1] = table[s]
    assert (out != -2).all(), "the cells do not cover the image"
    return out


def merge(tiles, n_ids, labels, geom, pairs, H, W, num=1, den=2):
    """All four steps: a dict of hist, owned, remap, n_merged, out."""
    N = np.asarray(labels).shape[1]
    hist = pair_counts(tiles, n_ids, pairs, N)
    owned = owned_counts(tiles, n_ids, geom, N)
    remap, n_merged = link(hist, pairs, labels, n_ids, owned, num, den)
    return {"hist": hist, "owned": owned, "remap": remap, "n_merged": n_merged,
            "out": compose(tiles, n_ids, geom, remap, H, W)}


def expected_segments(remap, n_merged, infos):
    """The merged segments_info from remap and the tiles' segments_info lists, in plain loops."""
    merged = [{"id": k, "label_id": None, "score": None, "was_fused": False, "members": []} for k in range(n_merged)]
    for t, info in enumerate(infos):
        for s in info:
            k = int(remap[t][s["id"]])
            if k >= 0:
                merged[k]["members"].append((t, s["id"]))
                merged[k]["label_id"] = s["label_id"] if merged[k]["label_id"] is None else merged[k]["label_id"]
                merged[k]["score"] = s["score"] if merged[k]["score"] is None else max(merged[k]["score"], s["score"])
    return merged


# ------------------------------------------------------------------------------------------------ shared cases
# (H, W, tile, overlap): the geometries pinned in the CPU tests
GEOMETRIES = [(97, 131, 64, 16), (64, 200, 64, 24), (150, 150, 64, 31), (129, 65, 64, 0), (200, 300, 96, 47),
              (40, 50, 64, 16), (128, 64, 64, 0)]


def scene(H, W, seed):
    """(H, W) int32 ids with -1 background and the label of every object: disjoint rectangles, one per 24 x 26 cell, and
    a one-pixel row across the whole image painted last."""
    rng = np.random.default_rng(seed)
    m = np.full((H, W), -1, np.int32)
    k = 0
    for y in range(0, H, 24):
        for x in range(0, W, 26):
            ch, cw = min(24, H - y), min(26, W - x)
            if ch < 3 or cw < 3:
                continue
            h, w = int(rng.integers(2, ch)), int(rng.integers(2, cw))
            y0, x0 = y + int(rng.integers(0, ch - h)), x + int(rng.integers(0, cw - w))
            m[y0:y0 + h, x0:x0 + w] = k
            k += 1
    m[int(rng.integers(0, H))] = k
    present = np.unique(m[m >= 0])  # the row may have painted a thin rectangle over
    m = np.where(m >= 0, np.searchsorted(present, m), -1).astype(np.int32)
    labels = rng.integers(0, 2, len(present)).astype(np.int32)
    return m, labels


def cut_scene(m, obj_labels, windows, n_perm, N, seed):
    """Exact crops of the scene, every tile renumbered by a random permutation into [0, n_perm): tiles (T, th, tw) int32,
    n_ids (T), labels (T, N) (random where no object stands)."""
    rng = np.random.default_rng(seed)
    T = len(windows)
    tiles, labels = [], rng.integers(0, 2, (T, N)).astype(np.int32)
    for t, (y0, x0, y1, x1) in enumerate(windows):
        crop = m[y0:y1, x0:x1]
        here = np.unique(crop[crop >= 0])
        assert len(here) <= n_perm
        new = rng.permutation(n_perm)[:len(here)]
        table = np.full(int(m.max()) + 2, -1, np.int32)
        table[here] = new
        tiles.append(np.where(crop >= 0, table[crop], -1).astype(np.int32))
        labels[t, new] = obj_labels[here]
    return np.stack(tiles), np.full(T, n_perm, np.int32), labels


def random_blocks(T, th, tw, N, seed):
    """Every tile on its own: random 4 x 4 blocks with ids in [-1, 6) and random labels in {0, 1} -- many pairs sit near
    the threshold and the sets chain."""
    rng = np.random.default_rng(seed)
    by, bx = -(-th // 4), -(-tw // 4)
    small = rng.integers(-1, 6, (T, by, bx))
    tiles = np.repeat(np.repeat(small, 4, 1), 4, 2)[:, :th, :tw].astype(np.int32)
    return tiles, np.full(T, min(6, N), np.int32), rng.integers(0, 2, (T, N)).astype(np.int32)


def same_up_to_bijection(out, truth):
    """out equals truth up to a bijection of the ids, background (-1) to background."""
    if out.shape != truth.shape or ((out < 0) != (truth < 0)).any():
        return False
    pairs = np.unique(np.stack([out[out >= 0], truth[truth >= 0]]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))
