"""The contracts of wm2f_labelmap_skeleton_prune and wm2f_labelmap_skeleton_graph (include/wm2f.h)
restated in numpy: array passes and one `scipy.ndimage.label` per key, a literal flood-fill reading for small maps, and
the maps the skeleton-graph tests share.

- `classes(s)`: (b, X, node, path, free) of a decoded (H, W) state.
- `components(s)`: (comp, node): the label (smallest linear index) of every live pixel's component, -1 for a dead one.
- `records(s, d2)`: the branch records as arrays indexed by branch label.
- `spurs(s, d2, min_pixels, ratio_q)`: the bool mask of the pixels one round deletes.
- `prune(skel, d2, N, ...)`: (out, status) as the kernel writes them, for one (H, W) map or a (B, H, W) stack.
- `graph(skel, N=None, ids=None)`: (labels, sums) as the kernel writes them.
- `graph_literal(skel, N)`, `prune_literal(...)`: the same of one small map, one pixel at a time.
- `traits(sums)`: the graph traits of `skeleton_graph_statistics` from the integer rows.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage

import skeleton_reference as S

EIGHT = np.ones((3, 3), int)
GRAPH_COLUMNS = 8
P_CAP = 1 << 20


# ---- classes ----------------------------------------------------------------------------------------------------------
def classes(s: np.ndarray):
    p = S._neighbours(s)
    b = sum(q.astype(np.int64) for q in p)
    X = sum((~p[k] & p[(k + 1) % 8]).astype(np.int64) for k in range(8))
    live = s >= 0
    node = live & (b >= 3)
    path = live & (b <= 2)
    free = path & ((b <= 1) | ((b == 2) & (X == 1)))
    return b, X, node, path, free


def components(s: np.ndarray):
    """comp (H, W) int64: the smallest linear index of the 8-connected set of equal key 2 k + [node] a live pixel lies
    in, -1 for a dead pixel; and the node mask."""
    H, W = s.shape
    _, _, node, _, _ = classes(s)
    key = np.where(s >= 0, 2 * s.astype(np.int64) + node, -1)
    lin = np.arange(H * W, dtype=np.int64).reshape(H, W)
    comp = np.full((H, W), -1, np.int64)
    for kv in np.unique(key[key >= 0]):
        lab, n = ndimage.label(key == kv, structure=EIGHT)
        first = np.asarray(ndimage.minimum(lin, lab, np.arange(1, n + 1))).astype(np.int64)
        comp[lab > 0] = first[lab[lab > 0] - 1]
    return comp, node


def _shift(a: np.ndarray, dy: int, dx: int, fill):
    """a[y + dy, x + dx], `fill` outside the image."""
    H, W = a.shape
    pad = np.full((H + 2, W + 2), fill, a.dtype)
    pad[1:-1, 1:-1] = a
    return pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def records(s: np.ndarray, d2: np.ndarray | None = None):
    """Arrays of H * W entries indexed by branch label: P, T, contacts, cmin, cmax, D; and (comp, node, path)."""
    H, W = s.shape
    n = H * W
    _, _, node, path, free = classes(s)
    comp, _ = components(s)
    dd = np.zeros((H, W), np.int64) if d2 is None else np.maximum(np.asarray(d2).astype(np.int64), 0)
    P = np.bincount(comp[path], minlength=n)
    T = np.bincount(comp[free], minlength=n)
    contacts = np.zeros(n, np.int64)
    cmin, cmax, D = np.full(n, n, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for dy, dx in S.OFFSETS:
        touch = path & _shift(node, dy, dx, False) & (_shift(s, dy, dx, -1) == s)
        br, cl, dq = comp[touch], _shift(comp, dy, dx, -1)[touch], _shift(dd, dy, dx, 0)[touch]
        contacts += np.bincount(br, minlength=n)
        np.minimum.at(cmin, br, cl)
        np.maximum.at(cmax, br, cl)
        np.maximum.at(D, br, dq)
    return P, T, contacts, cmin, cmax, D, comp, node, path


def spurs(s: np.ndarray, d2: np.ndarray, min_pixels: int, ratio_q: int) -> np.ndarray:
    P, T, contacts, cmin, cmax, D, comp, _, path = records(s, d2)
    Pc = np.minimum(P, P_CAP)  # Python-int-safe: 256 * 2^40 and 2^20 * 2^31 both fit an int64
    spur = (T >= 1) & (contacts > 0) & (cmin == cmax) & ((P <= min_pixels) | (256 * Pc * Pc <= int(ratio_q) ** 2 * D))
    return path & spur[np.where(comp >= 0, comp, 0)]


# ---- the two entry points -----------------------------------------------------------------------------------------------
def _state(skel, N: int) -> np.ndarray:
    v = np.asarray(skel).astype(np.int64)
    return np.where((v >= 0) & (v < N), v, -1).astype(np.int32)


def prune_round(s: np.ndarray, d2: np.ndarray, min_pixels: int, ratio_q: int, rethin: int) -> np.ndarray:
    s = np.where(spurs(s, d2, min_pixels, ratio_q), -1, s).astype(np.int32)
    t = s[None]
    for _ in range(int(rethin)):
        t, _ = S.iterate(t)
    return t[0]


def prune(skel, d2, N: int, min_pixels: int = 2, ratio_q: int = 16, rounds: int = 8, rethin: int = 4):
    a, d = np.asarray(skel), np.asarray(d2)
    stack, dd = (a, d) if a.ndim == 3 else (a[None], d[None])
    outs, status = [], []
    for m, e in zip(stack, dd):
        s = _state(m, N)
        first = int((s >= 0).sum())
        busy, last = 0, 0
        for _ in range(int(rounds)):
            before = int((s >= 0).sum())
            s = prune_round(s, e, min_pixels, ratio_q, rethin)
            last = before - int((s >= 0).sum())
            busy += last > 0
        left = int((s >= 0).sum())
        outs.append(s)
        status.append([left, busy, last, first - left])
    out, status = np.stack(outs), np.array(status, np.int32)
    return (out, status) if a.ndim == 3 else (out[0], status[0])


def settles_in(skel, d2, N: int, min_pixels: int = 2, ratio_q: int = 16, rethin: int = 4, limit: int = 64) -> int:
    """The rounds that remove something, of one (H, W) map."""
    s = _state(skel, N)
    for n in range(limit):
        t = prune_round(s, np.asarray(d2), min_pixels, ratio_q, rethin)
        if np.array_equal(t, s):
            return n
        s = t
    raise RuntimeError("no fixed point within the limit")


def _sums_of(s: np.ndarray, rows_of) -> tuple:
    P, T, contacts, cmin, cmax, _, comp, node, path = records(s)
    labels = np.where(s < 0, -1, np.where(node, -2 - comp, comp)).astype(np.int32)
    sums = np.zeros((len(rows_of), GRAPH_COLUMNS), np.int64)
    for r, k in enumerate(rows_of):
        sel = s == k
        if k < 0 or not sel.any():
            continue
        br = np.unique(comp[sel & path])
        end = br[(T[br] >= 1) & (contacts[br] > 0)]
        sums[r] = [len(br), len(end), len(np.unique(comp[sel & node])), int((sel & node).sum()), int(T[br].sum()),
                   int(P[end].max()) if len(end) else 0, int(P[br].max()) if len(br) else 0,
                   int(((T[br] == 0) & ((contacts[br] == 0) | (cmin[br] == cmax[br]))).sum())]
    return labels, sums


def graph(skel, N: int | None = None, ids=None):
    """(labels, sums) of the ids 0 .. N-1, or of the raw ids listed in `ids` (in that order; a pixel whose value is not
    listed is dead), of one (H, W) int32 map or a (B, H, W) stack."""
    a = np.asarray(skel)
    stack = a if a.ndim == 3 else a[None]
    rows_of = list(range(int(N))) if ids is None else [int(v) for v in ids]
    alive = [k for k in rows_of if k >= 0]
    labels, sums = [], []
    for m in stack:
        v = m.astype(np.int64)
        s = np.where(np.isin(v, alive), v, -1).astype(np.int32)
        l, r = _sums_of(s, rows_of)
        labels.append(l)
        sums.append(r)
    labels, sums = np.stack(labels), np.stack(sums)
    return (labels, sums) if a.ndim == 3 else (labels[0], sums[0])


def traits(sums: np.ndarray) -> dict:
    sums = np.asarray(sums, np.int64)
    return {"branches": sums[..., 0], "end_branches": sums[..., 1], "nodes": sums[..., 2], "longest_end_branch": sums[..., 5],
            "longest_branch": sums[..., 6], "closed_branches": sums[..., 7]}


# ---- a literal reading: flood fills, one pixel at a time ----------------------------------------------------------------
def _ring(s, y, x):
    H, W = s.shape
    return [0 <= y + dy < H and 0 <= x + dx < W and s[y + dy, x + dx] == s[y, x] for dy, dx in S.OFFSETS]


def graph_literal(skel, N: int):
    """(labels, branch records {label: dict}, cluster labels) of one small map."""
    s = _state(skel, N)
    H, W = s.shape
    kind = {}  # (y, x) -> (is node, is free end)
    for y in range(H):
        for x in range(W):
            if s[y, x] < 0:
                continue
            p = _ring(s, y, x)
            b = sum(p)
            X = sum((not p[i]) and p[(i + 1) % 8] for i in range(8))
            kind[(y, x)] = (b >= 3, b <= 1 or (b == 2 and X == 1))
    label = {}
    for start in sorted(kind):  # row-major: the first pixel met of a component has its smallest linear index
        if start in label:
            continue
        todo, label[start] = [start], start[0] * W + start[1]
        while todo:
            y, x = todo.pop()
            for dy, dx in S.OFFSETS:
                q = (y + dy, x + dx)
                if q in kind and q not in label and s[q] == s[y, x] and kind[q][0] == kind[(y, x)][0]:
                    label[q] = label[start]
                    todo.append(q)
    labels = np.full((H, W), -1, np.int32)
    rec = {}
    for (y, x), (node, free) in kind.items():
        labels[y, x] = -2 - label[(y, x)] if node else label[(y, x)]
        if node:
            continue
        r = rec.setdefault(label[(y, x)], {"P": 0, "T": 0, "clusters": [], "id": int(s[y, x])})
        r["P"] += 1
        r["T"] += int(free)
        for dy, dx in S.OFFSETS:
            q = (y + dy, x + dx)
            if q in kind and s[q] == s[y, x] and kind[q][0]:
                r["clusters"].append((label[q], q))
    clusters = {(int(s[q]), l) for q, l in label.items() if kind[q][0]}
    return labels, rec, clusters


def prune_literal(skel, d2, N: int, min_pixels: int, ratio_q: int, rounds: int, rethin: int) -> np.ndarray:
    s = _state(skel, N)
    d2 = np.asarray(d2)
    for _ in range(int(rounds)):
        labels, rec, _ = graph_literal(s, N)
        for l, r in rec.items():
            if r["T"] < 1 or not r["clusters"] or len({c for c, _ in r["clusters"]}) != 1:
                continue
            D = max(max(int(d2[q]), 0) for _, q in r["clusters"])
            P = min(r["P"], P_CAP)
            if r["P"] <= min_pixels or 256 * P * P <= ratio_q * ratio_q * D:
                s[labels == l] = -1
        s = S.skeleton_literal(s, N, rethin)
    return s


# ---- the maps the tests share -------------------------------------------------------------------------------------------
def plant(H, W, cy, cx, leaves, L, wd, seed, noise, phase=0.3):
    rng = np.random.default_rng(seed); yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    m = (yy-cy)**2 + (xx-cx)**2 <= (wd*1.2)**2
    for i in range(leaves):
        a = phase + 2*np.pi*i/leaves
        u = (xx-cx)*np.cos(a) + (yy-cy)*np.sin(a); v = -(xx-cx)*np.sin(a) + (yy-cy)*np.cos(a)
        m |= ((u - L/2)/(L/2))**2 + (v/wd)**2 <= 1.0
    by, bx = np.nonzero(m & ~ndimage.binary_erosion(m))
    for j in rng.choice(len(by), int(noise*len(by)), replace=False):
        r = rng.integers(1, 3); m |= (yy-by[j])**2 + (xx-bx[j])**2 <= r*r
    return m


# (leaves, L, wd, noise): the four plants of the issue's table, at 140 x 140, centre 70, seeds 1 .. 3
PLANTS = ((5, 50, 6, 0.08), (3, 40, 9, 0.08), (7, 56, 4, 0.1), (2, 60, 3, 0.1))


def plant_map(leaves, L, wd, noise, seed) -> np.ndarray:
    return np.where(plant(140, 140, 70, 70, leaves, L, wd, seed, noise), 0, -1).astype(np.int32)


def tips(skel, N: int) -> int:
    return int(S.skeleton_stats(skel, N)[..., 3].sum())


def _blank(H, W):
    return np.full((H, W), -1, np.int32)


def hand_t():
    """A bar with a 2-pixel stem below its middle: the stem is a spur by `min_pixels` alone (d2 = 1 everywhere)."""
    m = _blank(12, 16)
    m[4, 2:14] = 0
    m[5:7, 8] = 0
    return m, np.ones_like(m), 1


def hand_plus():
    """A "+" with arms of 7 pixels: four end branches on one node cluster, none of them a spur."""
    m = _blank(17, 17)
    m[8, 1:16] = 0
    m[1:16, 8] = 0
    return m, np.ones_like(m), 1


def hand_line_and_pixel():
    """An isolated diagonal line (id 0) and a single pixel (id 1): no contact, never touched."""
    m = _blank(12, 12)
    m[np.arange(2, 9), np.arange(1, 8)] = 0
    m[2, 9] = 1
    return m, np.full_like(m, 100), 2


def hand_ring():
    """The thinned ring of an annulus with a 2-pixel spur on its outside: the spur goes, the hole stays."""
    yy, xx = np.mgrid[0:40, 0:40]
    r2 = (yy - 20) ** 2 + (xx - 20) ** 2
    ring, _ = S.skeleton(np.where((r2 >= 100) & (r2 <= 196), 0, -1).astype(np.int32), 1, 64)
    y = 20
    x = int(np.nonzero(ring[y] == 0)[0].max())
    ring = ring.copy()
    ring[y, x + 1:x + 3] = 0
    return ring, np.full_like(ring, 4), 1


def hand_two_ids():
    """Two T's of different ids whose bars touch end to end: each is pruned as it would be alone."""
    m = _blank(12, 28)
    m[4, 2:14] = 0
    m[5:7, 8] = 0
    m[4, 14:26] = 1
    m[5:7, 20] = 1
    return m, np.ones_like(m), 2


HAND = {"t": hand_t, "plus": hand_plus, "line_and_pixel": hand_line_and_pixel, "ring": hand_ring, "two_ids": hand_two_ids}


def across_corners():
    """A 130 x 130 skeleton map laid over the labelling tile's corner (32, 32) and the thinning tile's corner (64, 64):
    id 0 a "+" whose node cluster has a pixel in each of the four tiles around (32, 32), with a diagonal spur out of that
    cluster (two path pixels: a spur by `min_pixels`) and a spur of three path pixels up from its right arm (a spur by the
    ratio, at equality: 256 * 3^2 = 16^2 * 9); id 1 the same around (64, 64); id 2 a line along the tile border y = 32
    with a 3-pixel spur, a line that alternates between the rows 63 and 64, and a line down the border column x = 96.
    d2 = 9 everywhere (a half-width of 3)."""
    m = _blank(130, 130)
    for k, c in ((0, 32), (1, 64)):
        m[c, c - 20:c + 20] = k       # the row below the corner
        m[c - 20:c + 20, c - 1] = k   # the column left of it
        for i in range(3):
            m[c - 1 - i, c + i] = k   # out of the node cluster, across the corner
        m[c - 4:c, c + 8] = k
    m[32, 70:128] = 2
    m[29:32, 100] = 2
    xs = np.arange(90, 128)
    m[63 + (xs % 2), xs] = 2
    m[70:128, 96] = 2
    return m, np.full_like(m, 9), 3
