"""The contracts of wm2f_labelmap_skeleton and wm2f_labelmap_skeleton_stats (include/wm2f.h) restated
in numpy with array passes, a literal pixel-by-pixel reading of the thinning rule for small maps, and the maps the
skeleton tests share.

- `decode(maps, N)`: the int32 state of a typed map, id in [0, N) or -1.
- `skeleton(maps, N, rounds)`: (out, status) as the kernel writes them, for one (H, W) map or a (B, H, W) stack.
- `skeleton_literal(map, N, rounds)`: the same `out` of one small map, one pixel at a time.
- `settles_in(maps, N)`: the iterations that delete something (so `rounds` >= this settles every image).
- `skeleton_stats(skel, N=None, ids=None, d2=None)`: the (..., N, 8) int64 rows.
- `traits(rows, area)`: the float traits of `skeleton_statistics` from those integers (numpy float64).
"""
from __future__ import annotations

import numpy as np

# (dy, dx) of p2 .. p9: N, NE, E, SE, S, SW, W, NW
OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def decode(maps, N: int) -> np.ndarray:
    a = np.asarray(maps)
    if a.dtype.kind == "f":
        ok = np.isfinite(a) & (a == np.floor(np.where(np.isfinite(a), a, 0))) & (a >= 0) & (a < N)
        return np.where(ok, np.where(ok, a, 0).astype(np.int64), -1).astype(np.int32)
    v = a.astype(np.int64)
    return np.where((v >= 0) & (v < N), v, -1).astype(np.int32)


def _neighbours(s: np.ndarray):
    """p2 .. p9 of a (..., H, W) state as bool arrays: inside the image, alive and of the centre's id."""
    H, W = s.shape[-2:]
    pad = np.full(s.shape[:-2] + (H + 2, W + 2), -1, s.dtype)
    pad[..., 1:-1, 1:-1] = s
    live = s >= 0
    return [(pad[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == s) & live for dy, dx in OFFSETS]


def _deletable(p, j: int):
    p2, p3, p4, p5, p6, p7, p8, p9 = p
    i = lambda a: a.astype(np.int32)
    C = i(~p2 & (p3 | p4)) + i(~p4 & (p5 | p6)) + i(~p6 & (p7 | p8)) + i(~p8 & (p9 | p2))
    N1 = i(p9 | p2) + i(p3 | p4) + i(p5 | p6) + i(p7 | p8)
    N2 = i(p2 | p3) + i(p4 | p5) + i(p6 | p7) + i(p8 | p9)
    Nm = np.minimum(N1, N2)
    m = ((p6 | p7 | ~p9) & p8) if j == 0 else ((p2 | p3 | ~p5) & p4)
    return (C == 1) & (Nm >= 2) & (Nm <= 3) & ~m


def iterate(s: np.ndarray):
    """One iteration of a (B, H, W) state -> (new state, deletions per image)."""
    gone = np.zeros(s.shape[0], np.int64)
    for j in (0, 1):
        d = _deletable(_neighbours(s), j) & (s >= 0)
        gone += d.sum(axis=(-2, -1))
        s = np.where(d, -1, s).astype(np.int32)
    return s, gone


def skeleton(maps, N: int, rounds: int):
    a = np.asarray(maps)
    s = decode(a if a.ndim == 3 else a[None], N)
    B = s.shape[0]
    busy, last = np.zeros(B, np.int64), np.zeros(B, np.int64)
    done = False
    for _ in range(int(rounds)):
        if done:  # a fixed point: every later iteration deletes nothing
            last[:] = 0
            continue
        s, gone = iterate(s)
        busy += gone > 0
        last = gone
        done = not gone.any()
    status = np.stack([(s >= 0).sum(axis=(-2, -1)), busy, last, np.full(B, int(rounds))], -1).astype(np.int32)
    return (s, status) if a.ndim == 3 else (s[0], status[0])


def settles_in(maps, N: int, limit: int = 4096) -> int:
    a = np.asarray(maps)
    s = decode(a if a.ndim == 3 else a[None], N)
    n = 0
    while n < limit:
        s, gone = iterate(s)
        if not gone.any():
            return n
        n += 1
    raise RuntimeError("no fixed point within the limit")


def skeleton_literal(m, N: int, rounds: int) -> np.ndarray:
    s = decode(np.asarray(m), N)
    H, W = s.shape
    for _ in range(int(rounds)):
        for j in (0, 1):
            gone = []
            for y in range(H):
                for x in range(W):
                    k = s[y, x]
                    if k < 0:
                        continue
                    p = [0 <= y + dy < H and 0 <= x + dx < W and s[y + dy, x + dx] == k for dy, dx in OFFSETS]
                    p2, p3, p4, p5, p6, p7, p8, p9 = p
                    C = int(not p2 and (p3 or p4)) + int(not p4 and (p5 or p6)) + int(not p6 and (p7 or p8)) + int(not p8 and (p9 or p2))
                    N1 = int(p9 or p2) + int(p3 or p4) + int(p5 or p6) + int(p7 or p8)
                    N2 = int(p2 or p3) + int(p4 or p5) + int(p6 or p7) + int(p8 or p9)
                    m_j = ((p6 or p7 or not p9) and p8) if j == 0 else ((p2 or p3 or not p5) and p4)
                    if C == 1 and 2 <= min(N1, N2) <= 3 and not m_j:
                        gone.append((y, x))
            for y, x in gone:
                s[y, x] = -1
    return s


STAT_COLUMNS = 8


def skeleton_stats(skel, N: int | None = None, ids=None, d2=None) -> np.ndarray:
    """Rows of the ids 0 .. N-1, or of the raw ids listed in `ids` (in that order), of an int32 skeleton map."""
    s = np.asarray(skel).astype(np.int32)
    stack = s if s.ndim == 3 else s[None]
    dd = None if d2 is None else (np.asarray(d2) if s.ndim == 3 else np.asarray(d2)[None]).astype(np.int64)
    rows_of = list(range(int(N))) if ids is None else [int(v) for v in ids]
    p = _neighbours(stack)
    p2, p3, p4, p5, p6, p7, p8, p9 = p
    i = lambda a: a.astype(np.int64)
    b = sum(i(q) for q in p)
    X = sum(i(~p[k] & p[(k + 1) % 8]) for k in range(8))
    orth = i(p4) + i(p6)
    diag = i(p5 & ~p4 & ~p6) + i(p7 & ~p8 & ~p6)
    out = np.zeros((stack.shape[0], len(rows_of), STAT_COLUMNS), np.int64)
    for bi in range(stack.shape[0]):
        for r, k in enumerate(rows_of):
            sel = stack[bi] == k
            if k < 0 or not sel.any():
                continue
            out[bi, r, 0] = sel.sum()
            out[bi, r, 1] = orth[bi][sel].sum()
            out[bi, r, 2] = diag[bi][sel].sum()
            out[bi, r, 3] = ((X[bi] == 1) & (b[bi] <= 2) & sel).sum()
            out[bi, r, 4] = ((X[bi] >= 3) & sel).sum()
            out[bi, r, 5] = ((b[bi] == 0) & sel).sum()
            if dd is not None:
                v = np.maximum(dd[bi][sel], 0)
                out[bi, r, 6], out[bi, r, 7] = v.sum(), v.max()
    return out if s.ndim == 3 else out[0]


def traits(rows: np.ndarray, area: np.ndarray | None = None) -> dict:
    """The float64 traits of `skeleton.skeleton_from_sums` from the integer rows, by the same formulas in numpy."""
    rows = np.asarray(rows, np.int64)
    px = rows[..., 0].astype(np.float64)
    some = rows[..., 0] > 0
    nan = np.full(px.shape, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        length = rows[..., 1].astype(np.float64) + np.sqrt(2.0) * rows[..., 2].astype(np.float64)
        out = {"skeleton_length": np.where(some, length, nan),
               "mean_width": np.where(some, 2.0 * np.sqrt(rows[..., 6].astype(np.float64) / px) - 1.0, nan),
               "max_width": np.where(some, 2.0 * np.sqrt(rows[..., 7].astype(np.float64)) - 1.0, nan)}
        if area is not None:
            a = np.asarray(area).astype(np.float64)
            out["length_per_area"] = np.where(some & (a > 0), length / a, nan)
    return out


# ---- the maps the tests share -------------------------------------------------------------------------------------------
def ragged(H: int, W: int, seed: int, n: int = 23) -> np.ndarray:
    """n ragged blobs (ids 0 .. n-1, later ones painted over earlier ones, -1 background) with a few holes punched in."""
    rng = np.random.default_rng(seed)
    m = np.full((H, W), -1, np.int32)
    side = min(H, W)
    for k in range(n):
        r = int(rng.integers(2, max(3, side // 5)))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        y0, y1, x0, x1 = max(0, cy - 2 * r), min(H, cy + 2 * r + 1), max(0, cx - 2 * r), min(W, cx + 2 * r + 1)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        edge = 1.0 + 0.3 * np.sin(np.arctan2(yy - cy, xx - cx) * int(rng.integers(3, 9)) + rng.random() * 6.28)
        m[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 < (r * edge) ** 2] = k
        if k % 3 == 0 and r >= 4:  # a hole at the blob's centre
            m[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= (r // 4) ** 2] = -1
    for _ in range(max(1, n // 4)):
        r = int(rng.integers(1, max(2, side // 24)))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        yy, xx = np.mgrid[0:H, 0:W]
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = -1
    return m


def pieces(mask: np.ndarray, eight: bool) -> int:
    """The number of connected pieces of a bool mask (8- or 4-connected)."""
    from scipy import ndimage
    return int(ndimage.label(mask, structure=np.ones((3, 3), int) if eight else None)[1])


def holes(mask: np.ndarray) -> int:
    """4-connected pieces of the complement on a map padded by one pixel, less the outside."""
    return pieces(~np.pad(mask, 1), eight=False) - 1
