"""Plain-loop restatement of the tracing contract of include/wm2f.h: the boundary sides of an id map as
directed edges, the left-first successor, a walk round every loop from its leader, both emission rules, the CSR layout
of ops.labelmap_trace, and an even-odd rasteriser for crack loops."""
import numpy as np

# heading of side s (0 top, 1 right, 2 bottom, 3 left): east, south, west, north as (dx, dy), y down
STEP = [(1, 0), (0, 1), (-1, 0), (0, -1)]
# tail vertex of side s of pixel (x, y), as an offset
TAIL = [(0, 0), (1, 0), (1, 1), (0, 1)]


def id_of(v, N):
    """The id a map value stands for: -1 background, 0 .. N-1, None for anything else."""
    if v != int(v):
        return None
    v = int(v)
    return v if -1 <= v < N else None


def ids_of(m, N):
    m = np.asarray(m)
    return [[id_of(m[y, x], N) for x in range(m.shape[1])] for y in range(m.shape[0])]


def out_of_range(m, N):
    return sum(v is None for row in ids_of(m, N) for v in row)


def edges(m, N):
    """key -> id of every boundary side; key = 4 * (y * W + x) + side."""
    ids = ids_of(m, N)
    H, W = len(ids), len(ids[0])
    at = lambda y, x: ids[y][x] if 0 <= y < H and 0 <= x < W else "outside"
    out = {}
    for y in range(H):
        for x in range(W):
            k = ids[y][x]
            if k is None or k < 0:
                continue
            for s, (ny, nx) in enumerate([(y - 1, x), (y, x + 1), (y + 1, x), (y, x - 1)]):
                if at(ny, nx) != k:
                    out[4 * (y * W + x) + s] = k
    return out


def successor(ids, key):
    """The key of the edge that follows `key`."""
    H, W = len(ids), len(ids[0])
    at = lambda y, x: ids[y][x] if 0 <= y < H and 0 <= x < W else "outside"
    p, d = divmod(key, 4)
    y, x = divmod(p, W)
    k = ids[y][x]
    rx, ry = x + STEP[d][0], y + STEP[d][1]  # ahead-right
    left = (d + 3) % 4
    lx, ly = rx + STEP[left][0], ry + STEP[left][1]  # ahead-left
    if at(ly, lx) == k:
        return 4 * (ly * W + lx) + left
    if at(ry, rx) == k:
        return 4 * (ry * W + rx) + d
    return 4 * p + (d + 1) % 4


def loops_of(m, N):
    """The loops of one map as [(id, [keys from the leader along successors])], ordered by id, then leader key."""
    ids = ids_of(m, N)
    todo = edges(m, N)
    out = []
    for key in sorted(todo):  # ascending: the first edge met of a loop is its leader
        if key not in todo:
            continue
        k = todo[key]
        walk, e = [], key
        while True:
            walk.append(e)
            assert todo.pop(e) == k
            e = successor(ids, e)
            if e == key:
                break
        out.append((k, walk))
    out.sort(key=lambda t: (t[0], t[1][0]))
    return out


def twice_area(walk, W):
    total = 0
    for key in walk:
        p, d = divmod(key, 4)
        y, x = divmod(p, W)
        xa, ya = x + TAIL[d][0], y + TAIL[d][1]
        xb, yb = xa + STEP[d][0], ya + STEP[d][1]
        total += xa * yb - xb * ya
    return total


def crack_points(walk, W, simplify):
    pts = []
    for i, key in enumerate(walk):
        p, d = divmod(key, 4)
        if simplify and walk[i - 1] % 4 == d:  # i - 1 = -1 is the leader's predecessor
            continue
        y, x = divmod(p, W)
        pts.append((x + TAIL[d][0], y + TAIL[d][1]))
    return pts


def pixel_points(walk, W, simplify):
    pts = []
    for i, key in enumerate(walk):
        if walk[i - 1] // 4 != key // 4:
            y, x = divmod(key // 4, W)
            pts.append((x, y))
    if not pts:
        y, x = divmod(walk[0] // 4, W)
        pts = [(x, y)]
    if simplify and len(pts) > 2:
        n = len(pts)
        keep = []
        for i in range(n):
            a, b, c = pts[i - 1], pts[i], pts[(i + 1) % n]
            if (b[0] - a[0], b[1] - a[1]) != (c[0] - b[0], c[1] - b[1]):
                keep.append(b)
        pts = keep
    return pts


def trace(m, N, coords, simplify=True, loops=None):
    """[(id, points as a list of (x, y), twice_area)] of one map in loop order; coords 0 crack, 1 pixel.  `loops`:
    loops_of(m, N), when the caller has walked the map already."""
    W = np.asarray(m).shape[1]
    return [(k, (pixel_points if coords else crack_points)(walk, W, simplify), twice_area(walk, W))
            for k, walk in (loops_of(m, N) if loops is None else loops)]


def csr(maps, N, coords, simplify=True, loops=None):
    """(points (P, 2), loop_offsets (L + 1), loop_image (L), loop_id (L), twice_area (L), slot_offsets (B * N + 1)) of a
    stack of maps, as ops.labelmap_trace lays them out.  `loops`: [loops_of(m, N) for m in maps], when walked already."""
    points, loop_offsets, image, ident, area = [], [0], [], [], []
    slot_counts = np.zeros(len(maps) * N, np.int64)
    for b, m in enumerate(maps):
        assert out_of_range(m, N) == 0
        for k, pts, a2 in trace(m, N, coords, simplify, None if loops is None else loops[b]):
            points += pts
            loop_offsets.append(len(points))
            image.append(b)
            ident.append(k)
            area.append(a2)
            slot_counts[b * N + k] += 1
    return (np.array(points, np.int32).reshape(-1, 2), np.array(loop_offsets, np.int64), np.array(image, np.int64),
            np.array(ident, np.int64), np.array(area, np.int64), np.concatenate([[0], np.cumsum(slot_counts)]))


def fill_even_odd(loops, H, W):
    """The even-odd interior of crack loops (lists of (x, y) lattice points, axis-parallel sides) at pixel centres: every
    vertical side toggles the pixels of its rows from its column on; a running XOR along each row does the rest."""
    toggle = np.zeros((H, W + 1), bool)
    for pts in loops:
        n = len(pts)
        for i in range(n):
            (xa, ya), (xb, yb) = pts[i], pts[(i + 1) % n]
            assert xa == xb or ya == yb
            if xa == xb:
                for y in range(min(ya, yb), max(ya, yb)):
                    toggle[y, xa] ^= True
    out = np.zeros((H, W), bool)
    for y in range(H):
        inside = False
        for x in range(W):
            inside ^= bool(toggle[y, x])
            out[y, x] = inside
    return out
