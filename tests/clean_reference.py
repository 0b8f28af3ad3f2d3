"""The contract of wm2f_labelmap_clean (include/wm2f.h) restated with numpy and scipy.ndimage: one
`label` call per id with the 3 x 3 structure for the pieces, one with the default cross for the free components, the
ring of a hole by one 4-neighbour dilation.  Also the generators the CPU and the GPU tests share."""
import itertools

import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), dtype=bool)
CROSS = ndimage.generate_binary_structure(2, 1)
STATS = ("area_in", "pieces_in", "pieces_kept", "area_kept", "holes_filled", "pixels_filled", "area_out", "new_id")


def id_keys(maps, n):
    """The id of every pixel in [0, n), -1 for a free one: wm2f_labelmap_instance_stats's rule for floats (the integer
    the value equals, +-0 is 0; negative, fractional, not finite or >= 2^24 is no id), then the range."""
    a = np.asarray(maps)
    if a.dtype.kind == "f":
        ok = np.isfinite(a) & (a >= 0) & (a < 2.0 ** 24)
        whole = np.zeros(a.shape, bool)
        whole[ok] = np.floor(a[ok]) == a[ok]
        k = np.where(whole, np.where(whole, a, 0).astype(np.int64), -1)
    else:
        k = a.astype(np.int64)
    return np.where((k >= 0) & (k < n), k, -1)


def choose_pieces(key, n, keep="all", min_area=0):
    """Steps 1-3 on one (H, W) key map -> (kept map, stats (n, 8) with columns 0-3 filled, dropped pieces)."""
    H, W = key.shape
    stats = np.zeros((n, 8), np.int64)
    kept = np.full((H, W), -1, np.int64)
    dropped = 0
    for k in range(n):
        lab, cnt = ndimage.label(key == k, structure=EIGHT)
        if cnt == 0:
            continue
        flat = lab.ravel()
        areas = np.bincount(flat, minlength=cnt + 1)[1:]
        first = np.full(cnt + 1, H * W, np.int64)
        np.minimum.at(first, flat, np.arange(H * W))
        first = first[1:]
        stay = np.ones(cnt, bool)
        if keep == "largest":
            best = min(range(cnt), key=lambda i: (-int(areas[i]), int(first[i])))
            stay[:] = False
            stay[best] = True
        stay &= areas >= min_area
        dropped += int(cnt - stay.sum())
        kept[np.concatenate([[False], stay])[lab]] = k
        stats[k, :4] = areas.sum(), cnt, stay.sum(), areas[stay].sum()
    return kept, stats, dropped


def free_components(kept):
    """Step 4's judgement of one kept map -> (labels of the free pixels, [(area, id)] per component): id >= 0 for a hole
    of that id, -1 for a component on the image border, -2 for one bounded by two or more ids."""
    H, W = kept.shape
    lab, cnt = ndimage.label(kept < 0, structure=CROSS)
    records = []
    for i, sl in enumerate(ndimage.find_objects(lab)):
        y0, y1, x0, x1 = sl[0].start, sl[0].stop, sl[1].start, sl[1].stop
        area = int((lab[sl] == i + 1).sum())
        if y0 == 0 or x0 == 0 or y1 == H or x1 == W:
            records.append((area, -1))
            continue
        # the component's box grown by one pixel lies inside the image: its ring by one 4-neighbour dilation
        big = (slice(y0 - 1, y1 + 1), slice(x0 - 1, x1 + 1))
        comp = lab[big] == i + 1
        ring = ndimage.binary_dilation(comp, structure=CROSS) & ~comp
        around = np.unique(kept[big][ring])  # ids only: two free components are never 4-adjacent
        records.append((area, int(around[0]) if len(around) == 1 else -2))
    return lab, records


def finish(kept, stats, free, fill_holes, max_hole_area, relabel, census=None):
    """Steps 4-5 from the kept map, its partial stats and `free_components(kept)`."""
    n = stats.shape[0]
    stats = stats.copy()
    out = kept
    kinds = {"filled": 0, "over_limit": 0, "border": 0, "two_id": 0}
    if fill_holes:
        lab, records = free
        paint = np.full(len(records) + 1, -1, np.int64)
        for i, (area, k) in enumerate(records):
            if k < 0:
                kinds["border" if k == -1 else "two_id"] += 1
            elif max_hole_area is not None and area > max_hole_area:
                kinds["over_limit"] += 1
            else:
                kinds["filled"] += 1
                paint[i + 1] = k
                stats[k, 4] += 1
                stats[k, 5] += area
        out = np.where(lab > 0, paint[lab], kept)
    stats[:, 6] = stats[:, 3] + stats[:, 5]
    alive = stats[:, 6] > 0
    stats[:, 7] = np.where(alive, np.cumsum(alive) - 1 if relabel else np.arange(n), -1)
    if relabel and n:
        out = np.where(out >= 0, stats[np.maximum(out, 0), 7], -1)
    if census is not None:
        for name, v in kinds.items():
            census[name] = census.get(name, 0) + v
    return out, stats, int(alive.sum())


class Cleaner:
    """The reference on one (B, H, W) stack with ids 0 .. n-1, remembering the stages that options share: the chosen
    pieces per (keep, min_area) and the free components of that kept map."""

    def __init__(self, maps, n):
        self.keys = [id_keys(m, n) for m in maps]
        self.n = n
        self._pieces, self._free = {}, {}

    def run(self, keep="all", min_area=0, fill_holes=False, max_hole_area=None, relabel=False, census=None):
        """-> (out (B, H, W) int64 with -1 free, stats (B, n, 8) int64, n_out (B) int32)"""
        stage = (keep, min_area)
        if stage not in self._pieces:
            self._pieces[stage] = [choose_pieces(k, self.n, keep, min_area) for k in self.keys]
        if fill_holes and stage not in self._free:
            self._free[stage] = [free_components(kept) for kept, _, _ in self._pieces[stage]]
        res = []
        for b, (kept, stats, dropped) in enumerate(self._pieces[stage]):
            if census is not None:
                census["dropped"] = census.get("dropped", 0) + dropped
            res.append(finish(kept, stats, self._free[stage][b] if fill_holes else None, fill_holes, max_hole_area, relabel,
                              census))
        return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]).reshape(len(res), self.n, 8),
                np.asarray([r[2] for r in res], np.int32))


def clean(maps, n, **options):
    """A (B, H, W) stack -> (out (B, H, W) int64, stats (B, n, 8) int64, n_out (B) int32)."""
    return Cleaner(maps, n).run(**options)


def clean_one(m, n, **options):
    """One (H, W) map -> (out (H, W), stats (n, 8), n_out)."""
    out, stats, n_out = clean(np.asarray(m)[None], n, **options)
    return out[0], stats[0], int(n_out[0])


# ------------------------------------------------------------------------------------------------ generators
def block_map(H, W, s=0):
    """3 x 3 cells of ids 0-5, a quarter of the cells free, then H * W / 40 single-pixel salt values in -1 .. 5, seeded by
    H * 1000 + W + s.  int64 with -1 free."""
    rng = np.random.default_rng(H * 1000 + W + s)
    cells = rng.integers(0, 6, ((H + 2) // 3, (W + 2) // 3))
    cells[rng.random(cells.shape) < 0.25] = -1
    m = np.kron(cells, np.ones((3, 3), np.int64))[:H, :W]
    n_salt = (H * W) // 40
    ys, xs = rng.integers(0, H, n_salt), rng.integers(0, W, n_salt)
    m[ys, xs] = rng.integers(-1, 6, n_salt)
    return m


def typed_maps(dtype, H, W, B=3):
    """B block maps of one numpy dtype with the values that are no id planted: float32 NaN, 2.5, -0.0 and 2^24; int32
    70000 and -7; uint8 255 (free pixels are 255 there, since 0 is an id)."""
    out = []
    for b in range(B):
        m = block_map(H, W, b)
        if dtype == np.uint8:
            m = np.where(m < 0, 255, m)
            out.append(m.astype(np.uint8))
        elif dtype == np.int32:
            if H * W > 8:
                m[H // 2, W // 2] = 70000
                m[H // 3, W // 3] = -7
            out.append(m.astype(np.int32))
        else:
            f = m.astype(np.float32)
            if H * W > 8:
                f[H // 2, W // 2] = 2.5
                f[H // 3, W // 3] = np.nan
                f[H // 4, W // 4] = 2.0 ** 24
                zeros = np.argwhere(m == 0)
                if len(zeros):
                    f[tuple(zeros[len(zeros) // 2])] = -0.0
                else:
                    f[0, 0] = -0.0
            out.append(f)
    return np.stack(out)


def serpentine(H, W, open_to_border=False):
    """A one-pixel-wide wall of id 0 that snakes over the whole map and closes on itself, around ONE corridor of free
    pixels that snakes with it.  Rows 1 and H-2 and columns 1 and W-2 are the outer ring (row and column 0 stay free,
    so the ring touches no border); inside it horizontal walls every 4 rows leave a gap alternately at the right and at
    the left end."""
    m = np.full((H, W), -1, np.int64)
    m[1, 1:W - 1] = 0
    m[H - 2, 1:W - 1] = 0
    m[1:H - 1, 1] = 0
    m[1:H - 1, W - 2] = 0
    right = True
    for y in range(5, H - 4, 4):
        if right:
            m[y, 2:W - 5] = 0
        else:
            m[y, 5:W - 2] = 0
        right = not right
    if open_to_border:
        m[1, W // 2] = -1
    return m


def spiral(H, W, open_to_border=False):
    """A one-pixel-wide rectangular spiral wall of id 0 inside a closed outer ring: the free corridor between its turns
    is one component winding to the centre."""
    m = np.full((H, W), -1, np.int64)
    m[1, 1:W - 1] = 0
    m[H - 2, 1:W - 1] = 0
    m[1:H - 1, 1] = 0
    m[1:H - 1, W - 2] = 0
    t, b, l, r = 1, H - 2, 1, W - 2  # the wall already drawn
    # the spiral arm starts on the left wall and turns inwards, 3 pixels between turns
    y = t + 3
    while b - t > 8 and r - l > 8:
        m[y, l:r - 2] = 0            # rightwards, stops 3 short of the right wall
        m[y:b - 2, r - 3] = 0        # down
        m[b - 3, l + 3:r - 2] = 0    # leftwards
        m[y + 3:b - 2, l + 3] = 0    # up, stops 3 below the arm it started from
        t, b, l, r = y, b - 3, l + 3, r - 3
        y = t + 3
    if open_to_border:
        m[1, W // 2] = -1
    return m


def border_rule_map(c, o):
    """A 96 x 96 map (3 x 3 tiles of 32) of the values 0-2 on which the merge rule across tile borders meets all 16
    combinations of the four facts it reads, on the top border y = 32 and on the left border x = 64: the border pixel p
    has value c, and of `chain` (the pixel before p along the border), `back`, `across` and `ahead` (the three pixels
    across the border, in the border's direction) those of combination k have value c too, the others o."""
    m = np.random.default_rng(0).integers(0, 3, (96, 96))
    for k, (chain, back, across, ahead) in enumerate(itertools.product([0, 1], repeat=4)):
        x = 4 * k + 2
        m[31:33, x - 2:x + 3] = o
        m[32, x] = c
        for bit, at in ((chain, (32, x - 1)), (back, (31, x - 1)), (across, (31, x)), (ahead, (31, x + 1))):
            if bit:
                m[at] = c
        y = 4 * k + 2
        m[y - 2:y + 3, 63:65] = o
        m[y, 64] = c
        for bit, at in ((chain, (y - 1, 64)), (back, (y - 1, 63)), (across, (y, 63)), (ahead, (y + 1, 63))):
            if bit:
                m[at] = c
    return m


def border_rule_cases(m, c, tile=32):
    """The distinct (chain, back, across, ahead) that pixels of value c show on tile top rows and on tile left columns
    of m, as the merge kernels read them: chain only inside the pixel's own tile, back and ahead only inside the map."""
    H, W = m.shape
    top, left = set(), set()
    for y, x in np.argwhere(m == c):
        if y % tile == 0 and y > 0:
            top.add((x % tile != 0 and m[y, x - 1] == c, x > 0 and m[y - 1, x - 1] == c, m[y - 1, x] == c,
                     x + 1 < W and m[y - 1, x + 1] == c))
        if x % tile == 0 and x > 0:
            left.add((y % tile != 0 and m[y - 1, x] == c, y > 0 and m[y - 1, x - 1] == c, m[y, x - 1] == c,
                      y + 1 < H and m[y + 1, x - 1] == c))
    return top, left
