"""Plain-loop restatements of the run-length contract of include/wm2f.h: toggle lists by walking the
flattened map, COCO counts by walking columns, the COCO string codec transcribed from the published algorithm, decoding."""
import numpy as np


def flatten(m, order):
    """The (H, W) map in scan order: 0 row-major, 1 column-major."""
    m = np.asarray(m)
    return [m[y, x] for y in range(m.shape[0]) for x in range(m.shape[1])] if order == 0 else \
        [m[y, x] for x in range(m.shape[1]) for y in range(m.shape[0])]


def slot_of(v, N):
    """Slot 0 is id -1, slot k + 1 id k in [0, N); None for any other value."""
    if v != int(v):
        return None
    v = int(v)
    return v + 1 if -1 <= v < N else None


def toggle_lists(m, N, order):
    """(lists, out_of_range): lists[s] = the ascending positions where membership of slot s flips along the scan, the
    map's two ends included."""
    v = [slot_of(x, N) for x in flatten(m, order)]
    lists = [[] for _ in range(N + 1)]
    for t in range(len(v) + 1):
        prev = v[t - 1] if t > 0 else None
        cur = v[t] if t < len(v) else None
        if prev != cur:
            if prev is not None:
                lists[prev].append(t)
            if cur is not None:
                lists[cur].append(t)
    return lists, sum(s is None for s in v)


def csr(maps, N, order):
    """counts (B, N + 1), positions and offsets of a stack of maps, as ops.labelmap_toggles lays them out."""
    counts, positions = [], []
    for m in maps:
        lists, bad = toggle_lists(m, N, order)
        assert bad == 0
        counts.append([len(l) for l in lists])
        for l in lists:
            positions += l
    counts = np.array(counts, np.int64).reshape(len(maps), N + 1)
    offsets = np.concatenate([[0], np.cumsum(counts.reshape(-1))])
    return counts, np.array(positions, np.int64), offsets


def coco_counts(mask):
    """COCO's rleEncode: walk the mask column by column, count the pixels until the value changes, starting with 0s."""
    mask = np.asarray(mask)
    counts, value, run = [], 0, 0
    for x in range(mask.shape[1]):
        for y in range(mask.shape[0]):
            p = 1 if mask[y, x] else 0
            if p != value:
                counts.append(run)
                value, run = p, 0
            run += 1
    counts.append(run)
    return counts


def hf_rle(mask):
    """binary_mask_to_rle by a walk: [start + 1, length, ...] of the 1-runs of the row-major mask."""
    out, run_start = [], None
    flat = flatten(mask, 0) + [0]
    for t, p in enumerate(flat):
        if p and run_start is None:
            run_start = t
        if not p and run_start is not None:
            out += [run_start + 1, t - run_start]
            run_start = None
    return out


def to_string(counts):
    """rleToString of the COCO API."""
    s = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(chr(c + 48))
    return "".join(s)


def from_string(s):
    """rleFrString of the COCO API."""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def decode_coco(counts, H, W):
    """Alternating run counts, column-major, starting with 0s -> the (H, W) bool mask."""
    flat, value = [], 0
    for c in counts:
        flat += [value] * int(c)
        value = 1 - value
    flat += [0] * (H * W - len(flat))
    assert len(flat) == H * W
    return np.array(flat, bool).reshape(W, H).T


def paint(out, runs, order):
    """(B, H, W) maps painted with runs (image, start, length, value) in scan order, in order."""
    out = np.array(out)
    B, H, W = out.shape
    for b, s, n, v in runs:
        for t in range(s, s + n):
            y, x = (t // W, t % W) if order == 0 else (t % H, t // H)
            out[b, y, x] = v
    return out
