"""The contracts of wm2f_labelmap_row_votes, wm2f_labelmap_row_bands and crop_rows (include/wm2f.h)
restated in numpy.  Nothing here shares the kernels' structure: the votes are one np.bincount per direction over the
voting pixels' coordinates, the bands one distance table pixel by pixel, the host steps are written with Fractions and
plain loops.  `row_field` generates a synthetic row crop with its truth."""
from fractions import Fraction

import numpy as np

ONE = 1 << 14


def angle_table(T):
    t = np.arange(T, dtype=np.float64)
    return np.rint(np.cos(np.pi * t / T) * 16384.0).astype(np.int64), np.rint(np.sin(np.pi * t / T) * 16384.0).astype(np.int64)


def n_bins(H, W, shift):
    return (((W + H - 2) * ONE) >> shift) + 1


def decode(m, N):
    """A map of any accepted dtype -> int64 ids, -1 where the value is no id of [0, N)."""
    a = np.asarray(m)
    if a.dtype.kind == "f":
        ok = np.isfinite(a) & (a == np.floor(np.where(np.isfinite(a), a, 0))) & (a >= 0) & (a < N)
        return np.where(ok, np.where(ok, a, 0).astype(np.int64), -1)
    a = a.astype(np.int64)
    return np.where((a >= 0) & (a < N), a, -1)


def votes_reference(m, vote, T, shift):
    """One (H, W) map and its (N,) vote flags -> acc (T, R) int64, energy (T,) Python ints."""
    H, W = m.shape
    vote = np.asarray(vote)
    ids = decode(m, len(vote))
    ys, xs = np.nonzero((ids >= 0) & (vote[np.clip(ids, 0, None)] != 0))
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    R = n_bins(H, W, shift)
    cos, sin = angle_table(T)
    acc = np.zeros((T, R), np.int64)
    for t in range(T):
        c, s = int(cos[t]), int(sin[t])
        off = -min(0, c) * (W - 1)
        acc[t] = np.bincount((xs * c + ys * s + off) >> shift, minlength=R)
    return acc, [int((row.astype(object) ** 2).sum()) for row in acc]


_FOOTPRINTS = {}


def footprint_reference(H, W, T, shift):
    """The energies of an all-voting (H, W) map, computed once per shape."""
    key = (H, W, T, shift)
    if key not in _FOOTPRINTS:
        _FOOTPRINTS[key] = votes_reference(np.zeros((H, W), np.uint8), [1], T, shift)[1]
    return _FOOTPRINTS[key]


def direction_reference(E, FE):
    """(t*, contrast): the largest E / FE as exact fractions, the first among equals; contrast in float64."""
    ratios = [Fraction(int(e), int(f)) for e, f in zip(E, FE)]
    t = ratios.index(max(ratios))
    scores = np.array([int(e) / int(f) for e, f in zip(E, FE)], np.float64)
    med = float(np.median(scores))
    if med > 0:
        return t, float(scores[t]) / med
    return t, (float("inf") if scores[t] > 0 else 0.0)


def peaks_reference(profile, smooth, min_spacing, peak_fraction, shift):
    """rho of the rows of one profile, ascending (units of 2^-14 pixel)."""
    p = np.asarray(profile, np.int64)
    R = len(p)
    box = np.array([p[max(0, j - smooth): j + smooth + 1].sum() for j in range(R)], np.int64)
    if R == 0 or box.max() <= 0:
        return []
    left = box.copy()
    taken = []
    while True:
        j = int(np.argmax(left))  # the first of the largest
        if left[j] <= 0 or not (left[j] >= peak_fraction * box.max()):
            break
        left[j] = -1
        if any(abs(j - k) * 2 ** (shift - 14) < min_spacing for k in taken):
            continue
        taken.append(j)
    out = []
    for j in taken:
        idx = np.arange(max(0, j - smooth), min(R, j + smooth + 1))
        out.append(int((int(((2 * idx + 1) * p[idx]).sum()) * 2 ** (shift - 1)) // int(p[idx].sum())))
    return sorted(out)


def bands_reference(m, line, rho, band, ids=None, N=None):
    """One (H, W) map -> counts (N, 3) int64 and zone (H, W) uint8, pixel by pixel."""
    H, W = m.shape
    c, s, off, K = (int(v) for v in line)
    rho = np.asarray(rho, np.int64)[:max(0, K)]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    p = xx * c + yy * s + off
    if len(rho):
        zone = (np.abs(p[:, :, None] - rho[None, None, :]).min(-1) <= band)
    else:
        zone = np.zeros((H, W), bool)
    a = np.asarray(m)
    if ids is None:
        rows = decode(a, N)
    else:
        N = len(ids) if N is None else N
        rows = np.full((H, W), -1, np.int64)
        for r, v in enumerate(ids):
            rows[a == v] = r
    counts = np.zeros((N, 3), np.int64)
    for r in range(N):
        sel = rows == r
        counts[r] = [sel.sum(), (sel & zone).sum(), p[sel].sum()]
    return counts, zone.astype(np.uint8)


def line_reference(c, s, off, rho, H, W):
    """Where c x + s y + off = rho meets the border of [0, W-1] x [0, H-1]: the smallest and the largest (x, y)."""
    r = rho - off
    pts = []
    if s:
        for x in (0, W - 1):
            y = Fraction(r - c * x, s)
            if 0 <= y <= H - 1:
                pts.append((float(x), (r - c * x) / s))
    if c:
        for y in (0, H - 1):
            x = Fraction(r - s * y, c)
            if 0 <= x <= W - 1:
                pts.append(((r - s * y) / c, float(y)))
    if not pts:
        return None
    return [list(min(pts)), list(max(pts))]


def crop_rows_reference(m, flags, infos=None, angles=180, bin=1, smooth=2, min_spacing=16, peak_fraction=0.3, band=None,
                        min_contrast=1.5):
    """`crop_rows` on the host: m (H, W), flags (N,) which ids vote, infos [(id, label)] or None."""
    H, W = m.shape
    N = len(flags)
    shift = 14 + int(np.log2(bin))
    acc, E = votes_reference(m, flags, angles, shift)
    FE = footprint_reference(H, W, angles, shift)
    t, contrast = direction_reference(E, FE)
    cos, sin = angle_table(angles)
    c, s = int(cos[t]), int(sin[t])
    off = -min(0, c) * (W - 1)
    rho = peaks_reference(acc[t], smooth, min_spacing, peak_fraction, shift) if contrast >= min_contrast else []
    spacing = float(np.median(np.diff(rho))) / ONE if len(rho) > 1 else float("nan")
    if band is None:
        band = (spacing if len(rho) > 1 else min_spacing) / 4
    band_fixed = int(np.floor(band * ONE))
    counts, zone = bands_reference(m, [c, s, off, len(rho)], rho, band_fixed, N=N)
    per = []
    for i, label in (infos if infos is not None else [(i, None) for i in range(N)]):
        area, inside, total = (int(v) for v in counts[i])
        k = -1
        if area and rho:
            d = [abs(Fraction(total, area) - r) for r in rho]
            k = d.index(min(d))
        per.append({"id": i, "label_id": label, "area": area, "row": k,
                    "offset": (total - area * rho[k]) / (area * ONE) if k >= 0 else float("nan"),
                    "in_row": bool(k >= 0 and Fraction(inside, area) >= Fraction(1, 2))})
    return {"found": len(rho) > 0, "angle": np.pi * t / angles - np.pi / 2 if t else np.pi / 2, "normal": (c / ONE, s / ONE),
            "t": t, "shift": shift, "line": [c, s, off], "rho": [r / ONE for r in rho], "rho_fixed": rho, "spacing": spacing,
            "band": float(band), "band_fixed": band_fixed, "contrast": contrast,
            "lines": [line_reference(c, s, off, r, H, W) for r in rho], "per_instance": per, "image_size": (H, W),
            "zone": zone}


# ---- synthetic fields -------------------------------------------------------------------------------------------------------
def row_field(rng, shape, normal_deg, spacing, radius=5, step=None, jitter=1.5, gap=0.15, weeds=None, min_chord=0.6):
    """A row crop: discs of `radius` along parallel lines `spacing` apart whose normal points at `normal_deg` (y down),
    a plant every `step` pixels (default 2.6 radius + 4) with Gaussian jitter and a fraction `gap` missing, plus `weeds`
    discs of radius 3 scattered anywhere (default: one per 4096 pixels).  A line whose chord inside the image is shorter
    than `min_chord` of the longest is left unplanted: by the peak rule a row needs `peak_fraction` of the strongest
    row's votes, which a corner row of three plants beside one of thirteen cannot have.  Returns (map int32 with -1 background, labels (n,) 0 crop / 1 weed, truth):
    truth has `theta` (radians in [0, pi)), `rows` [(rho in true pixels: x cos + y sin, plants painted, the mean x and y
    of their centres)], and `plant_row` per crop id."""
    H, W = shape
    th = np.deg2rad(normal_deg % 180)
    n = np.array([np.cos(th), np.sin(th)])
    d = np.array([-np.sin(th), np.cos(th)])
    step = 2.6 * radius + 4 if step is None else step
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], float)
    lo, hi = (corners @ n).min(), (corners @ n).max()
    along = corners @ d
    m = np.full(shape, -1, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    labels, rows, plant_row = [], [], []
    weeds = round(H * W / 4096) if weeds is None else weeds
    r0 = lo + rng.uniform(0.3, 0.7) * spacing
    grid = np.arange(np.floor(along.min()), np.ceil(along.max()) + 1)

    def chord(r):
        pts = r * n[None, :] + grid[:, None] * d[None, :]
        return int(((pts[:, 0] >= radius) & (pts[:, 0] <= W - 1 - radius) & (pts[:, 1] >= radius) & (pts[:, 1] <= H - 1 - radius)).sum())

    longest = max(chord(r) for r in np.arange(r0, hi, spacing))
    k = 0
    while r0 < hi:
        count, centres = 0, []
        if chord(r0) < min_chord * longest:
            rows.append((float(r0), 0, float("nan"), float("nan")))
            r0 += spacing
            k += 1
            continue
        a = along.min() + rng.uniform(0, step)
        while a < along.max():
            centre = r0 * n + a * d + rng.normal(0, jitter, 2)
            a += step
            if not (radius <= centre[0] <= W - 1 - radius and radius <= centre[1] <= H - 1 - radius):
                continue
            if rng.random() < gap:
                continue
            m[(xx - centre[0]) ** 2 + (yy - centre[1]) ** 2 <= radius ** 2] = len(labels)
            labels.append(0)
            plant_row.append(k)
            centres.append(centre)
            count += 1
        mean = np.mean(centres, 0) if centres else np.array([np.nan, np.nan])
        rows.append((float(r0), count, float(mean[0]), float(mean[1])))
        r0 += spacing
        k += 1
    for _ in range(weeds):
        cx, cy = rng.uniform(3, W - 4), rng.uniform(3, H - 4)
        sel = ((xx - cx) ** 2 + (yy - cy) ** 2 <= 9) & (m < 0)
        if sel.any():
            m[sel] = len(labels)
            labels.append(1)
    return m, np.array(labels, np.int64), {"theta": float(th), "rows": rows, "plant_row": plant_row}


def clutter_field(rng, shape, plants=60, radius=5):
    """Discs scattered uniformly: no rows."""
    H, W = shape
    m = np.full(shape, -1, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    k = 0
    for _ in range(plants):
        cx, cy = rng.uniform(radius, W - 1 - radius), rng.uniform(radius, H - 1 - radius)
        sel = ((xx - cx) ** 2 + (yy - cy) ** 2 <= radius ** 2) & (m < 0)
        if sel.any():
            m[sel] = k
            k += 1
    return m, np.zeros(k, np.int64)


def row_errors(result, truth, min_plants=3):
    """Per true row with at least `min_plants` plants: the distance in pixels from the mean of its plant centres to the
    nearest row line of `result` (inf without rows)."""
    c, s, off = result["line"]
    out = []
    for _, count, cx, cy in truth["rows"]:
        if count >= min_plants:
            p = (cx * c + cy * s + off) / ONE
            out.append(min((abs(p - r) for r in result["rho"]), default=float("inf")))
    return out


def angle_steps(t, theta, T):
    """The circular distance in steps between direction t of T and the true theta."""
    d = abs(t - theta * T / np.pi) % T
    return min(d, T - d)
