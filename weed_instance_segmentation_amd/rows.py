"""Crop rows on the GPU: the direction and the positions of the rows of a row crop from the id map of
a segmentation result, every plant's row and sideways offset, and the mask of the row bands.

    from weed_instance_segmentation_amd import RowOptions, crop_rows, annotate_rows, treatment_grid
    rows = crop_rows(result, RowOptions(vote_labels=[0]))            # label 0: the crop
    result = annotate_rows(result, rows)                             # row / row_offset / in_row per segment
    hoe = treatment_grid(result, options, rows=rows, zone="inter_row")

The pixels of the voting instances vote for every candidate direction of the row normal (`ops.labelmap_row_votes`, a
Hough accumulator in LDS histograms); the rest is exact host arithmetic on T energies and ONE accumulator row, and one
more read of the map (`ops.labelmap_row_bands`).  Positions along the normal are integers in units of 2^-14 pixel.
"""
from __future__ import annotations

import bisect
import dataclasses
import math

import numpy as np
import torch

from . import _lib, ops
from .instances import _id_maps
from .ops.rows import ROW_FIXED_BITS, ROW_MAX_ANGLES, ROW_MAX_ROWS, row_angle_table, row_offset

ONE = 1 << ROW_FIXED_BITS
ZONES = ("inter_row", "intra_row")


def _integer(v, name: str, low: int, high: int | None = None) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low or (high is not None and v > high):
        raise ValueError(f"RowOptions: {name} must be an integer in [{low}, {'...' if high is None else high}], got {v!r}")
    return int(v)


def _number(v, name: str, low: float, high: float, open_low: bool = False) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"RowOptions: {name} must be a finite number, got {v!r}")
    if not (low < v if open_low else low <= v) or v > high:
        raise ValueError(f"RowOptions: {name} must be in {'(' if open_low else '['}{low}, {high}], got {v!r}")
    return float(v)


@dataclasses.dataclass(frozen=True)
class RowOptions:
    """What `crop_rows` does.

    - `vote_labels` (required): the `label_id`s whose instances vote -- the crop.
    - `angles` in [1, 1024]: the candidate directions of the row normal, th_t = pi t / angles.
    - `bin`: the accumulator's bin width in pixels, a power of two in [1, 64].
    - `smooth` in [0, 64]: a peak of the chosen profile is a maximum of the box sums over +-smooth bins.
    - `min_spacing` in (0, 16384] pixels: a candidate peak nearer than this to one already taken is skipped.
    - `peak_fraction` in (0, 1]: a peak needs at least this fraction of the largest box sum.
    - `band` in [0, 16384] pixels: the half-width of a row band; None: a quarter of the row spacing (of `min_spacing`
      when fewer than two rows were found).
    - `min_contrast` >= 0: below this ratio of the best direction's score to the median score no rows are reported."""
    vote_labels: tuple
    angles: int = 180
    bin: int = 1
    smooth: int = 2
    min_spacing: float = 16
    peak_fraction: float = 0.3
    band: float | None = None
    min_contrast: float = 1.5

    def __post_init__(self):
        try:
            labels = tuple(self.vote_labels)
        except TypeError:
            raise ValueError(f"RowOptions: vote_labels must be an iterable of label ids, got {self.vote_labels!r}") from None
        for x in labels:
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
                raise ValueError(f"RowOptions: vote_labels must hold integer label ids, got {x!r}")
        object.__setattr__(self, "vote_labels", tuple(int(x) for x in labels))
        object.__setattr__(self, "angles", _integer(self.angles, "angles", 1, ROW_MAX_ANGLES))
        b = _integer(self.bin, "bin", 1, 64)
        if b & (b - 1):
            raise ValueError(f"RowOptions: bin must be a power of two, got {b}")
        object.__setattr__(self, "bin", b)
        object.__setattr__(self, "smooth", _integer(self.smooth, "smooth", 0, 64))
        object.__setattr__(self, "min_spacing", _number(self.min_spacing, "min_spacing", 0, 16384, open_low=True))
        object.__setattr__(self, "peak_fraction", _number(self.peak_fraction, "peak_fraction", 0, 1, open_low=True))
        if self.band is not None:
            object.__setattr__(self, "band", _number(self.band, "band", 0, 16384))
        object.__setattr__(self, "min_contrast", _number(self.min_contrast, "min_contrast", 0, float("inf")))

    @property
    def shift(self) -> int:
        return ROW_FIXED_BITS + self.bin.bit_length() - 1


# ---- the exact host steps -------------------------------------------------------------------------------------------------
def pick_direction(energy, footprint):
    """(t*, contrast): t* maximises E_t / FE_t, compared as E_a FE_b > E_b FE_a in Python integers, the lowest t among
    equals; contrast = score(t*) / median_t score in float64 with score_t = E_t / FE_t (0 when nothing voted, inf when
    the median is 0 and the best is not)."""
    E, FE = [int(v) for v in energy], [int(v) for v in footprint]
    if len(E) != len(FE) or not E or min(FE) <= 0:
        raise ValueError("pick_direction: one positive footprint energy per direction")
    best = 0
    for t in range(1, len(E)):
        if E[t] * FE[best] > E[best] * FE[t]:
            best = t
    scores = np.array([e / f for e, f in zip(E, FE)], np.float64)
    med = float(np.median(scores))
    top = float(scores[best])
    contrast = top / med if med > 0 else (float("inf") if top > 0 else 0.0)
    return best, contrast


def pick_peaks(profile, smooth: int, min_spacing: float, peak_fraction: float, shift: int):
    """The rows of one accumulator profile, as (bins, rho): the box sums over +-smooth bins (clipped at the ends) are
    taken greedily by descending sum, the lowest bin first among equals, while the sum is >= peak_fraction * the largest
    sum and > 0; a candidate whose bin is nearer than `min_spacing` pixels to a bin already taken (|j - j'| 2^(shift-14)
    < min_spacing) is skipped.  A peak's position is rho = ((sum_j (2j+1) p_j) << (shift-1)) // sum_j p_j over its
    window: the votes' mean bin centre, in units of 2^-14 pixel.  Both lists are ascending in rho."""
    p = [int(v) for v in np.asarray(profile).reshape(-1)]
    R = len(p)
    pre = [0]
    for v in p:
        pre.append(pre[-1] + v)
    sums = [pre[min(R, j + smooth + 1)] - pre[max(0, j - smooth)] for j in range(R)]
    top = max(sums, default=0)
    if top <= 0:
        return [], []
    width = 1 << (shift - ROW_FIXED_BITS)
    taken = []
    for j in sorted(range(R), key=lambda j: (-sums[j], j)):
        if sums[j] <= 0 or not sums[j] >= peak_fraction * top:
            break
        if all(abs(j - k) * width >= min_spacing for k in taken):
            taken.append(j)
    rows = []
    for j in taken:
        lo, hi = max(0, j - smooth), min(R, j + smooth + 1)
        rows.append(((sum((2 * i + 1) * p[i] for i in range(lo, hi)) << (shift - 1)) // sums[j], j))
    rows.sort()
    return [j for _, j in rows], [r for r, _ in rows]


def row_line(c: int, s: int, off: int, rho: int, H: int, W: int):
    """The two end points [[x0, y0], [x1, y1]] of the row c x + s y + off = rho (units of 2^-14) on the border of the
    pixel rectangle [0, W-1] x [0, H-1], the smaller (x, y) first; None when the line misses it.  A point on a vertical
    border has its x exact and y = (r - c x) / s with r = rho - off, one on a horizontal border its y exact and
    x = (r - s y) / c, each one division of exact integers."""
    r = int(rho) - int(off)
    pts = set()
    for xe in (0, W - 1):
        if s != 0:
            num = r - c * xe  # = s y
            if 0 <= num <= s * (H - 1):
                pts.add((float(xe), num / s))
    for ye in (0, H - 1):
        if c != 0:
            num = r - s * ye  # = c x
            lo, hi = sorted((0, c * (W - 1)))
            if lo <= num <= hi:
                pts.add((num / c, float(ye)))
    if not pts:
        return None
    pts = sorted(pts)
    return [list(pts[0]), list(pts[-1])]


def _nearest_row(total: int, area: int, rho):
    """The index of the row nearest the mean position total / area, by integer comparison, the lowest among equals."""
    best, dist = -1, None
    at = bisect.bisect_left(rho, total // area)  # the nearest of an ascending list is next to where the mean would go
    for k in range(max(0, at - 1), min(len(rho), at + 2)):
        d = abs(total - area * rho[k])
        if dist is None or d < dist:
            best, dist = k, d
    return best


# ---- the public functions ---------------------------------------------------------------------------------------------------
_footprints: dict = {}


def _footprint(H: int, W: int, T: int, shift: int, dev, cs: torch.Tensor):
    key = (H, W, T, shift, str(dev))
    if key not in _footprints:
        zero = torch.zeros(1, H, W, device=dev, dtype=torch.uint8)
        _, fe = ops.labelmap_row_votes(zero, torch.ones(1, 1, device=dev, dtype=torch.uint8), cs, shift)
        _footprints[key] = [int(v) for v in fe[0].cpu().numpy()]
    return _footprints[key]


def _result_map(result, vote, options, who: str):
    """(seg (H, W) tensor, infos [(id, label)] or None, host vote flags (n,))."""
    if isinstance(result, dict):
        if "segmentation" not in result or "segments_info" not in result:
            raise ValueError(f"{who}: result must be a dict with 'segmentation' and 'segments_info'")
        if vote is not None:
            raise ValueError(f"{who}: `vote` goes with a bare map; a result votes through options.vote_labels")
        seg = _id_maps(result["segmentation"], who)
        infos = [(int(s["id"]), int(s["label_id"])) for s in result["segments_info"]]
        if any(i < 0 for i, _ in infos) or len(set(i for i, _ in infos)) != len(infos):
            raise ValueError(f"{who}: segment ids must be distinct and not negative")
        n = max((i for i, _ in infos), default=-1) + 1
        flags = np.zeros(max(n, 1), np.uint8)
        for i, label in infos:
            flags[i] = label in options.vote_labels
    else:
        if vote is None:
            raise ValueError(f"{who}: a bare map needs `vote`, one flag per id")
        seg = _id_maps(result, who)
        flags = np.asarray(vote.cpu().numpy() if isinstance(vote, torch.Tensor) else vote)
        if flags.ndim != 1 or flags.size < 1 or flags.dtype.kind not in "biu":
            raise ValueError(f"{who}: vote must be a non-empty 1-d array of flags, got shape {flags.shape} {flags.dtype}")
        flags = (flags != 0).astype(np.uint8)
        infos = None
    if seg.dim() != 2:
        raise ValueError(f"{who}: the segmentation must be (H, W), got {tuple(seg.shape)}")
    if flags.size > 4096:
        raise ValueError(f"{who}: at most 4096 ids, got {flags.size}")
    return seg, infos, flags


def crop_rows(result, options: RowOptions, vote=None, return_zone: bool = False) -> dict:
    """The crop rows of one segmentation result -- what the post-processor, `merge_tile_results` or `segment_tiled`
    return; the map may be on the host or the device -- or of a bare (H, W) id map with `vote`, one flag per id of
    [0, len(vote)) (ids are classes for a semantic map).

    Returns a dict: `found`; `angle`, the direction of the rows themselves in radians in (-pi/2, pi/2] with y down
    (th - pi/2 for th > 0 and pi/2 for th = 0, th = pi t* / angles the direction of the normal); `normal` (cos, sin) from
    the integer table; `t`, `shift`, `line` [c, s, off]; `rho` (pixels, floats) and `rho_fixed` (the exact integers,
    units of 2^-14 pixel, ascending); `spacing` (the median difference of neighbouring rows in pixels, NaN with fewer than
    two), `band` (pixels) and `band_fixed`, `contrast`; `lines`, per row [[x0, y0], [x1, y1]] on the image border (None
    for a row that misses the image); `per_instance`, per id `id`, `label_id` (None for a bare map), `area`, `row` (the
    row nearest its mean position, -1 without rows or pixels), `offset` (signed pixels from that row along the normal,
    NaN without) and `in_row` (at least half its pixels in a band); with return_zone=True `zone`, the device (H, W) uint8
    map of the bands.  Without rows (`found` False: contrast below `min_contrast`, or no peak) the lists are empty and
    every instance has row -1."""
    if not isinstance(options, RowOptions):
        raise TypeError(f"crop_rows: options must be a RowOptions, got {type(options).__name__}")
    seg, infos, flags = _result_map(result, vote, options, "crop_rows")
    if not torch.cuda.is_available():
        raise _lib.Wm2fError("crop_rows runs on a GPU only (no CPU fallback): no device is visible")
    dev = seg.device if seg.is_cuda else torch.device("cuda", torch.cuda.current_device())
    maps = seg.to(dev).unsqueeze(0).contiguous()
    H, W = int(seg.shape[0]), int(seg.shape[1])
    N, T, shift = int(flags.size), options.angles, options.shift
    table = row_angle_table(T)
    cs = torch.from_numpy(table).to(dev)

    acc, energy = ops.labelmap_row_votes(maps, torch.from_numpy(flags).to(dev).unsqueeze(0), cs, shift)
    t, contrast = pick_direction(energy[0].cpu().numpy(), _footprint(H, W, T, shift, dev, cs))
    c, s = int(table[t, 0]), int(table[t, 1])
    off = row_offset(c, W)
    rho = []
    if contrast >= options.min_contrast:
        _, rho = pick_peaks(acc[0, t].cpu().numpy(), options.smooth, options.min_spacing, options.peak_fraction, shift)
        rho = rho[:ROW_MAX_ROWS]
    found = bool(rho)
    spacing = float(np.median(np.diff(np.array(rho, np.int64)))) / ONE if len(rho) >= 2 else float("nan")
    band = options.band if options.band is not None else (spacing if len(rho) >= 2 else options.min_spacing) / 4
    band_fixed = int(math.floor(band * ONE))

    line = torch.tensor([[c, s, off, len(rho)]], dtype=torch.int32, device=dev)
    rho_dev = torch.tensor([rho if rho else [0]], dtype=torch.int32, device=dev)
    got = ops.labelmap_row_bands(maps, line, rho_dev, band_fixed, N=N, zone=return_zone)
    counts, zone = got if return_zone else (got, None)
    counts = counts[0].cpu().numpy()
    rows = []
    for i, label in (infos if infos is not None else [(i, None) for i in range(N)]):
        area, inside, total = (int(v) for v in counts[i])
        k = _nearest_row(total, area, rho) if area else -1
        rows.append({"id": i, "label_id": label, "area": area, "row": k,
                     "offset": (total - area * rho[k]) / (area * ONE) if k >= 0 else float("nan"),
                     "in_row": bool(k >= 0 and 2 * inside >= area)})
    theta = math.pi * t / T
    out = {"found": found, "angle": theta - math.pi / 2 if t > 0 else math.pi / 2, "normal": (c / ONE, s / ONE), "t": t,
           "shift": shift, "line": [c, s, off], "rho": [r / ONE for r in rho], "rho_fixed": list(rho), "spacing": spacing,
           "band": float(band), "band_fixed": band_fixed, "contrast": float(contrast),
           "lines": [row_line(c, s, off, r, H, W) for r in rho], "per_instance": rows, "image_size": (H, W)}
    if return_zone:
        out["zone"] = zone[0]
    return out


def annotate_rows(result: dict, rows: dict) -> dict:
    """A new result dict whose `segments_info` entries carry `row`, `row_offset` and `in_row` from `crop_rows(result,
    ...)`: -1, NaN and False for a segment `rows` does not list.  The input is not modified."""
    if not isinstance(result, dict) or "segments_info" not in result:
        raise ValueError("annotate_rows: result must be a dict with 'segments_info'")
    if not isinstance(rows, dict) or "per_instance" not in rows:
        raise ValueError("annotate_rows: rows must be what crop_rows returned")
    by_id = {int(r["id"]): r for r in rows["per_instance"]}
    infos = []
    for seg in result["segments_info"]:
        r = by_id.get(int(seg["id"]))
        infos.append({**seg, "row": int(r["row"]) if r else -1, "row_offset": float(r["offset"]) if r else float("nan"),
                      "in_row": bool(r["in_row"]) if r else False})
    out = dict(result)
    out["segments_info"] = infos
    return out


def row_zone(maps: torch.Tensor, rows: dict) -> torch.Tensor:
    """The (H, W) uint8 device mask of the row bands of `rows` over the (1, H, W) device map they were found on."""
    if not isinstance(rows, dict) or not rows.get("found"):
        raise ValueError("the zone needs rows that were found (crop_rows(...)['found'] is True)")
    if tuple(rows["image_size"]) != tuple(maps.shape[1:]):
        raise ValueError(f"the rows belong to a {tuple(rows['image_size'])} image, the map is {tuple(maps.shape[1:])}")
    rho = list(rows["rho_fixed"])
    line = torch.tensor([[*rows["line"], len(rho)]], dtype=torch.int32, device=maps.device)
    rho_dev = torch.tensor([rho], dtype=torch.int32, device=maps.device)
    return ops.labelmap_row_bands(maps, line, rho_dev, int(rows["band_fixed"]), N=1, zone=True)[1][0]
