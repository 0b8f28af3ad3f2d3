"""cv2.fillPoly's rules as a literal CPU port, the oracle of tests/test_polygons_gpu.py, pinned on
cases a reader can check by hand; host-side parsing of the VIA-JSON and CWFID-YAML loaders; refusals; symbols.

The oracle ports OpenCV 4.x drawing.cpp as restated in DESIGN section 17: clipLine in float64, LineIterator's error
recurrence (8-connected, left to right), CollectPolyEdges (16.16 fixed point, clipped edges without the half-pixel) and
FillEdgeCollection with its insertion-ordered active-edge list and bubble sort.  No GPU needed."""
import json
import os

import numpy as np
import pytest
import torch

from weed_instance_segmentation_amd import annotations as A
from weed_instance_segmentation_amd._lib import Wm2fError

XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT
INT_MAX = 2 ** 31 - 1


def i64(v: int) -> int:
    """C int64 wrap-around."""
    return (v + 2 ** 63) % 2 ** 64 - 2 ** 63


def i32(v: int) -> int:
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def cdiv(a: int, b: int) -> int:
    """C integer division (truncates toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


# ------------------------------------------------------------------------------------------- the oracle
def clip_line(W: int, H: int, x1: int, y1: int, x2: int, y2: int):
    """OpenCV's clipLine(Size2l, Point2l&, Point2l&).  Returns (inside, x1, y1, x2, y2)."""
    right, bottom = W - 1, H - 1

    def code(x, y):
        return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8

    c1, c2 = code(x1, y1), code(x2, y2)
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def _outside(x, y, W, H):
    return not (0 <= x < W and 0 <= y < H)


def line_pixels(W: int, H: int, x0: int, y0: int, x1: int, y1: int):
    """LineIterator(img, (x0, y0), (x1, y1), 8, leftToRight=true): the pixels it visits, in order."""
    if _outside(x0, y0, W, H) or _outside(x1, y1, W, H):
        ok, x0, y0, x1, y1 = clip_line(W, H, x0, y0, x1, y1)
        if not ok:
            return []
    if x1 < x0:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, y1 - y0
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    vert = dy > dx
    major, minor = (dy, dx) if vert else (dx, dy)
    err = major - 2 * minor
    x, y = x0, y0
    out = []
    for _ in range(major + 1):
        out.append((x, y))
        step = err < 0
        if vert:
            y += sy
            x += 1 if step else 0
        else:
            x += 1
            y += sy if step else 0
        err += -2 * minor + (2 * major if step else 0)
    return out


class PolyEdge:
    __slots__ = ("y0", "y1", "x", "dx", "next")

    def __init__(self, y0=0, y1=0, x=0, dx=0):
        self.y0, self.y1, self.x, self.dx, self.next = y0, y1, x, dx, None


def collect_edge(W: int, H: int, x0: int, y0: int, x1: int, y1: int):
    """CollectPolyEdges for the edge (x0, y0) -> (x1, y1) (LINE_8, shift 0): its PolyEdge, or None if horizontal."""
    p0x, p0y, p1x, p1y = x0 * XY_ONE, y0, x1 * XY_ONE, y1
    if _outside(x0, y0, W, H) or _outside(x1, y1, W, H):
        _, tx0, ty0, tx1, ty1 = clip_line(W, H, x0, y0, x1, y1)
        if ty0 != ty1:
            p0x, p0y, p1x, p1y = tx0 * XY_ONE, ty0, tx1 * XY_ONE, ty1
    else:
        p0x += XY_ONE >> 1
        p1x += XY_ONE >> 1
    if y0 == y1:
        return None
    dx = cdiv(p1x - p0x, p1y - p0y)
    if y0 < y1:
        return PolyEdge(y0, y1, i64(p0x + i64((y0 - p0y) * dx)), dx)
    return PolyEdge(y1, y0, i64(p1x + i64((y1 - p1y) * dx)), dx)


def fill_edge_collection(img: np.ndarray, edges: list, color: int):
    """FillEdgeCollection (LINE_8): the active-edge list kept in insertion order, pairs drawn as the list is walked,
    then one bubble sort of the list per row."""
    H, W = img.shape
    total = len(edges)
    if total < 2:
        return
    y_min, y_max, x_min, x_max = INT_MAX, -INT_MAX - 1, 2 ** 63 - 1, -1
    for e in edges:
        xe = i64(e.x + i64((e.y1 - e.y0) * e.dx))
        y_min, y_max = min(y_min, e.y0), max(y_max, e.y1)
        x_min, x_max = min(x_min, e.x, xe), max(x_max, e.x, xe)
    if y_max < 0 or y_min >= H or x_max < 0 or x_min >= (W << XY_SHIFT):
        return
    edges = sorted(edges, key=lambda e: (e.y0, e.x, e.dx))
    edges.append(PolyEdge(INT_MAX))  # the end marker (a copy of tmp in OpenCV)
    head = PolyEdge(INT_MAX)         # tmp: the head of the active list
    i = 0
    e = edges[0]
    y_max = min(y_max, H)
    y = e.y0
    while y < y_max:
        draw = 0
        clipline = y < 0
        prelast, last = head, head.next
        while last is not None or e.y0 == y:
            if last is not None and last.y1 == y:
                prelast.next = last.next  # the edge ends on this row
                last = last.next
                continue
            keep_prelast = prelast
            if last is not None and (e.y0 > y or last.x < e.x):
                prelast, last = last, last.next
            elif i < total:
                prelast.next = e  # the edge starts on this row
                e.next = last
                prelast = e
                i += 1
                e = edges[i]
            else:
                break
            if draw:
                if not clipline:
                    if keep_prelast.x > prelast.x:
                        xa, xb = i32(prelast.x >> XY_SHIFT), i32(keep_prelast.x >> XY_SHIFT)
                    else:
                        xa, xb = i32(keep_prelast.x >> XY_SHIFT), i32(prelast.x >> XY_SHIFT)
                    if xa < W and xb >= 0:
                        img[y, max(xa, 0):min(xb, W - 1) + 1] = color
                keep_prelast.x = i64(keep_prelast.x + keep_prelast.dx)
                prelast.x = i64(prelast.x + prelast.dx)
            draw ^= 1
        keep_prelast = None
        while True:  # bubble sort of the active list
            prelast, last = head, head.next
            last_exchange = None
            while last is not keep_prelast and last.next is not None:
                te = last.next
                if last.x > te.x:
                    prelast.next = te
                    last.next = te.next
                    te.next = last
                    prelast = te
                    last_exchange = prelast
                else:
                    prelast, last = last, te
            if last_exchange is None:
                break
            keep_prelast = last_exchange
            if keep_prelast is head.next or keep_prelast is head:
                break
        y += 1


def fill_poly(img: np.ndarray, contours, color: int) -> np.ndarray:
    """cv2.fillPoly(img, contours, color) on an (H, W) int32 numpy map, in place (LINE_8, shift 0, no offset)."""
    H, W = img.shape
    edges = []
    for pts in contours:
        pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2)]
        x0, y0 = pts[-1]
        for x1, y1 in pts:
            for x, y in line_pixels(W, H, x0, y0, x1, y1):
                if not _outside(x, y, W, H):
                    img[y, x] = color
            e = collect_edge(W, H, x0, y0, x1, y1)
            if e is not None:
                edges.append(e)
            x0, y0 = x1, y1
    fill_edge_collection(img, edges, color)
    return img


def paint(size, polygons, ids, background=255) -> np.ndarray:
    """The loaders' instance map: fillPoly(map, [polygons[i]], ids[i]) in order on a map of `background`."""
    img = np.full(size, background, dtype=np.int32)
    for p, i in zip(polygons, ids):
        fill_poly(img, [p], i)
    return img


def fill_by_parity(img: np.ndarray, contours, color: int) -> np.ndarray:
    """The GPU kernel's row rule on the same edge records: with a_i = crossing >> 16, pixel x is filled iff
    #{a_i < x} is odd or x is some a_i (no sort).  Outline as in fill_poly."""
    H, W = img.shape
    cover = np.zeros((H, W), dtype=bool)
    edges = []
    for pts in contours:
        pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2)]
        x0, y0 = pts[-1]
        for x1, y1 in pts:
            for x, y in line_pixels(W, H, x0, y0, x1, y1):
                if not _outside(x, y, W, H):
                    cover[y, x] = True
            e = collect_edge(W, H, x0, y0, x1, y1)
            if e is not None:
                edges.append(e)
            x0, y0 = x1, y1
    cols = np.arange(W)
    for y in range(H):
        a = np.array([i64(e.x + i64((y - e.y0) * e.dx)) >> XY_SHIFT for e in edges if e.y0 <= y < e.y1], dtype=np.int64)
        if a.size:
            lt = (a[None, :] < cols[:, None]).sum(axis=1)
            cover[y] |= (lt % 2 == 1) | np.isin(cols, a)
    img[cover] = color
    return img


# ------------------------------------------------------------------------------------------- hand cases
def _fp(size, contours, color=1, background=0):
    return fill_poly(np.full(size, background, dtype=np.int32), contours, color)


def test_rectangle_fills_its_closed_box():
    got = _fp((8, 9), [[(2, 1), (6, 1), (6, 5), (2, 5)]])
    exp = np.zeros((8, 9), np.int32)
    exp[1:6, 2:7] = 1
    np.testing.assert_array_equal(got, exp)


def test_triangle_rows():
    got = _fp((6, 6), [[(0, 0), (4, 0), (0, 4)]])
    exp = np.zeros((6, 6), np.int32)
    for y in range(5):
        exp[y, :5 - y] = 1
    np.testing.assert_array_equal(got, exp)


def test_single_point_paints_one_pixel():
    got = _fp((5, 5), [[(3, 2)]], color=7)
    exp = np.zeros((5, 5), np.int32)
    exp[2, 3] = 7
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("p0,p1", [((0, 0), (6, 2)), ((1, 5), (4, 0)), ((0, 3), (6, 3)), ((2, 0), (2, 5)),
                                   ((0, 0), (5, 5)), ((6, 1), (0, 4))])
def test_two_point_polygon_paints_its_line(p0, p1):
    got = _fp((6, 7), [[p0, p1]])
    exp = np.zeros((6, 7), np.int32)
    for x, y in line_pixels(7, 6, *p0, *p1):
        exp[y, x] = 1
    np.testing.assert_array_equal(got, exp)


def test_flat_polygon_paints_only_its_outline():
    got = _fp((4, 10), [[(1, 2), (8, 2), (5, 2), (3, 2)]])
    exp = np.zeros((4, 10), np.int32)
    exp[2, 1:9] = 1
    np.testing.assert_array_equal(got, exp)


def test_line_octants_and_error_recurrence():
    # shallow: err = 4 - 2 = 2, then 0, -2 (the minor step follows the third pixel), 4, 2
    assert line_pixels(10, 10, 0, 0, 4, 1) == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1)]
    # steep, drawn from the left end: y moves every step, x where err < 0
    assert line_pixels(10, 10, 1, 4, 0, 0) == [(0, 0), (0, 1), (0, 2), (1, 3), (1, 4)]
    # right to left is drawn left to right
    assert line_pixels(10, 10, 4, 1, 0, 0) == line_pixels(10, 10, 0, 0, 4, 1)
    # |dx| == |dy|: x is the major axis, every step diagonal
    assert line_pixels(10, 10, 0, 3, 3, 0) == [(0, 3), (1, 2), (2, 1), (3, 0)]


def test_clip_line_snaps_y_then_x_in_float64():
    assert clip_line(10, 10, -5, 5, 15, 5) == (True, 0, 5, 9, 5)
    assert clip_line(10, 10, 2, -4, 2, 20) == (True, 2, 0, 2, 9)
    # y-snap of endpoint 1 to y = 0: x1 += trunc((0 - -3) * (9 - 0) / (6 - -3)) = 3
    assert clip_line(10, 10, 0, -3, 9, 6) == (True, 3, 0, 9, 6)
    # wholly outside on one side: untouched, not inside
    assert clip_line(10, 10, -5, 1, -1, 8) == (False, -5, 1, -1, 8)
    # misses the corner: snapped to y = 0 then both left of the image
    ok, *_ = clip_line(10, 10, -10, 5, 5, -20)
    assert not ok


def test_concave_arrow():
    arrow = [(1, 4), (5, 0), (9, 4), (7, 4), (7, 8), (3, 8), (3, 4)]
    got = _fp((10, 11), [arrow])
    exp = np.zeros((10, 11), np.int32)
    for y in range(5):
        exp[y, 5 - y:6 + y] = 1  # the head: row y spans 5 - y .. 5 + y
    exp[4:9, 3:8] = 1  # the shaft
    np.testing.assert_array_equal(got, exp)


def test_bow_tie_fills_both_lobes():
    got = _fp((9, 9), [[(0, 0), (8, 8), (8, 0), (0, 8)]])
    # even-odd over the crossing edges: each row spans from the left diagonal to the right one, with the waist at 4
    for y in range(9):
        lo, hi = min(y, 8 - y), max(y, 8 - y)
        assert set(np.flatnonzero(got[y])) == set(range(0, lo + 1)) | set(range(hi, 9)), y
    np.testing.assert_array_equal(got, got[:, ::-1])
    np.testing.assert_array_equal(got, got[::-1, :])


@pytest.mark.parametrize("poly", [
    [(-3, 2), (5, 2), (5, 6), (-3, 6)],     # left border
    [(4, 2), (12, 2), (12, 6), (4, 6)],     # right border
    [(2, -4), (6, -4), (6, 3), (2, 3)],     # top border
    [(2, 5), (6, 5), (6, 14), (2, 14)],     # bottom border
])
def test_rectangle_crossing_a_border_is_clipped_box(poly):
    got = _fp((10, 9), [poly])
    xs, ys = [p[0] for p in poly], [p[1] for p in poly]
    exp = np.zeros((10, 9), np.int32)
    exp[max(min(ys), 0):min(max(ys), 9) + 1, max(min(xs), 0):min(max(xs), 8) + 1] = 1
    np.testing.assert_array_equal(got, exp)


def test_triangle_crossing_borders_matches_the_parity_rule():
    tri = [(-6, -3), (14, 4), (3, 17)]
    got = _fp((12, 10), [tri])
    assert got.any() and not got.all()
    np.testing.assert_array_equal(got, fill_by_parity(np.zeros((12, 10), np.int32), [tri], 1))


def test_polygon_wholly_outside_paints_nothing():
    for poly in ([(-9, 1), (-2, 1), (-2, 6)], [(20, 1), (30, 4), (25, 9)], [(1, -9), (6, -2), (3, -1)],
                 [(1, 40), (6, 30), (3, 31)]):
        assert not _fp((10, 10), [poly]).any()


def test_vertex_at_x_equal_w():
    # An annotation touching the right edge and scaled by int(x * s) lands on x = W.  The edges through it are clipped
    # (no half-pixel), and the column W - 1 is painted.
    W = 8
    got = _fp((6, W), [[(2, 0), (W, 0), (W, 5), (2, 5)]])
    exp = np.zeros((6, W), np.int32)
    exp[:, 2:] = 1
    np.testing.assert_array_equal(got, exp)
    tri = [(1, 1), (W, 3), (2, 5)]
    got = _fp((6, W), [tri])
    np.testing.assert_array_equal(got, fill_by_parity(np.zeros((6, W), np.int32), [tri], 1))
    assert got[3, W - 1] == 1


def test_clipped_edge_has_no_half_pixel():
    # (3, 0) -> (8, 5) on an 8-wide map: clipLine snaps (8, 5) to (7, 4); the record takes the clipped points at 16.16
    # without the half-pixel.  The edge (8, 0) -> (8, 5) lies wholly right of the map: clipLine leaves it, and so does
    # the record (again no half-pixel).  An in-image edge gets the half-pixel.
    e = collect_edge(8, 6, 3, 0, 8, 5)
    assert (e.y0, e.y1, e.x, e.dx) == (0, 5, 3 * XY_ONE, XY_ONE)
    e = collect_edge(8, 6, 8, 0, 8, 5)
    assert (e.y0, e.y1, e.x, e.dx) == (0, 5, 8 * XY_ONE, 0)
    e = collect_edge(8, 6, 3, 0, 3, 5)
    assert (e.y0, e.y1, e.x, e.dx) == (0, 5, 3 * XY_ONE + XY_ONE // 2, 0)
    assert collect_edge(8, 6, 1, 2, 5, 2) is None


def test_holes_follow_even_odd():
    outer = [(0, 0), (9, 0), (9, 9), (0, 9)]
    inner = [(3, 3), (6, 3), (6, 6), (3, 6)]
    got = _fp((10, 10), [outer, inner])
    exp = np.ones((10, 10), np.int32)
    exp[4:6, 4:6] = 0  # the hole's interior; its outline is painted
    np.testing.assert_array_equal(got, exp)


def test_painters_order():
    img = paint((6, 6), [[(0, 0), (4, 0), (4, 4), (0, 4)], [(2, 2), (5, 2), (5, 5), (2, 5)]], [1, 2])
    assert img[0, 0] == 1 and img[3, 3] == 2 and img[5, 5] == 2 and img[0, 5] == 255 and img[4, 1] == 1


def test_literal_list_equals_sorted_pairing_on_random_polygons():
    """The GPU kernel pairs sorted crossings through a parity rule; here it meets the literal active-edge list."""
    rng = np.random.default_rng(3)
    for t in range(60):
        H, W = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        n = int(rng.integers(1, 12))
        k = int(rng.integers(1, 3))
        contours = [np.stack([rng.integers(-8, W + 8, n), rng.integers(-8, H + 8, n)], 1) for _ in range(k)]
        a = _fp((H, W), contours)
        b = fill_by_parity(np.zeros((H, W), np.int32), contours, 1)
        np.testing.assert_array_equal(a, b, err_msg=f"case {t}")


# ------------------------------------------------------------------------------------------- host-side parsing
def _via_entry(filename, regions):
    return {"filename": filename, "size": 1, "regions": regions}


def _region(xs, ys, cls, shape="polygon"):
    return {"shape_attributes": {"name": shape, "all_points_x": xs, "all_points_y": ys},
            "region_attributes": {"classname": cls}}


def test_via_parsing_rules():
    label2id = {"crop": 0, "weed": 1}
    regions = [_region([0, 4, 4], [0, 0, 4], "weed"),
               _region([1, 2], [1, 2], "crop", shape="rect"),      # not a polygon: no id
               _region([0, 4, 4], [0, 0, 4], "tree"),              # unknown class: no id
               _region([10, 21, 33], [5, 7, 9], "crop")]
    polys, ids, d = A._via_polygons(_via_entry("a.png", regions), label2id, 0.5, 0.5, skip_255=True)
    assert ids == [1, 2] and d == {1: 1, 2: 0}
    np.testing.assert_array_equal(polys[1], [[5, 2], [10, 3], [16, 4]])  # int(v * 0.5)
    polys, ids, d = A._via_polygons(_via_entry("a.png", regions), label2id, 0.5, 0.25, skip_255=False)
    np.testing.assert_array_equal(polys[1], [[5, 1], [10, 1], [16, 2]])


def test_via_255_skip():
    regions = [_region([0, 1, 1], [0, 0, 1], "weed")] * 256
    _, ids, d = A._via_polygons(_via_entry("a.png", regions), {"weed": 1}, 1.0, 1.0, skip_255=True)
    assert ids[253:] == [254, 256, 257] and 255 not in d
    _, ids, _ = A._via_polygons(_via_entry("a.png", regions), {"weed": 1}, 1.0, 1.0, skip_255=False)
    assert ids == list(range(1, 257))


def test_cwfid_parsing_rules():
    label2id = {"crop": 0, "weed": 1}
    ann = {"filename": "x.png", "annotation": [
        {"type": "weed", "points": {"x": [0.0, 10.6, 10.2], "y": [0.0, 0.0, 8.9]}},
        {"type": "crop", "points": {"x": 3.5, "y": 4.5}},               # one float pair: dropped by the < 3 rule
        {"type": "crop", "points": {"x": 3, "y": 4}},                   # int scalars: skipped
        {"type": "crop", "points": {"x": [1.0, 2.0, 3.0], "y": [1.0, 2.0]}},  # length mismatch: skipped
        {"type": "tree", "points": {"x": [1.0, 2.0, 3.0], "y": [1.0, 2.0, 3.0]}},
        {"type": "crop", "points": {"x": [2, 4, 6, 8], "y": [1, 3, 5, 7]}},
    ]}
    polys, ids, d = A._cwfid_polygons(ann, label2id, 0.5)
    assert ids == [1, 2] and d == {1: 1, 2: 0}
    np.testing.assert_array_equal(polys[0], [[0, 0], [5, 0], [5, 4]])
    np.testing.assert_array_equal(polys[1], [[1, 0], [2, 1], [3, 2], [4, 3]])
    assert A._cwfid_polygons({"filename": "x.png", "annotation": None}, label2id, 1.0) == ([], [], {})
    ann = {"annotation": [{"type": "weed", "points": {"x": [0, 1, 1], "y": [0, 0, 1]}}] * 256}
    _, ids, d = A._cwfid_polygons(ann, {"weed": 1}, 1.0)
    assert ids[253:] == [254, 256, 257] and 255 not in d


def _png(path, w, h):
    from PIL import Image
    Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(path)


def test_sorghum_entry_filter(tmp_path):
    (tmp_path / "img").mkdir()
    _png(str(tmp_path / "img" / "a.png"), 4, 4)
    _png(str(tmp_path / "img" / "c.png"), 4, 4)
    data = {"k1": _via_entry("a.png", [_region([0, 1, 1], [0, 0, 1], "weed")]),
            "k2": _via_entry("b.png", [_region([0, 1, 1], [0, 0, 1], "weed")]),   # no image
            "k3": _via_entry("c.png", []),                                          # no regions
            "k4": _via_entry("c.png", [_region([0, 1, 1], [0, 0, 1], "weed")])}
    ann = tmp_path / "via.json"
    ann.write_text(json.dumps(data))
    ds = A.SorghumWeedDataset(str(tmp_path / "img"), str(ann), None, {"weed": 1}, device="cpu")
    assert [e["filename"] for e in ds.valid_entries] == ["a.png", "c.png"] and len(ds) == 2
    ds = A.SorghumWeedDataset(str(tmp_path / "img"), str(ann), None, {"weed": 1}, max_images=1, device="cpu")
    assert len(ds) == 1


def test_cwfid_file_scan(tmp_path):
    import yaml
    (tmp_path / "img").mkdir()
    (tmp_path / "ann").mkdir()
    _png(str(tmp_path / "img" / "001.png"), 4, 4)
    _png(str(tmp_path / "img" / "003.png"), 4, 4)
    for name, body in [("b.yaml", {"filename": "003.png"}), ("a.yaml", {"filename": "001.png"}),
                       ("c.yaml", {"filename": "002.png"}), ("d.yaml", {"annotation": []}), ("e.yaml", None)]:
        (tmp_path / "ann" / name).write_text(yaml.safe_dump(body))
    (tmp_path / "ann" / "f.yaml").write_text("filename: [unclosed\n")
    ds = A.CropWeedYamlDataset(str(tmp_path / "img"), str(tmp_path / "ann"), None, {}, device="cpu")
    assert [(os.path.basename(i), os.path.basename(y)) for i, y in ds.valid_files] == [("001.png", "a.yaml"),
                                                                                       ("003.png", "b.yaml")]


def test_load_ground_truth_returns_none_as_the_reference(tmp_path, capsys):
    assert A.load_ground_truth("a.png", (4, 4), str(tmp_path / "missing.json"), str(tmp_path), {}) is None
    bad = tmp_path / "bad.json"
    bad.write_text("{not json")
    assert A.load_ground_truth("a.png", (4, 4), str(bad), str(tmp_path), {}) is None
    good = tmp_path / "via.json"
    good.write_text(json.dumps({"k": _via_entry("b.png", [])}))
    assert A.load_ground_truth("a.png", (4, 4), str(good), str(tmp_path), {}) is None
    out = capsys.readouterr().out
    assert "Annotation file not found" in out and "Error loading JSON" in out and 'No annotation found for "a.png"' in out


# ------------------------------------------------------------------------------------------- refusals
def test_host_maps_are_refused():
    img = torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(Wm2fError):
        A.fill_poly(img, [np.array([[0, 0], [2, 0], [2, 2]])], 1)
    from weed_instance_segmentation_amd import ops
    with pytest.raises(Wm2fError):
        ops.fill_polygons(img, [[0, 0]], [0, 1], [0, 1], [1])
    with pytest.raises(Wm2fError):
        A.polygons_to_instance_map([np.array([[0, 0]])], [1], (4, 4), device="cpu")


def test_bad_sizes_and_contours_are_refused():
    with pytest.raises(ValueError):
        A.polygons_to_instance_map([], [], (0, 4))
    with pytest.raises(ValueError):
        A.polygons_to_instance_map([], [], (4, -1))
    with pytest.raises(ValueError):
        A._contour(np.zeros((0, 2), np.int32), "p")
    with pytest.raises(ValueError):
        A._contour(np.array([[0, 0], [2 ** 24 + 1, 0]]), "p")
    with pytest.raises(ValueError):
        A._contour(np.array([[0, 0], [0, -2 ** 24 - 1]]), "p")
    A._contour(np.array([[-2 ** 24, 2 ** 24]]), "p")
    with pytest.raises(ValueError):
        A._contour(np.array([[0.5, 1.0]]), "p")


def test_symbols_are_declared_and_bound():
    from weed_instance_segmentation_amd import _build, _lib
    hdr = open(os.path.join(os.path.dirname(_build.HERE), "include", "wm2f.h")).read()
    for name in ("wm2f_poly_workspace", "wm2f_poly_fill"):
        assert name + "(" in hdr and name in _lib.SIGNATURES
    assert "polygon.hip" in _build.SOURCES
    assert "#define WM2F_POLY_MAX_SIDE 16384" in hdr and _lib.WM2F_POLY_MAX_SIDE == 16384
    assert "#define WM2F_POLY_MAX_COORD (1 << 24)" in hdr and _lib.WM2F_POLY_MAX_COORD == 2 ** 24
