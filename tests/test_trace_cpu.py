"""Tracing id maps into polygons on the host: the plain-loop restatement pinned by hand cases and by
round trips through two independent rasterisers, the host layer fed with the restatement's CSR, the VIA export parsed
back by the loaders' own parser, and the C ABI."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import trace_reference as R
from test_polygons_cpu import fill_poly
from weed_instance_segmentation_amd import contours as M

CRACK, PIXEL = 0, 1


def _loops(m, N, coords, simplify=True):
    return [(k, pts, a) for k, pts, a in R.trace(np.asarray(m), N, coords, simplify)]


# ------------------------------------------------------------------------------------------------------------ hand cases
def test_single_pixel():
    m = [[0]]
    assert _loops(m, 1, CRACK) == [(0, [(0, 0), (1, 0), (1, 1), (0, 1)], 2)]
    assert _loops(m, 1, CRACK, simplify=False) == [(0, [(0, 0), (1, 0), (1, 1), (0, 1)], 2)]
    assert _loops(m, 1, PIXEL) == [(0, [(0, 0)], 2)] == _loops(m, 1, PIXEL, simplify=False)
    # the same pixel away from the origin, with background round it
    m = np.full((3, 4), -1)
    m[1, 2] = 0
    assert _loops(m, 1, CRACK) == [(0, [(2, 1), (3, 1), (3, 2), (2, 2)], 2)]
    assert _loops(m, 1, PIXEL) == [(0, [(2, 1)], 2)]


def test_block_of_2_by_3_gives_its_corners():
    m = np.full((4, 5), -1)
    m[1:3, 1:4] = 0  # rows 1..2, columns 1..3
    assert _loops(m, 1, CRACK) == [(0, [(1, 1), (4, 1), (4, 3), (1, 3)], 12)]
    assert _loops(m, 1, PIXEL) == [(0, [(3, 1), (3, 2), (1, 2), (1, 1)], 12)]  # from the first change of pixel on
    unsimplified = _loops(m, 1, CRACK, simplify=False)[0][1]
    assert len(unsimplified) == 10 and unsimplified[:4] == [(1, 1), (2, 1), (3, 1), (4, 1)]
    assert _loops(m, 1, PIXEL, simplify=False)[0][1] == [(2, 1), (3, 1), (3, 2), (2, 2), (1, 2), (1, 1)]


def test_ring_has_an_outer_loop_and_a_hole():
    m = np.zeros((3, 3), int)
    m[1, 1] = -1
    crack = _loops(m, 1, CRACK)
    assert [(k, a) for k, _, a in crack] == [(0, 18), (0, -2)]
    assert crack[0][1] == [(0, 0), (3, 0), (3, 3), (0, 3)]
    # the hole's leader is the bottom side of pixel (x 1, y 0), heading west from (2, 1): anticlockwise on screen, the
    # segment stays on the right
    assert crack[1][1] == [(2, 1), (1, 1), (1, 2), (2, 2)]
    pixel = _loops(m, 1, PIXEL)
    assert pixel[0][1] == [(2, 0), (2, 2), (0, 2), (0, 0)] and pixel[0][2] == 18
    # the hole loop runs over the ring's pixels next to the hole, from the leader's own pixel on
    assert pixel[1][1] == [(1, 0), (0, 1), (1, 2), (2, 1)] and pixel[1][2] == -2
    assert sum(a for _, _, a in crack) == 2 * 8


def test_diagonal_pixels_are_one_loop():
    m = np.array([[0, -1], [-1, 0]])
    crack = _loops(m, 1, CRACK)
    assert len(crack) == 1 and crack[0][2] == 4
    assert crack[0][1] == [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)]
    assert _loops(m, 1, PIXEL)[0][1] == [(1, 1), (0, 0)]
    # the anti-diagonal too (the saddle is entered from the other side), and two ids do not join
    assert len(_loops(np.array([[-1, 0], [0, -1]]), 1, CRACK)) == 1
    assert [k for k, _, _ in _loops(np.array([[0, 1], [1, 0]]), 2, CRACK)] == [0, 1]


@pytest.mark.parametrize("n", [2, 3, 7])
def test_bar_gives_two_points_in_pixel_mode(n):
    assert _loops(np.zeros((1, n), int), 1, PIXEL) == [(0, [(n - 1, 0), (0, 0)], 2 * n)]
    assert _loops(np.zeros((n, 1), int), 1, PIXEL) == [(0, [(0, n - 1), (0, 0)], 2 * n)]
    assert _loops(np.zeros((1, n), int), 1, CRACK) == [(0, [(0, 0), (n, 0), (n, 1), (0, 1)], 2 * n)]


def test_full_map_gives_its_corners():
    m = np.full((4, 6), 2)
    assert _loops(m, 3, CRACK) == [(2, [(0, 0), (6, 0), (6, 4), (0, 4)], 48)]
    assert _loops(m, 3, PIXEL) == [(2, [(5, 0), (5, 3), (0, 3), (0, 0)], 48)]


def test_loop_order_is_id_then_leader_key_and_bad_values_are_counted():
    m = np.array([[1, -1, 0, -1, 1], [-1, -1, -1, -1, -1], [0, -1, -1, -1, 0]])
    assert [(k, pts[0]) for k, pts, _ in _loops(m, 2, PIXEL)] == [(0, (2, 0)), (0, (0, 2)), (0, (4, 2)), (1, (0, 0)), (1, (4, 0))]
    assert R.out_of_range(m, 1) == 2 and R.out_of_range(np.array([[0.5, -2.0, 0.0]]), 1) == 2


# ------------------------------------------------------------------------------------------------------------ round trips
def _random_maps():
    rng = np.random.default_rng(27)
    maps = []
    for t in range(96):
        H, W = (int(v) for v in rng.integers(1, 20, 2))
        kind = t % 4
        if kind == 0:  # noise
            m = np.where(rng.random((H, W)) < (0.2, 0.5, 0.8)[(t // 4) % 3], 0, -1)
        elif kind == 1:  # XOR-ed rectangles
            inside = np.zeros((H, W), bool)
            for _ in range(3):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                inside[y0:int(rng.integers(y0, H)) + 1, x0:int(rng.integers(x0, W)) + 1] ^= True
            m = np.where(inside, 0, -1)
        elif kind == 2:  # a noisy disc
            yy, xx = np.mgrid[0:H, 0:W]
            disc = (yy - H / 2) ** 2 + (xx - W / 2) ** 2 <= (min(H, W) / 2.2) ** 2
            m = np.where(disc ^ (rng.random((H, W)) < 0.1), 0, -1)
        else:  # a full map with one hole
            m = np.zeros((H, W), int)
            m[int(rng.integers(0, H)), int(rng.integers(0, W))] = -1
        maps.append(m)
        if t % 8 == 7:  # and several ids at once
            maps.append(rng.integers(-1, 3, (H, W)))
    return maps


def test_round_trips_on_random_maps():
    loops_seen = 0
    for m in _random_maps():
        H, W = m.shape
        N = 3
        for k in range(N):
            mask = m == k
            for simplify in (True, False):
                crack = [(pts, a) for i, pts, a in R.trace(m, N, CRACK, simplify) if i == k]
                assert np.array_equal(R.fill_even_odd([p for p, _ in crack], H, W), mask)
                assert sum(a for _, a in crack) == 2 * int(mask.sum())
                pixel = [(pts, a) for i, pts, a in R.trace(m, N, PIXEL, simplify) if i == k]
                assert [a for _, a in pixel] == [a for _, a in crack]  # the crack value in both systems
                img = np.zeros((H, W), np.int32)
                if pixel:
                    fill_poly(img, [np.array(p) for p, _ in pixel], 1)
                assert np.array_equal(img.astype(bool), mask), (m, k, simplify)
                for pts, _ in pixel:
                    n = len(pts)
                    steps = {(pts[i][0] - pts[i - 1][0], pts[i][1] - pts[i - 1][1]) for i in range(n)} if n > 1 else set()
                    if not simplify:  # all steps are among the 8 directions
                        assert all(max(abs(dx), abs(dy)) == 1 for dx, dy in steps)
                loops_seen += len(crack)
    assert loops_seen > 500


# ------------------------------------------------------------------------------------- the host layer on the reference CSR
def test_loops_from_csr_cuts_the_reference_layout():
    maps = [np.array([[0, 0, -1], [0, -1, 2]]), np.full((2, 3), -1), np.array([[2, 2, 2], [2, -1, 2]])]
    N = 3
    csr = R.csr(maps, N, PIXEL)
    points, loop_offsets, image, ident, area, slot_offsets = csr
    assert loop_offsets[0] == 0 and loop_offsets[-1] == len(points) and len(slot_offsets) == 3 * N + 1
    assert slot_offsets.tolist() == [0, 1, 1, 2, 2, 2, 2, 2, 2, 3]
    out = M.loops_from_csr(points, loop_offsets, image, ident, area, len(maps))
    assert [sorted(d) for d in out] == [[0, 2], [], [2]]
    for b, m in enumerate(maps):
        want = {}
        for k, pts, a in R.trace(m, N, PIXEL):
            want.setdefault(k, []).append((pts, a < 0))
        assert {k: [([tuple(p) for p in l["points"].tolist()], l["hole"]) for l in v] for k, v in out[b].items()} == want
        for v in out[b].values():
            assert all(l["points"].dtype == np.int32 and l["points"].shape[1] == 2 for l in v)


def _result_from_map(m, labels, scores=None):
    """A post-processor result for an id map, with the restatement's polygons attached."""
    N = len(labels)
    loops = M.loops_from_csr(*R.csr([m], N, PIXEL)[:5], 1)[0]
    infos = []
    for k, label in enumerate(labels):
        info = {"id": k, "label_id": label, "was_fused": False, "score": 1.0 if scores is None else scores[k]}
        if k in loops:
            info["polygons"] = loops[k]
        infos.append(info)
    return {"segmentation": torch.from_numpy(np.asarray(m, np.float32)), "segments_info": infos}


def test_via_export_is_read_back_by_the_loaders_parser(tmp_path):
    from weed_instance_segmentation_amd.annotations import _via_polygons
    m = np.full((6, 7), -1)
    m[0:3, 0:3] = 0
    m[1, 1] = -1       # a hole in instance 0: not exported
    m[4, 1:6] = 1      # a bar: two points
    m[0, 6] = 2        # a single pixel: one point
    # id 3 owns no pixel
    result = _result_from_map(m, labels=[1, 0, 1, 0], scores=[0.9, 0.8, 0.3, 0.7])
    id2label = {0: "sorghum", 1: "weed"}
    project = M.via_annotations([result], ["field.png"], id2label)
    assert json.loads(json.dumps(project)) == project  # plain ints and strings only
    (key, entry), = project.items()
    assert key == "field.png-1" and entry["filename"] == "field.png" and entry["size"] == -1
    regions = entry["regions"]
    assert [r["shape_attributes"]["name"] for r in regions] == ["polygon"] * 3
    assert [r["region_attributes"]["classname"] for r in regions] == ["weed", "sorghum", "weed"]
    assert regions[0]["shape_attributes"]["all_points_x"] == [2, 2, 0, 0]
    assert regions[0]["shape_attributes"]["all_points_y"] == [0, 2, 2, 0]
    assert (regions[1]["shape_attributes"]["all_points_x"], regions[1]["shape_attributes"]["all_points_y"]) == ([5, 1], [4, 4])
    assert (regions[2]["shape_attributes"]["all_points_x"], regions[2]["shape_attributes"]["all_points_y"]) == ([6], [0])
    assert all(type(v) is int for r in regions for v in r["shape_attributes"]["all_points_x"])
    polygons, ids, id_to_semantic = _via_polygons(entry, {"sorghum": 0, "weed": 1}, 1.0, 1.0, skip_255=False)
    assert ids == [1, 2, 3] and id_to_semantic == {1: 1, 2: 0, 3: 1}
    img = np.full((6, 7), -1, np.int32)
    for p, i in zip(polygons, ids):
        fill_poly(img, [p], i - 1)
    want = m.copy()
    want[1, 1] = 0  # VIA has no holes: the loader fills it
    assert np.array_equal(img, want)
    # the score threshold, string keys as a JSON config carries them, and the file
    assert len(M.via_annotations([result], ["f"], {"0": "a", "1": "b"}, score_threshold=0.5)["f-1"]["regions"]) == 2
    path = tmp_path / "via.json"
    assert M.save_via_annotations(str(path), [result], ["field.png"], id2label) == project
    assert json.loads(path.read_text()) == project
    with pytest.raises(ValueError):
        M.via_annotations([result], ["a", "b"], id2label)
    with pytest.raises(KeyError):
        M.via_annotations([result], ["a"], {0: "sorghum"})


# ---------------------------------------------------------------------------------------- argument errors, the C ABI
def test_host_tensors_and_bad_arguments_are_refused():
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    with pytest.raises(Wm2fError):
        ops.labelmap_trace(torch.zeros(1, 4, 4), N=3)
    with pytest.raises(Wm2fError):
        ops.labelmap_trace(torch.zeros(1, 4, 4, dtype=torch.uint8), N=3, coords=0, simplify=False)
    with pytest.raises(TypeError):
        ops.labelmap_trace(np.zeros((1, 4, 4), np.float32), N=3)
    with pytest.raises(ValueError):
        M.trace_label_maps(torch.zeros(4, 4), coords="subpixel")
    with pytest.raises(ValueError):
        M.instance_polygons({"segmentation": [[1, 2]], "segments_info": []})
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            M.trace_label_maps(torch.zeros(4, 4), n=2)


def test_header_declares_and_lib_binds_the_entry_points():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    want = {
        "wm2f_trace_workspace": ["int B", "int H", "int W", "int N"],
        "wm2f_trace_edge_workspace": ["int64_t E"],
        "wm2f_trace_rounds": ["int64_t E"],
        "wm2f_trace_count": ["const void* map", "int dtype", "int32_t* counts", "void* workspace", "int B", "int H", "int W",
                             "int N", "void* stream"],
        "wm2f_trace_link": ["const void* map", "int dtype", "const void* workspace", "void* edge_workspace", "int E", "int B",
                            "int H", "int W", "int N", "void* stream"],
        "wm2f_trace_rank": ["void* edge_workspace", "int E", "void* stream"],
        "wm2f_trace_flags": ["const void* edge_workspace", "int32_t* flag", "int32_t* lead", "int E", "int H", "int W",
                             "int coords", "int simplify", "void* stream"],
        "wm2f_trace_loops": ["const void* map", "int dtype", "const void* edge_workspace", "const int32_t* lead_prefix",
                             "int64_t* loop_key", "int32_t* loop_len", "int E", "int n_loops", "int B", "int H", "int W",
                             "int N", "void* stream"],
        "wm2f_trace_scatter": ["const void* edge_workspace", "const int32_t* flag", "const int32_t* lead_prefix",
                               "const int32_t* loop_place", "const int32_t* loop_base", "int32_t* flag_sorted",
                               "int32_t* edge_sorted", "int32_t* term_sorted", "int E", "int n_loops", "int H", "int W",
                               "void* stream"],
        "wm2f_trace_emit": ["const void* edge_workspace", "const int32_t* flag_sorted", "const int32_t* edge_sorted",
                            "const int32_t* flag_prefix", "int32_t* points", "int E", "int P", "int H", "int W", "int coords",
                            "void* stream"],
    }
    for name, args in want.items():
        proto = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*)\);", header, re.M)
        assert proto is not None, name
        assert [a.strip() for a in " ".join(proto.group(1).split()).split(",")] == args
        assert len(_lib.SIGNATURES[name][1]) == len(args)
    assert "trace.hip" in _build.SOURCES


def test_library_sizes_its_workspaces_and_rounds():
    from weed_instance_segmentation_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    lib = _lib.load()
    assert lib.wm2f_trace_workspace(1, 1, 1, 1) == 8  # a word for the pixel, a word for its block
    assert lib.wm2f_trace_workspace(2, 16, 16, 4) == (512 + 2) * 4
    assert lib.wm2f_trace_workspace(1, 0, 4, 1) == -1 and lib.wm2f_trace_workspace(0, 4, 4, 1) == -1
    assert lib.wm2f_trace_workspace(1, 4, 4, _lib.WM2F_RLE_MAX_IDS + 1) == -1
    assert lib.wm2f_trace_workspace(2, 16384, 16384, 1) == -1  # 4 * B * H * W = 2^31
    assert lib.wm2f_trace_workspace(1, 16384, 16384, 1) > 0
    assert lib.wm2f_trace_edge_workspace(10) == 360 and lib.wm2f_trace_edge_workspace(0) == -1
    assert [lib.wm2f_trace_rounds(e) for e in (1, 2, 4, 5, 8, 9, 1 << 20, (1 << 20) + 1)] == [1, 1, 2, 3, 3, 4, 20, 21]


def test_package_exports():
    import inspect
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    for name in ("trace_label_maps", "instance_polygons", "via_annotations", "save_via_annotations"):
        assert getattr(pkg, name) is getattr(M, name)
    assert callable(ops.labelmap_trace)
    sig = inspect.signature(ops.labelmap_trace)
    assert list(sig.parameters) == ["maps", "N", "coords", "simplify"] and sig.parameters["simplify"].default is True
    sig = inspect.signature(Mask2FormerInstancePostProcessor.post_process_instance_segmentation)
    assert sig.parameters["return_polygons"].default is False
