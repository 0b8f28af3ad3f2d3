"""The repair of id maps on the host: hand cases that pin tests/clean_reference.py to the contract
of include/wm2f.h, its agreement with scipy's binary_fill_holes, the host halves of the public layer, and that the maps
the GPU test compares on exercise every branch."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import clean_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _map(rows):
    """'.' free, a digit an id"""
    return np.array([[-1 if c == "." else int(c) for c in r] for r in rows], np.int64)


def test_ring_with_a_diagonal_gap_is_one_piece_and_does_not_leak():
    m = _map(["......",
              ".000..",
              ".0..0.",   # the ring's corner at (1, 4) is missing: (1, 3) and (2, 4) touch diagonally only
              ".0..0.",
              ".0000.",
              "......"])
    out, stats, n_out = R.clean_one(m, 1, keep="largest", fill_holes=True)
    assert stats[0].tolist() == [11, 1, 1, 11, 1, 4, 15, 0] and n_out == 1
    assert (out[2:4, 2:4] == 0).all() and out[1, 4] == -1  # the gap itself lies outside: it joins the border component


def test_hole_between_two_ids_stays():
    m = _map(["00011",
              "0..11",
              "00011"])
    out, stats, _ = R.clean_one(m, 2, fill_holes=True)
    assert np.array_equal(out, m) and stats[:, 4].tolist() == [0, 0]
    census = {}
    R.clean_one(m, 2, fill_holes=True, census=census)
    assert census["two_id"] == 1 and census["filled"] == 0


def test_hole_on_the_border_stays():
    m = _map(["0.0",
              "0.0",
              "000"])
    out, stats, _ = R.clean_one(m, 1, fill_holes=True)
    assert np.array_equal(out, m) and stats[0, 4] == 0


def test_ring_inside_the_hole_of_another_ring():
    m = _map(["0000000",
              "0.....0",
              "0.111.0",
              "0.1.1.0",
              "0.111.0",
              "0.....0",
              "0000000"])
    out, stats, _ = R.clean_one(m, 2, fill_holes=True)
    # the inner ring's hole is a hole of 1; the moat between the rings is bounded by both ids and stays
    assert out[3, 3] == 1 and (out[1, 1:6] == -1).all()
    assert stats[:, 4].tolist() == [0, 1] and stats[:, 5].tolist() == [0, 1]
    # without the inner ring's id (n = 1 makes id 1 free) the whole inside is one hole of 0
    out, stats, _ = R.clean_one(m, 1, fill_holes=True)
    assert (out == 0).all() and stats[0].tolist() == [24, 1, 1, 24, 1, 25, 49, 0]


def test_area_tie_goes_to_the_first_pixel():
    m = _map(["...00",
              ".....",
              "00...",
              ".....",
              "..0..",
              "...0."])
    out, stats, _ = R.clean_one(m, 1, keep="largest")
    want = np.full_like(m, -1)
    want[0, 3:5] = 0  # three pieces of two pixels (one of them joined diagonally): first pixels 3, 10 and 22
    assert np.array_equal(out, want) and stats[0].tolist() == [6, 3, 1, 2, 0, 0, 2, 0]


def test_dropped_speck_inside_a_plant_is_filled_by_the_plant():
    m = _map(["00000",
              "00100",
              "00000",
              ".....",
              "..11."])
    out, stats, n_out = R.clean_one(m, 2, keep="largest", fill_holes=True, relabel=True)
    assert (out[:3] == 0).all() and out[4].tolist() == [-1, -1, 1, 1, -1] and n_out == 2
    assert stats[0].tolist() == [14, 1, 1, 14, 1, 1, 15, 0] and stats[1].tolist() == [3, 2, 1, 2, 0, 0, 2, 1]
    # min_area alone does the same, and here also removes id 1 altogether: the ids close up
    out, stats, n_out = R.clean_one(m, 2, min_area=3, fill_holes=True, relabel=True)
    assert (out[:3] == 0).all() and (out[3:] == -1).all() and n_out == 1 and stats[:, 7].tolist() == [0, -1]
    # under KEEP_LARGEST an id whose largest piece is too small disappears
    _, stats, _ = R.clean_one(m, 2, keep="largest", min_area=3)
    assert stats[1].tolist() == [3, 2, 0, 0, 0, 0, 0, -1]


def test_max_hole_area_at_the_area_and_one_below():
    m = _map(["00000",
              "0...0",
              "00000"])
    out, stats, _ = R.clean_one(m, 1, fill_holes=True, max_hole_area=3)
    assert (out == 0).all() and stats[0, 4:6].tolist() == [1, 3]
    out, stats, _ = R.clean_one(m, 1, fill_holes=True, max_hole_area=2)
    assert np.array_equal(out, m) and stats[0, 4:6].tolist() == [0, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.uint8])
def test_no_op_call_returns_the_ids(dtype):
    maps = R.typed_maps(dtype, 37, 53)
    for min_area in (0, 1):
        out, stats, n_out = R.clean(maps, 6, keep="all", min_area=min_area)
        assert np.array_equal(out, R.id_keys(maps, 6))
        assert np.array_equal(stats[:, :, 0], stats[:, :, 6]) and np.array_equal(stats[:, :, 7] >= 0, stats[:, :, 0] > 0)
    if dtype == np.float32:  # what is planted is no id, -0.0 is id 0
        k = R.id_keys(maps, 6)
        assert (k[:, 37 // 2, 53 // 2] == -1).all() and (k[:, 37 // 3, 53 // 3] == -1).all() and (k[:, 37 // 4, 53 // 4] == -1).all()
        assert (k[np.signbit(maps) & (maps == 0)] == 0).all()


def test_equals_binary_fill_holes_on_single_id_maps():
    rng = np.random.default_rng(0)
    filled = 0
    for _ in range(20):
        mask = ndimage.binary_dilation(rng.random((40, 50)) < 0.12, iterations=2)
        out, stats, _ = R.clean_one(np.where(mask, 0, -1), 1, fill_holes=True)
        assert np.array_equal(out == 0, ndimage.binary_fill_holes(mask))
        filled += stats[0, 4]
    assert filled > 20


# ------------------------------------------------------------------------------------------------ host logic
def test_clean_options_validate():
    from weed_instance_segmentation_amd import CleanOptions
    o = CleanOptions()
    assert (o.min_area, o.keep, o.fill_holes, o.max_hole_area) == (0, "all", False, None)
    assert CleanOptions(min_area=16, keep="largest", fill_holes=True, max_hole_area=0).kernel_arguments() == {
        "keep": "largest", "min_area": 16, "fill_holes": True, "max_hole_area": 0}
    for bad in (dict(keep="biggest"), dict(min_area=-1), dict(min_area=2.5), dict(min_area=True), dict(max_hole_area=-1),
                dict(fill_holes="yes")):
        with pytest.raises(ValueError):
            CleanOptions(**bad)
    with pytest.raises(Exception):  # frozen
        o.min_area = 3


def test_segments_are_dropped_and_renumbered():
    from weed_instance_segmentation_amd.instances import cleaned_segments_info
    segments = [{"id": k, "label_id": k % 2, "was_fused": False, "score": 0.9 - 0.1 * k} for k in range(4)]
    stats = np.zeros((6, 8), np.int64)  # a fabricated kernel result: ids 1 and 3 survive (rows 4, 5: unused slots)
    stats[:, 7] = [-1, 0, -1, 1, -1, -1]
    got = cleaned_segments_info(segments, stats[:, 7])
    assert got == [{"id": 0, "label_id": 1, "was_fused": False, "score": 0.8}, {"id": 1, "label_id": 1, "was_fused": False, "score": 0.6}]
    assert segments[1]["id"] == 1  # the input is left as it was
    assert cleaned_segments_info([], stats[:, 7]) == []


def test_public_layer_refuses_to_run_without_a_gpu_and_checks_arguments():
    import torch
    from weed_instance_segmentation_amd import CleanOptions, _lib, clean_label_maps
    m = np.zeros((4, 4), np.int32)
    with pytest.raises(ValueError):
        clean_label_maps(m, 1, keep="biggest")
    with pytest.raises(TypeError):
        clean_label_maps(m, 1, options={"keep": "all"})
    if not torch.cuda.is_available():
        with pytest.raises(_lib.Wm2fError):
            clean_label_maps(m, 1, CleanOptions(keep="largest"))


def test_header_binding_and_build_list_agree():
    from weed_instance_segmentation_amd import _build, _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wm2f.h")).read(), flags=re.S)
    for name in ("wm2f_labelmap_clean_workspace", "wm2f_labelmap_clean"):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m and name in _lib.SIGNATURES
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
    for name in ("KEEP_ALL", "KEEP_LARGEST", "ALL", "PIECES", "CHOOSE", "HOLES", "PAINT"):
        m = re.search(r"#define\s+WM2F_CLEAN_" + name + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == getattr(_lib, "WM2F_CLEAN_" + name)
    assert "clean.hip" in _build.SOURCES


# ------------------------------------------------------------------------------------------------ non-vacuity
@pytest.mark.parametrize("shape", [(33, 33), (37, 53), (64, 64), (65, 257), (130, 516)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.uint8])
def test_the_gpu_tests_maps_exercise_every_branch(shape, dtype):
    """The maps tests/test_clean_gpu.py compares on (same generator, seeds, dtypes and options) drop pieces, fill holes,
    refuse holes over the limit, and hold free components on the border and between two ids."""
    ref = R.Cleaner(R.typed_maps(dtype, *shape), 6)
    for keep, min_area in (("all", 10), ("largest", 0)):
        census = {}
        ref.run(keep, min_area, census=census)
        assert census["dropped"] >= 1
    census = {}
    ref.run("all", 10, True, None, census=census)
    assert census["filled"] >= 1 and census["border"] >= 1 and census["two_id"] >= 1, census
    limited = {}
    ref.run("all", 10, True, 4, census=limited)
    assert limited["filled"] >= 1 and limited["filled"] + limited["over_limit"] == census["filled"]
    plain = {}
    ref.run("all", 0, True, None, census=plain)
    assert plain["border"] >= 1 and plain["two_id"] >= 1


@pytest.mark.parametrize("c,o", [(1, 2), (1, 0), (2, 0), (0, 1)])
def test_the_border_rule_map_shows_every_case(c, o):
    """The constructed map of the GPU tests holds all 16 combinations of the merge rule's four facts on both border kinds."""
    top, left = R.border_rule_cases(R.border_rule_map(c, o), c)
    assert len(top) == 16 and len(left) == 16
