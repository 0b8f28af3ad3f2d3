"""Nearest-instance maps, growth, cell counts and the treatment grid without a device: brute force
over all pairs agrees with the two-pass form exactly as the kernels walk it (and with the whole-array form the GPU tests
compare against), on inputs that hold ties, claimed pixels and pixels with nothing in range in numbers; scipy's distance
transform; hand cases; the cell-count restatement's geometry; the C ABI; and the public interface's argument checks."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import nearest_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = [0, 1, 2, 9, 10, 50, 24 * 24 * 2 + 1]  # the last is larger than any diagonal here


def _random_maps():
    """40 maps of sides 1 .. 24 and their N: sparse speckle of ids, 3 x 5 blocks, very sparse points among values that
    are no id of [0, N) and so are free."""
    rng = np.random.default_rng(38)
    maps = []
    for i in range(40):
        H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        if i % 3 == 0:
            m = np.where(rng.random((H, W)) < 0.12, rng.integers(0, 6, (H, W)), -1)
            N = 6
        elif i % 3 == 1:
            blocks = np.where(rng.random(((H + 2) // 3, (W + 4) // 5)) < 0.35, rng.integers(0, 4, ((H + 2) // 3, (W + 4) // 5)), -1)
            m = np.kron(blocks, np.ones((3, 5), np.int64))[:H, :W]
            N = 4
        else:
            m = np.where(rng.random((H, W)) < 0.03, rng.integers(0, 5, (H, W)), rng.integers(5, 9, (H, W)))  # 5 .. 8: free
            m[rng.random((H, W)) < 0.3] = -1
            N = 5
        maps.append((m.astype(np.int32), N, rng.random(N) < 0.5))
    return maps


MAPS = _random_maps()


@pytest.mark.parametrize("blocked", [False, True], ids=["query", "blocked"])
@pytest.mark.parametrize("subset", [False, True], ids=["all", "subset"])
def test_brute_force_equals_two_pass(blocked, subset):
    ties, claimed, none = [], 0, 0
    for m, N, some in MAPS:
        source = some if subset else None
        for cap in CAPS:
            bn, bd = R.nearest_brute(m, N, cap, source, blocked, ties=ties)
            for f in (R.nearest_two_pass, R.nearest_separable):
                tn, td = f(m, N, cap, source, blocked)
                assert np.array_equal(tn, bn) and np.array_equal(td, bd), (f.__name__, m.shape, cap, blocked, subset)
            claimed += int(((bn >= 0) & (bd > 0)).sum())
            none += int((bn < 0).sum())
            assert ((bn < 0) == (bd == R.INT32_MAX)).all() and bn.dtype == bd.dtype == np.int32
    # conditions on the inputs, not measurements: the sweep is one of ties, of claimed pixels and of pixels out of range
    assert len(ties) >= 500, len(ties)
    assert claimed >= 5000, claimed
    assert none >= 5000, none


def test_walk_without_the_prefix_count_gives_the_same():
    for m, N, some in MAPS[:12]:
        for cap in (1, 10, 50):
            a = R.nearest_two_pass(m, N, cap, some, False, use_prefix=True)
            b = R.nearest_two_pass(m, N, cap, some, False, use_prefix=False)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_uncapped_distance_is_scipys_transform():
    from scipy import ndimage
    n = 0
    for m, N, some in MAPS:
        key, is_src = R.source_mask(m, N, some)
        if not is_src.any():
            continue
        edt = ndimage.distance_transform_edt(~is_src)
        _, d2 = R.nearest_brute(m, N, CAPS[-1], some, False)
        assert np.array_equal(d2, np.rint(edt ** 2).astype(np.int32)), m.shape
        n += 1
    assert n >= 30


def test_hand_cases():
    m = np.full((5, 5), -1, np.int32)
    m[1, 1], m[3, 3] = 5, 2  # 5 up-left, 2 down-right, (2, 2) midway
    for f in (R.nearest_brute, R.nearest_two_pass, R.nearest_separable):
        near, d2 = f(m, 6, 50)
        assert near[2, 2] == 2 and d2[2, 2] == 2
        assert near[1, 1] == 5 and d2[1, 1] == 0 and near[0, 0] == 5 and near[4, 4] == 2
        # the cap's edge: d2 == max_d2 is claimed, max_d2 + 1 is not
        one = np.full((1, 9), -1, np.int32)
        one[0, 0] = 0
        near, d2 = f(one, 1, 9)
        assert near[0].tolist() == [0, 0, 0, 0, -1, -1, -1, -1, -1] and d2[0, 3] == 9 and d2[0, 4] == R.INT32_MAX
        near, d2 = f(one, 1, 8)
        assert near[0].tolist() == [0, 0, 0, -1, -1, -1, -1, -1, -1]
        # no source at all; every pixel a source; N = 1
        near, d2 = f(np.full((4, 6), -1, np.int32), 3, 100)
        assert (near == -1).all() and (d2 == R.INT32_MAX).all()
        near, d2 = f(np.full((4, 6), 7, np.int32), 3, 100)  # 7 is no id of [0, 3)
        assert (near == -1).all()
        full = np.arange(24, dtype=np.int32).reshape(4, 6) % 3
        near, d2 = f(full, 3, 100)
        assert np.array_equal(near, full) and (d2 == 0).all()
        near, d2 = f(full, 1, 0)  # N = 1: only id 0 is an instance, cap 0: only its own pixels
        assert np.array_equal(near, np.where(full == 0, 0, -1)) and (d2[full == 0] == 0).all()
        # a pixel of an instance that is no source: a query without the flag, its own id with it
        two = np.array([[0, -1, 1]], np.int32)
        near, d2 = f(two, 2, 4, [True, False], False)
        assert near.tolist() == [[0, 0, 0]] and d2.tolist() == [[0, 1, 4]]
        near, d2 = f(two, 2, 4, [True, False], True)
        assert near.tolist() == [[0, 0, 1]] and d2.tolist() == [[0, 1, 0]]


def test_growth_never_changes_an_instance_pixel():
    for m, N, some in MAPS:
        key, _ = R.source_mask(m, N)
        zero = R.grow(m, N, 0)
        assert np.array_equal(zero, key)  # margin 0: the identity on instance pixels, -1 elsewhere
        for margin, src in ((1.5, None), (3, np.nonzero(some)[0]), (Fraction(7, 2), some)):
            out = R.grow(m, N, margin, src)
            assert np.array_equal(out[key >= 0], key[key >= 0])
            assert ((out >= -1) & (out < N)).all()
    assert R.grow(np.zeros((3, 3), np.int32), 0, 2).tolist() == [[-1] * 3] * 3


# ----------------------------------------------------------------------------------------------------- cell counts
def test_cell_count_restatement_geometry():
    rng = np.random.default_rng(381)
    m = rng.integers(-1, 6, (13, 17)).astype(np.int32)
    group = np.array([0, 1, 255, 2, 0, 1], np.uint8)
    veto = rng.integers(0, 20, (13, 17)).astype(np.int32)
    grouped = int(np.isin(m, [0, 1, 3, 4, 5]).sum())
    for cell, off in (((4, 5), (0, 0)), ((4, 5), (3, 2)), ((1, 1), (0, 0)), ((20, 30), (7, 11)), ((13, 17), (0, 0)), ((3, 3), (2, 0))):
        GH, GW = R.grid_shape(13, 17, cell, off)
        for vd in (None, veto):
            c = R.cell_counts(m, group, 3, cell, off, vd, 9)
            assert c.shape == (GH, GW, 6) and c.dtype == np.int32
            assert int(c.sum()) == grouped  # kept and vetoed columns together hold every grouped pixel once
            if vd is None:
                assert (c[..., 3:] == 0).all()
            else:
                assert int(c[..., 3:].sum()) == int((np.isin(m, [0, 1, 3, 4, 5]) & (veto <= 9)).sum())
        if cell == (1, 1):
            assert np.array_equal(c[..., 0] + c[..., 3], np.isin(m, [0, 4]).astype(np.int32))
        if cell == (20, 30):
            assert (GH, GW) == (1, 1)
    # the cell of a pixel: (y + off_y) // h
    one = np.full((6, 6), -1, np.int32)
    one[2, 3] = 0
    c = R.cell_counts(one, np.array([0], np.uint8), 1, (3, 3), (2, 1))
    assert c.shape == (3, 3, 2) and c[1, 1, 0] == 1 and c.sum() == 1
    assert R.cell_counts(one, np.array([255], np.uint8), 1, (3, 3)).sum() == 0


def test_treatment_restatement_on_a_hand_case():
    m = np.full((8, 8), -1, np.int32)
    m[1:3, 1:3] = 0
    t = R.treatment(m, [(0, 1)], (4, 4), margin=1)
    assert t["cells"].tolist() == [[True, False], [False, False]] and t["coverage"][0, 0] == 12
    assert t["treated_fraction_exact"] == Fraction(1, 4) and t["instances"][0]["treated"] == 1.0
    t = R.treatment(m, [(0, 1)], (4, 4), margin=2)  # rows 0 .. 4 and columns 0 .. 4: the disc reaches three more cells
    assert t["cells"].tolist() == [[True, True], [True, False]]
    t = R.treatment(m, [(0, 1)], (4, 4), margin=2, min_pixels=3)
    assert t["cells"].tolist() == [[True, False], [False, False]]


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_lib_binds_the_entry_points():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    want = {
        "int64_t wm2f_labelmap_nearest_workspace": ["int B", "int H", "int W"],
        "int wm2f_labelmap_nearest": ["const void* map", "int dtype", "const uint8_t* source", "int32_t* nearest",
                                      "int32_t* d2", "void* workspace", "int B", "int H", "int W", "int N", "int max_d2",
                                      "int flags", "void* stream"],
        "int wm2f_labelmap_cell_counts": ["const void* map", "int dtype", "const uint8_t* group", "const int32_t* veto_d2",
                                          "int veto_max", "int32_t* counts", "int B", "int H", "int W", "int N", "int G",
                                          "int cell_h", "int cell_w", "int off_y", "int off_x", "void* stream"],
    }
    for decl, args in want.items():
        proto = re.search(re.escape(decl) + r"\(([^;]*)\);", header)
        assert proto is not None, decl
        assert [a.strip() for a in " ".join(proto.group(1).split()).split(",")] == args
        res, argtypes = _lib.SIGNATURES[decl.split()[1]]
        assert len(argtypes) == len(args)
    assert "nearest.hip" in _build.SOURCES
    assert "#define WM2F_NEAREST_BLOCKED 1" in header and "Voronoi" in header  # the uncapped map is named as out of scope


# ------------------------------------------------------------------------------------------ the public interface
def test_public_interface_checks_arguments_before_it_needs_a_device(tmp_path):
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import (TreatmentOptions, grow_label_maps, load_treatment_grid, nearest_instance_maps,
                                                ops, save_treatment_grid, treatment_grid)
    from weed_instance_segmentation_amd._lib import Wm2fError
    assert pkg.grow_label_maps is grow_label_maps and pkg.treatment_grid is treatment_grid
    m = torch.zeros(4, 4)
    for f in (lambda *a, **k: nearest_instance_maps(*a, **k), lambda *a, **k: grow_label_maps(*a, **k)):
        with pytest.raises(ValueError):
            f(m, 2, -1)
        with pytest.raises(ValueError):
            f(m, 2, 1025)
        with pytest.raises(ValueError):
            f(m, 2, float("nan"))
        with pytest.raises(ValueError):
            f(m, -1, 2)
        with pytest.raises(ValueError):
            f(m, 2, 2, sources=[2])
        with pytest.raises(ValueError):
            f(m, 2, 2, sources=np.array([True]))
        with pytest.raises(TypeError):
            f(m, 2, 2, sources=[0.5])
        with pytest.raises(TypeError):
            f(torch.zeros(4, 4, dtype=torch.int64), 2, 2)
        with pytest.raises(ValueError):
            f(torch.zeros(4), 2, 2)
    for bad in ({"cell": (0, 4)}, {"cell": (4, 4), "offset": (4, 0)}, {"cell": 4}, {"margin": -1}, {"protect": 2000},
                {"min_pixels": 0}, {"target_labels": [1], "protect_labels": [1]}, {"target_labels": [0.5]}, {"cell": (4.0, 4)}):
        with pytest.raises(ValueError):
            TreatmentOptions(**bad)
    opt = TreatmentOptions(cell=[8, 4], offset=(1, 3), margin=2.5, protect=Fraction(3, 2), target_labels=[1], protect_labels=[0])
    assert opt.cell == (8, 4) and opt.is_target(1) and not opt.is_target(0) and opt.is_protected(0)
    assert TreatmentOptions(protect_labels=[0]).is_target(3) and not TreatmentOptions(protect_labels=[0]).is_target(0)
    with pytest.raises(Exception):
        opt.cell = (1, 1)  # frozen
    with pytest.raises(TypeError):
        treatment_grid({"segmentation": m, "segments_info": []}, {"cell": (4, 4)})
    with pytest.raises(ValueError):
        treatment_grid({"segmentation": m}, opt)
    with pytest.raises(ValueError):
        treatment_grid({"segmentation": torch.zeros(1, 4, 4), "segments_info": []}, opt)
    with pytest.raises(ValueError):
        treatment_grid({"segmentation": m, "segments_info": [{"id": 0, "label_id": 1}, {"id": 0, "label_id": 1}]}, opt)
    with pytest.raises(Wm2fError):  # the kernels take device tensors only
        ops.labelmap_nearest(torch.zeros(1, 4, 4), 2, 4)
    with pytest.raises(Wm2fError):
        ops.labelmap_cell_counts(torch.zeros(1, 4, 4), torch.zeros(1, 2, dtype=torch.uint8), 1, (2, 2))
    with pytest.raises(TypeError):
        ops.labelmap_nearest(np.zeros((1, 4, 4), np.float32), 2, 4)
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            nearest_instance_maps(m, 2, 3)
        with pytest.raises(Wm2fError):
            grow_label_maps(m.numpy(), 2, 1.5, sources=[0])
        with pytest.raises(Wm2fError):
            treatment_grid({"segmentation": m, "segments_info": [{"id": 0, "label_id": 1}]}, opt)
    # the file format needs no device
    grid = {"cells": np.array([[True, False], [False, True]]), "treated_fraction_exact": Fraction(1, 3), "treated_fraction": 1 / 3,
            "instances": [{"id": 0, "label_id": 1, "treated": 0.5, "vetoed_fraction": float("nan")}],
            "cell": (4, 4), "offset": (0, 1), "image_size": (8, 7), "grid_size": (2, 2)}
    path = tmp_path / "grid.json"
    save_treatment_grid(path, grid, transform=(0.5, 0, 10, 0, -0.5, 20))
    back = load_treatment_grid(path)
    assert np.array_equal(back["cells"], grid["cells"]) and back["treated_fraction_exact"] == Fraction(1, 3)
    assert back["transform"] == (0.5, 0.0, 10.0, 0.0, -0.5, 20.0) and back["cell"] == (4, 4) and back["offset"] == (0, 1)
    assert back["instances"][0]["treated"] == 0.5 and np.isnan(back["instances"][0]["vetoed_fraction"])
    with pytest.raises(ValueError):
        save_treatment_grid(path, grid, transform=(1, 2, 3))
