"""Skeletons without a GPU: the numpy restatement against a literal reading of the rule, the pinned
literals, what thinning must keep (pieces, holes, idempotence), the meaning of `status`, the options, the C ABI's
declarations and the errors that need no device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import skeleton_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every (H, W, seed, ids) of a ragged map the GPU tests use
RAGGED = [(31, 31, 31, 5), (32, 32, 32, 5), (33, 33, 33, 5), (65, 33, 65, 6), (33, 65, 5, 6), (40, 1, 4, 3), (1, 40, 4, 3),
          (70, 90, 7, 9), (70, 90, 8, 9), (128, 128, 1, 23), (256, 256, 1, 23)]


def _framed(mask, pad=2):
    return np.where(np.pad(mask, pad), 0, -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_against_the_literal_reading(seed):
    m = R.ragged(19 + seed, 23 - seed, seed, n=4)
    m[0, :] = 1  # live pixels on the image border
    m[:, -1] = 2
    for rounds in (1, 2, 9):
        assert np.array_equal(R.skeleton(m, 4, rounds)[0], R.skeleton_literal(m, 4, rounds)), (seed, rounds)
    f = m.astype(np.float32)
    f[3, 3], f[4, 4], f[5, 5] = 0.5, np.nan, 7.0
    assert np.array_equal(R.skeleton(f, 4, 9)[0], R.skeleton_literal(f, 4, 9))
    assert np.array_equal(R.skeleton(np.where(m < 0, 255, m).astype(np.uint8), 4, 9)[0], R.skeleton(m, 4, 9)[0])


def _settling(m, N):
    """(skeleton pixels, the first iteration that deletes nothing) of a map."""
    busy = R.settles_in(m, N)
    out, status = R.skeleton(m, N, busy + 1)
    assert status.tolist() == [int((out >= 0).sum()), busy, 0, busy + 1]
    return out, busy + 1


def test_pinned_literals():
    out, n = _settling(_framed(np.ones((2, 2), bool)), 1)
    assert n == 2 and np.argwhere(out >= 0).tolist() == [[2, 3]]  # the block's top-right pixel
    out, n = _settling(_framed(np.ones((5, 40), bool)), 1)
    assert n == 3 and R.skeleton_stats(out, 1)[0].tolist() == [36, 35, 0, 2, 0, 0, 0, 0]
    yy, xx = np.mgrid[0:48, 0:48]
    out, n = _settling(np.where((yy - 24) ** 2 + (xx - 24) ** 2 <= 400, 0, -1).astype(np.int32), 1)
    assert n == 21 and (out >= 0).sum() == 3
    for side, iterations in ((16, 9), (64, 33)):
        for m in (_framed(np.ones((side, side), bool)), np.zeros((side, side), np.int32)):  # framed, and filling its map
            out, n = _settling(m, 1)
            assert n == iterations and (out >= 0).sum() == 1
    assert _settling(np.zeros((96, 96), np.int32), 1)[1] == 49  # the GPU test's many-launch case


def test_plus_has_four_tips_and_a_junction():
    m = np.full((41, 41), -1, np.int32)
    m[18:23, 2:39] = 0
    m[2:39, 18:23] = 0
    out, _ = _settling(m, 1)
    row = R.skeleton_stats(out, 1)[0]
    assert row[0] == 65 and row[3] == 4 and row[4] >= 1 and row[5] == 0
    assert row[1] + row[2] == 64  # a tree: one link fewer than pixels
    y, x = 20, 20  # Guo and Hall's C is 0 at the centre of a 4-connected "+": the crossing number is what sees it
    assert out[y, x] == 0 and all(out[y + dy, x + dx] == 0 for dy, dx in R.OFFSETS[0::2])
    assert not any(out[y + dy, x + dx] == 0 for dy, dx in R.OFFSETS[1::2])


def test_ring_keeps_its_hole_and_has_no_tip():
    yy, xx = np.mgrid[0:64, 0:64]
    r2 = (yy - 32) ** 2 + (xx - 32) ** 2
    m = np.where((r2 >= 196) & (r2 <= 484), 0, -1).astype(np.int32)
    out, _ = _settling(m, 1)
    row = R.skeleton_stats(out, 1)[0]
    assert row[3] == 0 and row[5] == 0 and R.holes(out == 0) == 1 == R.holes(m == 0) and R.pieces(out == 0, True) == 1
    assert row[1] + row[2] == row[0]  # a closed curve: as many links as pixels


def test_two_ids_thin_independently():
    m = np.zeros((20, 20), np.int32)
    m[:, 10:] = 1
    out, _ = _settling(m, 2)
    for k, half in ((0, m == 0), (1, m == 1)):
        alone, _ = _settling(np.where(half, k, -1).astype(np.int32), 2)
        assert np.array_equal(out == k, alone == k) and (out == k).sum() == 11
    assert R.skeleton_stats(out, 2).tolist() == [[11, 10, 0, 2, 0, 0, 0, 0]] * 2


@pytest.mark.parametrize("H,W,seed,n", RAGGED)
def test_ragged_maps_keep_pieces_and_holes(H, W, seed, n):
    m = R.ragged(H, W, seed, n)
    out, settle = _settling(m, n)
    assert ((out == m) | (out == -1)).all()  # the skeleton lies inside the mask, with the mask's ids
    for k in range(n):
        assert R.pieces(out == k, True) == R.pieces(m == k, True), k
        assert R.holes(out == k) == R.holes(m == k), k
    again, status = R.skeleton(out, n, 3)
    assert np.array_equal(again, out) and status.tolist() == [int((out >= 0).sum()), 0, 0, 3]  # idempotent
    # status at R = 1, one short of settling, at the settling iteration and one past it
    first, s1 = R.skeleton(m, n, 1)
    assert s1[3] == 1 and s1[1] == (1 if settle > 1 else 0) and s1[2] == (m >= 0).sum() - (first >= 0).sum()
    if settle > 1:
        short, s = R.skeleton(m, n, settle - 1)
        assert s[2] != 0 and s[1] == settle - 1 and np.array_equal(short, out)  # the last busy iteration gave the result
    past, s = R.skeleton(m, n, settle + 1)
    assert np.array_equal(past, out) and s.tolist() == [int((out >= 0).sum()), settle - 1, 0, settle + 1]


def test_ragged_maps_have_holes_to_keep():
    assert sum(R.holes(R.ragged(H, W, seed, n) == k) for H, W, seed, n in RAGGED for k in range(n)) >= 5


def test_stats_columns_on_small_shapes():
    stairs = np.full((6, 6), -1, np.int32)
    for i in range(4):  # a staircase: its diagonal neighbours are joined by 4-links already
        stairs[1 + i, 1 + i] = 0
        if i < 3:
            stairs[1 + i, 2 + i] = 0
    assert R.skeleton_stats(stairs, 1)[0].tolist() == [7, 6, 0, 2, 0, 0, 0, 0]
    diag = np.full((6, 6), -1, np.int32)
    diag[np.arange(1, 5), np.arange(1, 5)] = 0
    diag[0, 5] = 1  # an isolated pixel of another id
    d2 = np.arange(36).reshape(6, 6)
    rows = R.skeleton_stats(diag, 2, d2=d2)
    assert rows.tolist() == [[4, 0, 3, 2, 0, 0, 7 + 14 + 21 + 28, 28], [1, 0, 0, 0, 0, 1, 5, 5]]
    assert np.array_equal(R.skeleton_stats(diag, ids=[1, 5, 0], d2=d2), np.stack([rows[1], np.zeros(8, np.int64), rows[0]]))
    t = R.traits(rows, area=np.array([4, 1]))
    assert t["skeleton_length"].tolist() == [3 * np.sqrt(2.0), 0.0] and t["max_width"][1] == 2 * np.sqrt(5.0) - 1
    assert np.isnan(R.traits(np.zeros((1, 8), np.int64))["mean_width"][0])


# ---------------------------------------------------------------------------------------------------- the host layer
def test_options_validation():
    from weed_instance_segmentation_amd import SkeletonOptions
    o = SkeletonOptions()
    assert (o.max_iterations, o.border, o.widths) == (64, "outside", True)
    with pytest.raises(Exception):
        o.widths = False  # frozen
    for bad in ({"max_iterations": 0}, {"max_iterations": 1025}, {"max_iterations": 2.0}, {"max_iterations": True},
                {"border": "edge"}, {"widths": 1}):
        with pytest.raises(ValueError):
            SkeletonOptions(**bad)
    assert SkeletonOptions(max_iterations=np.int64(1024), border="inside", widths=np.bool_(False)).max_iterations == 1024


def test_header_declares_and_lib_binds_the_entry_points():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    want = {
        "int64_t wm2f_labelmap_skeleton_workspace": ["int B", "int H", "int W"],
        "int wm2f_labelmap_skeleton": ["const void* map", "int dtype", "int32_t* out", "int32_t* status", "void* workspace",
                                       "int B", "int H", "int W", "int N", "int rounds", "int per_launch", "void* stream"],
        "int wm2f_labelmap_skeleton_stats": ["const int32_t* skel", "const int32_t* d2", "const int32_t* ids",
                                             "const int32_t* n_ids", "int64_t* stats", "int B", "int H", "int W", "int N",
                                             "void* stream"],
    }
    for decl, args in want.items():
        proto = re.search(re.escape(decl) + r"\(([^;]*)\);", header)
        assert proto is not None, decl
        assert [a.strip() for a in " ".join(proto.group(1).split()).split(",")] == args
        res, argtypes = _lib.SIGNATURES[decl.split()[1]]
        assert len(argtypes) == len(args)
    assert "skeleton.hip" in _build.SOURCES
    assert "m0 = (p6 | p7 | !p9) & p8" in header and "m1 = (p2 | p3 | !p5) & p4" in header  # the rule is there in full
    with open(os.path.join(ROOT, "profiles", "skeleton_resources.txt")) as f:
        record = f.read()
    rows = [[c.strip() for c in line.split("|")] for line in record.splitlines()[4:] if "|" in line]
    assert len(rows) == 15 and {r[4] for r in rows} == {"0"}  # init, status, stats, 3 dtypes x 4 per_launch: no scratch


def test_public_interface_and_errors_without_a_device():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import ops, skeleton, tiling
    from weed_instance_segmentation_amd._lib import Wm2fError
    assert pkg.skeleton_maps is skeleton.skeleton_maps and pkg.annotate_skeletons is skeleton.annotate_skeletons
    assert pkg.skeleton_statistics is skeleton.skeleton_statistics and pkg.SkeletonOptions is skeleton.SkeletonOptions
    assert list(inspect.signature(ops.labelmap_skeleton).parameters) == ["maps", "N", "rounds", "per_launch"]
    assert inspect.signature(ops.labelmap_skeleton).parameters["rounds"].default == 64
    assert list(inspect.signature(ops.labelmap_skeleton_stats).parameters) == ["skel", "ids", "n_ids", "N", "d2"]
    assert list(inspect.signature(pkg.skeleton_maps).parameters) == ["maps", "n", "options", "return_status"]
    assert list(inspect.signature(pkg.skeleton_statistics).parameters) == ["segmentation", "n", "ids", "options"]
    assert list(inspect.signature(pkg.annotate_skeletons).parameters) == ["result", "options"]
    for fn in (pkg.Mask2FormerInstancePostProcessor.post_process_instance_segmentation, tiling.merge_tile_results, tiling.segment_tiled):
        assert "skeleton" not in " ".join(inspect.signature(fn).parameters)  # the three entry points keep their signatures
    assert pkg.SKELETON_TRAITS == ("skeleton_pixels", "skeleton_length", "tips", "junction_pixels", "mean_width", "max_width",
                                   "length_per_area", "settled")
    m = np.zeros((4, 4), np.int32)
    with pytest.raises(ValueError):
        pkg.skeleton_statistics(m)
    with pytest.raises(ValueError):
        pkg.skeleton_statistics(m, n=1, ids=[0])
    with pytest.raises(ValueError):
        pkg.skeleton_statistics(m, ids=[1, 1])
    with pytest.raises(ValueError):
        pkg.skeleton_statistics(m, ids=[4096])
    with pytest.raises(TypeError):
        pkg.skeleton_statistics(m.astype(np.int64), n=1)
    with pytest.raises(ValueError):
        pkg.skeleton_maps(m[0], 1)
    with pytest.raises(ValueError):
        pkg.skeleton_maps(m, 4097)
    with pytest.raises(TypeError):
        pkg.skeleton_maps(m, 1, {"max_iterations": 3})
    with pytest.raises(ValueError):
        pkg.annotate_skeletons({"segmentation": m})
    with pytest.raises(ValueError):
        pkg.annotate_skeletons({"segmentation": m, "segments_info": [{"id": 0}, {"id": 0}]})
    z = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(Wm2fError):  # no CPU fallback
        ops.labelmap_skeleton(z, 1)
    with pytest.raises(Wm2fError):
        ops.labelmap_skeleton_stats(z, N=1)
    with pytest.raises(TypeError):
        ops.labelmap_skeleton(z.numpy(), 1)
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            pkg.skeleton_maps(m, 1)
        with pytest.raises(Wm2fError):
            pkg.skeleton_statistics(m, n=1)
    rows = torch.tensor([[5, 2, 2, 2, 0, 0, 45, 16], [0, 0, 0, 0, 0, 0, 0, 0]])
    t = pkg.skeleton_from_sums(rows, torch.tensor([20, 0]))
    want = R.traits(rows.numpy(), np.array([20, 0]))
    for k in ("skeleton_length", "mean_width", "max_width", "length_per_area"):
        assert t[k][0].item() == want[k][0] and torch.isnan(t[k][1]) and t[k].dtype == torch.float64
    assert t["mean_width"][0].item() == 5.0 and t["max_width"][0].item() == 7.0


def test_c_abi_reports_sizes_before_pointers():
    """The library loads and answers without a device: limits and argument errors never touch the GPU."""
    import ctypes
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    assert lib.wm2f_labelmap_skeleton(null, _lib.WM2F_I32, null, null, null, 1, 16385, 4, 2, 8, 0, null) == _lib.WM2F_EUNSUPPORTED
    assert lib.wm2f_labelmap_skeleton(null, _lib.WM2F_I32, null, null, null, 1, 4, 4, 4097, 8, 0, null) == _lib.WM2F_EUNSUPPORTED
    assert lib.wm2f_labelmap_skeleton(null, _lib.WM2F_I32, null, null, null, 1, 4, 4, 2, 1025, 0, null) == _lib.WM2F_EINVAL
    assert lib.wm2f_labelmap_skeleton(null, _lib.WM2F_I32, null, null, null, 1, 4, 4, 2, 8, 3, null) == _lib.WM2F_EINVAL
    assert lib.wm2f_labelmap_skeleton(null, _lib.WM2F_I32, null, null, null, 1, 4, 4, 2, 8, 4, null) == _lib.WM2F_EINVAL  # null pointer
    assert b"null pointer" in lib.wm2f_last_error()
    assert lib.wm2f_labelmap_skeleton_workspace(1, 64, 64) == 64 * 64 * 4 + 8192
    assert lib.wm2f_labelmap_skeleton_stats(null, null, null, null, null, 33, 4, 4, 2, null) == _lib.WM2F_EUNSUPPORTED
