"""Per-plant shape traits, the part that needs no GPU: the numpy / scipy restatement on hand cases,
`shape_from_sums` on CPU tensors against independent numpy (np.var, np.cov, np.linalg.eigvalsh), the cancellation case
far from the origin, the C ABI's declarations and the public keywords."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from shape_reference import ellipse_scene, hull_reference, mask_hull, mask_shape_row, shape_stats_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQRT2 = np.sqrt(2.0)


# ------------------------------------------------------------------------------------------------- the restatement
def test_reference_on_hand_cases():
    one = np.zeros((5, 7), bool)
    one[2, 3] = True
    assert mask_shape_row(one) == [1, 3, 2, 9, 4, 6, 4, 0, 0, 0]
    row, v = mask_hull(one)
    assert row == [4, 2, 2] and v.tolist() == [[3, 2], [4, 2], [4, 3], [3, 3]]

    sq = np.zeros((6, 6), bool)
    sq[1:5, 1:5] = True
    assert mask_shape_row(sq)[6:] == [16, 12, 0, 0]
    row, v = mask_hull(sq)
    assert row == [4, 32, 32] and v.tolist() == [[1, 1], [5, 1], [5, 5], [1, 5]]

    whole = np.ones((4, 5), bool)  # the outside of the image is not the instance
    assert mask_shape_row(whole)[6:] == [18, 14, 0, 0]
    assert mask_hull(whole)[0] == [4, 40, 41]

    assert mask_shape_row(np.zeros((3, 3), bool)) == [0] * 10 and mask_hull(np.zeros((3, 3), bool))[0] == [0, 0, 0]


def test_reference_diagonal_ring_and_pieces():
    diag = np.eye(9, dtype=bool)
    row = mask_shape_row(diag)
    assert row[6:] == [36, 0, 7, 0]  # the two end pixels have code 11, which counts nowhere
    assert mask_hull(diag)[0][0] == 6

    disc = np.zeros((12, 12), bool)
    disc[2:10, 2:10] = True
    ring = disc.copy()
    ring[4:8, 4:8] = False
    assert mask_shape_row(ring)[6] == mask_shape_row(disc)[6] + 16
    assert mask_shape_row(ring)[7:] != mask_shape_row(disc)[7:]
    assert mask_hull(ring)[0] == mask_hull(disc)[0] and np.array_equal(mask_hull(ring)[1], mask_hull(disc)[1])

    two = np.zeros((20, 30), bool)
    two[1:3, 2:4] = True
    two[15:18, 25:27] = True
    row, v = mask_hull(two)
    assert row[0] == 6 and v[0].tolist() == [2, 1] and v[1].tolist() == [4, 1]
    e, f = np.roll(v, -1, 0) - v, np.roll(v, -2, 0) - np.roll(v, -1, 0)
    assert (e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0] > 0).all()  # the documented sign


def test_reference_sides_are_even_and_at_least_four():
    rng = np.random.default_rng(5)
    seen = 0
    for shape, N in (((7, 9), 3), ((33, 65), 6), ((40, 57), 12)):
        m = ellipse_scene(rng, shape, N)
        rows = shape_stats_reference(m, N=N)
        hull, verts = hull_reference(m, N=N)
        for r in range(N):
            if rows[r, 0] == 0:
                assert not rows[r].any() and not hull[r].any() and len(verts[r]) == 0
                continue
            seen += 1
            assert rows[r, 6] % 2 == 0 and rows[r, 6] >= 4
            assert rows[r, 7:].sum() <= rows[r, 0] and hull[r, 1] >= 2 * rows[r, 0] and hull[r, 0] == len(verts[r]) >= 4
    assert seen >= 12


# ------------------------------------------------------------------------------------------------- shape_from_sums
def _numpy_traits(mask):
    ys, xs = np.nonzero(mask)
    x, y = xs.astype(np.float64), ys.astype(np.float64)
    cov = np.array([[np.var(x), np.mean((x - x.mean()) * (y - y.mean()))], [0, np.var(y)]])
    cov[1, 0] = cov[0, 1]
    l2, l1 = np.linalg.eigvalsh(cov)
    w, v = np.linalg.eigh(cov)
    major = v[:, 1]  # the eigenvector of the larger eigenvalue
    return {"mu": (cov[0, 0], cov[1, 1], cov[0, 1]), "l": (l1, max(l2, 0.0)), "angle": np.arctan2(major[1], major[0]),
            "centroid": (x.mean(), y.mean())}


def test_shape_from_sums_against_numpy():
    from weed_instance_segmentation_amd.instances import shape_from_sums
    from instance_stats_reference import instance_stats_reference
    rng = np.random.default_rng(17)
    checked = oriented = 0
    for shape, N in (((33, 65), 6), ((40, 57), 12), ((130, 70), 9)):
        m = ellipse_scene(rng, shape, N)
        rows = shape_stats_reference(m, N=N)
        hull, verts = hull_reference(m, N=N)
        K = max(1, int(hull[:, 0].max()))
        pts = np.full((N, K, 2), -1, np.int32)
        for r in range(N):
            pts[r, :len(verts[r])] = verts[r]
        stats = instance_stats_reference(m, N=N)
        t = shape_from_sums(torch.from_numpy(rows), torch.from_numpy(stats), (torch.from_numpy(hull), torch.from_numpy(pts)))
        assert all(v.dtype in (torch.float64, torch.int64) for v in t.values())
        for r in range(N):
            if rows[r, 0] == 0:
                for name in ("orientation", "axis_major_length", "eccentricity", "perimeter", "circularity", "extent", "solidity",
                             "area_convex", "feret_diameter_max", "hull_perimeter", "convexity", "equivalent_diameter"):
                    assert torch.isnan(t[name][r]), name
                assert torch.isnan(t["centroid"][r]).all() and t["area"][r] == 0
                continue
            checked += 1
            want = _numpy_traits(m == r)
            A = float(rows[r, 0])
            np.testing.assert_allclose(t["centroid"][r].numpy(), want["centroid"], rtol=1e-12)
            np.testing.assert_allclose(t["moments_central"][r].numpy(), want["mu"], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(t["axis_major_length"][r], 4 * np.sqrt(want["l"][0]), rtol=1e-9)
            np.testing.assert_allclose(t["axis_minor_length"][r], 4 * np.sqrt(want["l"][1]), rtol=1e-9, atol=1e-7)
            ecc = np.sqrt(1 - want["l"][1] / want["l"][0]) if want["l"][0] > 0 else 0.0
            np.testing.assert_allclose(t["eccentricity"][r], ecc, rtol=1e-9, atol=1e-7)
            mu20, mu02, mu11 = want["mu"]
            if np.sqrt(4 * mu11 ** 2 + (mu20 - mu02) ** 2) > 1e-6 * (mu20 + mu02):
                oriented += 1
                diff = (float(t["orientation"][r]) - want["angle"]) % np.pi
                assert min(diff, np.pi - diff) < 1e-9, (r, float(t["orientation"][r]), want["angle"])
            assert -np.pi / 2 < float(t["orientation"][r]) <= np.pi / 2
            per = rows[r, 7] + SQRT2 * rows[r, 8] + (1 + SQRT2) / 2 * rows[r, 9]
            np.testing.assert_allclose(t["perimeter"][r], per, rtol=1e-12)
            if per > 0:
                np.testing.assert_allclose(t["circularity"][r], 4 * np.pi * A / per ** 2, rtol=1e-9)
            else:
                assert torch.isnan(t["circularity"][r])
            assert int(t["crack_length"][r]) == rows[r, 6]
            np.testing.assert_allclose(t["equivalent_diameter"][r], np.sqrt(4 * A / np.pi), rtol=1e-12)
            ys, xs = np.nonzero(m == r)
            np.testing.assert_allclose(t["extent"][r], A / ((np.ptp(xs) + 1) * (np.ptp(ys) + 1)), rtol=1e-12)
            np.testing.assert_allclose(t["area_convex"][r], hull[r, 1] / 2, rtol=1e-12)
            np.testing.assert_allclose(t["solidity"][r], 2 * A / hull[r, 1], rtol=1e-12)
            np.testing.assert_allclose(t["feret_diameter_max"][r], np.sqrt(hull[r, 2]), rtol=1e-12)
            v = verts[r].astype(np.float64)
            hp = np.sqrt(((np.roll(v, -1, 0) - v) ** 2).sum(1)).sum()
            np.testing.assert_allclose(t["hull_perimeter"][r], hp, rtol=1e-9)
            np.testing.assert_allclose(t["convexity"][r], hp / rows[r, 6], rtol=1e-9)
            assert int(t["n_hull_vertices"][r]) == len(v)
    assert checked >= 15 and 2 * oriented >= checked


def test_orientation_convention_and_degenerate_shapes():
    from weed_instance_segmentation_amd.instances import shape_from_sums
    bar_x, bar_y, dot = np.zeros((9, 9), bool), np.zeros((9, 9), bool), np.zeros((9, 9), bool)
    bar_x[4, 1:8] = True
    bar_y[1:8, 4] = True
    dot[3, 3] = True
    down = np.eye(9, dtype=bool)  # runs towards +x and +y: y is down, so the angle is +pi/4
    rows = torch.tensor([mask_shape_row(k) for k in (bar_x, bar_y, dot, down, down[::-1])])
    t = shape_from_sums(rows)
    np.testing.assert_allclose(t["orientation"].numpy(), [0, np.pi / 2, 0, np.pi / 4, -np.pi / 4], atol=1e-12)
    assert t["eccentricity"].tolist()[:3] == [1.0, 1.0, 0.0]
    assert t["axis_minor_length"].tolist()[:3] == [0.0, 0.0, 0.0] and t["axis_major_length"][2] == 0
    assert torch.isnan(t["circularity"][2]) and t["perimeter"][2] == 0  # a lone pixel has perimeter 0
    assert "extent" not in t and "solidity" not in t and "hull_perimeter" not in t


def test_central_moments_do_not_cancel_far_from_the_origin():
    from weed_instance_segmentation_amd.instances import shape_from_sums
    rng = np.random.default_rng(2)
    blob = rng.random((3, 5)) < 0.7
    blob[1, 2] = True
    near, far = np.zeros((8, 16384), bool), np.zeros((16384, 16384 // 64), bool)
    near[2:5, 3:8] = blob
    wide = np.zeros((8, 16384), bool)
    wide[2:5, 16003:16008] = blob
    rows = torch.tensor([mask_shape_row(near), mask_shape_row(wide)])
    t = shape_from_sums(rows)
    for name in ("moments_central", "axis_major_length", "axis_minor_length", "orientation", "eccentricity"):
        np.testing.assert_allclose(t[name][1].numpy(), t[name][0].numpy(), rtol=1e-12, atol=0, err_msg=name)
    far[16000:16003, 100:105] = blob  # and along y
    tall = shape_from_sums(torch.tensor([mask_shape_row(far)]))
    np.testing.assert_allclose(tall["moments_central"][0].numpy(), t["moments_central"][0].numpy(), rtol=1e-12)


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_lib_binds_the_entry_points():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    want = {
        "int wm2f_labelmap_shape_stats": ["const void* map", "int dtype", "const int32_t* ids", "const int32_t* n_ids",
                                          "int64_t* shape", "int B", "int H", "int W", "int N", "void* stream"],
        "int64_t wm2f_labelmap_hull_workspace": ["int B", "int N", "int64_t rows"],
        "int wm2f_labelmap_hull": ["const void* map", "int dtype", "const int32_t* ids", "const int32_t* n_ids",
                                   "const int64_t* stats", "int64_t* hull", "void* workspace", "int64_t rows", "int B", "int H",
                                   "int W", "int N", "void* stream"],
        "int wm2f_labelmap_hull_vertices": ["const int64_t* stats", "const int64_t* hull", "const void* workspace",
                                            "int64_t rows", "int32_t* vertices", "int B", "int H", "int N", "int K",
                                            "void* stream"],
    }
    for decl, args in want.items():
        proto = re.search(re.escape(decl) + r"\(([^;]*)\);", header)
        assert proto is not None, decl
        assert [a.strip() for a in " ".join(proto.group(1).split()).split(",")] == args
        res, argtypes = _lib.SIGNATURES[decl.split()[1]]
        assert len(argtypes) == len(args)
    assert "shape.hip" in _build.SOURCES
    assert "fits int64" in header and "POSITIVE" in header  # the header says why the sums fit and which sign the hull has


# ------------------------------------------------------------------------------------------ the public interface
def test_public_interface():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import instances, ops, tiling
    from weed_instance_segmentation_amd._lib import Wm2fError
    assert pkg.shape_statistics is instances.shape_statistics and pkg.shape_from_sums is instances.shape_from_sums
    assert str(inspect.signature(ops.labelmap_shape_stats)).startswith("(maps: 'torch.Tensor', ids:")
    assert list(inspect.signature(ops.labelmap_shape_stats).parameters) == ["maps", "ids", "n_ids", "N"]
    assert list(inspect.signature(ops.labelmap_hull).parameters)[:4] == ["maps", "ids", "n_ids", "N"]
    assert list(inspect.signature(pkg.shape_statistics).parameters) == ["segmentation", "n", "ids", "hull", "return_hull_vertices"]
    for fn in (pkg.Mask2FormerInstancePostProcessor.post_process_instance_segmentation, tiling.merge_tile_results, tiling.segment_tiled):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "return_shape_stats" and p["return_shape_stats"].default is False
    m = np.zeros((4, 4), np.int32)
    with pytest.raises(ValueError):
        pkg.shape_statistics(m)
    with pytest.raises(ValueError):
        pkg.shape_statistics(m, n=1, ids=[0])
    with pytest.raises(ValueError):
        pkg.shape_statistics(m, ids=[1, 1])
    with pytest.raises(TypeError):
        pkg.shape_statistics(m.astype(np.int64), n=1)
    with pytest.raises(ValueError):
        pkg.shape_statistics(m[0], n=1)
    with pytest.raises(ValueError):
        pkg.shape_statistics(m, n=1, hull=False, return_hull_vertices=True)
    with pytest.raises(Wm2fError):  # no CPU fallback
        ops.labelmap_shape_stats(torch.zeros(1, 4, 4, dtype=torch.int32), N=1)
    with pytest.raises(Wm2fError):
        ops.labelmap_hull(torch.zeros(1, 4, 4, dtype=torch.int32), N=1)
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            pkg.shape_statistics(m, n=1)
