"""Interior distance maps and aim points without a device: the restatements of the squared
distance agree -- brute force over all pairs, scipy's distance transform per id, the two-pass form (columns, then an
outward walk along the row that stops at step^2 >= best) and that form as the rows kernel walks it (bounded by the
pixel's run, reading no ids), which pins the kernel's exactness claim --
the aim-point rule on the shapes it was made for, the id rule for floats, the C ABI, and the public interface's argument
checks."""
import os
import re

import numpy as np
import pytest
import torch

import distance_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_maps():
    """About 40 maps of sides 1 .. 24: few ids in blobs, many ids per pixel, with and without background."""
    rng = np.random.default_rng(36)
    maps = []
    for i in range(36):
        H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        if i % 3 == 0:
            m = rng.integers(-1, 4, (H, W))
        elif i % 3 == 1:
            blocks = rng.integers(-1, 3, ((H + 2) // 3, (W + 4) // 5))
            m = np.kron(blocks, np.ones((3, 5), np.int64))[:H, :W]
        else:
            m = np.zeros((H, W), np.int64)
            m[rng.random((H, W)) < 0.1] = -1  # one large instance with pinholes
        maps.append(m.astype(np.int32))
    maps += [np.full((7, 9), 3, np.int32), np.full((1, 1), 0, np.int32), np.full((24, 2), 5, np.int32),  # one id fills it
             np.full((6, 5), -1, np.int32)]  # no id at all
    return maps


@pytest.mark.parametrize("border_outside", [True, False], ids=["outside", "inside"])
def test_restatements_agree(border_outside):
    n_far = 0
    for m in _random_maps():
        brute = R.d2_brute(m, border_outside)
        assert np.array_equal(R.d2_scipy(m, border_outside), brute), (m.shape, border_outside)
        assert np.array_equal(R.d2_two_pass(m, border_outside), brute), (m.shape, border_outside)
        assert np.array_equal(R.d2_run_bounded(m, border_outside), brute), (m.shape, border_outside)
        assert brute.dtype == np.int32 and (brute[R.id_keys(m) < 0] == 0).all() and (brute[R.id_keys(m) >= 0] >= 1).all()
        n_far += int((brute > 4).sum())
    assert n_far > 100  # the comparison is not one of maps without interiors


def test_one_id_and_no_id():
    full = np.full((7, 9), 3, np.int32)
    for f in (R.d2_brute, R.d2_scipy, R.d2_two_pass, R.d2_run_bounded):
        assert (f(full, False) == R.INT32_MAX).all()
        assert np.array_equal(f(full, True), np.minimum.outer(np.minimum(np.arange(7) + 1, 7 - np.arange(7)),
                                                               np.minimum(np.arange(9) + 1, 9 - np.arange(9))) ** 2)
        assert (f(np.full((6, 5), -1, np.int32), True) == 0).all() and (f(np.full((6, 5), -1, np.int32), False) == 0).all()
    assert (R.column_distance(full, False) == R.G_NONE).all()


def c_shape():
    """A 12 x 12 C on a 16 x 16 map: a square with the middle of its right side cut out."""
    m = np.full((16, 16), -1, np.int32)
    m[2:14, 2:14] = 0
    m[5:11, 5:14] = -1
    return m


def test_c_shape_centroid_is_background_aim_point_is_not():
    m = c_shape()
    cx, cy = R.rounded_centroid(R.id_keys(m), 0)
    ys, xs = np.nonzero(m == 0)
    assert abs(xs.mean() - 6.6) < 0.05 and abs(ys.mean() - 7.5) < 1e-9
    assert m[cy, cx] == -1 and m[int(ys.mean()), int(xs.mean())] == -1  # the centroid lies on bare soil
    for outside in (True, False):
        d2 = R.squared_distance(m, outside)
        x, y, d2max, zero = R.aim_points(m, d2, [0])[0]
        assert m[y, x] == 0 and d2[y, x] == d2max == d2[m == 0].max() and zero == 0
        assert d2max == 4  # the arms are 3 px wide: 2 px to the nearest soil


def test_bar_aims_at_the_middle_of_the_medial_line():
    m = np.full((9, 46), -1, np.int32)
    m[2:7, 3:43] = 1  # 5 x 40: the whole medial line y = 4, x = 5 .. 40 ties at d2 = 9
    d2 = R.squared_distance(m, True)
    assert d2.max() == 9 and int((d2 == 9).sum()) == 36
    assert R.aim_points(m, d2, [1], centred=False)[0].tolist() == [5, 4, 9, 0]  # its first pixel without the centroid
    cx, cy = R.rounded_centroid(R.id_keys(m), 1)
    assert (cx, cy) == (23, 4)  # (2 * sum + area) // (2 * area) of x = 3 .. 42: 22.5 rounds up
    assert R.aim_points(m, d2, [1])[0].tolist() == [23, 4, 9, 0]
    assert R.aim_points(m, d2, [1, 7])[1].tolist() == [-1, -1, 0, 0]  # an id without a pixel


def test_float_id_rule():
    f = np.array([[-1.0, 0.5, np.nan, 2.0 ** 24, -0.0, 3.0, np.inf, 2.0 ** 24 - 1]], np.float32)
    assert R.id_keys(f).tolist() == [[-1, -1, -1, -1, 0, 3, -1, 2 ** 24 - 1]]
    assert R.id_keys(np.array([[-5, 0, 70000]], np.int32)).tolist() == [[-1, 0, 70000]]
    assert R.id_keys(np.array([[0, 255]], np.uint8)).tolist() == [[0, 255]]
    # values that are no id end a run and get 0; -0.0 inside a region of 0 changes nothing
    g = np.zeros((5, 5), np.float32)
    plain = R.squared_distance(g, True)
    g[2, 2] = -0.0
    assert np.array_equal(R.squared_distance(g, True), plain)
    g[2, 2] = 0.5
    d2 = R.squared_distance(g, True)
    assert d2[2, 2] == 0 and d2[2, 1] == 1 and d2[1, 1] == 2


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_lib_binds_the_entry_points():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    want = {
        "int64_t wm2f_labelmap_distance_workspace": ["int B", "int H", "int W"],
        "int wm2f_labelmap_distance": ["const void* map", "int dtype", "int32_t* d2", "void* workspace", "int B", "int H",
                                       "int W", "int border_outside", "void* stream"],
        "int64_t wm2f_labelmap_aim_points_workspace": ["int B", "int N"],
        "int wm2f_labelmap_aim_points": ["const void* map", "int dtype", "const int32_t* d2", "const int32_t* ids",
                                         "const int32_t* n_ids", "const int64_t* stats", "int32_t* points",
                                         "void* workspace", "int B", "int H", "int W", "int N", "void* stream"],
    }
    for decl, args in want.items():
        proto = re.search(re.escape(decl) + r"\(([^;]*)\);", header)
        assert proto is not None, decl
        assert [a.strip() for a in " ".join(proto.group(1).split()).split(",")] == args
        res, argtypes = _lib.SIGNATURES[decl.split()[1]]
        assert len(argtypes) == len(args)
    assert "distance.hip" in _build.SOURCES


# ------------------------------------------------------------------------------------------ the public interface
def test_public_interface_checks_arguments_before_it_needs_a_device():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import aim_points, distance_maps, ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    assert pkg.distance_maps is distance_maps and pkg.aim_points is aim_points
    m = torch.zeros(4, 4)
    with pytest.raises(ValueError):
        aim_points(m, n=2, ids=[1])
    with pytest.raises(ValueError):
        aim_points(m)
    with pytest.raises(ValueError):
        aim_points(m, ids=[3, 3])
    with pytest.raises(ValueError):
        aim_points(m, n=2, border="beyond")
    with pytest.raises(ValueError):
        distance_maps(m, border="beyond")
    for f, kw in ((distance_maps, {}), (aim_points, {"n": 2})):
        with pytest.raises(TypeError):
            f(torch.zeros(4, 4, dtype=torch.int64), **kw)
        with pytest.raises(TypeError):
            f(np.zeros((4, 4), np.float64), **kw)
        with pytest.raises(ValueError):
            f(torch.zeros(4), **kw)
        with pytest.raises(ValueError):
            f(torch.zeros(1, 1, 4, 4), **kw)
    with pytest.raises(Wm2fError):  # the kernels take device tensors only
        ops.labelmap_distance(torch.zeros(1, 4, 4))
    with pytest.raises(Wm2fError):
        ops.labelmap_aim_points(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int32), N=2)
    with pytest.raises(TypeError):
        ops.labelmap_distance(np.zeros((1, 4, 4), np.float32))
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            distance_maps(m)
        with pytest.raises(Wm2fError):
            aim_points(m, n=2)
        with pytest.raises(Wm2fError):
            aim_points(m.numpy(), ids=[0, 5], border="inside")
