"""Boundary bands and Boundary AP on the host: the numpy restatements of tests/boundary_reference.py
against an independent construction and a hand-derived case, the band width rule, the metric's argument checking and
the header's declarations.  tests/test_boundary_gpu.py holds the kernels to these restatements."""
import os
import re

import numpy as np
import pytest

import boundary_reference as R
from oracle import coco_eval as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocky_map(rng, H, W, n_ids=4, block=5, holes=True):
    """Random rectangles of a few ids on a -1 background, so that interiors exist at small d."""
    m = np.full((H, W), -1, np.int32)
    for _ in range(6):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w = int(rng.integers(1, 3 * block)), int(rng.integers(1, 3 * block))
        m[y:y + h, x:x + w] = int(rng.integers(0, n_ids))
    if holes and H * W > 4:
        m[int(rng.integers(0, H)), int(rng.integers(0, W))] = -1
    return m


SIDES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (5, 11), (11, 5), (12, 12), (17, 23), (30, 21), (40, 40), (23, 40)]


@pytest.mark.parametrize("d", [1, 2, 5])
def test_square_form_equals_iterated_3x3_erosion(d):
    """The contract's first form, built independently: pad the mask with a ring of zeros, erode d times with a 3 x 3
    square (nothing beyond the ring erodes: border_value=1), crop, subtract."""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(d)
    n_bands = 0
    for H, W in SIDES:
        for rep in range(3):
            m = _blocky_map(rng, H, W)
            got = R.boundary_map(m, d)
            assert got.dtype == np.int32 and got.shape == m.shape
            assert (got[m < 0] == -1).all()
            for k in np.unique(m[m >= 0]):
                mask = m == k
                er = ndi.binary_erosion(np.pad(mask, 1), np.ones((3, 3)), iterations=d, border_value=1)[1:-1, 1:-1]
                assert np.array_equal(got == k, mask & ~er), (H, W, rep, int(k))
                n_bands += int((mask & er).any())
    assert n_bands > 0  # interiors do occur: the comparison is not one of full masks only
    big = np.full((40, 40), -1, np.int32)
    big[3:35, 2:30] = 7  # a 32 x 28 rectangle keeps (32 - 2d) x (28 - 2d) interior pixels
    assert (R.boundary_map(big, d) == 7).sum() == 32 * 28 - (32 - 2 * d) * (28 - 2 * d)


@pytest.mark.parametrize("d", [1, 2, 5])
def test_separable_form_equals_square_form(d):
    rng = np.random.default_rng(10 + d)
    for H, W in SIDES:
        for rep in range(2):
            m = _blocky_map(rng, H, W)
            assert np.array_equal(R.boundary_map_separable(m, d), R.boundary_map(m, d)), (H, W, rep)
    f = _blocky_map(rng, 30, 30).astype(np.float32)
    f[0, 0], f[1, 1], f[2, 2], f[3, 3] = -0.0, 2.5, np.nan, 2.0 ** 24
    assert np.array_equal(R.boundary_map_separable(f, d), R.boundary_map(f, d))


@pytest.mark.parametrize("d", [1, 2, 5, 50])
def test_every_present_id_has_a_band(d):
    rng = np.random.default_rng(20 + d)
    for H, W in SIDES:
        m = _blocky_map(rng, H, W)
        got = R.boundary_map(m, d)
        for k in np.unique(m[m >= 0]):
            assert (got == k).any(), (H, W, int(k))
        assert set(np.unique(got)) <= set(np.unique(m)) | {-1}


def test_float_id_rule():
    f = np.array([[-1.0, -0.0, 2.5, np.nan, np.inf, 3.0, 2.0 ** 24, 2.0 ** 24 - 1]], np.float32)
    assert R.id_keys(f).tolist() == [[-1, 0, -1, -1, -1, 3, -1, 2 ** 24 - 1]]
    assert R.id_keys(np.array([[-5, 0, 7]], np.int32)).tolist() == [[-1, 0, 7]]
    assert R.id_keys(np.array([[0, 255]], np.uint8)).tolist() == [[0, 255]]


@pytest.mark.parametrize("h,w,want", [(1024, 1024, 29), (256, 256, 7), (37, 53, 1), (8, 8, 1)])
def test_boundary_dilation(h, w, want):
    from weed_instance_segmentation_amd.instances import boundary_dilation
    assert boundary_dilation(h, w) == want == R.boundary_dilation(h, w)
    assert isinstance(boundary_dilation(h, w), int)


def test_boundary_dilation_ratio_and_arguments():
    from weed_instance_segmentation_amd import metrics
    from weed_instance_segmentation_amd.instances import boundary_dilation
    assert boundary_dilation(1024, 1024, 0.01) == 14 and boundary_dilation(600, 800, 0.02) == 20
    assert metrics.boundary_dilation is boundary_dilation and callable(metrics.boundary_maps)
    with pytest.raises(ValueError):
        boundary_dilation(0, 10)
    with pytest.raises(ValueError):
        boundary_dilation(10, 10, 0.0)


def test_iou_type_validation_touches_no_device():
    from weed_instance_segmentation_amd.metrics import IOU_TYPES, MeanAveragePrecision
    assert IOU_TYPES == ("segm", "bbox", "boundary")
    assert MeanAveragePrecision(iou_type="boundary").iou_type == ("boundary",)
    assert MeanAveragePrecision(iou_type=("segm", "boundary")).iou_type == ("segm", "boundary")
    assert MeanAveragePrecision(iou_type=["boundary", "bbox", "segm"], boxes_from_masks=True).iou_type == ("boundary", "bbox", "segm")
    m = MeanAveragePrecision(iou_type="boundary", dilation_ratio=0.05)
    assert m.dilation_ratio == 0.05 and MeanAveragePrecision().dilation_ratio == 0.02
    with pytest.raises(ValueError, match="boxes_from_masks"):
        MeanAveragePrecision(iou_type=("boundary", "bbox"))
    for bad in ("boundaries", ("boundary", "boundary"), (), ("segm", "edge"), 3):
        with pytest.raises(ValueError):
            MeanAveragePrecision(iou_type=bad)
    for bad in (0, -0.1, 1.0, "0.02", None):
        with pytest.raises(ValueError, match="dilation_ratio"):
            MeanAveragePrecision(iou_type="boundary", dilation_ratio=bad)
    for types in ("boundary", ("segm", "boundary")):  # the mask-stack route says where to go instead
        with pytest.raises(ValueError, match="update_from_maps"):
            MeanAveragePrecision(iou_type=types).update([], [])
    with pytest.raises(ValueError):
        MeanAveragePrecision(iou_type=("segm", "boundary")).compute_per_image()
    with pytest.raises(ValueError):
        MeanAveragePrecision(iou_type="segm").compute_per_image("boundary")


def test_merge_results_prefixes_boundary():
    import torch
    from weed_instance_segmentation_amd.metrics import merge_results
    one = {"map": torch.tensor(0.5), "classes": torch.tensor([1])}
    assert merge_results({"boundary": one}) is one
    both = merge_results({"segm": one, "boundary": one})
    assert set(both) == {"segm_map", "boundary_map", "classes"}


def test_header_declares_the_new_symbols():
    from weed_instance_segmentation_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wm2f.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wm2f_[a-z0-9_]+)\s*\(", src))
    for name in ("wm2f_labelmap_boundary", "wm2f_labelmap_boundary_workspace", "wm2f_coco_match_min"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wm2f_coco_match_min"][1]) == len(_lib.SIGNATURES["wm2f_coco_match"][1]) + 3
    assert "boundary.hip" in __import__("weed_instance_segmentation_amd._build", fromlist=["SOURCES"]).SOURCES


def test_hand_case_pins_the_reference_subclass():
    """One 40 x 40 GT square at rows 10..49, columns 10..49 of a 64 x 64 image, the prediction the same square moved 3 px
    to the right (columns 13..52), dilation 2.

    Mask IoU: the squares share 40 x 37 = 1480 px, union 1600 + 1600 - 1480 = 1720: 1480 / 1720 = 0.8605, which reaches
    the eight thresholds 0.50 .. 0.85 and not 0.90, 0.95.
    Bands: a square's interior at d = 2 is 36 x 36, so each band is the ring of width 2 with 1600 - 1296 = 304 px.  The
    two rings share the top and bottom strips (2 rows each) over the common columns 13..49: 2 * 2 * 37 = 148 px; the
    vertical strips (columns 10-11 and 48-49 against 13-14 and 51-52) share nothing on rows 12..47.  Union 608 - 148
    = 460, boundary IoU 148 / 460 = 0.3217, the minimum of the two, below every threshold.
    So "segm" matches at thresholds {0.50 .. 0.85} (AP 0.8) and "boundary" at none (AP 0)."""
    import torch
    gt = np.zeros((1, 64, 64), bool)
    gt[0, 10:50, 10:50] = True
    dt = np.zeros((1, 64, 64), bool)
    dt[0, 10:50, 13:53] = True
    assert R.mask_band(gt[0], 2).sum() == 304 and R.mask_band(dt[0], 2).sum() == 304
    assert int((R.mask_band(gt[0], 2) & R.mask_band(dt[0], 2)).sum()) == 148
    assert C.mask_iou(dt, gt)[0, 0] == 1480 / 1720
    assert R.boundary_iou_matrix(dt, gt, 2)[0, 0] == 148 / 460
    preds = [{"masks": torch.from_numpy(dt), "scores": torch.tensor([0.9]), "labels": torch.tensor([1])}]
    target = [{"masks": torch.from_numpy(gt), "labels": torch.tensor([1])}]
    segm, bnd = C.CocoSegmEval(), R.BoundaryCocoEval(dilation=2)
    segm.update(preds, target)
    bnd.update(preds, target)
    m_segm = segm.evaluate([1])[0][0][0]["dtMatches"][:, 0]
    m_bnd = bnd.evaluate([1])[0][0][0]["dtMatches"][:, 0]
    assert m_segm.tolist() == [1] * 8 + [0] * 2 and m_bnd.tolist() == [0] * 10
    assert float(segm.compute()["map"]) == pytest.approx(0.8) and float(bnd.compute()["map"]) == 0.0
    # a prediction equal to the GT has boundary IoU 1: the subclass does not just reject everything
    same = R.BoundaryCocoEval(dilation=2)
    same.update([{**preds[0], "masks": torch.from_numpy(gt)}], target)
    assert float(same.compute()["map"]) == 1.0
    # the ratio rule: 64 x 64 -> d = 2
    auto = R.BoundaryCocoEval()
    auto.update(preds, target)
    assert R.boundary_dilation(64, 64) == 2 and auto.evaluate([1])[0][0][0]["dtMatches"][:, 0].tolist() == [0] * 10


def test_reference_boundary_ap_differs_from_segm_ap_on_the_fixtures():
    """The fixtures of the GPU comparison: the reference's boundary result must differ from its segm result, or the GPU
    test could pass with both routes computing plain mask AP."""
    segs, infos, maps, mappings = R.ap_fixtures()
    assert len(segs) == 3 and all(s.shape == (96, 128) and g.shape == (96, 128) for s, g in zip(segs, maps))
    preds, target = R.fixtures_as_stacks(segs, infos, maps, mappings)
    n_diff = 0
    for i in range(3):
        segm, bnd = C.CocoSegmEval(), R.BoundaryCocoEval()
        segm.update(preds[i:i + 1], target[i:i + 1])
        bnd.update(preds[i:i + 1], target[i:i + 1])
        a, b = float(segm.compute()["map"]), float(bnd.compute()["map"])
        assert b <= a  # min(mask IoU, boundary IoU) never matches more
        n_diff += a != b
    assert n_diff >= 1
    segm, bnd = C.CocoSegmEval(), R.BoundaryCocoEval()
    segm.update(preds, target)
    bnd.update(preds, target)
    rs, rb = segm.compute(), bnd.compute()
    assert 0.0 < float(rb["map"]) < float(rs["map"]) < 1.0
    assert rs["classes"].tolist() == rb["classes"].tolist()
