"""Per-instance statistics and box mAP on the host: the numpy restatement of the kernel's contract on
hand cases, the box mAP semantics -- COCOeval on the boxes cut from the masks -- against the segmentation oracle fed
with filled rectangles, the result naming of the two-type metric, argument errors, and the C ABI declaration."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from instance_stats_reference import bbox_records_cpu, boxes_reference, filled, instance_stats_reference, records_from_counts
from oracle import coco_eval as C

EMPTY = lambda H, W: [0, W, H, -1, -1, 0, 0, 0]


# ------------------------------------------------------------------------------------- the restatement on hand cases
def test_reference_single_pixel():
    m = np.full((5, 7), -1, np.float32)
    m[3, 4] = 0
    s = instance_stats_reference(m, N=2)
    assert s[0].tolist() == [1, 4, 3, 4, 3, 4, 3, 0] and s[1].tolist() == EMPTY(5, 7)
    area, bbox, cen = boxes_reference(s)
    assert area.tolist() == [1, 0] and bbox.tolist() == [[4, 3, 1, 1], [0, 0, 0, 0]]
    assert cen[0].tolist() == [4.0, 3.0] and np.isnan(cen[1]).all()


def test_reference_instance_touching_all_borders():
    m = np.zeros((4, 6), np.int32)  # a frame of id 1 around a hole of id 0
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 1
    s = instance_stats_reference(m, N=2)
    assert s[1].tolist() == [16, 0, 0, 5, 3, 40, 24, 0]  # 24 pixels less the 2 x 4 hole; sums by symmetry 16 * 2.5, 16 * 1.5
    assert s[0].tolist() == [8, 1, 1, 4, 2, 20, 12, 0]
    assert boxes_reference(s)[1].tolist() == [[1, 1, 4, 2], [0, 0, 6, 4]]


def test_reference_absent_and_out_of_range_ids():
    m = np.full((3, 3), -1, np.float32)
    m[0, 0], m[1, 1], m[2, 2] = 0, 2, 7  # id 1 has no pixel; 7 is outside [0, 3); -1 is background
    s = instance_stats_reference(m, N=3)
    assert s.tolist() == [[1, 0, 0, 0, 0, 0, 0, 0], EMPTY(3, 3), [1, 1, 1, 1, 1, 1, 1, 0]]
    assert s[:, 0].sum() == 2


def test_reference_id_list_omits_255():
    m = np.array([[255, 255, 3], [9, 3, 3], [0, 0, 255]], np.uint8)
    s = instance_stats_reference(m, ids=[3, 9], N=4)  # raw 0 and 255 are not listed; rows 2 and 3 are padding
    assert s.tolist() == [[3, 1, 0, 2, 1, 5, 2, 0], [1, 0, 1, 0, 1, 0, 1, 0], EMPTY(3, 3), EMPTY(3, 3)]


# ------------------------------------------------------------------- box mAP: the host half against the oracle on rectangles
def _blob(h, w, y0, y1, x0, x1, cut=True):
    """A mask whose tight box is [y0, y1) x [x0, x1) but which does not fill it (a corner is cut off)."""
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    if cut and y1 - y0 > 2 and x1 - x0 > 2:
        m[y0:y0 + (y1 - y0) // 2, x0 + 1:x0 + (x1 - x0) // 2] = False
        m[y0, x0:x1] = True  # the top row keeps the box tight
    return m


def _image(pm, ps, pl, gm, gl):
    return (pm, np.array(ps, np.float32), np.array(pl, np.int64), gm, np.array(gl, np.int64))


def _cases():
    H = W = 160
    b = lambda *a, **k: _blob(H, W, *a, **k)
    g = b(10, 110, 10, 110)
    out = {"perfect": [_image([b(10, 110, 10, 110, cut=False)], [0.9], [0], [g], [0])]}
    # a 100 x 100 box shifted by 0 .. 40 columns: box IoU (100 - s) / (100 + s) runs from 1 down through every threshold
    out["shifted"] = [_image([b(10, 110, 10 + s, 110 + s)], [0.9 - 0.01 * i], [0], [g], [0])
                      for i, s in enumerate((0, 2, 5, 8, 11, 14, 18, 22, 27, 33, 40))]
    out["missed_gt"] = [_image([b(10, 110, 10, 110)], [0.8], [0], [g, b(120, 150, 120, 150)], [0, 0])]
    out["false_positive"] = [_image([b(10, 110, 10, 110), b(120, 150, 120, 150)], [0.6, 0.9], [0, 0], [g], [0])]
    out["two_classes"] = [_image([b(10, 110, 10, 110), b(112, 150, 5, 60), b(112, 150, 70, 150)], [0.9, 0.8, 0.7], [0, 1, 0],
                                 [g, b(114, 150, 5, 60), b(112, 150, 100, 150)], [0, 1, 1]),
                          _image([b(0, 50, 0, 50)], [0.95], [1], [b(0, 50, 2, 52)], [1])]
    # box areas on each side of 32^2 = 1024 and 96^2 = 9216: 31 x 33 = 1023, 32 x 32, 32 x 33 = 1056; 96 x 96, 96 x 97 = 9312,
    # 95 x 97 = 9215 -- every mask thinner than its box, so the pixel areas would fall in other ranges
    sizes = [(31, 33), (32, 32), (32, 33), (96, 96), (96, 97), (95, 97)]
    out["area_ranges"] = [_image([b(3, 3 + h, 5, 5 + w)], [0.9 - 0.1 * i], [0], [b(2, 2 + h, 5, 5 + w)], [0])
                          for i, (h, w) in enumerate(sizes)]
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_box_map_host_half_equals_oracle_on_rectangles(name):
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    images = CASES[name]
    ev = C.CocoSegmEval(class_metrics=True)
    ev.update([{"masks": np.stack([filled(m) for m in pm]), "scores": ps, "labels": pl} for pm, ps, pl, _, _ in images],
              [{"masks": np.stack([filled(m) for m in gm]), "labels": gl} for _, _, _, gm, gl in images])
    ref = ev.compute()
    got = MeanAveragePrecision("bbox", class_metrics=True, boxes_from_masks=True)._compute(bbox_records_cpu(images))
    assert sorted(got) == sorted(ref) and len(got) == 15  # the twelve numbers, two per-class vectors, classes
    for k in ref:
        assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (name, k, got[k], ref[k])
    if name == "area_ranges":
        assert float(got["map_small"]) > -1 and float(got["map_medium"]) > -1 and float(got["map_large"]) > -1
    if name == "shifted":
        assert 0.0 < float(got["map"]) < float(got["map_50"]) < 1.0


def test_box_iou_is_not_mask_iou():
    """The same images through the pixel masks give other numbers: the rectangle comparison above is about boxes."""
    images = CASES["shifted"]
    ev = C.CocoSegmEval()
    ev.update([{"masks": np.stack(pm), "scores": ps, "labels": pl} for pm, ps, pl, _, _ in images],
              [{"masks": np.stack(gm), "labels": gl} for _, _, _, gm, gl in images])
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    got = MeanAveragePrecision("bbox", boxes_from_masks=True)._compute(bbox_records_cpu(images))
    assert float(ev.compute()["map"]) != float(got["map"])


def test_box_pair_counts_by_hand():
    from weed_instance_segmentation_amd.metrics import box_pair_counts
    # boxes x 2..5, y 1..3 (4 x 3) and x 4..9, y 3..4 (6 x 2): they share x 4..5, y 3 -> 2; an empty instance meets nothing
    p = torch.tensor([[[7, 2, 1, 5, 3, 0, 0, 0], [0, 12, 8, -1, -1, 0, 0, 0]]])
    g = torch.tensor([[[9, 4, 3, 9, 4, 0, 0, 0]]])
    inter, da, ga = box_pair_counts(p, g)
    assert inter.tolist() == [[[2], [0]]] and da.tolist() == [[12, 0]] and ga.tolist() == [[12]]
    assert inter.dtype == da.dtype == ga.dtype == torch.int32


# --------------------------------------------------------------------------------------------- the two-type result
def test_two_types_key_names_and_segm_half():
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision, merge_results
    images = CASES["two_classes"]
    box_rec = bbox_records_cpu(images)
    # the segm records of the same images: pixel counts of the masks themselves
    counted = []
    for pm, ps, pl, gm, gl in images:
        inter = np.array([[int((a & b).sum()) for b in gm] for a in pm]).reshape(len(pm), len(gm))
        counted.append((ps, pl, [int(a.sum()) for a in pm], gl, [int(b.sum()) for b in gm], inter))
    segm_rec = records_from_counts(counted)
    both = MeanAveragePrecision(("bbox", "segm"), class_metrics=True, boxes_from_masks=True)
    assert both.iou_type == ("bbox", "segm")
    plain = MeanAveragePrecision("segm", class_metrics=True)._compute(segm_rec)
    res = merge_results({"bbox": both._compute(box_rec), "segm": both._compute(segm_rec)})
    names = ["map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small",
             "mar_medium", "mar_large", "map_per_class", "mar_100_per_class"]
    assert sorted(res) == sorted([f"{t}_{k}" for t in ("bbox", "segm") for k in names] + ["classes"])
    for k in names:
        assert torch.equal(res[f"segm_{k}"], plain[k]), k
    assert torch.equal(res["classes"], plain["classes"]) and res["classes"].tolist() == [0, 1]
    assert any(not torch.equal(res[f"bbox_{k}"], res[f"segm_{k}"]) for k in names)
    one = merge_results({"segm": plain})
    assert one is plain  # a single type keeps the twelve names as they are
    # an empty two-type metric computes (no GPU needed) to the prefixed names, all undefined
    empty = MeanAveragePrecision(["segm", "bbox"], boxes_from_masks=True).compute()
    assert sorted(empty) == sorted(res) and float(empty["bbox_map"]) == -1.0 and float(empty["segm_mar_100"]) == -1.0


def test_print_blocks_per_type(capsys):
    from weed_instance_segmentation_amd.metrics import print_metrics_evaluation
    r = {f"{t}_{k}": torch.tensor(v) for t, vs in (("segm", (0.5, 0.75, 0.25)), ("bbox", (0.4, 0.6, 0.2)))
         for k, v in zip(("map", "map_50", "map_75"), vs)}
    print_metrics_evaluation(r, "Best Model")
    out = capsys.readouterr().out
    assert out.index("[segm]") < out.index("mAP:            50.00 %") < out.index("[bbox]") < out.index("mAP:            40.00 %")
    assert "mAP (IoU=0.75): 20.00 %" in out


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    for bad in ("keypoints", ("segm", "boxes"), (), ("bbox", "bbox"), None):
        with pytest.raises(ValueError):
            MeanAveragePrecision(iou_type=bad, boxes_from_masks=True)
    for kind in ("bbox", ("segm", "bbox")):  # caller-supplied boxes (torchmetrics' meaning of "bbox") are not implemented
        with pytest.raises(ValueError, match="boxes_from_masks"):
            MeanAveragePrecision(iou_type=kind)
    assert MeanAveragePrecision("bbox", boxes_from_masks=True).iou_type == ("bbox",)
    assert MeanAveragePrecision().iou_type == ("segm",) and MeanAveragePrecision(boxes_from_masks=True).iou_type == ("segm",)
    p = {"masks": torch.zeros(1, 4, 4, dtype=torch.bool), "scores": torch.tensor([0.5]), "labels": torch.tensor([0])}
    t = {"masks": torch.zeros(1, 4, 4, dtype=torch.bool), "labels": torch.tensor([0])}
    for kind in ("bbox", ("segm", "bbox")):
        with pytest.raises(ValueError, match="update_from_maps"):
            MeanAveragePrecision(kind, boxes_from_masks=True).update([p], [t])
    with pytest.raises(ValueError):
        MeanAveragePrecision(("segm", "bbox"), boxes_from_masks=True).compute_per_image()
    with pytest.raises(ValueError):
        MeanAveragePrecision("segm").compute_per_image("bbox")


def test_ops_refuse_host_tensors_and_bad_arguments():
    from weed_instance_segmentation_amd import instance_statistics, ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    with pytest.raises(Wm2fError):
        ops.labelmap_instance_stats(torch.zeros(1, 4, 4), N=3)
    with pytest.raises(TypeError):
        ops.labelmap_instance_stats(np.zeros((1, 4, 4), np.float32), N=3)
    with pytest.raises(ValueError):
        instance_statistics(torch.zeros(4, 4))
    with pytest.raises(ValueError):
        instance_statistics(torch.zeros(4, 4), n=2, ids=[1])
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            instance_statistics(torch.zeros(4, 4), n=2)


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_lib_binds_the_entry_point():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    proto = re.search(r"int wm2f_labelmap_instance_stats\(([^;]*)\);", header)
    assert proto is not None
    args = [a.strip() for a in " ".join(proto.group(1).split()).split(",")]
    assert args == ["const void* map", "int dtype", "const int32_t* ids", "const int32_t* n_ids", "int64_t* stats", "int B",
                    "int H", "int W", "int N", "void* stream"]
    res, argtypes = _lib.SIGNATURES["wm2f_labelmap_instance_stats"]
    assert len(argtypes) == len(args) and "instance_stats.hip" in _build.SOURCES
