"""Segmentation mAP on the host: the oracle against hand-derived cases, the product's host
accumulate / summarize against the oracle on synthetic match records, and the new ops refusing host tensors."""
import numpy as np
import pytest
import torch

from oracle import coco_eval as C

EPS1 = 1.0 / (1.0 + np.spacing(1))  # tp / (tp + fp + spacing(1)) with tp = 1, fp = 0: the double below 1 - 2^-53


def _stats(preds, target, max_dets=None, class_metrics=False):
    ev = C.CocoSegmEval(max_dets, class_metrics)
    ev.update(preds, target)
    cats = ev.classes()
    return ev.summarize(*ev.accumulate(ev.evaluate(cats))), ev


def _rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    return m


def _p(masks, scores, labels):
    return {"masks": np.stack(masks) if masks else np.zeros((0, 4, 4), bool), "scores": np.array(scores, np.float32),
            "labels": np.array(labels)}


def _t(masks, labels):
    return {"masks": np.stack(masks) if masks else np.zeros((0, 4, 4), bool), "labels": np.array(labels)}


def test_epsilon_of_a_perfect_match():
    assert EPS1 == 1 - 2.0 ** -52 and EPS1 < 1.0  # a perfect score is not 1.0 (as float32 it rounds to 1)


def test_oracle_prediction_equals_gt():
    # one image, one class, a 100 x 100 GT (area 10 000 >= 96^2: large).  Every threshold: tp = 1, fp = 0, so precision
    # 1 / (1 + spacing(1)) at all 101 recall thresholds and recall 1; small / medium have no GT: -1.
    g = _rect(128, 128, 10, 110, 10, 110)
    s, _ = _stats([_p([g], [0.9], [0])], [_t([g], [0])])
    for k in ("map", "map_50", "map_75", "map_large"):
        assert s[k] == np.mean([EPS1] * (1010 if k in ("map", "map_large") else 101)) and 1 - 3e-16 < s[k] < 1.0, k
    for k in ("mar_1", "mar_10", "mar_100", "mar_large"):
        assert s[k] == 1.0, k
    for k in ("map_small", "map_medium", "mar_small", "mar_medium"):
        assert s[k] == -1.0, k


def test_oracle_iou_exactly_one_half():
    # GT rows 0..59, detection rows 20..79 of a 200-wide image: areas 12 000 each, intersection 40 x 200 = 8 000,
    # union 16 000: IoU 0.5 exactly, which matches at t = 0.5 (iou < best is the skip test) and nowhere else.
    # map_50 = 1 / (1 + eps); map = (one threshold at 1 / (1 + eps), nine at 0) / 10; mar_100 = (1 + 9 * 0) / 10.
    g, d = _rect(100, 200, 0, 60, 0, 200), _rect(100, 200, 20, 80, 0, 200)
    s, _ = _stats([_p([d], [0.8], [1])], [_t([g], [1])])
    assert s["map_50"] == np.mean([EPS1] * 101) and s["map_50"] < 1.0 and s["map_75"] == 0.0
    assert s["map"] == pytest.approx(0.1, abs=1e-15) and s["map"] == np.mean([EPS1] * 101 + [0.0] * 909)
    assert s["mar_100"] == pytest.approx(0.1, abs=1e-15)


def test_oracle_three_detections_two_gt():
    # GT1, GT2 disjoint 100 x 100 squares; detections: = GT1 (.9), a square touching neither (.8), = GT2 (.7).
    # Every threshold: tp = [1, 1, 2], fp = [0, 1, 1], rc = [.5, .5, 1], pr = [1/(1+e), .5, 2/3] -> envelope
    # [1/(1+e), 2/3, 2/3].  Recall thresholds 0 .. .50 (51 of them) land on index 0, .51 .. 1 (50) on index 2:
    # map = (51 * 1 + 50 * 2/3) / 101 = 253 / 303 (up to the eps).  mar_1: the top detection only -> .5; mar_10 = 1.
    H, W = 128, 384
    g1, g2, fp = _rect(H, W, 0, 100, 0, 100), _rect(H, W, 0, 100, 120, 220), _rect(H, W, 0, 100, 250, 350)
    s, _ = _stats([_p([g1, fp, g2], [0.9, 0.8, 0.7], [0, 0, 0])], [_t([g1, g2], [0, 0])])
    assert s["map"] == pytest.approx(253 / 303, abs=1e-15)
    assert s["mar_1"] == 0.5 and s["mar_10"] == 1.0 and s["mar_100"] == 1.0


def _ev(dt, gt, rng, max_det=100):
    return C.evaluate_img([(s, a, np.array(r, float)) for s, a, r in dt], gt, rng, max_det)


def test_oracle_equal_iou_later_gt_wins():
    # both GT at IoU .6 with the first detection: the later GT wins, so the second detection (IoU .6 with GT 0 only)
    # still finds GT 0 -> two matches at t <= .6, none above.
    e = _ev([(0.9, 10000, [0.6, 0.6]), (0.8, 10000, [0.6, 0.0])], [10000, 10000], C.AREA_RNG[0])
    t55, t65 = list(C.IOU_THRS).index(0.55), 3
    assert e["dtMatches"][0].tolist() == [1, 1] and e["dtMatches"][t55].tolist() == [1, 1]
    assert e["dtMatches"][t65].tolist() == [0, 0]


def test_oracle_unmatched_out_of_range_detection_is_ignored():
    # small range [0, 1024]: an unmatched detection of area 5 000 is ignored, one of area 500 counts as a false positive;
    # 1 024 itself is inside.
    e = _ev([(0.9, 5000, [0.0]), (0.8, 500, [0.0]), (0.7, 1024, [0.0])], [300], C.AREA_RNG[1])
    assert e["dtIgnore"][:, 0].all() and not e["dtIgnore"][:, 1].any() and not e["dtIgnore"][:, 2].any()


def test_oracle_stops_at_the_ignored_gt_boundary():
    # small range: GT 0 (area 500) counts, GT 1 (area 5 000) is ignored and sorts after it.  At t = .5 the detection
    # takes GT 0 (.55) and stops before GT 1 (.9); at t >= .6 GT 0 fails, the walk reaches GT 1 and the matched detection
    # inherits its ignore flag.
    e = _ev([(0.9, 600, [0.55, 0.9])], [500, 5000], C.AREA_RNG[1])
    assert e["dtMatches"][0, 0] == 1 and e["dtIgnore"][0, 0] == 0
    assert e["dtMatches"][2, 0] == 1 and e["dtIgnore"][2, 0] == 1
    assert e["dtMatches"][9, 0] == 0  # .9 < min(.95, 1 - 1e-10)
    assert e["gtIgnore"].tolist() == [0, 1]


def test_oracle_more_than_100_detections():
    # 100 empty false positives outrank the exact detection of the only GT: with maxDets 100 it is cut (tp = 0:
    # map 0, recall 0); with [1, 10, 150] it is the 101st: recall 1, precision 1/101 from recall .01 on.
    H = W = 100
    g = _rect(H, W, 0, 100, 0, 100)
    fps = [np.zeros((H, W), bool) for _ in range(100)]  # painted-over instances: area 0, IoU 0, false positives in "all"
    preds = [_p(fps + [g], [0.9] * 100 + [0.5], [0] * 101)]
    s, _ = _stats(preds, [_t([g], [0])])
    assert s["map"] == 0.0 and s["mar_100"] == 0.0
    s150, _ = _stats(preds, [_t([g], [0])], max_dets=[1, 10, 150])
    assert s150["mar_150"] == 1.0 and s150["map"] == pytest.approx(1 / 101, rel=1e-12)


def test_oracle_category_without_gt_and_empty_image():
    # class 0 is perfect; class 1 has a detection but no GT anywhere: its cells stay -1 and drop out of the means.
    # An image with neither predictions nor GT changes nothing.
    g = _rect(128, 128, 0, 100, 0, 100)
    d1 = _rect(128, 128, 100, 128, 100, 128)
    empty_p, empty_t = _p([], [], []), _t([], [])
    empty_p["masks"] = np.zeros((0, 128, 128), bool)
    empty_t["masks"] = np.zeros((0, 128, 128), bool)
    s, ev = _stats([_p([g, d1], [0.9, 0.95], [0, 1]), empty_p], [_t([g], [0]), empty_t], class_metrics=True)
    assert s["map"] == np.mean([EPS1] * 1010) and s["mar_100"] == 1.0
    r = ev.compute()
    assert r["classes"].tolist() == [0, 1] and r["map_per_class"].tolist() == [pytest.approx(1.0), -1.0]
    alone = C.CocoSegmEval()
    alone.update([empty_p], [empty_t])
    assert float(alone.compute()["map"]) == -1.0


def test_oracle_refuses_crowd():
    g = _rect(8, 8, 0, 4, 0, 4)
    t = _t([g], [0])
    t["iscrowd"] = np.array([1])
    with pytest.raises(ValueError):
        C.CocoSegmEval().update([_p([g], [0.5], [0])], [t])


# ---------------------------------------------------------------- product host accumulate / summarize vs the oracle
def _synthetic(seed, n_images=5, max_det_last=100):
    """Random per-image detections / GT with ties (scores from a small set, within and across images), IoUs on the
    thresholds, areas on the range edges; returns the oracle's evalImgs and the product's records of the same matches."""
    from weed_instance_segmentation_amd.metrics import _Records
    rng = np.random.default_rng(seed)
    cats = [0, 1, 2]
    ious = np.concatenate([C.IOU_THRS, [0.0, 0.0, 0.0, 0.3, 0.62, 0.81, 1.0]])
    areas = np.array([10, 500, 1024, 1025, 5000, 9216, 9217, 20000])
    imgs = []
    for i in range(n_images):
        nd = int(rng.integers(0, 14)) if i != 2 else 120  # one image past 100 detections of a category
        ng = int(rng.integers(0, 6)) if i != 3 else 0
        dl = rng.integers(0, 2 if i == 2 else 3, nd)
        if i == 2:
            dl[:] = 1
        ds = rng.choice(np.array([0.9, 0.8, 0.8, 0.55, 0.3], np.float32), nd)
        gl = rng.integers(0, 2, ng)  # category 2: detections only
        rows = rng.choice(ious, (nd, ng))
        imgs.append((ds, dl, rng.choice(areas, nd), gl, rng.choice(areas, ng), rows))
    ev = C.CocoSegmEval([1, 10, max_det_last])
    eval_imgs = []
    for c in cats:
        per_a = []
        for rng_a in C.AREA_RNG:
            per_i = []
            for ds, dl, da, gl, ga, rows in imgs:
                di, gi = np.where(dl == c)[0], np.where(gl == c)[0]
                dt = [(float(ds[d]), int(da[d]), rows[d, gi]) for d in di]
                per_i.append(C.evaluate_img(dt, [int(ga[g]) for g in gi], rng_a, max_det_last))
            per_a.append(per_i)
        eval_imgs.append(per_a)
    # the same matches as device records: per detection (original order) its rank and flags
    cols = {k: [] for k in ("img", "score", "label", "rank", "m", "ig", "gimg", "glab", "gig")}
    for i, (ds, dl, da, gl, ga, rows) in enumerate(imgs):
        nd, ng = len(ds), len(gl)
        rank = np.full(nd, -1)
        m = np.zeros((4, 10, nd), bool)
        ig = np.zeros((4, 10, nd), bool)
        gig = np.zeros((4, ng), bool)
        for c in cats:
            di, gi = np.where(dl == c)[0], np.where(gl == c)[0]
            order = sorted(range(len(di)), key=lambda j: -float(ds[di[j]]))
            for r, j in enumerate(order):
                rank[di[j]] = r
            for a, rng_a in enumerate(C.AREA_RNG):
                e = eval_imgs[c][a][i]
                if e is None:
                    continue
                for r, j in enumerate(order[:max_det_last]):
                    m[a, :, di[j]] = e["dtMatches"][:, r] > 0
                    ig[a, :, di[j]] = e["dtIgnore"][:, r] > 0
                gig[a, gi] = [ga[g] < rng_a[0] or ga[g] > rng_a[1] for g in gi]
        for k, v in zip(cols, (np.full(nd, i), ds.astype(np.float64), dl, rank, m, ig, np.full(ng, i), gl, gig)):
            cols[k].append(v)
    cat = lambda k, ax=0: np.concatenate(cols[k], axis=ax)
    rec = _Records(cat("img"), cat("score"), cat("label"), cat("rank"), cat("m", 2), cat("ig", 2), cat("gimg"),
                   cat("glab"), cat("gig", 1), n_images)
    return ev, eval_imgs, rec, cats


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("last", [100, 150])
def test_product_host_accumulate_equals_oracle(seed, last):
    from weed_instance_segmentation_amd import metrics as M
    ev, eval_imgs, rec, cats = _synthetic(seed, max_det_last=last)
    assert rec.classes() == cats
    p0, r0 = ev.accumulate(eval_imgs)
    p1, r1 = M.accumulate(rec, cats, [1, 10, last])
    assert np.array_equal(p0, p1) and np.array_equal(r0, r1)  # bit for bit
    s0, s1 = ev.summarize(p0, r0), M.summarize(p1, r1, [1, 10, last])
    assert s0 == s1 and f"mar_{last}" in s1
    assert any(v not in (-1.0, 0.0) for v in s1.values())


def test_product_per_image_equals_fresh_oracle():
    from weed_instance_segmentation_amd import metrics as M
    ev, eval_imgs, rec, cats = _synthetic(7)
    for i in range(rec.n_images):
        sub = rec.subset(i)
        sub_cats = sub.classes()
        ks = [cats.index(c) for c in sub_cats]
        only = [[[eval_imgs[k][a][i]] for a in range(4)] for k in ks]
        p0, r0 = ev.accumulate(only)
        p1, r1 = M.accumulate(sub, sub_cats, [1, 10, 100])
        assert np.array_equal(p0, p1) and np.array_equal(r0, r1)


def test_metric_arguments():
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    with pytest.raises(ValueError):
        MeanAveragePrecision(iou_type="bbox")
    with pytest.raises(ValueError):
        MeanAveragePrecision(max_detection_thresholds=[10, 1, 100])
    assert MeanAveragePrecision(max_detection_thresholds=[1, 10, 150]).max_detection_thresholds == [1, 10, 150]


def test_print_and_json_helpers(capsys):
    from weed_instance_segmentation_amd.metrics import prepare_metrics_for_json, print_metrics_evaluation
    r = {"map": torch.tensor(0.5), "map_50": torch.tensor(0.75), "map_75": torch.tensor(0.25),
         "classes": torch.tensor([1, 3], dtype=torch.int32)}
    print_metrics_evaluation(r, "Best Model")
    out = capsys.readouterr().out
    assert "--- Best Model Metrics ---" in out and "mAP:            50.00 %" in out and "mAP (IoU=0.75): 25.00 %" in out
    assert prepare_metrics_for_json(r) == {"map": 0.5, "map_50": 0.75, "map_75": 0.25, "classes": [1, 3]}
    assert prepare_metrics_for_json({}) is None


def test_metric_ops_refuse_host_tensors():
    """No CPU form: the ops raise on host tensors, and the metric raises without a GPU."""
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    calls = [
        lambda: ops.labelmap_pair_counts(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8), i32(1, 2), i32(1), 3),
        lambda: ops.mask_pair_counts(torch.zeros(2, 4, 4, dtype=torch.bool), torch.zeros(1, 4, 4, dtype=torch.bool)),
        lambda: ops.coco_match(i32(1, 2, 3), i32(1, 2), i32(1, 3), i32(1, 2), i32(1, 3), i32(1, 2), i32(1), i32(1),
                               torch.zeros(10, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64), 100),
    ]
    for call in calls:
        with pytest.raises(Wm2fError):
            call()
    if torch.cuda.is_available():
        return  # the metric itself moves host tensors to the GPU by design
    from weed_instance_segmentation_amd import MeanAveragePrecision
    m = MeanAveragePrecision()
    p = {"masks": torch.zeros(1, 4, 4, dtype=torch.bool), "scores": torch.tensor([0.5]), "labels": torch.tensor([0])}
    t = {"masks": torch.zeros(1, 4, 4, dtype=torch.bool), "labels": torch.tensor([0])}
    with pytest.raises(Wm2fError):
        m.update([p], [t])
    with pytest.raises(Wm2fError):
        m.update_from_maps([torch.zeros(4, 4)], [[]], [np.zeros((4, 4), np.int32)], [{}])
