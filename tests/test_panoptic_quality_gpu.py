"""Panoptic quality and semantic mIoU on the GPU: wm2f_panoptic_match, wm2f_semantic_confusion and the
metric classes against the plain-loop reference (tests/panoptic_quality_reference.py) on random maps of rectangles.
Needs an MI355X (-m gpu).

Agreement: gt_match and pred_state equal; gt_iou bit-equal (one IEEE division of the same integers); per-class tp / fp /
fn and IoU sums equal; PQ / SQ / RQ equal (the reference adds in the documented order); confusion matrices equal."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import panoptic_quality_reference as R

pytestmark = pytest.mark.gpu

THINGS, STUFFS = {1, 2, 4}, {0, 3}
CATS = R.categories_of(THINGS, STUFFS)
SIZES = [(64, 96), (37, 53)]  # the second: odd, no four-pixel path


@pytest.fixture(scope="module")
def wm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from weed_instance_segmentation_amd import _lib, ops
    from weed_instance_segmentation_amd import panoptic_metrics as M
    from weed_instance_segmentation_amd.metrics import MeanIoU, PanopticQuality
    return SimpleNamespace(ops=ops, M=M, PanopticQuality=PanopticQuality, MeanIoU=MeanIoU, Wm2fError=_lib.Wm2fError)


def _rects(rng, h, w, n, max_side):
    out = []
    for _ in range(n):
        rh, rw = int(rng.integers(2, max_side + 1)), int(rng.integers(2, max_side + 1))
        y, x = int(rng.integers(0, max(1, h - rh))), int(rng.integers(0, max(1, w - rw)))
        out.append((y, x, rh, rw))
    return out


def _scene(rng, h, w, n_gt, gt_dtype, n_extra_pred, empty_pred=False):
    """A GT raw-id map of rectangles (later ones paint over earlier ones), its id -> class mapping, and a prediction in the
    panoptic post-processor's form that repeats most GT rectangles -- shifted by up to 2 pixels, usually with the right
    class -- and adds spurious ones, many of them on the unlisted 255."""
    gt = np.full((h, w), 255, gt_dtype)
    if gt_dtype == np.uint8:
        raw = rng.choice(np.arange(0, 255), size=n_gt, replace=False)
    else:
        raw = rng.choice(np.concatenate([np.arange(0, 255), np.arange(256, 1200)]), size=n_gt, replace=False)
    classes = [0, 1, 2, 3, 4, 9]  # 9: outside things | stuffs, void
    mapping, rects = {}, _rects(rng, h, w, n_gt, max(6, h // 4))
    for rid, (y, x, rh, rw) in zip(raw.tolist(), rects):
        gt[y:y + rh, x:x + rw] = rid
        mapping[rid] = int(rng.choice(classes, p=[0.15, 0.25, 0.2, 0.15, 0.2, 0.05]))
    mapping[int(raw.max()) + 1 if int(raw.max()) + 1 != 255 else 1201] = 1  # a listed id without a pixel
    if empty_pred:
        return torch.full((h, w), -1.0), [], gt, mapping
    pred = np.zeros((h, w), np.int32)
    info, next_id = [], 1
    for rid, (y, x, rh, rw) in zip(raw.tolist(), rects):
        if rng.random() < 0.25 or mapping[rid] == 9:
            continue
        dy, dx = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        label = mapping[rid] if rng.random() < 0.8 else int(rng.choice(sorted(THINGS | STUFFS)))
        pred[y + dy:y + dy + rh, x + dx:x + dx + rw] = next_id
        info.append({"id": next_id, "label_id": label, "was_fused": label in STUFFS, "score": 0.9})
        if rng.random() < 0.15:
            info.append(dict(info[-1]))  # a fused pair lists its id twice
        next_id += 1
    for (y, x, rh, rw) in _rects(rng, h, w, n_extra_pred, 8):
        pred[y:y + rh, x:x + rw] = next_id
        info.append({"id": next_id, "label_id": int(rng.choice(sorted(THINGS | STUFFS))), "was_fused": False, "score": 0.5})
        next_id += 1
    present = set(np.unique(pred).tolist())
    return torch.from_numpy(pred), [s for s in info if s["id"] in present], gt, mapping


@pytest.fixture(scope="module")
def batches():
    """Per size B = 3 images: ~40 and a few prediction segments and the float map of -1; GT as int32 with raw ids above
    255 (up to ~70 of them) and as uint8."""
    rng = np.random.default_rng(22)
    out = {}
    for (h, w) in SIZES:
        out[(h, w)] = [_scene(rng, h, w, 70, np.int32, 6), _scene(rng, h, w, 9, np.uint8, 2),
                       _scene(rng, h, w, 12, np.int32, 0, empty_pred=True)]
    return out


@pytest.fixture(scope="module")
def expected(batches):
    """The reference, computed once: per (size, void_as_background) the per-image results, sums and totals."""
    out = {}
    for size, scenes in batches.items():
        for vab in (False, True):
            out[(size, vab)] = R.panoptic_quality_from_maps([s[0].numpy() for s in scenes], [s[1] for s in scenes],
                                                            [s[2] for s in scenes], [s[3] for s in scenes], THINGS, STUFFS, vab)
    return out


# ---------------------------------------------------------------------------------------------- panoptic quality
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("vab", [False, True])
def test_panoptic_quality_matches_reference(wm, batches, expected, size, vab):
    scenes = batches[size]
    results, sums, total = expected[(size, vab)]
    assert sum(len(r["matches"]) for r in results) >= 5 and sum(len(r["false_pos"]) for r in results) >= 3
    if not vab:
        assert sum(len(r["dropped"]) for r in results) >= 1  # the void rule is exercised
    assert len(scenes[0][1]) >= 30
    merged = lambda keys: any(isinstance(k, tuple) for k in keys)  # a stuff class, several components in one segment
    assert merged(k for r in results for k in list(r["matches"]) + r["false_neg"])
    assert merged(k for r in results for k in [v[0] for v in r["matches"].values()] + r["false_pos"] + r["dropped"])
    metric = wm.PanopticQuality(THINGS, STUFFS, return_sq_and_rq=True, return_per_class=True, void_as_background=vab)
    args = ([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes], [s[3] for s in scenes])
    metric.update_from_maps(*args)
    counts = metric.compute_counts()
    print("tp", counts["true_positives"].tolist(), "fp", counts["false_positives"].tolist(), "fn",
          counts["false_negatives"].tolist(), "want", total[:, 1:].T.tolist())
    assert counts["true_positives"].tolist() == total[:, 1].tolist()
    assert counts["false_positives"].tolist() == total[:, 2].tolist()
    assert counts["false_negatives"].tolist() == total[:, 3].tolist()
    assert np.array_equal(counts["iou_sum"].numpy(), total[:, 0])  # bit-equal: same divisions, same order of additions
    per, mean = R.quality(total)
    assert np.array_equal(metric.compute().numpy(), per.T)
    metric.return_per_class = False
    assert np.array_equal(metric.compute().numpy(), mean)
    assert metric.compute_per_image().tolist() == [R.quality(s)[1][0] for s in sums]
    # the records themselves, image by image
    gt_match, gt_iou, gt_label, pred_state, pred_label = (t.cpu().numpy() for t in metric._records[0])
    for i, (scene, res) in enumerate(zip(scenes, results)):
        assert int((gt_match[i] >= 0).sum()) == len(res["matches"])
        assert int((gt_match[i] == -1).sum()) == len(res["false_neg"])
        assert sorted(gt_iou[i][gt_match[i] >= 0].tolist()) == sorted(v[1] for v in res["matches"].values())
        assert int((pred_state[i] == 1).sum()) == len(res["false_pos"])
        assert int((pred_state[i] == 2).sum()) == len(res["dropped"])
        assert int((pred_state[i] == 0).sum()) == len(res["matches"])
    # a second metric, the images one call each: the same bits
    again = wm.PanopticQuality(THINGS, STUFFS, return_sq_and_rq=True, void_as_background=vab)
    for i in range(len(scenes)):
        again.update_from_maps(*([a[i]] for a in args))
    assert np.array_equal(again.compute().numpy(), mean)


def test_panoptic_update_torchmetrics_format(wm, batches, expected):
    """(B, H, W, 2) (category, instance) tensors built from the same scenes give the same sums."""
    size = SIZES[1]
    scenes = batches[size][:2]
    preds, target = [], []
    for seg, info, gt, mapping in scenes:
        lab = {s["id"]: s["label_id"] for s in info}
        p = np.zeros(size + (2,), np.int64)
        p[..., 0] = 77  # unpainted: an unknown category, void
        for sid, l in lab.items():
            p[seg.numpy() == sid] = (l, sid)
        t = np.zeros(size + (2,), np.int64)
        t[..., 0] = 55
        for rid, c in mapping.items():
            if rid != 255:
                t[gt == rid] = (c, rid + 5)
        preds.append(p)
        target.append(t)
    metric = wm.PanopticQuality(THINGS, STUFFS, allow_unknown_preds_category=True)
    metric.update(torch.from_numpy(np.stack(preds)), torch.from_numpy(np.stack(target)))
    total = expected[(size, False)][1][0] + expected[(size, False)][1][1]
    counts = metric.compute_counts()
    assert counts["true_positives"].tolist() == total[:, 1].tolist()
    assert counts["false_positives"].tolist() == total[:, 2].tolist()
    assert counts["false_negatives"].tolist() == total[:, 3].tolist()
    np.testing.assert_allclose(counts["iou_sum"].numpy(), total[:, 0], rtol=1e-15)  # segments are numbered differently
    with pytest.raises(ValueError):
        wm.PanopticQuality(THINGS, STUFFS).update(torch.from_numpy(np.stack(preds)), torch.from_numpy(np.stack(target)))


def _match_reference(pred, gt, gt_ids, plab, glab, vab):
    """The kernel's contract on one image: prediction value v is row v, raw id gt_ids[c] column c; keys are the numbers.
    Void is column 0 alone, so a column that does not exist stands here as a segment of a class nobody predicts, and is
    taken out of the false negatives afterwards."""
    ABSENT = -2 ** 31
    pred_seg = {v: v for v in range(len(plab)) if plab[v] != ABSENT}
    gt_seg = {int(gt_ids[c]): c for c in range(len(gt_ids))}
    res = R.match_image(pred, pred_seg, {v: int(plab[v]) for v in pred_seg}, gt, gt_seg,
                        {c: int(glab[c]) for c in gt_seg.values()}, vab)
    P, G = len(plab), len(glab)
    gt_match, gt_iou, state = np.full(G, -2, np.int32), np.zeros(G), np.full(P, 3, np.uint8)
    for c, (p, iou) in res["matches"].items():
        gt_match[c], gt_iou[c], state[p] = p, iou, 0
    gt_match[[c for c in res["false_neg"] if glab[c] != ABSENT]] = -1
    state[res["false_pos"]] = 1
    state[res["dropped"]] = 2
    return gt_match, gt_iou, state


@pytest.mark.parametrize("case", ["few", "P1024"])
@pytest.mark.parametrize("vab", [False, True])
def test_panoptic_match_kernel(wm, case, vab):
    """ops.panoptic_match on the raw histogram (no merging): rows 0 .. P-1 are the map values, with absent labels, rows
    beyond n_pred, an image without predictions, and P at its cap."""
    rng = np.random.default_rng(5 if case == "few" else 6)
    h, w = 64, 96
    B = 3 if case == "few" else 2
    P = 41 if case == "few" else 1024
    ABSENT = -2 ** 31
    preds, gts, ids, plabs, glabs, n_preds, n_gts = [], [], [], [], [], [], []
    for i in range(B):
        if case == "few":
            seg, info, gt, mapping = _scene(rng, h, w, 30, np.int32, 5)
            pred = seg.numpy().astype(np.int32) - 1  # values 0 .. n-1, -1 unpainted
            n_pred = 0 if i == 2 else int(pred.max()) + 1
        else:  # 2 x 3 cells, one value each.  GT: the same cells (IoU 1), then 4 x 3 cells shifted by one column, where
            # the inner cells meet a prediction on 4 of its 6 pixels and the shifted 2 x 3 halves would be at IoU 1/2
            yy, xx = np.mgrid[0:h, 0:w]
            pred = ((yy // 2) * (w // 3) + xx // 3).astype(np.int32)  # 32 * 32 = 1024 values
            gt = ((yy // (2 if i == 0 else 4)) * 40 + np.minimum(xx + i, w - 1) // 3 + 256).astype(np.int32)
            mapping = {int(v): 0 for v in np.unique(gt)}
            n_pred = P - 3 * i
        gids = sorted(mapping)
        plab = rng.integers(0, 3, P).astype(np.int32)
        glab = rng.integers(0, 3, len(gids)).astype(np.int32)
        if case == "P1024":
            plab[:] = 0
            glab[:] = 0
        plab[rng.integers(0, P, 3)] = ABSENT
        glab[rng.integers(0, len(gids), 2)] = ABSENT
        plab[n_pred:] = ABSENT  # the reference has no n_pred: such rows do not exist
        preds.append(pred)
        gts.append(gt)
        ids.append(gids)
        plabs.append(plab)
        glabs.append(glab)
        n_preds.append(n_pred)
        n_gts.append(len(gids) - (1 if case == "few" and i == 1 else 0))  # hides the listed id without a pixel
    G = max(len(g) for g in ids)
    ids_t = torch.zeros(B, G, dtype=torch.int32)
    glab_t = torch.full((B, G), 1, dtype=torch.int32)  # padding carries a live label: n_gt must hide it
    for i in range(B):
        ids_t[i, :len(ids[i])] = torch.tensor(ids[i], dtype=torch.int32)
        glab_t[i, :len(ids[i])] = torch.from_numpy(glabs[i])
    plab_t = torch.from_numpy(np.stack(plabs))
    plab_dev = plab_t.clone()
    for i in range(B):
        plab_dev[i, n_preds[i]:] = 1  # likewise for rows beyond n_pred
    n_ids = torch.tensor([len(g) for g in ids], dtype=torch.int32).cuda()
    hist = wm.ops.labelmap_pair_counts(torch.from_numpy(np.stack(preds)).cuda(), torch.from_numpy(np.stack(gts)).cuda(),
                                       ids_t.cuda(), n_ids, P)
    out = wm.ops.panoptic_match(hist, plab_dev.cuda(), glab_t.cuda(), torch.tensor(n_preds, dtype=torch.int32).cuda(),
                                torch.tensor(n_gts, dtype=torch.int32).cuda(), vab)
    gt_match, gt_iou, state = (t.cpu().numpy() for t in out)
    assert gt_match.dtype == np.int32 and gt_iou.dtype == np.float64 and state.dtype == np.uint8
    matched = 0
    for i in range(B):
        n = len(ids[i])
        want = _match_reference(preds[i], gts[i], ids[i], plabs[i], glabs[i], vab)
        assert np.array_equal(gt_match[i, :n], want[0]) and np.array_equal(state[i], want[2])
        assert np.array_equal(gt_iou[i, :n], want[1])  # bit-equal
        assert (gt_match[i, n_gts[i]:] == -2).all() and (gt_iou[i, n_gts[i]:] == 0).all()
        matched += int((want[0] >= 0).sum())
    assert matched >= (5 if case == "few" else 500)
    again = wm.ops.panoptic_match(hist, plab_dev.cuda(), glab_t.cuda(), torch.tensor(n_preds, dtype=torch.int32).cuda(),
                                  torch.tensor(n_gts, dtype=torch.int32).cuda(), vab)
    assert all(torch.equal(a, b) for a, b in zip(out, again))  # two runs, the same bits


# ------------------------------------------------------------------------------------------------------ mean IoU
def _class_maps(rng, B, h, w, C, out_of_range=0):
    gt = np.zeros((B, h, w), np.int32)
    for b in range(B):
        for (y, x, rh, rw) in _rects(rng, h, w, 12, max(8, h // 2)):
            gt[b, y:y + rh, x:x + rw] = int(rng.integers(0, C))
    pred = gt.copy()
    flip = rng.random(gt.shape) < 0.2
    pred[flip] = rng.integers(0, C, int(flip.sum()))
    ignore = rng.random(gt.shape) < 0.1
    gt[ignore] = 255
    if out_of_range:
        idx = np.argwhere(~ignore)[:out_of_range]
        pred[tuple(idx.T)] = C + 3
    return pred, gt


def _misaligned(t):
    """The same values at an address one element past an aligned one."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % (4 * t.element_size()) != 0 and out.is_contiguous()
    return out


@pytest.mark.parametrize("C", [3, 19, 133])  # 133: above the LDS budget, the global-atomic path
@pytest.mark.parametrize("pred_dtype", [torch.int64, torch.int32, torch.uint8])
def test_confusion_class_maps(wm, C, pred_dtype):
    rng = np.random.default_rng(C)
    metric = wm.MeanIoU(C, ignore_index=255, per_class=True)
    want = np.zeros((C, C), np.int64)
    for k, (h, w) in enumerate(SIZES + [(64, 96)]):
        pred, gt = _class_maps(rng, 3, h, w, C)
        p = torch.from_numpy(pred).to(pred_dtype).cuda()
        g = torch.from_numpy(gt).cuda() if k == 0 else torch.from_numpy(gt.astype(np.uint8)).cuda()
        if k == 2:  # lists of maps, each misaligned: the pixel-by-pixel path on a size that allows four at a time
            metric.update([_misaligned(m) for m in p], [_misaligned(m) for m in g])
        else:
            metric.update(p, g)
        c, out = R.confusion(pred, gt, C, ignore_index=255)
        assert out == 0
        want += c
    got = metric.confusion_matrix().numpy()
    assert np.array_equal(got, want)
    res = metric.compute()
    miou, iou, acc = R.mean_iou(want)
    assert res["iou_per_class"].tolist() == iou.tolist() and float(res["pixel_accuracy"]) == acc
    assert abs(float(res["miou"]) - miou) <= 1e-15 * C  # the mean of up to C numbers in [0, 1], added in two orders


@pytest.mark.parametrize("C", [3, 19, 133])
def test_confusion_raw_ids_and_split_updates(wm, batches, C):
    """The raw-id GT form, with and without a background label; two update calls equal one on the concatenation; two runs
    give the same bits."""
    rng = np.random.default_rng(100 + C)
    for size in SIZES:
        scenes = batches[size]
        gts = [s[2] for s in scenes]
        mappings = [{k: int(rng.integers(0, C + 1)) for k in s[3]} for s in scenes]  # class C: out of range, ignored
        preds = [rng.integers(0, C, size).astype(np.int64) for _ in scenes]
        for bg in (None, C - 1):
            want = np.zeros((C, C), np.int64)
            for p, g, m in zip(preds, gts, mappings):
                want += R.confusion(p, g, C, mapping=m, background_label=bg)[0]
            one, two, rerun = (wm.MeanIoU(C, background_label=bg) for _ in range(3))
            tp = [torch.from_numpy(p).cuda() for p in preds]
            one.update_from_maps(tp, gts, mappings)
            two.update_from_maps(tp[:1], gts[:1], mappings[:1])
            two.update_from_maps(tp[1:], gts[1:], mappings[1:])
            rerun.update_from_maps(tp, gts, mappings)
            assert np.array_equal(one.confusion_matrix().numpy(), want)
            assert torch.equal(one.confusion_matrix(), two.confusion_matrix())
            assert torch.equal(one.confusion_matrix(), rerun.confusion_matrix())
            assert float(one.compute()["miou"]) == float(two.compute()["miou"])
    # (B, n) stacks in one launch, split in two along B
    pred, gt = _class_maps(rng, 4, 64, 96, C)
    whole, halves = wm.MeanIoU(C, ignore_index=255), wm.MeanIoU(C, ignore_index=255)
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    whole.update(p, g)
    halves.update(p[:1], g[:1])
    halves.update(p[1:], g[1:])
    assert torch.equal(whole.confusion_matrix(), halves.confusion_matrix())
    assert np.array_equal(whole.confusion_matrix().numpy(), R.confusion(pred, gt, C, ignore_index=255)[0])


@pytest.mark.parametrize("C", [19, 133])
def test_out_of_range_prediction_raises_at_compute(wm, C):
    rng = np.random.default_rng(3)
    pred, gt = _class_maps(rng, 2, 37, 53, C, out_of_range=5)
    want, out = R.confusion(pred, gt, C, ignore_index=255)
    assert out == 5
    metric = wm.MeanIoU(C, ignore_index=255)
    metric.update(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())  # no error here: update does not synchronise
    assert np.array_equal(metric.confusion_matrix().numpy(), want)
    with pytest.raises(ValueError, match="5 counted pixels"):
        metric.compute()
    metric.reset()
    assert float(metric.compute()["miou"]) == 0.0


# ------------------------------------------------------------------------------------------------------ end to end
def _tiled_blob_logits(B, Q, C, h, w, seed):
    """Mask logits that tile the image (a 16 x 16 grid of cells, each owned by one random query) and class logits in which
    about a fifth of the queries name a class strongly -- the small inputs of the post-processing tests."""
    g = torch.Generator().manual_seed(seed)
    owner = torch.randint(0, Q, (B, 1, 16, 16), generator=g)
    low = torch.where(owner == torch.arange(Q).view(1, Q, 1, 1), 6.0, -6.0) + torch.randn(B, Q, 16, 16, generator=g)
    m = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)
    m += 0.2 * torch.randn(B, Q, h, w, generator=g)
    cls = torch.randn(B, Q, C + 1, generator=g)
    strong = torch.rand(B, Q, generator=g) < 0.2
    lab = torch.randint(0, C, (B, Q), generator=g)
    cls.scatter_(2, lab.unsqueeze(-1), torch.where(strong, 6.0 + torch.rand(B, Q, generator=g), torch.zeros(B, Q)).unsqueeze(-1))
    cls[..., C] += torch.where(strong, torch.zeros(B, Q), torch.full((B, Q), 4.0))
    return cls.cuda(), m.cuda()


def test_end_to_end_from_post_processing(wm):
    """post_process_panoptic_segmentation and post_process_semantic_segmentation feed both metrics; the reference scores
    host copies of the same maps.  The GT is the panoptic prediction moved two pixels to the right, its segments renamed
    to raw ids, one of them relabelled."""
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    proc = Mask2FormerInstancePostProcessor()
    cls, m = _tiled_blob_logits(2, 100, 3, 64, 64, seed=7)
    out = SimpleNamespace(class_queries_logits=cls, masks_queries_logits=m)
    ts = [(97, 131), (64, 80)]
    pan = proc.post_process_panoptic_segmentation(out, label_ids_to_fuse=set(), target_sizes=ts)
    sem = proc.post_process_semantic_segmentation(out, target_sizes=ts)
    things, stuffs = {0, 1}, {2}
    gts, mappings = [], []
    for r in pan:
        seg = r["segmentation"].cpu().numpy()
        gt = np.full(seg.shape, 255, np.int32)
        gt[:, 2:] = np.where(seg[:, :-2] > 0, seg[:, :-2] * 3 + 250, 255)
        mapping = {s["id"] * 3 + 250: s["label_id"] for s in r["segments_info"]}
        first = sorted(mapping)[0]
        mapping[first] = (mapping[first] + 1) % 3
        gts.append(gt)
        mappings.append(mapping)
    assert sum(len(r["segments_info"]) for r in pan) >= 6
    pq = wm.PanopticQuality(things, stuffs, return_sq_and_rq=True, void_as_background=True)
    pq.update_from_maps([r["segmentation"] for r in pan], [r["segments_info"] for r in pan], gts, mappings)
    _, _, total = R.panoptic_quality_from_maps([r["segmentation"].cpu().numpy() for r in pan], [r["segments_info"] for r in pan],
                                               gts, mappings, things, stuffs, void_as_background=True)
    counts = pq.compute_counts()
    assert counts["true_positives"].sum() >= 3
    assert np.array_equal(np.stack([counts[k].numpy().astype(np.float64) for k in
                                    ("iou_sum", "true_positives", "false_positives", "false_negatives")], 1), total)
    assert np.array_equal(pq.compute().numpy(), R.quality(total)[1])
    miou = wm.MeanIoU(3, background_label=2, per_class=True)
    miou.update_from_maps(sem, gts, mappings)
    want = sum(R.confusion(s.cpu().numpy(), g, 3, mapping=mp, background_label=2)[0] for s, g, mp in zip(sem, gts, mappings))
    assert np.array_equal(miou.confusion_matrix().numpy(), want)
    assert miou.compute()["iou_per_class"].tolist() == R.mean_iou(want)[1].tolist()


# ------------------------------------------------------------------------------------------------ argument checks
def test_caps_are_refused(wm):
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    with pytest.raises(wm.Wm2fError, match="code -2"):
        wm.ops.panoptic_match(i32(1, 1026, 2), i32(1, 1025), i32(1, 1), i32(1), i32(1))
    with pytest.raises(wm.Wm2fError, match="code -2"):
        wm.ops.panoptic_match(i32(1, 2, 4098), i32(1, 1), i32(1, 4097), i32(1), i32(1))
    conf = torch.zeros(1025, 1025, dtype=torch.int64, device="cuda")
    n_out = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(wm.Wm2fError, match="code -2"):
        wm.ops.semantic_confusion_(conf, n_out, torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda"),
                                   torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(wm.Wm2fError, match="code -2"):
        wm.ops.semantic_confusion_(conf[:3, :3].contiguous(), n_out, torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda"),
                                   torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"), gt_ids=i32(1, 4097),
                                   gt_cls=i32(1, 4097), n_ids=i32(1))
    assert int(conf.sum()) == 0 and int(n_out) == 0  # refused before any launch
    with pytest.raises(TypeError):
        wm.ops.semantic_confusion_(conf[:3, :3].contiguous(), n_out, torch.zeros(1, 8, 8, device="cuda"),
                                   torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"))
