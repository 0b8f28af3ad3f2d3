"""Plain restatement of torchmetrics `MeanAveragePrecision(iou_type="segm")` with its default arguments, i.e.
pycocotools COCOeval evaluate() / accumulate() / summarize() on binary masks (DESIGN section 11 is the contract).

Loops as written, nothing vectorised: this is the checker of weed_instance_segmentation_amd/metrics.py, not a product.
Neither torchmetrics nor pycocotools exists where this project runs, so the module is pinned by hand-derived cases
(tests/test_metrics_cpu.py).  `test_with_metrics` restates the reference's models/metrics.py flow on this package's
oracle forward and post-processor.
"""
from __future__ import annotations

import numpy as np
import torch

from . import m2f_oracle as O

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]  # all, small, medium, large
AREA_LBL = ["all", "small", "medium", "large"]


def mask_iou(dt_masks, gt_masks):
    """(D, G) float64: integer pixel counts, inter / union, 0 where the masks do not intersect.  The counts come from
    bit-packed rows (exact, and fast enough for full-size images)."""
    dp = [np.packbits(np.asarray(m, bool).reshape(-1)) for m in dt_masks]
    gp = [np.packbits(np.asarray(m, bool).reshape(-1)) for m in gt_masks]
    da = [int(np.bitwise_count(x).sum()) for x in dp]
    ga = [int(np.bitwise_count(x).sum()) for x in gp]
    ious = np.zeros((len(dp), len(gp)))
    for d in range(len(dp)):
        for g in range(len(gp)):
            inter = int(np.bitwise_count(dp[d] & gp[g]).sum())
            if inter == 0:
                continue
            union = da[d] + ga[g] - inter
            ious[d, g] = float(inter) / float(union)
    return ious


def evaluate_img(dt, gt, area_rng, max_det, iou_thrs=IOU_THRS):
    """COCOeval.evaluateImg for one (image, category, area range).  dt: list of (score, area, iou row over gt);
    gt: list of areas.  None when the image has neither."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    gt_ig = [1 if (a < area_rng[0] or a > area_rng[1]) else 0 for a in gt]
    gtind = sorted(range(len(gt)), key=lambda g: gt_ig[g])  # stable: non-ignored first
    gt_ig = [gt_ig[g] for g in gtind]
    dtind = sorted(range(len(dt)), key=lambda d: -dt[d][0])  # stable: descending score
    dts = [dt[d] for d in dtind[:max_det]]
    T, G, D = len(iou_thrs), len(gt), len(dts)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    dt_ig = np.zeros((T, D))
    for ti, t in enumerate(iou_thrs):
        for di, (score, area, row) in enumerate(dts):
            best = min(t, 1 - 1e-10)
            m = -1
            for gi in range(G):
                if gtm[ti, gi] > 0:
                    continue
                if m > -1 and gt_ig[m] == 0 and gt_ig[gi] == 1:
                    break
                iou = row[gtind[gi]]
                if iou < best:
                    continue
                best = iou
                m = gi
            if m == -1:
                continue
            dt_ig[ti, di] = gt_ig[m]
            dtm[ti, di] = 1
            gtm[ti, m] = 1
    for di, (score, area, row) in enumerate(dts):
        out = area < area_rng[0] or area > area_rng[1]
        for ti in range(T):
            if dtm[ti, di] == 0 and out:
                dt_ig[ti, di] = 1
    return {"dtScores": [s for s, _, _ in dts], "dtMatches": dtm, "dtIgnore": dt_ig, "gtIgnore": np.array(gt_ig)}


class CocoSegmEval:
    """Images are added as binary masks; `compute()` returns torchmetrics' result dictionary."""

    def __init__(self, max_detection_thresholds=None, class_metrics=False):
        self.max_dets = list(max_detection_thresholds) if max_detection_thresholds is not None else [1, 10, 100]
        self.class_metrics = class_metrics
        self.images = []  # (dt_masks, dt_scores, dt_labels, gt_masks, gt_labels) as numpy

    def update(self, preds, target):
        for p, t in zip(preds, target):
            if "iscrowd" in t and np.any(np.asarray(t["iscrowd"]) != 0):
                raise ValueError("crowd annotations are not supported")
            self.images.append((np.asarray(p["masks"]).astype(bool), np.asarray(p["scores"], dtype=np.float32),
                                np.asarray(p["labels"]).astype(np.int64), np.asarray(t["masks"]).astype(bool),
                                np.asarray(t["labels"]).astype(np.int64)))

    def classes(self):
        labs = set()
        for _, _, dl, _, gl in self.images:
            labs.update(int(x) for x in dl)
            labs.update(int(x) for x in gl)
        return sorted(labs)

    def evaluate(self, cat_ids):
        """evalImgs[k][a][i] for categories k, area ranges a, images i."""
        out = []
        for c in cat_ids:
            per_img = []  # COCOeval.computeIoU: once per (image, category)
            for dm, ds, dl, gm, gl in self.images:
                dsel = [d for d in range(len(dl)) if dl[d] == c]
                gsel = [g for g in range(len(gl)) if gl[g] == c]
                # computeIoU's own truncation: the maxDets[-1] best by score (stable), before evaluateImg's
                dsel = [dsel[i] for i in sorted(range(len(dsel)), key=lambda i: -float(ds[dsel[i]]))][:self.max_dets[-1]]
                ious = mask_iou([dm[d] for d in dsel], [gm[g] for g in gsel])
                dt = [(float(ds[d]), int(dm[d].sum()), ious[i]) for i, d in enumerate(dsel)]
                per_img.append((dt, [int(gm[g].sum()) for g in gsel]))
            out.append([[evaluate_img(dt, gt, rng, self.max_dets[-1]) for dt, gt in per_img] for rng in AREA_RNG])
        return out

    def accumulate(self, eval_imgs):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(eval_imgs), len(AREA_RNG), len(self.max_dets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        for k in range(K):
            for a in range(A):
                E = [e for e in eval_imgs[k][a] if e is not None]
                if len(E) == 0:
                    continue
                for m, max_det in enumerate(self.max_dets):
                    dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                    inds = np.argsort(-dt_scores, kind="mergesort")
                    dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gt_ig == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp, fp = np.array(tp), np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = pr.tolist()
                        q = [0.0] * R
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        ids = np.searchsorted(rc, REC_THRS, side="left")
                        for ri, pi in enumerate(ids):
                            if pi >= nd:
                                break
                            q[ri] = pr[pi]
                        precision[t, :, k, a, m] = np.array(q)
        return precision, recall

    def summarize(self, precision, recall):
        def s(ap, iou_thr=None, area="all", max_det=None):
            a = AREA_LBL.index(area)
            m = self.max_dets.index(max_det if max_det is not None else self.max_dets[-1])
            if ap:
                x = precision
                if iou_thr is not None:
                    x = x[np.where(iou_thr == IOU_THRS)[0]]
                x = x[:, :, :, a, m]
            else:
                x = recall[:, :, a, m]
            return -1.0 if len(x[x > -1]) == 0 else float(np.mean(x[x > -1]))

        last = self.max_dets[-1]
        out = {"map": s(1), "map_50": s(1, 0.5), "map_75": s(1, 0.75), "map_small": s(1, area="small"),
               "map_medium": s(1, area="medium"), "map_large": s(1, area="large")}
        for md in self.max_dets:
            out[f"mar_{md}"] = s(0, max_det=md)
        out.update({"mar_small": s(0, area="small"), "mar_medium": s(0, area="medium"), "mar_large": s(0, area="large")})
        return out

    def compute(self):
        cats = self.classes()
        stats = self.summarize(*self.accumulate(self.evaluate(cats)))
        res = {k: torch.tensor(v, dtype=torch.float32) for k, v in stats.items()}
        last = self.max_dets[-1]
        if self.class_metrics and cats:
            per = [self.summarize(*self.accumulate(self.evaluate([c]))) for c in cats]
            res["map_per_class"] = torch.tensor([p["map"] for p in per], dtype=torch.float32)
            res[f"mar_{last}_per_class"] = torch.tensor([p[f"mar_{last}"] for p in per], dtype=torch.float32)
        else:
            res["map_per_class"] = torch.tensor(-1.0)
            res[f"mar_{last}_per_class"] = torch.tensor(-1.0)
        res["classes"] = torch.tensor(cats, dtype=torch.int32)
        return res


def targets_from_maps(original_maps, id_mappings):
    """models/metrics.py:27-52: one binary mask per raw id present in the map and accepted by the mapping, 255 excepted."""
    targets = []
    for gt_map, mapping in zip(original_maps, id_mappings):
        masks, labels = [], []
        for uid in np.unique(gt_map):
            if uid == 255 or uid not in mapping:
                continue
            masks.append(torch.from_numpy(gt_map == uid).bool())
            labels.append(mapping[uid])
        if masks:
            targets.append({"masks": torch.stack(masks), "labels": torch.tensor(labels)})
        else:
            targets.append({"masks": torch.zeros((0, *gt_map.shape), dtype=torch.bool),
                            "labels": torch.tensor(data=[], dtype=torch.long)})
    return targets


def preds_from_postprocess(predictions):
    """models/metrics.py:65-90: masks `segmentation == id` per segment, scores / labels from segments_info."""
    out = []
    for pred in predictions:
        info = pred["segments_info"]
        if not info:
            out.append({"masks": torch.empty(0, *pred["segmentation"].shape, dtype=torch.bool),
                        "scores": torch.empty(0), "labels": torch.empty(0, dtype=torch.long)})
            continue
        seg = pred["segmentation"].cpu()
        out.append({"masks": torch.stack([seg == s["id"] for s in info]),
                    "scores": torch.tensor([s["score"] for s in info]),
                    "labels": torch.tensor([s["label_id"] for s in info])})
    return out


def test_with_metrics(sd, cfg, data_loader):
    """The reference's flow on the oracle forward (no auxiliary loss inputs) and the oracle post-processor."""
    metric = CocoSegmEval()
    for batch in data_loader:
        targets = targets_from_maps(batch["original_maps"], batch["id_mappings"])
        with torch.no_grad():
            out = O.forward(sd, cfg, batch["pixel_values"])
        preds = O.post_process_instance_segmentation(out["class_queries_logits"], out["masks_queries_logits"], 0.5,
                                                     batch["target_sizes"])
        metric.update(preds_from_postprocess(preds), targets)
    return metric.compute()


test_with_metrics.__test__ = False  # a flow, not a pytest test
