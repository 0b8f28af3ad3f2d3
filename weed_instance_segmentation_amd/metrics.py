"""Segmentation mAP on the GPU: the drop-in for the reference's `models/metrics.py`.

    from weed_instance_segmentation_amd.metrics import test_with_metrics, print_metrics_evaluation, prepare_metrics_for_json

`MeanAveragePrecision(iou_type="segm")` returns what torchmetrics' class of that name returns with its default
arguments (pycocotools COCOeval on binary masks).  The pixel work and the greedy matching run in the HIP kernels of
csrc/coco_eval.hip; `update` keeps per-image match records on the device, and `compute()` copies them once and
accumulates on the host in float64 numpy, with the same floats COCOeval.accumulate produces.

Two routes in:
  - `update(preds, target)`: torchmetrics' dictionaries of (N, H, W) mask stacks (bit-packed, AND + popcount);
  - `update_from_maps(...)`: the post-processor's id maps and the dataset's raw GT maps, one joint histogram per
    image -- what `test_with_metrics` uses; no mask stack is ever built.

`iou_type="bbox"` (or both types at once) with `boxes_from_masks=True` evaluates the boxes cut from the same maps -- COCOeval with iouType "bbox" on
the tight box of every prediction and GT mask -- on the label-map route: one launch of
csrc/instance_stats.hip per map stack gives the boxes, their integer intersections and areas go through the same
matching kernel.

`iou_type="boundary"` (alone or next to the others) is Boundary AP (Cheng et al., CVPR 2021) on the
label-map route: the IoU of a pair is the smaller of its mask IoU and the IoU of the two masks' boundary bands, the area
ranges still see mask areas.  The bands of a whole id map come from two launches of csrc/boundary.hip, their
intersections from the same joint histogram, and the matching kernel takes both triples (`ops.coco_match_min`).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from .instances import boundary_dilation, boundary_maps  # noqa: F401  (re-exported: where callers look for metrics)

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)
REC_THRESHOLDS = np.linspace(0.0, 1.0, 101)
AREA_RANGES = np.array([[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]])  # all/small/medium/large
AREA_NAMES = ("all", "small", "medium", "large")
ABSENT = -2 ** 31  # gt_label of a GT column that has no pixel in its map (models/metrics.py never builds one)
IGNORE_ID = 255  # raw GT id the reference skips (datasets/pheno_bench/dataset.py:85)


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.Wm2fError("MeanAveragePrecision runs on a GPU only (no CPU fallback): no device is visible")
    _lib.load()
    return torch.device("cuda", torch.cuda.current_device())


IOU_TYPES = ("segm", "bbox", "boundary")


def box_pair_counts(pred_stats: torch.Tensor, gt_stats: torch.Tensor):
    """Box intersections and areas from `ops.labelmap_instance_stats` rows: pred_stats (B, P, 8), gt_stats (B, G, 8) int64
    -> inter (B, P, G), det_area (B, P), gt_area (B, G) int32.  The boxes have integer corners (xmax / ymax inclusive), so
    the counts are exact and go to the matching as pixel counts do; an empty instance has area 0 and meets nothing."""
    def corners(st):
        return st[..., 1], st[..., 2], st[..., 3] + 1, st[..., 4] + 1  # half-open; empty: x0 = W > x1 = 0

    px0, py0, px1, py1 = (c.unsqueeze(2) for c in corners(pred_stats))
    gx0, gy0, gx1, gy1 = (c.unsqueeze(1) for c in corners(gt_stats))
    iw = (torch.minimum(px1, gx1) - torch.maximum(px0, gx0)).clamp(min=0)
    ih = (torch.minimum(py1, gy1) - torch.maximum(py0, gy0)).clamp(min=0)

    def area(st):
        x0, y0, x1, y1 = corners(st)
        return ((x1 - x0).clamp(min=0) * (y1 - y0).clamp(min=0)).to(torch.int32)

    return (iw * ih).to(torch.int32), area(pred_stats), area(gt_stats)


def merge_results(per_type: dict) -> dict:
    """One type: its result as it is.  Several: every name prefixed `bbox_` / `segm_`, `classes` once, unprefixed."""
    if len(per_type) == 1:
        return next(iter(per_type.values()))
    out = {}
    for kind, res in per_type.items():
        out.update({f"{kind}_{k}": v for k, v in res.items() if k != "classes"})
    out["classes"] = next(iter(per_type.values()))["classes"]
    return out


class _Records:
    """Host view of the device records of every image: flat det / GT arrays with the image they belong to."""

    def __init__(self, det_img, det_score, det_label, det_rank, det_matched, det_ignored, gt_img, gt_label, gt_ignored,
                 n_images):
        self.det_img, self.det_score, self.det_label, self.det_rank = det_img, det_score, det_label, det_rank
        self.det_matched, self.det_ignored = det_matched, det_ignored  # (A, T, nd) bool
        self.gt_img, self.gt_label, self.gt_ignored = gt_img, gt_label, gt_ignored  # gt_ignored (A, ng) bool
        self.n_images = n_images

    def subset(self, image: int) -> "_Records":
        d, g = self.det_img == image, self.gt_img == image
        return _Records(self.det_img[d], self.det_score[d], self.det_label[d], self.det_rank[d], self.det_matched[:, :, d],
                        self.det_ignored[:, :, d], self.gt_img[g], self.gt_label[g], self.gt_ignored[:, g], self.n_images)

    def classes(self) -> list[int]:
        return sorted(set(np.unique(self.det_label).tolist()) | set(np.unique(self.gt_label).tolist()))


def accumulate(rec: _Records, cats, max_dets):
    """COCOeval.accumulate: precision (T, R, K, A, M) and recall (T, K, A, M), -1 where undefined.  Vectorised over
    detections; every float equals the per-detection loops' (oracle/coco_eval.py)."""
    T, R, K, A, M = len(IOU_THRESHOLDS), len(REC_THRESHOLDS), len(cats), len(AREA_RANGES), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, c in enumerate(cats):
        dsel, gsel = rec.det_label == c, rec.gt_label == c
        if not dsel.any() and not gsel.any():
            continue  # no image has GT or detections of this category
        img, score, rank = rec.det_img[dsel], rec.det_score[dsel], rec.det_rank[dsel]
        base = np.lexsort((rank, img))  # concatenation in image order, each image's detections in score order
        for a in range(A):
            npig = int(np.count_nonzero(~rec.gt_ignored[a, gsel]))
            if npig == 0:
                continue
            dtm_a, dtig_a = rec.det_matched[a][:, dsel], rec.det_ignored[a][:, dsel]
            for m, md in enumerate(max_dets):
                keep = base[rank[base] < md]
                inds = keep[np.argsort(-score[keep], kind="mergesort")]
                dtm, dtig = dtm_a[:, inds], dtig_a[:, inds]
                tp = np.cumsum(np.logical_and(dtm, ~dtig), axis=1).astype(float)
                fp = np.cumsum(np.logical_and(~dtm, ~dtig), axis=1).astype(float)
                nd = tp.shape[1]
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                recall[:, k, a, m] = rc[:, -1] if nd else 0
                if nd == 0:
                    precision[:, :, k, a, m] = 0.0
                    continue
                env = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                for t in range(T):
                    ids = np.searchsorted(rc[t], REC_THRESHOLDS, side="left")
                    q = np.zeros(R)
                    inside = ids < nd
                    q[inside] = env[t, ids[inside]]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall, max_dets) -> dict:
    """COCOeval.summarize's twelve numbers, named as torchmetrics names them."""
    def mean(x):
        x = x[x > -1]
        return -1.0 if len(x) == 0 else float(np.mean(x))

    last = len(max_dets) - 1
    ap = lambda t, a: mean((precision if t is None else precision[np.where(IOU_THRESHOLDS == t)[0]])[:, :, :, a, last])
    out = {"map": ap(None, 0), "map_50": ap(0.5, 0), "map_75": ap(0.75, 0), "map_small": ap(None, 1),
           "map_medium": ap(None, 2), "map_large": ap(None, 3)}
    for m, md in enumerate(max_dets):
        out[f"mar_{md}"] = mean(recall[:, :, 0, m])
    out.update({"mar_small": mean(recall[:, :, 1, last]), "mar_medium": mean(recall[:, :, 2, last]),
                "mar_large": mean(recall[:, :, 3, last])})
    return out


class MeanAveragePrecision:
    """torchmetrics.detection.MeanAveragePrecision on the GPU: update / compute / reset.  iou_type "segm", "bbox",
    "boundary" or a tuple / list of them.  torchmetrics' "bbox" scores boxes the caller supplies; those are not
    implemented, so "bbox" alone still raises.  `boxes_from_masks=True` selects what is: the tight box of every
    prediction and GT mask, cut from the id maps of `update_from_maps`.  "boundary" is Boundary AP on the same route:
    a pair's IoU is min(mask IoU, boundary IoU), the bands `dilation_ratio` of the image diagonal wide
    (`boundary_dilation`), the area ranges on mask areas."""

    def __init__(self, iou_type="segm", max_detection_thresholds=None, class_metrics: bool = False,
                 boxes_from_masks: bool = False, dilation_ratio: float = 0.02):
        types = (iou_type,) if isinstance(iou_type, str) else tuple(iou_type) if isinstance(iou_type, (tuple, list)) else None
        if not types or any(t not in IOU_TYPES for t in types) or len(set(types)) != len(types):
            raise ValueError(f"iou_type={iou_type!r}: expected 'segm', 'bbox', 'boundary' or a tuple of them")
        if not (isinstance(dilation_ratio, (int, float)) and 0 < dilation_ratio < 1):
            raise ValueError(f"dilation_ratio={dilation_ratio!r}: expected a fraction of the image diagonal in (0, 1)")
        self.dilation_ratio = float(dilation_ratio)
        if "bbox" in types and not boxes_from_masks:
            raise ValueError(f"iou_type={iou_type!r}: boxes supplied by the caller are not implemented; pass "
                             "boxes_from_masks=True to evaluate the tight boxes of the masks (update_from_maps)")
        self.iou_type = types
        self.boxes_from_masks = bool(boxes_from_masks)
        md = [1, 10, 100] if max_detection_thresholds is None else [int(v) for v in max_detection_thresholds]
        if len(md) != 3 or sorted(md) != md or md[0] < 1:
            raise ValueError(f"max_detection_thresholds must be a sorted list of three positive ints, got {md}")
        self.max_detection_thresholds = md
        self.class_metrics = bool(class_metrics)
        self._thr = self._rng = None
        self.reset()

    def reset(self) -> None:
        self._batches = {t: [] for t in self.iou_type}  # per type the device records, one dict per update call

    # ---------------------------------------------------------------------------------------------- update routes
    def _constants(self, dev):
        if self._thr is None or self._thr.device != dev:
            self._thr = torch.tensor(IOU_THRESHOLDS, dtype=torch.float64).to(dev)
            self._rng = torch.tensor(AREA_RANGES, dtype=torch.float64).to(dev)
        return self._thr, self._rng

    def _match(self, dev, inter, det_area, gt_area, det_score, det_label, gt_label, n_det, n_gt, kind="segm", second=None):
        """All (B, D[, G]) device tensors, padded; launches the matching and stores the records of type `kind`.
        `second`: another (inter, det_area, gt_area) triple -- the pair's IoU is the smaller of the two."""
        order = torch.sort(det_score, dim=1, descending=True, stable=True).indices.to(torch.int32)
        thr, rng = self._constants(dev)
        if second is None:
            rank, matched, ignored, gt_ig = ops.coco_match(inter, det_area, gt_area, det_label, gt_label, order, n_det,
                                                           n_gt, thr, rng, self.max_detection_thresholds[-1])
        else:
            rank, matched, ignored, gt_ig = ops.coco_match_min(inter, det_area, gt_area, *second, det_label, gt_label,
                                                               order, n_det, n_gt, thr, rng,
                                                               self.max_detection_thresholds[-1])
        self._batches[kind].append({"n_det": n_det, "n_gt": n_gt, "score": det_score, "label": det_label, "rank": rank,
                              "matched": matched, "ignored": ignored, "gt_label": gt_label, "gt_ignored": gt_ig})

    def update(self, preds: list[dict], target: list[dict]) -> None:
        """torchmetrics' format: preds [{"masks" (D, H, W) bool, "scores" (D), "labels" (D)}], target [{"masks" (G, H, W),
        "labels" (G)}].  Host tensors are moved to the GPU."""
        if "bbox" in self.iou_type:
            raise ValueError("iou_type 'bbox' evaluates the boxes of id maps: use update_from_maps (free-standing boxes "
                             "and mask stacks are not implemented for it)")
        if "boundary" in self.iou_type:
            raise ValueError("iou_type 'boundary' takes its bands from id maps: use update_from_maps (mask stacks, which "
                             "may overlap, would need one erosion per mask and are not implemented for it)")
        if len(preds) != len(target):
            raise ValueError("preds and target must have the same length")
        dev = _device()
        B = len(preds)
        if B == 0:
            return
        for t in target:
            if "iscrowd" in t and bool(torch.as_tensor(t["iscrowd"]).ne(0).any()):
                raise ValueError("crowd annotations are not supported")
        per = []
        for p, t in zip(preds, target):
            dm, gm = torch.as_tensor(p["masks"]).to(dev), torch.as_tensor(t["masks"]).to(dev)
            if dm.dim() != 3 or gm.dim() != 3:
                raise ValueError("masks must be (N, H, W)")
            if dm.shape[0] and gm.shape[0] and dm.shape[1:] != gm.shape[1:]:
                raise ValueError(f"prediction masks {tuple(dm.shape)} and target masks {tuple(gm.shape)} differ in size")
            dm = dm if dm.dtype in (torch.bool, torch.uint8) else dm.ne(0)
            gm = gm if gm.dtype in (torch.bool, torch.uint8) else gm.ne(0)
            per.append((ops.mask_pair_counts(dm, gm), torch.as_tensor(p["scores"]), torch.as_tensor(p["labels"]),
                        torch.as_tensor(t["labels"])))
        D = max(1, max(x[1].numel() for x in per))
        G = max(1, max(x[3].numel() for x in per))
        inter = torch.zeros(B, D, G, device=dev, dtype=torch.int32)
        det_area = torch.zeros(B, D, device=dev, dtype=torch.int32)
        gt_area = torch.zeros(B, G, device=dev, dtype=torch.int32)
        det_score = torch.full((B, D), float("-inf"), device=dev)
        det_label = torch.zeros(B, D, device=dev, dtype=torch.int32)
        gt_label = torch.zeros(B, G, device=dev, dtype=torch.int32)
        nd_host, ng_host = [], []
        for i, ((it, da, ga), sc, dl, gl) in enumerate(per):
            d, g = int(da.numel()), int(ga.numel())
            if sc.numel() != d or dl.numel() != d or gl.numel() != g:
                raise ValueError(f"image {i}: masks, scores and labels disagree in length")
            nd_host.append(d)
            ng_host.append(g)
            inter[i, :d, :g] = it
            det_area[i, :d] = da
            gt_area[i, :g] = ga
            det_score[i, :d] = sc.to(dev, torch.float32)
            det_label[i, :d] = dl.to(dev, torch.int32)
            gt_label[i, :g] = gl.to(dev, torch.int32)
        n_det = torch.tensor(nd_host, dtype=torch.int32).to(dev)
        n_gt = torch.tensor(ng_host, dtype=torch.int32).to(dev)
        self._match(dev, inter, det_area, gt_area, det_score, det_label, gt_label, n_det, n_gt)

    def update_from_maps(self, segmentations, segments_infos, original_maps, id_mappings) -> None:
        """The label-map route: per image the post-processor's id map (`segmentation`, fp32 with -1 background or int32)
        and `segments_info`, the dataset's raw GT id map and its id -> class mapping.  Equals `update` with the masks
        models/metrics.py:27-90 builds from the same inputs (GT ids absent from the map, and 255, make no GT)."""
        B = len(segmentations)
        if not (len(segments_infos) == len(original_maps) == len(id_mappings) == B):
            raise ValueError("update_from_maps: the four lists must have the same length")
        dev = _device()
        if B == 0:
            return
        preds, gts, scores, labels, gt_ids, gt_cls = [], [], [], [], [], []
        for i in range(B):
            seg = torch.as_tensor(segmentations[i])
            gm = original_maps[i]
            gm = torch.from_numpy(np.ascontiguousarray(gm)) if isinstance(gm, np.ndarray) else torch.as_tensor(gm)
            if tuple(seg.shape) != tuple(gm.shape) or seg.dim() != 2:
                raise ValueError(f"image {i}: prediction map {tuple(seg.shape)} and GT map {tuple(gm.shape)} differ")
            if seg.dtype not in (torch.float32, torch.int32):
                seg = seg.to(torch.float32)
            if gm.dtype not in (torch.uint8, torch.int32):
                gm = gm.to(torch.int32)
            info = segments_infos[i]
            if [s["id"] for s in info] != list(range(len(info))):
                raise ValueError(f"image {i}: segment ids must be 0 .. n-1 in order (the post-processor's numbering)")
            # models/metrics.py:79-80: torch.tensor of the rounded Python floats -> float32
            scores.append(torch.tensor([s["score"] for s in info], dtype=torch.float32))
            labels.append(torch.tensor([int(s["label_id"]) for s in info], dtype=torch.int32))
            ids = sorted(int(k) for k in id_mappings[i] if int(k) != IGNORE_ID)
            gt_ids.append(ids)
            gt_cls.append([int(id_mappings[i][k]) for k in ids])
            preds.append(seg)
            gts.append(gm)
        P = max(1, max(len(x) for x in scores))
        G = max(1, max(len(x) for x in gt_ids))
        ids_t = torch.zeros(B, G, dtype=torch.int32)
        cls_t = torch.zeros(B, G, dtype=torch.int32)
        score_t = torch.full((B, P), float("-inf"))
        label_t = torch.zeros(B, P, dtype=torch.int32)
        for i in range(B):
            ids_t[i, :len(gt_ids[i])] = torch.tensor(gt_ids[i], dtype=torch.int32)
            cls_t[i, :len(gt_cls[i])] = torch.tensor(gt_cls[i], dtype=torch.int32)
            score_t[i, :len(scores[i])] = scores[i]
            label_t[i, :len(labels[i])] = labels[i]
        n_ids = torch.tensor([len(x) for x in gt_ids], dtype=torch.int32).to(dev)
        n_det = torch.tensor([len(x) for x in scores], dtype=torch.int32).to(dev)
        ids_t, cls_t, score_t, label_t = ids_t.to(dev), cls_t.to(dev), score_t.to(dev), label_t.to(dev)
        segm, bbox, boundary = "segm" in self.iou_type, "bbox" in self.iou_type, "boundary" in self.iou_type
        inter = torch.empty(B, P, G, device=dev, dtype=torch.int32)
        det_area = torch.empty(B, P, device=dev, dtype=torch.int32)
        gt_area = torch.empty(B, G, device=dev, dtype=torch.int32)
        binter, bdet_area, bgt_area = (torch.empty_like(t) for t in (inter, det_area, gt_area))
        einter, edet_area, egt_area = (torch.empty_like(t) for t in (inter, det_area, gt_area))  # the boundary bands'
        present = torch.empty(B, G, device=dev, dtype=torch.bool)  # the GT id has a pixel in its map
        groups: dict = {}
        for i in range(B):  # one launch per (size, prediction dtype, GT dtype)
            groups.setdefault((tuple(preds[i].shape), preds[i].dtype, gts[i].dtype), []).append(i)
        for rows in groups.values():
            pm = torch.stack([preds[i].to(dev) for i in rows])
            gm = torch.stack([gts[i].to(dev) for i in rows])  # each host map copied once, stacked on the device
            ridx = torch.tensor(rows, device=dev)
            gids, gn = ids_t[ridx].contiguous(), n_ids[ridx].contiguous()
            if segm or boundary:
                hist = ops.labelmap_pair_counts(pm, gm, gids, gn, P)
                inter[ridx] = hist[:, 1:, 1:]
                det_area[ridx] = hist[:, 1:, :].sum(2, dtype=torch.int32)
                gt_area[ridx] = hist[:, :, 1:].sum(1, dtype=torch.int32)
                present[ridx] = gt_area[ridx] > 0
            if bbox:  # the boxes of the same masks: ids 0 .. P-1 of the prediction map, the listed raw ids of the GT map
                gstats = ops.labelmap_instance_stats(gm, gids, gn)
                binter[ridx], bdet_area[ridx], bgt_area[ridx] = box_pair_counts(ops.labelmap_instance_stats(pm, N=P), gstats)
                present[ridx] = gstats[:, :, 0] > 0
            if boundary:  # the bands of both stacks as id maps of their own, then the same histogram on them
                d = boundary_dilation(pm.shape[1], pm.shape[2], self.dilation_ratio)
                ehist = ops.labelmap_pair_counts(ops.labelmap_boundary(pm, d), ops.labelmap_boundary(gm, d), gids, gn, P)
                einter[ridx] = ehist[:, 1:, 1:]
                edet_area[ridx] = ehist[:, 1:, :].sum(2, dtype=torch.int32)
                egt_area[ridx] = ehist[:, :, 1:].sum(1, dtype=torch.int32)
        cls_t = torch.where(present, cls_t, torch.full_like(cls_t, ABSENT))
        if segm:
            self._match(dev, inter, det_area, gt_area, score_t, label_t, cls_t, n_det, n_ids)
        if bbox:  # COCOeval with iouType "bbox": the area ranges see box areas on both sides
            self._match(dev, binter, bdet_area, bgt_area, score_t, label_t, cls_t, n_det, n_ids, kind="bbox")
        if boundary:  # Boundary AP: min(mask IoU, boundary IoU) per pair, the area ranges on mask areas
            self._match(dev, inter, det_area, gt_area, score_t, label_t, cls_t, n_det, n_ids, kind="boundary",
                        second=(einter, edet_area, egt_area))

    # ------------------------------------------------------------------------------------------------- compute
    def _records(self, kind: str | None = None) -> _Records:
        """The one device-to-host copy of every image's records of one type."""
        batches = self._batches[self.iou_type[0] if kind is None else kind]
        if not batches:
            return _Records(*(np.zeros(0, np.int64),) * 4, np.zeros((4, 10, 0), bool), np.zeros((4, 10, 0), bool),
                            np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((4, 0), bool), 0)
        parts, meta = [], []
        for r in batches:
            for k in ("n_det", "n_gt", "score", "label", "rank", "matched", "ignored", "gt_label", "gt_ignored"):
                t = r[k].contiguous()
                meta.append((k, t.dtype, tuple(t.shape), t.numel() * t.element_size()))
                parts.append(t.view(-1).view(torch.uint8))
        flat = torch.cat(parts).cpu().numpy()
        npdt = {torch.int32: np.int32, torch.float32: np.float32, torch.uint8: np.uint8}
        arrays, off = [], 0
        for k, dt, shape, nbytes in meta:
            arrays.append((k, flat[off:off + nbytes].view(npdt[dt]).reshape(shape)))
            off += nbytes
        cols = {k: [] for k in ("det_img", "score", "label", "rank", "matched", "ignored", "gt_img", "gt_label", "gt_ig")}
        img0 = 0
        for j in range(0, len(arrays), 9):
            r = dict(arrays[j:j + 9])
            for i in range(len(r["n_det"])):
                nd, ng = int(r["n_det"][i]), int(r["n_gt"][i])
                cols["det_img"].append(np.full(nd, img0 + i))
                cols["score"].append(r["score"][i, :nd].astype(np.float64))
                cols["label"].append(r["label"][i, :nd].astype(np.int64))
                cols["rank"].append(r["rank"][i, :nd].astype(np.int64))
                cols["matched"].append(r["matched"][i, :, :, :nd].astype(bool))
                cols["ignored"].append(r["ignored"][i, :, :, :nd].astype(bool))
                present = r["gt_label"][i, :ng] != ABSENT
                cols["gt_img"].append(np.full(int(present.sum()), img0 + i))
                cols["gt_label"].append(r["gt_label"][i, :ng][present].astype(np.int64))
                cols["gt_ig"].append(r["gt_ignored"][i, :, :ng][:, present].astype(bool))
            img0 += len(r["n_det"])
        return _Records(np.concatenate(cols["det_img"]), np.concatenate(cols["score"]), np.concatenate(cols["label"]),
                        np.concatenate(cols["rank"]), np.concatenate(cols["matched"], axis=2),
                        np.concatenate(cols["ignored"], axis=2), np.concatenate(cols["gt_img"]),
                        np.concatenate(cols["gt_label"]), np.concatenate(cols["gt_ig"], axis=1), img0)

    def _compute(self, rec: _Records) -> dict:
        md = self.max_detection_thresholds
        cats = rec.classes()
        precision, recall = accumulate(rec, cats, md)
        res = {k: torch.tensor(v, dtype=torch.float32) for k, v in summarize(precision, recall, md).items()}
        if self.class_metrics and cats:
            per = [summarize(precision[:, :, k:k + 1], recall[:, k:k + 1], md) for k in range(len(cats))]
            res["map_per_class"] = torch.tensor([p["map"] for p in per], dtype=torch.float32)
            res[f"mar_{md[-1]}_per_class"] = torch.tensor([p[f"mar_{md[-1]}"] for p in per], dtype=torch.float32)
        else:
            res["map_per_class"] = torch.tensor(-1.0)
            res[f"mar_{md[-1]}_per_class"] = torch.tensor(-1.0)
        res["classes"] = torch.tensor(cats, dtype=torch.int32)
        return res

    def compute(self) -> dict:
        return merge_results({kind: self._compute(self._records(kind)) for kind in self.iou_type})

    def compute_per_image(self, iou_type: str | None = None) -> torch.Tensor:
        """(N,) float32: entry i is the `map` of a fresh metric updated with image i alone (show_worst_predictions.py's
        ranking), from the stored records -- nothing is matched again.  With two types, `iou_type` names the one to
        rank by."""
        if iou_type is None:
            if len(self.iou_type) > 1:
                raise ValueError(f"compute_per_image: name the iou_type to rank by, one of {self.iou_type}")
            iou_type = self.iou_type[0]
        if iou_type not in self.iou_type:
            raise ValueError(f"compute_per_image: iou_type={iou_type!r} is not evaluated by this metric {self.iou_type}")
        rec = self._records(iou_type)
        out = []
        for i in range(rec.n_images):
            sub = rec.subset(i)
            out.append(summarize(*accumulate(sub, sub.classes(), self.max_detection_thresholds),
                                 self.max_detection_thresholds)["map"])
        return torch.tensor(out, dtype=torch.float32)


# --------------------------------------------------------------------------- drop-ins for models/metrics.py
def test_with_metrics(model, processor, data_loader, device, iou_type="segm", results_json=None, clean=None, split=None) -> dict:
    """models/metrics.py::test_with_metrics with the same arguments and result, through the label-map route.
    `iou_type` (not an argument of the reference) goes to MeanAveragePrecision: "segm", "bbox", "boundary" or a tuple of
    them; the boxes are those of the masks (`boxes_from_masks=True`), as this route has nothing else.
    `results_json` (not an argument of the reference either): a path that receives the evaluated predictions as a COCO
    results file (`rle.save_coco_results`), the images named by the batches' `file_names`, or numbered without them.
    `clean` (not an argument of the reference either): an `instances.CleanOptions` handed to the post-processor, so that
    AP can be read with and without the repair of the id maps; a processor is only given the keyword when it is set.
    `split` (not an argument of the reference either): an `instances.SplitOptions`, passed on in the same way."""
    model.eval()
    types = (iou_type,) if isinstance(iou_type, str) else tuple(iou_type) if isinstance(iou_type, (tuple, list)) else ()
    metric = MeanAveragePrecision(iou_type=iou_type, boxes_from_masks="bbox" in types)
    dumped: list = []
    n_seen = 0
    print("Calculating Metrics...")
    for i, batch in enumerate(data_loader):
        if (i + 1) % 5 == 0:
            print(f"  Processing batch {i + 1}/{len(data_loader)}")
        pixel_values = batch["pixel_values"].to(device)
        with torch.no_grad():
            outputs = model(pixel_values=pixel_values)
        predictions = processor.post_process_instance_segmentation(outputs=outputs, target_sizes=batch["target_sizes"],
                                                                   threshold=0.5, mask_threshold=0.5,
                                                                   **({} if results_json is None else {"return_instance_stats": True}),
                                                                   **({} if clean is None else {"clean": clean}),
                                                                   **({} if split is None else {"split": split}))
        metric.update_from_maps([p["segmentation"] for p in predictions], [p["segments_info"] for p in predictions],
                                batch["original_maps"], batch["id_mappings"])
        if results_json is not None:
            from .rle import coco_results
            names = batch.get("file_names") or list(range(n_seen, n_seen + len(predictions)))
            dumped += coco_results(predictions, names)
            n_seen += len(predictions)
    results = metric.compute()
    if results_json is not None:
        import json
        with open(results_json, "w") as f:
            json.dump(dumped, f)
    model.train()
    return results


test_with_metrics.__test__ = False  # not a pytest test


def print_metrics_evaluation(metrics_evaluation: dict, model_name: str = "Model") -> None:
    """The three headline numbers, printed as models/metrics.py prints them."""
    print(f"\n--- {model_name} Metrics ---")
    if not metrics_evaluation:
        print("No metrics calculated.")
        return

    def scalar(key) -> float:
        v = metrics_evaluation.get(key, torch.tensor(-1))
        return v.item() if v.numel() == 1 else -1

    kinds = [k for k in IOU_TYPES if f"{k}_map" in metrics_evaluation]  # both types: one block each
    for kind in kinds or [None]:
        if kind is not None:
            print(f"  [{kind}]")
        pre = "" if kind is None else f"{kind}_"
        for label, key in (("mAP:           ", "map"), ("mAP (IoU=0.50):", "map_50"), ("mAP (IoU=0.75):", "map_75")):
            print(f"  {label} {100 * scalar(pre + key):.2f} %")


def prepare_metrics_for_json(results: dict) -> dict | None:
    """Tensors to Python numbers (one element) or lists, everything else unchanged."""
    if not results:
        return None
    return {k: ((v.item() if v.numel() == 1 else v.tolist()) if isinstance(v, torch.Tensor) else v)
            for k, v in results.items()}


# panoptic quality and semantic mIoU live in panoptic_metrics.py; this is where callers look for metrics
from .panoptic_metrics import (MeanIoU, PanopticQuality, test_panoptic_with_metrics,  # noqa: E402,F401
                               test_semantic_with_metrics)
