"""Numpy restatements of the boundary bands and Boundary AP, written as the definition reads.

- `boundary_map`: a pixel with id k is interior iff the (2d+1) x (2d+1) square around it lies inside the image and every
  pixel of it has id k; every other pixel with an id is in its instance's band.  One loop over the (2d+1)^2 offsets.
- `boundary_map_separable`: the same through the row test h and a column walk -- the form the kernels take.
- `boundary_iou_matrix`: |P_d & G_d| / |P_d | G_d| of binary masks, 0 where the bands do not meet.
- `BoundaryCocoEval`: oracle.coco_eval.CocoSegmEval with min(mask IoU, boundary IoU) per pair; the area ranges keep
  seeing mask areas, as in the parent class.
"""
import numpy as np

from oracle import coco_eval as C


def boundary_dilation(height, width, dilation_ratio=0.02):
    return max(1, int(round(dilation_ratio * np.sqrt(height ** 2 + width ** 2))))


def id_keys(id_map):
    """(H, W) int64: the id of every pixel, -1 where the value is no id.  Floats: negative, fractional, not finite or
    >= 2^24 is no id and -0.0 is 0; integers: negative is no id."""
    a = np.asarray(id_map)
    if a.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(a) & (a >= 0) & (a < 2.0 ** 24) & (a == np.floor(a))
        return np.where(ok, np.where(ok, a, 0), -1).astype(np.int64)
    a = a.astype(np.int64)
    return np.where(a >= 0, a, -1)


def boundary_map(id_map, d):
    """(H, W) id map -> (H, W) int32: the id in the band, -1 in the interior and where there is no id."""
    key = id_keys(id_map)
    H, W = key.shape
    interior = np.zeros((H, W), bool)
    if 2 * d + 1 <= H and 2 * d + 1 <= W:  # otherwise no square fits into the image
        inner = np.ones((H - 2 * d, W - 2 * d), bool)
        centre = key[d:H - d, d:W - d]
        for dy in range(-d, d + 1):
            for dx in range(-d, d + 1):
                inner &= key[d + dy:H - d + dy, d + dx:W - d + dx] == centre
        interior[d:H - d, d:W - d] = inner
    return np.where((key >= 0) & ~interior, key, -1).astype(np.int32)


def boundary_map_separable(id_map, d):
    """The same result in two passes: h(p) = the 2d+1 pixels of p's row segment are in the image and equal to id(p);
    p is interior iff the 2d+1 pixels q of its column segment are in the image, have id(q) = id(p) and h(q)."""
    key = id_keys(id_map)
    H, W = key.shape
    h = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(d, W - d):
            h[y, x] = bool((key[y, x - d:x + d + 1] == key[y, x]).all())
    out = np.where(key >= 0, key, -1).astype(np.int32)
    for y in range(d, H - d):
        for x in range(W):
            if (key[y - d:y + d + 1, x] == key[y, x]).all() and h[y - d:y + d + 1, x].all():
                out[y, x] = -1
    return out


def mask_band(mask, d):
    """The boundary band of one binary mask."""
    return boundary_map(np.asarray(mask, bool).astype(np.int32), d) == 1


def pair_counts(dt_masks, gt_masks):
    """inter (D, G), dt_area (D), gt_area (G) int64 pixel counts of two lists of binary masks."""
    dp = [np.packbits(np.asarray(m, bool).reshape(-1)) for m in dt_masks]
    gp = [np.packbits(np.asarray(m, bool).reshape(-1)) for m in gt_masks]
    inter = np.zeros((len(dp), len(gp)), np.int64)
    for i, a in enumerate(dp):
        for j, b in enumerate(gp):
            inter[i, j] = int(np.bitwise_count(a & b).sum())
    return (inter, np.array([int(np.bitwise_count(x).sum()) for x in dp], np.int64),
            np.array([int(np.bitwise_count(x).sum()) for x in gp], np.int64))


def iou_from_counts(inter, dt_area, gt_area):
    """(D, G) float64: inter / union, 0 where inter is 0."""
    inter = np.asarray(inter, np.int64)
    union = np.asarray(dt_area, np.int64)[:, None] + np.asarray(gt_area, np.int64)[None, :] - inter
    out = np.zeros(inter.shape)
    nz = inter != 0
    out[nz] = inter[nz].astype(np.float64) / union[nz].astype(np.float64)
    return out


def min_iou(inter, dt_area, gt_area, inter2, dt_area2, gt_area2):
    """The IoU Boundary AP matches on: the smaller of the two quotients, pair by pair."""
    return np.minimum(iou_from_counts(inter, dt_area, gt_area), iou_from_counts(inter2, dt_area2, gt_area2))


def boundary_iou_matrix(dt_masks, gt_masks, d):
    """(D, G) float64 boundary IoU: inter / union of the bands in integers, 0 where they do not intersect."""
    return iou_from_counts(*pair_counts([mask_band(m, d) for m in dt_masks], [mask_band(m, d) for m in gt_masks]))


class BoundaryCocoEval(C.CocoSegmEval):
    """COCOeval with iouType "boundary": unchanged except that a pair's IoU is min(mask IoU, boundary IoU).  `dilation`
    fixes the band width in pixels; otherwise it is dilation_ratio of each image's diagonal."""

    def __init__(self, max_detection_thresholds=None, class_metrics=False, dilation_ratio=0.02, dilation=None):
        super().__init__(max_detection_thresholds, class_metrics)
        self.dilation_ratio, self.dilation = dilation_ratio, dilation

    def _d(self, dm, gm):
        if self.dilation is not None:
            return self.dilation
        H, W = (dm if len(dm) else gm).shape[1:]
        return boundary_dilation(H, W, self.dilation_ratio)

    def evaluate(self, cat_ids):
        out = []
        for c in cat_ids:
            per_img = []
            for dm, ds, dl, gm, gl in self.images:
                dsel = [d for d in range(len(dl)) if dl[d] == c]
                gsel = [g for g in range(len(gl)) if gl[g] == c]
                dsel = [dsel[i] for i in sorted(range(len(dsel)), key=lambda i: -float(ds[dsel[i]]))][:self.max_dets[-1]]
                dts, gts = [dm[d] for d in dsel], [gm[g] for g in gsel]
                w = self._d(dm, gm)
                ious = min_iou(*pair_counts(dts, gts), *pair_counts([mask_band(m, w) for m in dts], [mask_band(m, w) for m in gts]))
                dt = [(float(ds[d]), int(dm[d].sum()), ious[i]) for i, d in enumerate(dsel)]  # mask areas for the ranges
                per_img.append((dt, [int(gm[g].sum()) for g in gsel]))
            out.append([[C.evaluate_img(dt, gt, rng, self.max_dets[-1]) for dt, gt in per_img] for rng in C.AREA_RNG])
        return out


# ---------------------------------------------------------------------------------------------------- AP fixtures
def ap_fixtures():
    """Three 96 x 128 images for the Boundary AP tests (CPU: the reference alone; GPU: the metric against it): prediction
    id maps (fp32, -1 background), segments_info, raw GT maps and id -> class mappings.
    Image 2 is built from tests/golden/labelmap_masks.npz; the other two are drawn here: big squares whose predictions
    keep the body and lose or shift the rim (high mask IoU, low boundary IoU), a ragged comb, a small object, a GT
    without prediction, a 255 region and an accepted id that is never painted."""
    H, W = 96, 128
    segs, infos, maps, mappings = [], [], [], []

    def finish(seg, gt, labels, scores, mapping):
        segs.append(seg)
        infos.append([{"id": i, "label_id": int(l), "was_fused": False, "score": float(s)} for i, (l, s) in enumerate(zip(labels, scores))])
        maps.append(gt)
        mappings.append(mapping)

    # image 0: two squares; prediction 0 is GT 1 shrunk by 1 px all round, prediction 1 is GT 2 moved by 1 px
    gt = np.zeros((H, W), np.int32)
    gt[8:58, 6:56] = 1
    gt[30:90, 64:124] = 2
    gt[:4, :] = 255
    seg = np.full((H, W), -1.0, np.float32)
    seg[9:57, 7:55] = 0
    seg[31:91, 65:125] = 1
    finish(seg, gt, [1, 1], [0.9, 0.8], {1: 1, 2: 1, 3: 2})  # id 3 is accepted and absent
    # image 1: a comb (teeth 3 px wide) predicted as its filled hull, a small exact object, a missed GT, a false positive
    gt = np.zeros((H, W), np.int32)
    gt[10:20, 10:100] = 1
    for x in range(10, 100, 6):
        gt[20:60, x:x + 3] = 1
    gt[70:80, 10:20] = 2
    gt[66:92, 90:120] = 3
    seg = np.full((H, W), -1.0, np.float32)
    seg[10:60, 10:100] = 0
    seg[70:80, 10:20] = 1
    seg[64:72, 40:70] = 2
    finish(seg, gt, [1, 2, 2], [0.95, 0.7, 0.6], {1: 1, 2: 2, 3: 2})
    # image 2: the instance map of tests/golden/labelmap_masks.npz (48 x 64, raw ids up to 300, a 255 region) at twice
    # the size; the prediction is every accepted instance moved by 1 px to the right
    import json
    from conftest import load_golden
    g = load_golden("labelmap_masks.npz")
    gt = np.repeat(np.repeat(g["instance_map"].astype(np.int32), 2, axis=0), 2, axis=1)
    assert gt.shape == (H, W)
    mapping = {int(k): int(v) for k, v in json.loads(str(g["id2sem_json"])).items()}
    ids = [int(v) for v in np.unique(gt) if int(v) in mapping and int(v) != 255]
    seg = np.full((H, W), -1.0, np.float32)
    for k, v in enumerate(ids):
        seg[:, 1:][gt[:, :-1] == v] = k
    finish(seg, gt, [mapping[v] for v in ids], [round(0.9 - 0.05 * k, 6) for k in range(len(ids))], mapping)
    return segs, infos, maps, mappings


def fixtures_as_stacks(segs, infos, maps, mappings):
    """The fixtures in torchmetrics' format (mask stacks), as oracle.coco_eval builds them from the same inputs."""
    import torch
    preds = C.preds_from_postprocess([{"segmentation": torch.from_numpy(s), "segments_info": i} for s, i in zip(segs, infos)])
    return preds, C.targets_from_maps(maps, mappings)
