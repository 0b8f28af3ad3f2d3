"""Panoptic quality and semantic mIoU on the GPU: what scores the maps of
`post_process_panoptic_segmentation` and `post_process_semantic_segmentation`.

    from weed_instance_segmentation_amd.metrics import PanopticQuality, MeanIoU

`PanopticQuality` follows torchmetrics' class of that name (argument names, return shapes), whose matching is
panopticapi's pq_compute: a prediction and a GT segment of one class match iff their IoU, taken without the prediction's
void pixels, exceeds 1/2.  The joint histogram of a prediction and a GT map comes from `ops.labelmap_pair_counts` (the mAP
route's kernel), rows and columns that form one segment are added up on the device in integers, and
`ops.panoptic_match` (csrc/panoptic_eval.hip) matches all images of a call in one launch.  Per-image records stay on the
device; `compute()` copies them once and sums per class in float64 on the host, in image order, then GT-segment order.

`MeanIoU` keeps a (C, C) int64 confusion matrix on the device, filled by `ops.semantic_confusion_`; `update` never
synchronises, `compute()` makes the one copy.

The segment tables, the refusals and the sums are plain host code and run without a GPU (tests/test_panoptic_quality_cpu.py).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

ABSENT = -2 ** 31  # label of a row or column that does not exist (wm2f_panoptic_match)
IGNORE_ID = 255  # raw GT id the reference never lists (datasets/pheno_bench/dataset.py:85), as on the mAP route
MATCHED, FALSE_POSITIVE, MOSTLY_VOID, NO_SEGMENT = 0, 1, 2, 3  # pred_state
FALSE_NEGATIVE, NO_GT = -1, -2  # gt_match below 0


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.Wm2fError("PanopticQuality and MeanIoU run on a GPU only (no CPU fallback): no device is visible")
    _lib.load()
    return torch.device("cuda", torch.cuda.current_device())


def _categories(things, stuffs) -> tuple[set, set, list]:
    things, stuffs = {int(c) for c in things}, {int(c) for c in stuffs}
    if things & stuffs:
        raise ValueError(f"things and stuffs must be disjoint, both hold {sorted(things & stuffs)}")
    if not things | stuffs:
        raise ValueError("things and stuffs are both empty")
    return things, stuffs, sorted(things) + sorted(stuffs)  # torchmetrics' class order: things, then stuffs


# ------------------------------------------------------------------------------------------- segment tables (host)
def prediction_segments(image: int, segments_info, things: set, stuffs: set, allow_unknown: bool = False):
    """One image's `segments_info` -> (rows, labels).  rows: id painted in the map -> index of the segment it belongs
    to, -1 if the segment is void (a label outside things | stuffs, accepted only with `allow_unknown`).  labels[s]:
    class of segment s.  Segments of a stuff class are one segment per class; repeated entries of one (id, label_id)
    are one segment.  An id that carries two different labels -- the dependency's duplicate-id quirk -- cannot be decoded
    from the map and raises ValueError, as does id < 1 (0 is the unpainted value)."""
    label_of: dict[int, int] = {}
    for s in segments_info:
        sid, lab = int(s["id"]), int(s["label_id"])
        if sid < 1:
            raise ValueError(f"image {image}: segment id {sid} is not a panoptic id (ids start at 1, 0 is unpainted)")
        if label_of.setdefault(sid, lab) != lab:
            raise ValueError(f"image {image}: id {sid} is painted for labels {label_of[sid]} and {lab} (duplicate ids of "
                             "fused and unfused segments); the map cannot be decoded")
    rows: dict[int, int] = {}
    labels: list[int] = []
    stuff_row: dict[int, int] = {}
    for sid, lab in label_of.items():  # order of first appearance
        if lab in stuffs:
            if lab not in stuff_row:
                stuff_row[lab] = len(labels)
                labels.append(lab)
            rows[sid] = stuff_row[lab]
        elif lab in things:
            rows[sid] = len(labels)
            labels.append(lab)
        elif allow_unknown:
            rows[sid] = -1
        else:
            raise ValueError(f"image {image}: prediction label {lab} (id {sid}) is in neither things nor stuffs; pass "
                             "allow_unknown_preds_category=True to count such segments as void")
    return rows, labels


def gt_segments(id_mapping, things: set, stuffs: set):
    """One image's raw id -> class mapping -> (ids, cols, labels).  ids: the listed raw ids, ascending, 255 left out;
    cols[j]: index of the segment ids[j] belongs to, -1 if its class is outside things | stuffs (void); labels[t]: class
    of segment t.  Raw ids of a stuff class are one segment per class.  Segments are numbered by their smallest raw id."""
    pairs = sorted((int(k), int(v)) for k, v in id_mapping.items() if int(k) != IGNORE_ID)
    ids, cols, labels = [], [], []
    stuff_col: dict[int, int] = {}
    for rid, lab in pairs:
        ids.append(rid)
        if lab in stuffs:
            if lab not in stuff_col:
                stuff_col[lab] = len(labels)
                labels.append(lab)
            cols.append(stuff_col[lab])
        elif lab in things:
            cols.append(len(labels))
            labels.append(lab)
        else:
            cols.append(-1)
    return ids, cols, labels


# ------------------------------------------------------------------------------------------------- sums (host)
def accumulate_records(records, categories):
    """records: per update call (gt_match (B, G), gt_iou (B, G), gt_label (B, G), pred_state (B, P), pred_label (B, P)),
    arrays or host tensors.  Returns per image a (K, 4) float64 array [iou_sum, tp, fp, fn] over `categories`; the IoUs
    of an image are added in GT-column order."""
    index = {c: k for k, c in enumerate(categories)}
    out = []
    for rec in records:
        gt_match, gt_iou, gt_label, pred_state, pred_label = (np.asarray(t) for t in rec)
        for i in range(gt_match.shape[0]):
            s = np.zeros((len(categories), 4), np.float64)
            for c in range(gt_match.shape[1]):
                m = int(gt_match[i, c])
                if m == NO_GT:
                    continue
                k = index[int(gt_label[i, c])]
                if m >= 0:
                    s[k, 0] += float(gt_iou[i, c])
                    s[k, 1] += 1
                else:
                    s[k, 3] += 1
            for p in range(pred_state.shape[1]):
                if int(pred_state[i, p]) == FALSE_POSITIVE:
                    s[index[int(pred_label[i, p])], 2] += 1
            out.append(s)
    return out


def quality_from_sums(s: np.ndarray):
    """(K, 4) [iou_sum, tp, fp, fn] -> pq, sq, rq (K) float64 and the mask of classes that count (denominator > 0)."""
    iou, tp, fp, fn = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    den = tp + 0.5 * fp + 0.5 * fn
    sq = np.where(tp > 0, iou / np.where(tp > 0, tp, 1.0), 0.0)
    rq = np.where(den > 0, tp / np.where(den > 0, den, 1.0), 0.0)
    return sq * rq, sq, rq, den > 0


def mean_over(values: np.ndarray, valid: np.ndarray) -> float:
    """Mean of the valid entries, added one by one in class order; 0 without any."""
    picked = values[valid].tolist()
    return sum(picked) / len(picked) if picked else 0.0


def _to_host(tensors) -> list[np.ndarray]:
    """One device-to-host copy of a list of device tensors."""
    npdt = {torch.int32: np.int32, torch.float64: np.float64, torch.uint8: np.uint8, torch.int64: np.int64}
    tensors = [t.contiguous() for t in tensors]
    if not tensors:
        return []
    flat = torch.cat([t.view(-1).view(torch.uint8) for t in tensors]).cpu().numpy()
    out, off = [], 0
    for t in tensors:
        nbytes = t.numel() * t.element_size()
        out.append(flat[off:off + nbytes].view(npdt[t.dtype]).reshape(tuple(t.shape)))
        off += nbytes
    return out


def _as_map(m) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else torch.as_tensor(m)


class PanopticQuality:
    """torchmetrics.detection.PanopticQuality on the GPU: update / update_from_maps / compute / reset.

    things, stuffs: the class ids that count.  Per class sq = iou_sum / tp, rq = tp / (tp + fp / 2 + fn / 2), pq = sq * rq;
    the averages run over the classes whose denominator is positive.  `compute()` returns, as torchmetrics does, float64:
    pq (scalar); with return_sq_and_rq (3,) [pq, sq, rq]; with return_per_class (1, K) pq, or (K, 3) with both -- classes
    in the order sorted(things) + sorted(stuffs) (`categories`).

    A GT pixel that belongs to no listed segment is void: a raw id that is not listed (255 never is), or one whose class
    is outside things | stuffs.  By the rule of panopticapi an unmatched prediction that lies more than half in void is
    dropped, not counted as a false positive, and void pixels leave a prediction's area before the IoU is taken.
    `void_as_background=True` (not an argument of torchmetrics) switches both off: void is then ordinary unlabelled
    ground.  The reference's data sets need it: their maps paint background and ignore alike as 255, so under the default
    a spurious plant on bare soil would be excused as "mostly void"."""

    def __init__(self, things, stuffs, allow_unknown_preds_category: bool = False, return_sq_and_rq: bool = False,
                 return_per_class: bool = False, void_as_background: bool = False):
        self.things, self.stuffs, self.categories = _categories(things, stuffs)
        self.allow_unknown_preds_category = bool(allow_unknown_preds_category)
        self.return_sq_and_rq = bool(return_sq_and_rq)
        self.return_per_class = bool(return_per_class)
        self.void_as_background = bool(void_as_background)
        self.reset()

    def reset(self) -> None:
        self._records = []  # per update call: (gt_match, gt_iou, gt_label, pred_state, pred_label) on the device

    # ---------------------------------------------------------------------------------------------- update routes
    def _update(self, dev, pred_maps, pred_rows, pred_labels, gt_maps, gt_ids, gt_cols, gt_labels) -> None:
        """Per image: a prediction map (fp32 / int32) whose value v in [0, len(pred_rows[i])) belongs to segment
        pred_rows[i][v] (-1: none); a GT map (uint8 / int32) whose raw id gt_ids[i][j] (ascending) belongs to segment
        gt_cols[i][j] (-1: void); the segments' classes."""
        B = len(pred_maps)
        P_raw = max(1, max(len(r) for r in pred_rows))
        G_raw = max(1, max(len(g) for g in gt_ids))
        P = max(1, max(len(x) for x in pred_labels))
        G = max(1, max(len(x) for x in gt_labels))
        row_t = torch.zeros(B, P_raw + 1, dtype=torch.int64)  # histogram row -> merged row; 0 collects "no prediction"
        col_t = torch.zeros(B, G_raw + 1, dtype=torch.int64)
        ids_t = torch.zeros(B, G_raw, dtype=torch.int32)
        plab_t = torch.full((B, P), ABSENT, dtype=torch.int32)
        glab_t = torch.full((B, G), ABSENT, dtype=torch.int32)
        for i in range(B):
            row_t[i, 1:len(pred_rows[i]) + 1] = torch.tensor(pred_rows[i], dtype=torch.int64) + 1
            col_t[i, 1:len(gt_cols[i]) + 1] = torch.tensor(gt_cols[i], dtype=torch.int64) + 1
            ids_t[i, :len(gt_ids[i])] = torch.tensor(gt_ids[i], dtype=torch.int32)
            plab_t[i, :len(pred_labels[i])] = torch.tensor(pred_labels[i], dtype=torch.int32)
            glab_t[i, :len(gt_labels[i])] = torch.tensor(gt_labels[i], dtype=torch.int32)
        n_ids = torch.tensor([len(g) for g in gt_ids], dtype=torch.int32).to(dev)
        n_pred = torch.tensor([len(x) for x in pred_labels], dtype=torch.int32).to(dev)
        n_gt = torch.tensor([len(x) for x in gt_labels], dtype=torch.int32).to(dev)
        row_t, col_t, ids_t, plab_t, glab_t = (t.to(dev) for t in (row_t, col_t, ids_t, plab_t, glab_t))
        hist = torch.empty(B, P_raw + 1, G_raw + 1, device=dev, dtype=torch.int32)
        groups: dict = {}
        for i in range(B):  # one launch per (size, prediction dtype, GT dtype)
            groups.setdefault((tuple(pred_maps[i].shape), pred_maps[i].dtype, gt_maps[i].dtype), []).append(i)
        for rows in groups.values():
            pm = torch.stack([pred_maps[i].to(dev) for i in rows])
            gm = torch.stack([gt_maps[i].to(dev) for i in rows])
            ridx = torch.tensor(rows, device=dev)
            hist[ridx] = ops.labelmap_pair_counts(pm, gm, ids_t[ridx].contiguous(), n_ids[ridx].contiguous(), P_raw)
        # rows, then columns, of one segment added up: integer adds, so the order they happen in does not matter
        by_row = torch.zeros(B, P + 1, G_raw + 1, device=dev, dtype=torch.int32)
        by_row.scatter_add_(1, row_t.unsqueeze(2).expand(B, P_raw + 1, G_raw + 1), hist)
        merged = torch.zeros(B, P + 1, G + 1, device=dev, dtype=torch.int32)
        merged.scatter_add_(2, col_t.unsqueeze(1).expand(B, P + 1, G_raw + 1), by_row)
        gt_match, gt_iou, pred_state = ops.panoptic_match(merged, plab_t, glab_t, n_pred, n_gt, self.void_as_background)
        self._records.append((gt_match, gt_iou, glab_t, pred_state, plab_t))

    def update_from_maps(self, segmentations, segments_infos, original_maps, id_mappings) -> None:
        """Per image what `post_process_panoptic_segmentation` returns -- the int32 id map in which 0 is unpainted (or
        the float32 map of -1 of an image without a kept query, whose every GT segment becomes a false negative) and
        `segments_info` -- with the data set's raw GT id map and its id -> class mapping, as on the mAP route."""
        B = len(segmentations)
        if not (len(segments_infos) == len(original_maps) == len(id_mappings) == B):
            raise ValueError("update_from_maps: the four lists must have the same length")
        pred_maps, pred_rows, pred_labels, gt_maps, gt_ids, gt_cols, gt_labels = [], [], [], [], [], [], []
        for i in range(B):
            seg, gm = torch.as_tensor(segmentations[i]), _as_map(original_maps[i])
            if tuple(seg.shape) != tuple(gm.shape) or seg.dim() != 2:
                raise ValueError(f"image {i}: prediction map {tuple(seg.shape)} and GT map {tuple(gm.shape)} differ")
            rows, labels = prediction_segments(i, segments_infos[i], self.things, self.stuffs, self.allow_unknown_preds_category)
            table = [-1] * (max(rows) + 1 if rows else 0)  # value 0, and any id without an entry, is no prediction
            for sid, r in rows.items():
                table[sid] = r
            ids, cols, glabels = gt_segments(id_mappings[i], self.things, self.stuffs)
            pred_maps.append(seg if seg.dtype in (torch.float32, torch.int32) else seg.to(torch.int32))
            gt_maps.append(gm if gm.dtype in (torch.uint8, torch.int32) else gm.to(torch.int32))
            pred_rows.append(table)
            pred_labels.append(labels)
            gt_ids.append(ids)
            gt_cols.append(cols)
            gt_labels.append(glabels)
        dev = _device()
        if B:
            self._update(dev, pred_maps, pred_rows, pred_labels, gt_maps, gt_ids, gt_cols, gt_labels)

    def _colour_tables(self, image: int, colours, is_pred: bool):
        """(n, 2) distinct (category, instance) pairs of a map -> (segment per pair or -1, segment labels)."""
        segs, labels = [], []
        for cat, _ in colours:
            if cat in self.things or cat in self.stuffs:
                segs.append(len(labels))  # stuff instances were zeroed before: one pair per stuff class
                labels.append(cat)
            elif is_pred and not self.allow_unknown_preds_category:
                raise ValueError(f"image {image}: prediction category {cat} is in neither things nor stuffs; pass "
                                 "allow_unknown_preds_category=True to count such pixels as void")
            else:
                segs.append(-1)
        return segs, labels

    def update(self, preds, target) -> None:
        """torchmetrics' format: (B, H, W, 2) integer tensors of (category, instance) per pixel.  Instance ids of a stuff
        class are disregarded; a target category outside things | stuffs is void."""
        preds, target = torch.as_tensor(preds), torch.as_tensor(target)
        if preds.shape != target.shape or preds.dim() != 4 or preds.shape[-1] != 2:
            raise ValueError(f"update: preds and target must be (B, H, W, 2) of one shape, got {tuple(preds.shape)} and "
                             f"{tuple(target.shape)}")
        dev = _device()
        B = preds.shape[0]
        if B == 0:
            return
        stuffs = torch.tensor(sorted(self.stuffs), dtype=torch.int64, device=dev)
        maps, tables = {}, {}
        for name, x in (("pred", preds), ("gt", target)):
            x = x.to(dev).to(torch.int64).clone()
            x[..., 1].masked_fill_(torch.isin(x[..., 0], stuffs), 0)
            maps[name], tables[name] = [], []
            for i in range(B):
                colours, inverse = torch.unique(x[i].reshape(-1, 2), dim=0, return_inverse=True)
                maps[name].append(inverse.to(torch.int32).view(x.shape[1], x.shape[2]))
                tables[name].append(self._colour_tables(i, colours.tolist(), name == "pred"))
        self._update(dev, maps["pred"], [t[0] for t in tables["pred"]], [t[1] for t in tables["pred"]], maps["gt"],
                     [list(range(len(t[0]))) for t in tables["gt"]], [t[0] for t in tables["gt"]],
                     [t[1] for t in tables["gt"]])

    # ------------------------------------------------------------------------------------------------- compute
    def _per_image_sums(self):
        flat = _to_host([t for rec in self._records for t in rec])
        return accumulate_records([flat[j:j + 5] for j in range(0, len(flat), 5)], self.categories)

    def compute(self) -> torch.Tensor:
        total = np.zeros((len(self.categories), 4), np.float64)
        for s in self._per_image_sums():  # image order
            total += s
        pq, sq, rq, valid = quality_from_sums(total)
        if self.return_per_class:
            if self.return_sq_and_rq:
                return torch.from_numpy(np.stack([pq, sq, rq], axis=-1))
            return torch.from_numpy(pq).view(1, -1)
        avg = [mean_over(v, valid) for v in (pq, sq, rq)]
        if self.return_sq_and_rq:
            return torch.tensor(avg, dtype=torch.float64)
        return torch.tensor(avg[0], dtype=torch.float64)

    def compute_counts(self) -> dict:
        """The sums behind `compute()`: "iou_sum" (K) float64, "true_positives", "false_positives", "false_negatives"
        (K) int64, "classes" (K) -- over all images so far."""
        total = np.zeros((len(self.categories), 4), np.float64)
        for s in self._per_image_sums():
            total += s
        return {"iou_sum": torch.from_numpy(total[:, 0].copy()),
                "true_positives": torch.from_numpy(total[:, 1].astype(np.int64)),
                "false_positives": torch.from_numpy(total[:, 2].astype(np.int64)),
                "false_negatives": torch.from_numpy(total[:, 3].astype(np.int64)),
                "classes": torch.tensor(self.categories, dtype=torch.int64)}

    def compute_per_image(self) -> torch.Tensor:
        """(N,) float64: entry i is the pq of a fresh metric updated with image i alone (for worst-case listings), from
        the stored records -- nothing is matched again."""
        out = []
        for s in self._per_image_sums():
            pq, _, _, valid = quality_from_sums(s)
            out.append(mean_over(pq, valid))
        return torch.tensor(out, dtype=torch.float64)


def iou_from_confusion(conf: np.ndarray):
    """(C, C) counts, rows GT and columns prediction -> (mean IoU over the classes with a non-zero union, per-class IoU
    with -1 for a class without one, pixel accuracy), float64."""
    conf = np.asarray(conf, dtype=np.int64)
    inter = np.diag(conf).astype(np.float64)
    union = (conf.sum(0) + conf.sum(1)).astype(np.float64) - inter
    seen = union > 0
    iou = np.where(seen, inter / np.where(seen, union, 1.0), -1.0)
    total = float(conf.sum())
    return mean_over(iou, seen), iou, (float(inter.sum()) / total if total else 0.0)


class MeanIoU:
    """Mean intersection over union of class maps on the GPU: update / update_from_maps / compute / reset.

    num_classes: C; predictions must lie in [0, C).  A pixel whose GT class equals `ignore_index`, or lies outside [0, C),
    is left out.  On the raw-id route a GT raw id that is not listed in the image's mapping (255 never is) has class
    `background_label`, or is left out without one.  `compute()` returns {"miou": mean IoU over the classes with a
    non-zero union, "iou_per_class": (C,) with -1 for a class that appears nowhere (a scalar -1 unless per_class),
    "pixel_accuracy"} as float64 tensors, and raises ValueError if any counted pixel's prediction was outside [0, C)."""

    def __init__(self, num_classes: int, ignore_index: int | None = None, background_label: int | None = None,
                 per_class: bool = False):
        if int(num_classes) < 1:
            raise ValueError(f"num_classes must be positive, got {num_classes}")
        self.num_classes = int(num_classes)
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.background_label = None if background_label is None else int(background_label)
        if self.background_label is not None and not 0 <= self.background_label < self.num_classes:
            raise ValueError(f"background_label {background_label} is outside [0, {self.num_classes})")
        self.per_class = bool(per_class)
        self._conf = self._out = None

    def reset(self) -> None:
        self._conf = self._out = None

    def _state(self, dev):
        if self._conf is None:
            self._conf = torch.zeros(self.num_classes, self.num_classes, device=dev, dtype=torch.int64)
            self._out = torch.zeros(1, device=dev, dtype=torch.int64)
        return self._conf, self._out

    @staticmethod
    def _maps(x, dev, dtypes, fallback):
        """A (B, ...) tensor -> [it]; a list of maps -> each as a batch of one (no stacking copy)."""
        if isinstance(x, (torch.Tensor, np.ndarray)):
            x = _as_map(x)
            items = [x if x.dim() >= 3 else x.unsqueeze(0)]
        else:
            items = [_as_map(m).unsqueeze(0) for m in x]
        return [(m if m.dtype in dtypes else m.to(fallback)).to(dev) for m in items]

    def update(self, preds, target) -> None:
        """Class maps: (B, H, W) tensors, or lists of (H, W) maps whose sizes may differ (what
        `post_process_semantic_segmentation` returns).  preds int64 / int32 / uint8, target uint8 / int32."""
        dev = _device()
        conf, out = self._state(dev)
        ps = self._maps(preds, dev, (torch.int64, torch.int32, torch.uint8), torch.int64)
        ts = self._maps(target, dev, (torch.uint8, torch.int32), torch.int32)
        if len(ps) != len(ts):
            raise ValueError("update: preds and target must have the same length")
        for p, t in zip(ps, ts):
            ops.semantic_confusion_(conf, out, p, t, ignore_index=self.ignore_index)

    def update_from_maps(self, segmentations, original_maps, id_mappings) -> None:
        """Per image a predicted class map, the data set's raw GT id map and its id -> class mapping."""
        B = len(segmentations)
        if not (len(original_maps) == len(id_mappings) == B):
            raise ValueError("update_from_maps: the three lists must have the same length")
        dev = _device()
        if B == 0:
            return
        conf, out = self._state(dev)
        pairs = [sorted((int(k), int(v)) for k, v in m.items() if int(k) != IGNORE_ID) for m in id_mappings]
        G = max(1, max(len(p) for p in pairs))
        ids_t = torch.zeros(B, G, dtype=torch.int32)
        cls_t = torch.zeros(B, G, dtype=torch.int32)
        for i, p in enumerate(pairs):
            if p:
                ids_t[i, :len(p)] = torch.tensor([k for k, _ in p], dtype=torch.int32)
                cls_t[i, :len(p)] = torch.tensor([v for _, v in p], dtype=torch.int32)
        n_ids = torch.tensor([len(p) for p in pairs], dtype=torch.int32).to(dev)
        ids_t, cls_t = ids_t.to(dev), cls_t.to(dev)
        ps = self._maps(list(segmentations), dev, (torch.int64, torch.int32, torch.uint8), torch.int64)
        ts = self._maps(list(original_maps), dev, (torch.uint8, torch.int32), torch.int32)
        for i, (p, t) in enumerate(zip(ps, ts)):
            ops.semantic_confusion_(conf, out, p, t, ignore_index=self.ignore_index, gt_ids=ids_t[i:i + 1],
                                    gt_cls=cls_t[i:i + 1], n_ids=n_ids[i:i + 1], background_label=self.background_label)

    def confusion_matrix(self) -> torch.Tensor:
        """The (C, C) int64 counts so far, rows GT and columns prediction, on the host."""
        if self._conf is None:
            return torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64)
        return self._conf.cpu()

    def compute(self) -> dict:
        if self._conf is None:
            conf, bad = np.zeros((self.num_classes, self.num_classes), np.int64), 0
        else:
            flat = torch.cat([self._conf.view(-1), self._out]).cpu().numpy()  # the one copy
            conf, bad = flat[:-1].reshape(self.num_classes, self.num_classes), int(flat[-1])
        if bad:
            raise ValueError(f"{bad} counted pixels carry a prediction outside [0, {self.num_classes})")
        miou, iou, acc = iou_from_confusion(conf)
        return {"miou": torch.tensor(miou, dtype=torch.float64),
                "iou_per_class": torch.from_numpy(iou) if self.per_class else torch.tensor(-1.0, dtype=torch.float64),
                "pixel_accuracy": torch.tensor(acc, dtype=torch.float64)}


# ------------------------------------------------------------------------------------------------------ drivers
def test_panoptic_with_metrics(model, processor, data_loader, device, things, stuffs, *, void_as_background: bool = True,
                               **post_process_kwargs) -> dict:
    """Panoptic quality of a model over a data loader of the reference's `collate_fn` batches, as `test_with_metrics`
    does for mAP.  `post_process_kwargs` go to `post_process_panoptic_segmentation` (threshold, label_ids_to_fuse, ...);
    `label_ids_to_fuse` defaults to `stuffs`.  `void_as_background` defaults to True because the reference's maps paint
    background and ignore alike (see PanopticQuality).  Returns {"pq", "sq", "rq"} and their per-class (K) tensors
    with "classes"."""
    model.eval()
    metric = PanopticQuality(things, stuffs, return_sq_and_rq=True, return_per_class=True,
                             void_as_background=void_as_background)
    post_process_kwargs.setdefault("label_ids_to_fuse", set(metric.stuffs))
    print("Calculating Metrics...")
    for i, batch in enumerate(data_loader):
        if (i + 1) % 5 == 0:
            print(f"  Processing batch {i + 1}/{len(data_loader)}")
        pixel_values = batch["pixel_values"].to(device)
        with torch.no_grad():
            outputs = model(pixel_values=pixel_values)
        predictions = processor.post_process_panoptic_segmentation(outputs=outputs, target_sizes=batch["target_sizes"],
                                                                   **post_process_kwargs)
        metric.update_from_maps([p["segmentation"] for p in predictions], [p["segments_info"] for p in predictions],
                                batch["original_maps"], batch["id_mappings"])
    per_class = metric.compute()  # (K, 3)
    metric.return_per_class = False
    mean = metric.compute()
    model.train()
    return {"pq": mean[0], "sq": mean[1], "rq": mean[2], "pq_per_class": per_class[:, 0], "sq_per_class": per_class[:, 1],
            "rq_per_class": per_class[:, 2], "classes": torch.tensor(metric.categories, dtype=torch.int64)}


def test_semantic_with_metrics(model, processor, data_loader, device, num_classes: int, ignore_index: int | None = None,
                               background_label: int | None = None) -> dict:
    """Semantic mIoU of a model over a data loader of the reference's `collate_fn` batches: the maps of
    `post_process_semantic_segmentation` against the raw GT id maps and their id -> class mappings.  Returns MeanIoU's
    result with per-class IoUs."""
    model.eval()
    metric = MeanIoU(num_classes, ignore_index=ignore_index, background_label=background_label, per_class=True)
    print("Calculating Metrics...")
    for i, batch in enumerate(data_loader):
        if (i + 1) % 5 == 0:
            print(f"  Processing batch {i + 1}/{len(data_loader)}")
        pixel_values = batch["pixel_values"].to(device)
        with torch.no_grad():
            outputs = model(pixel_values=pixel_values)
        maps = processor.post_process_semantic_segmentation(outputs=outputs, target_sizes=batch["target_sizes"])
        metric.update_from_maps(maps, batch["original_maps"], batch["id_mappings"])
    results = metric.compute()
    model.train()
    return results


test_panoptic_with_metrics.__test__ = False  # not pytest tests
test_semantic_with_metrics.__test__ = False
