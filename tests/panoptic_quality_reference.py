"""The contract of panoptic quality and semantic mIoU (include/wm2f.h) restated in plain loops over
pixels and dictionaries of colour pairs -- the shape of panopticapi's pq_compute_single_core, which torchmetrics'
PanopticQuality follows.  No kernel, no histogram, no torch.  The hand cases of tests/test_panoptic_quality_cpu.py pin it.

A "segment key" is whatever names a segment: the tests of the kernels use the row / column number, the tests of the
classes use ("stuff", class) for a merged stuff class and the id otherwise.
"""
import numpy as np

IGNORE_ID = 255  # raw GT id the data sets never list


def _value(v):
    """A map value as an integer, None when it is none (negative, fractional)."""
    f = float(v)
    if f < 0 or f != int(f):
        return None
    return int(f)


def colour_pairs(pred_map, pred_seg, gt_map, gt_seg):
    """pred_seg: map value -> segment key (a value without an entry is no prediction); gt_seg: raw id -> segment key (a
    raw id without an entry is void).  Returns pred_area {pk: n}, gt_area {gk: n}, inter {(pk, gk): n}, void {pk: n}."""
    pred_map, gt_map = np.asarray(pred_map), np.asarray(gt_map)
    assert pred_map.shape == gt_map.shape
    pred_area, gt_area, inter, void = {}, {}, {}, {}
    for y in range(pred_map.shape[0]):
        for x in range(pred_map.shape[1]):
            pk = pred_seg.get(_value(pred_map[y, x]))
            gk = gt_seg.get(int(gt_map[y, x]))
            if pk is not None:
                pred_area[pk] = pred_area.get(pk, 0) + 1
            if gk is not None:
                gt_area[gk] = gt_area.get(gk, 0) + 1
            if pk is not None and gk is not None:
                inter[(pk, gk)] = inter.get((pk, gk), 0) + 1
            if pk is not None and gk is None:
                void[pk] = void.get(pk, 0) + 1
    return pred_area, gt_area, inter, void


def match_image(pred_map, pred_seg, pred_label, gt_map, gt_seg, gt_label, void_as_background=False):
    """pred_label / gt_label: segment key -> class.  Returns {"matches": {gk: (pk, iou)}, "false_pos": [pk],
    "dropped": [pk], "false_neg": [gk]}.  A segment without a pixel does not exist."""
    pred_area, gt_area, inter, void = colour_pairs(pred_map, pred_seg, gt_map, gt_seg)
    matches, matched_pred = {}, set()
    for (pk, gk), n in inter.items():
        if pred_label[pk] != gt_label[gk]:
            continue
        v = 0 if void_as_background else void.get(pk, 0)
        union = pred_area[pk] - v + gt_area[gk] - n
        if 2 * n > union:  # IoU > 1/2 in integers
            assert gk not in matches and pk not in matched_pred
            matches[gk] = (pk, n / union)
            matched_pred.add(pk)
    false_pos, dropped = [], []
    for pk, area in pred_area.items():
        if pk in matched_pred:
            continue
        v = 0 if void_as_background else void.get(pk, 0)
        (dropped if 2 * v > area else false_pos).append(pk)
    false_neg = [gk for gk in gt_area if gk not in matches]
    return {"matches": matches, "false_pos": false_pos, "dropped": dropped, "false_neg": false_neg}


def image_sums(result, pred_label, gt_label, categories, gt_order):
    """(K, 4) float64 [iou_sum, tp, fp, fn] of one image; the IoUs are added in `gt_order` (a list of GT segment keys)."""
    index = {c: k for k, c in enumerate(categories)}
    s = np.zeros((len(categories), 4), np.float64)
    for gk in gt_order:
        if gk in result["matches"]:
            s[index[gt_label[gk]], 0] += result["matches"][gk][1]
            s[index[gt_label[gk]], 1] += 1
    for gk in result["false_neg"]:
        s[index[gt_label[gk]], 3] += 1
    for pk in result["false_pos"]:
        s[index[pred_label[pk]], 2] += 1
    return s


def quality(s):
    """(K, 4) sums -> (pq, sq, rq) per class and (pq, sq, rq) averaged over the classes with tp + fp / 2 + fn / 2 > 0."""
    pq, sq, rq, used = [], [], [], []
    for iou, tp, fp, fn in s:
        den = tp + 0.5 * fp + 0.5 * fn
        sq.append(iou / tp if tp > 0 else 0.0)
        rq.append(tp / den if den > 0 else 0.0)
        pq.append(sq[-1] * rq[-1])
        used.append(den > 0)
    mean = []
    for values in (pq, sq, rq):  # added one by one in class order
        picked = [v for v, u in zip(values, used) if u]
        mean.append(sum(picked) / len(picked) if picked else 0.0)
    return np.array([pq, sq, rq], np.float64), np.array(mean, np.float64)


def categories_of(things, stuffs):
    return sorted(things) + sorted(stuffs)


def tables_from_maps(segments_info, id_mapping, things, stuffs, allow_unknown=False):
    """The segment tables of one image on the label-map route: pred_seg (map id -> key), pred_label, gt_seg (raw id -> key),
    gt_label, gt_order (GT keys by their smallest raw id).  Stuff segments share the key ("stuff", class)."""
    pred_seg, pred_label = {}, {}
    seen = {}
    for s in segments_info:
        sid, lab = int(s["id"]), int(s["label_id"])
        if sid in seen and seen[sid] != lab:
            raise ValueError(f"id {sid} carries two labels")
        seen[sid] = lab
        if lab in stuffs:
            key = ("stuff", lab)
        elif lab in things:
            key = sid
        elif allow_unknown:
            continue
        else:
            raise ValueError(f"unknown label {lab}")
        pred_seg[sid] = key
        pred_label[key] = lab
    gt_seg, gt_label, gt_order = {}, {}, []
    for rid in sorted(int(k) for k in id_mapping):
        lab = int(id_mapping[rid] if rid in id_mapping else id_mapping[str(rid)])
        if rid == IGNORE_ID or (lab not in things and lab not in stuffs):
            continue
        key = ("stuff", lab) if lab in stuffs else rid
        gt_seg[rid] = key
        if key not in gt_label:
            gt_label[key] = lab
            gt_order.append(key)
    return pred_seg, pred_label, gt_seg, gt_label, gt_order


def panoptic_quality_from_maps(segmentations, segments_infos, original_maps, id_mappings, things, stuffs,
                               void_as_background=False, allow_unknown=False):
    """Per-image results and sums, and the totals added in image order."""
    cats = categories_of(things, stuffs)
    results, sums = [], []
    for seg, info, gm, mapping in zip(segmentations, segments_infos, original_maps, id_mappings):
        pred_seg, pred_label, gt_seg, gt_label, gt_order = tables_from_maps(info, mapping, things, stuffs, allow_unknown)
        r = match_image(seg, pred_seg, pred_label, gm, gt_seg, gt_label, void_as_background)
        results.append(r)
        sums.append(image_sums(r, pred_label, gt_label, cats, gt_order))
    total = np.zeros((len(cats), 4), np.float64)
    for s in sums:
        total += s
    return results, sums, total


# --------------------------------------------------------------------------------------------- confusion matrix
def confusion(pred, gt, num_classes, ignore_index=None, mapping=None, background_label=None):
    """(C, C) int64 counts, rows GT and columns prediction, and the number of counted pixels whose prediction is outside
    [0, C).  gt holds classes, or with `mapping` (raw id -> class, 255 never listed) raw ids; an unlisted raw id has class
    background_label, or is left out without one.  A GT class equal to ignore_index or outside [0, C) is left out."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape
    conf = np.zeros((num_classes, num_classes), np.int64)
    out = 0
    table = None if mapping is None else {int(k): int(v) for k, v in mapping.items() if int(k) != IGNORE_ID}
    for p, g in zip(pred.reshape(-1).tolist(), gt.reshape(-1).tolist()):
        if table is not None:
            g = table.get(g, background_label)
            if g is None:
                continue
        if g == ignore_index or g < 0 or g >= num_classes:
            continue
        if p < 0 or p >= num_classes:
            out += 1
            continue
        conf[g, p] += 1
    return conf, out


def mean_iou(conf):
    """(mean IoU over classes with a non-zero union, per-class IoU with -1 for the others, pixel accuracy)."""
    C = conf.shape[0]
    ious, seen = [], []
    for c in range(C):
        inter = int(conf[c, c])
        union = int(conf[c, :].sum()) + int(conf[:, c].sum()) - inter
        ious.append(inter / union if union > 0 else -1.0)
        seen.append(union > 0)
    used = [v for v, s in zip(ious, seen) if s]
    total = int(conf.sum())
    return (sum(used) / len(used) if used else 0.0), np.array(ious), (int(np.trace(conf)) / total if total else 0.0)
