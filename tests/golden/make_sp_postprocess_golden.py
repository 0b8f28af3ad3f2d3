#!/usr/bin/env python3
"""Golden outputs of the dependency's own semantic and panoptic post-processing (transformers 5.15.0,
Mask2FormerImageProcessorPil.post_process_semantic_segmentation / post_process_panoptic_segmentation, torch CPU) on
small synthetic logits -> tests/golden/postprocess_semantic_panoptic.npz.

Each case stores its inputs, the maps (int8 / int16) and, in `info_json`, the arguments, the segments_info lists and
the margins of its decisions: the smallest relative top-two gap of the argmax maps and the number of pixels within
1e-5 of a tie, the smallest distance of a kept / dropped score to the threshold, of a score-weighted probability to
mask_threshold, and of a surviving / rejected area ratio to overlap_mask_area_threshold.  The GPU re-evaluates the
bilinear resizes and sigmoids in its own order, so a decision with no margin could flip; the generator fails if a
decision that is not meant to sit on its threshold has less than 1e-4.

Usage:  HF_HUB_OFFLINE=1 TRANSFORMERS_OFFLINE=1 python tests/golden/make_sp_postprocess_golden.py
"""
import json
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

import numpy as np
import torch
import transformers
from transformers.models.mask2former.image_processing_pil_mask2former import Mask2FormerImageProcessorPil

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from test_sp_postprocess_cpu import panoptic_weighted, rel_top2_gap, semantic_scores_at  # noqa: E402

NAME = "postprocess_semantic_panoptic.npz"
SCORE_STRIDE = 8  # 384 x 384 scores are stored subsampled [:, ::8, ::8]; target-size scores [:, ::5, ::5]
MARGIN = 1e-4


def smooth_logits(g, B, Q, h, w, scale=4.0, bias=-1.0):
    low = torch.randn(B, Q, 5, 6, generator=g) * scale + bias
    return torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False) + 0.3 * torch.randn(B, Q, h, w, generator=g)


def stripes(g, Q, h, w, spans, inside=5.0, outside=-7.0):
    """Query k covers columns spans[k] = (x0, x1) (None: empty mask), plus a little noise."""
    m = torch.full((Q, h, w), outside) + 0.2 * torch.randn(Q, h, w, generator=g)
    for k, sp in enumerate(spans):
        if sp is not None:
            m[k, :, sp[0]:sp[1]] = inside + 0.2 * torch.randn(h, sp[1] - sp[0], generator=g)
    return m


def class_logits(g, labels, C, strength):
    """One row per query: `labels[k]` gets logit strength[k] (C = the null class), the others small noise."""
    cls = 0.3 * torch.randn(len(labels), C + 1, generator=g)
    for k, (lab, s) in enumerate(zip(labels, strength)):
        cls[k, lab] = s
    return cls


def semantic_margins(cls, logits, ts):
    gaps = []
    for i in range(cls.shape[0]):
        S = semantic_scores_at(cls[i], logits[i], None if ts is None else ts[i])
        gaps.append(rel_top2_gap(S))
    allg = torch.cat([x.flatten() for x in gaps])
    return {"min_rel_top2_gap": float(allg.min()), "near_tie_pixels": int((allg < 1e-5).sum())}


def panoptic_margins(cls, logits, ts, threshold, mask_threshold, overlap, on_threshold=False):
    scores, labels = torch.softmax(cls, -1).max(-1)
    C = cls.shape[-1] - 1
    real = labels.ne(C)
    d = (scores[real] - threshold).abs()
    info = {"min_score_to_threshold": float(d.min()) if d.numel() else None, "scores_on_threshold": int((d == 0).sum())}
    gaps, vdist, rdist = [], [], []
    for i in range(cls.shape[0]):
        keep = real[i] & (scores[i] > threshold)
        if not keep.any():
            continue
        v = panoptic_weighted(logits[i][keep], scores[i][keep], None if ts is None else ts[i])
        gaps.append(rel_top2_gap(v).flatten() if v.shape[0] > 1 else torch.full((1,), float("inf")))
        vdist.append((v - mask_threshold).abs().flatten())
        arg = v.argmax(0)
        for k in range(v.shape[0]):
            owned, above = int((arg == k).sum()), int((v[k] >= mask_threshold).sum())
            if owned and above:
                rdist.append(abs(float(torch.tensor(owned) / torch.tensor(above)) - overlap))
    if gaps:
        g = torch.cat(gaps)
        info.update(min_rel_top2_gap=float(g.min()), near_tie_pixels=int((g < 1e-5).sum()),
                    min_value_to_mask_threshold=float(torch.cat(vdist).min()), min_ratio_to_overlap=min(rdist) if rdist else None)
    if not on_threshold and info["min_score_to_threshold"] is not None:
        assert info["min_score_to_threshold"] > MARGIN, info
    if gaps:
        assert info["near_tie_pixels"] == 0 and info["min_value_to_mask_threshold"] > 1e-6, info
        assert info["min_ratio_to_overlap"] is None or info["min_ratio_to_overlap"] > MARGIN, info
    return info


def main():
    proc = Mask2FormerImageProcessorPil()
    g = torch.Generator().manual_seed(47)
    arrays, info = {}, {}
    ns = lambda cls, m: __import__("types").SimpleNamespace(class_queries_logits=cls, masks_queries_logits=m)  # noqa: E731

    # ---------------- semantic: C = 3 and C = 1 logits, target sizes none / mixed
    sem = {"c3": (smooth_logits(g, 3, 10, 24, 20), torch.randn(3, 10, 4, generator=g) * 3.0),
           "c1": (smooth_logits(g, 2, 6, 17, 23), torch.randn(2, 6, 2, generator=g) * 3.0)}
    for tag, (m, cls) in sem.items():
        arrays[f"sem_{tag}_mask_logits"], arrays[f"sem_{tag}_class_logits"] = m, cls
    for case, tag, ts in (("sem_none", "c3", None), ("sem_mixed", "c3", [(50, 70), (400, 500), (33, 47)]),
                          ("sem_c1", "c1", [(61, 45), (384, 384)])):
        m, cls = sem[tag]
        res = proc.post_process_semantic_segmentation(ns(cls, m), target_sizes=ts, return_segmentation_scores=True)
        for i, r in enumerate(res):
            arrays[f"{case}_seg_{i}"] = r.segmentation.to(torch.int8)
            step = SCORE_STRIDE if ts is None else 5
            arrays[f"{case}_scores_{i}"] = r.segmentation_scores[:, ::step, ::step].contiguous()
        plain = proc.post_process_semantic_segmentation(ns(cls, m), target_sizes=ts)
        assert all(torch.equal(a, b.segmentation) for a, b in zip(plain, res))
        info[case] = {"inputs": f"sem_{tag}", "target_sizes": ts, "score_stride": SCORE_STRIDE if ts is None else 5,
                      "margins": semantic_margins(cls, m, ts)}

    # ---------------- panoptic, C = 3: image 0 fuses label 0 over queries labelled [0, 1, 0, 2] (duplicate ids),
    # image 1 keeps nothing, image 2 has an occluded query the area test rejects and a null-class query
    Q, h, w, C = 8, 24, 32, 3
    m0 = stripes(g, Q, h, w, [(0, 8), (8, 16), (16, 24), (24, 32), None, (0, 32), None, None])
    c0 = class_logits(g, [0, 1, 0, 2, 3, 1, 2, 0], C, [6.0, 5.5, 5.0, 4.5, 6.0, -2.0, -3.0, -2.5])
    m1 = smooth_logits(g, 1, Q, h, w)[0]
    c1 = class_logits(g, [3] * Q, C, [5.0] * Q)
    m2 = stripes(g, Q, h, w, [(0, 12), (4, 10), (12, 22), (22, 32), (20, 30), None, None, None])
    m2[1] -= 1.0  # query 1 lies inside query 0's stripe with a lower score: it owns almost none of its area
    c2 = class_logits(g, [1, 2, 0, 2, 3, 0, 1, 2], C, [6.0, 4.0, 5.0, 3.5, 6.0, -2.0, -2.0, -2.0])
    pm, pc = torch.stack([m0, m1, m2]), torch.stack([c0, c1, c2])
    # C = 1: two images, one fused label
    m3 = torch.stack([stripes(g, 5, 20, 18, [(0, 9), (9, 18), (3, 7), None, (0, 18)]),
                      stripes(g, 5, 20, 18, [(0, 6), (6, 12), (12, 18), None, None])])
    c3 = torch.stack([class_logits(g, [0, 0, 0, 1, 0], 1, [4.0, 3.0, 2.0, 4.0, -3.0]),
                      class_logits(g, [0, 1, 0, 0, 1], 1, [3.0, 4.0, 2.5, -3.0, 4.0])])
    arrays.update(pan_c3_mask_logits=pm, pan_c3_class_logits=pc, pan_c1_mask_logits=m3, pan_c1_class_logits=c3)
    # a threshold sitting exactly on the score of image 2's query 3 (strict `>` drops it)
    thr_on = float(torch.softmax(c2, -1).max(-1).values[3])
    cases = (("pan_mixed", "c3", [(50, 70), (400, 500), (33, 47)], 0.5, {0}),
             ("pan_none", "c3", None, 0.5, {0}),
             ("pan_nofuse", "c3", [(61, 45), (61, 45), (61, 45)], 0.5, set()),
             ("pan_thr", "c3", [(40, 40), (40, 40), (40, 40)], thr_on, {0}),
             ("pan_c1", "c1", [(45, 37), (20, 18)], 0.5, {0}))
    for case, tag, ts, thr, fuse in cases:
        m, cls = (pm, pc) if tag == "c3" else (m3, c3)
        res = proc.post_process_panoptic_segmentation(ns(cls, m), threshold=thr, mask_threshold=0.5,
                                                      overlap_mask_area_threshold=0.8, label_ids_to_fuse=fuse,
                                                      target_sizes=ts)
        for i, r in enumerate(res):
            seg = r["segmentation"]
            arrays[f"{case}_seg_{i}"] = seg.to(torch.int16)
            arrays[f"{case}_segdtype_{i}"] = np.asarray(str(seg.dtype))
        info[case] = {"inputs": f"pan_{tag}", "target_sizes": ts, "threshold": thr, "mask_threshold": 0.5,
                      "overlap_mask_area_threshold": 0.8, "label_ids_to_fuse": sorted(fuse),
                      "segments_info": [r["segments_info"] for r in res],
                      "margins": panoptic_margins(cls, m, ts, thr, 0.5, 0.8, on_threshold=case == "pan_thr")}
        print(case, [[(s["id"], s["label_id"], s["was_fused"]) for s in r["segments_info"]] for r in res])
    ids0 = [s["id"] for s in info["pan_mixed"]["segments_info"][0]]
    assert ids0 == [1, 2, 1, 2], ids0  # the dependency's duplicate ids
    assert info["pan_mixed"]["segments_info"][1] == [] and info["pan_thr"]["margins"]["scores_on_threshold"] >= 1

    out = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    out["info_json"] = np.asarray(json.dumps(info, default=lambda o: int(o)))
    out["hf_version"], out["torch_version"] = np.asarray(transformers.__version__), np.asarray(torch.__version__)
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **out)
    print(f"wrote {NAME}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
