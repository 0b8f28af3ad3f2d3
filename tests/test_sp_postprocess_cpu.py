"""Semantic and panoptic post-processing, CPU side: a plain-torch restatement of the dependency's
post_process_semantic_segmentation / post_process_panoptic_segmentation (transformers 5.15.0
image_processing_mask2former.py:550-625, :748-841, compute_segments :167-224), pinned to the dependency's own outputs
in tests/golden/postprocess_semantic_panoptic.npz; the host segment-id assignment on crafted counts; the CPU-input
error.  tests/test_sp_postprocess_gpu.py and tools/sp_postprocess_bench.py import the restatement and run it on GPU
tensors."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

GRID = (384, 384)


# ------------------------------------------------------------------ the restatement (works on any device)
def semantic_scores_at(cls, logits, size=None):
    """One image: (C, H, W) scores the dependency takes the argmax of (cls (Q, C+1), logits (Q, h, w))."""
    probs = F.interpolate(logits.float().unsqueeze(0), size=GRID, mode="bilinear", align_corners=False)[0].sigmoid()
    S = torch.einsum("qc,qhw->chw", cls.float().softmax(-1)[..., :-1], probs)
    if size is not None:
        S = F.interpolate(S.unsqueeze(0), size=tuple(size), mode="bilinear", align_corners=False)[0]
    return S


def semantic_reference(cls, logits, target_sizes=None):
    """post_process_semantic_segmentation(return_segmentation_scores=True) restated: [(map int64, scores (C, H, W))]."""
    masks_classes = cls.float().softmax(dim=-1)[..., :-1]
    probs = F.interpolate(logits.float(), size=GRID, mode="bilinear", align_corners=False).sigmoid()
    S = torch.einsum("bqc, bqhw -> bchw", masks_classes, probs)
    if target_sizes is None:
        return [(S[i].argmax(0), S[i]) for i in range(S.shape[0])]
    out = []
    for i in range(S.shape[0]):
        r = F.interpolate(S[i].unsqueeze(0), size=tuple(target_sizes[i]), mode="bilinear", align_corners=False)[0]
        out.append((r.argmax(0), r))
    return out


def panoptic_weighted(logits_kept, scores_kept, size=None):
    """(K, H, W) score-weighted probabilities of one image's kept queries, as compute_segments forms them."""
    p = F.interpolate(logits_kept.float().unsqueeze(0), size=GRID, mode="bilinear", align_corners=False)[0].sigmoid()
    if size is not None:
        p = F.interpolate(p.unsqueeze(0), size=tuple(size), mode="bilinear", align_corners=False)[0]
    return p * scores_kept.view(-1, 1, 1)


def rel_top2_gap(x):
    """(top1 - top2) / |top1| over dim 0, per pixel (inf with a single channel)."""
    if x.shape[0] < 2:
        return torch.full(x.shape[1:], float("inf"), device=x.device)
    t = x.topk(2, dim=0).values
    return (t[0] - t[1]) / t[0].abs().clamp_min(1e-30)


def panoptic_reference(cls, logits, threshold=0.5, mask_threshold=0.5, overlap_mask_area_threshold=0.8,
                       label_ids_to_fuse=frozenset(), target_sizes=None, with_gaps=False):
    """post_process_panoptic_segmentation restated; with_gaps=True adds per image the relative top-two gap map of the
    score-weighted values (None for an image without kept queries)."""
    probs = F.interpolate(logits.float(), size=GRID, mode="bilinear", align_corners=False).sigmoid()
    num_labels = cls.shape[-1] - 1
    pred_scores, pred_labels = F.softmax(cls.float(), dim=-1).max(-1)
    results, gaps = [], []
    for i in range(cls.shape[0]):
        keep = pred_labels[i].ne(num_labels) & (pred_scores[i] > threshold)
        mp, sc, lb = probs[i][keep], pred_scores[i][keep], pred_labels[i][keep]
        if mp.shape[0] <= 0:
            h, w = target_sizes[i] if target_sizes is not None else mp.shape[1:]
            results.append({"segmentation": torch.zeros((h, w), device=cls.device) - 1, "segments_info": []})
            gaps.append(None)
            continue
        size = target_sizes[i] if target_sizes is not None else None
        H, W = (mp.shape[1], mp.shape[2]) if size is None else size
        seg = torch.zeros((H, W), dtype=torch.int32, device=cls.device)
        if size is not None:
            mp = F.interpolate(mp.unsqueeze(0), size=tuple(size), mode="bilinear", align_corners=False)[0]
        mp = mp * sc.view(-1, 1, 1)
        lab_map = mp.argmax(0)
        segs, memory, current = [], {}, 0
        for k in range(lb.shape[0]):
            c = lb[k].item()
            fuse = c in label_ids_to_fuse
            mask_k = lab_map == k
            area, orig = mask_k.sum(), (mp[k] >= mask_threshold).sum()
            ok = bool(area > 0 and orig > 0)
            if ok and not (area / orig).item() > overlap_mask_area_threshold:
                ok = False
            if ok:
                current = memory[c] if c in memory else current + 1
                seg[mask_k] = current
                segs.append({"id": current, "label_id": c, "was_fused": fuse, "score": round(sc[k].item(), 6)})
                if fuse:
                    memory[c] = current
        results.append({"segmentation": seg, "segments_info": segs})
        gaps.append(rel_top2_gap(mp) if with_gaps else None)
    return (results, gaps) if with_gaps else results


# ------------------------------------------------------------------ the restatement against the dependency
def _fixture():
    g = load_golden("postprocess_semantic_panoptic.npz")
    return g, json.loads(str(g["info_json"]))


def _inputs(g, name):
    return torch.from_numpy(g[f"{name}_class_logits"]), torch.from_numpy(g[f"{name}_mask_logits"])


@pytest.mark.parametrize("case", ["sem_none", "sem_mixed", "sem_c1"])
def test_semantic_restatement_matches_dependency(case):
    g, info = _fixture()
    c = info[case]
    cls, m = _inputs(g, c["inputs"])
    st = c["score_stride"]
    for i, (seg, S) in enumerate(semantic_reference(cls, m, c["target_sizes"])):
        assert seg.dtype == torch.int64
        assert torch.equal(seg.to(torch.int8), torch.from_numpy(g[f"{case}_seg_{i}"]))
        assert torch.equal(S[:, ::st, ::st], torch.from_numpy(g[f"{case}_scores_{i}"]))


@pytest.mark.parametrize("case", ["pan_mixed", "pan_none", "pan_nofuse", "pan_thr", "pan_c1"])
def test_panoptic_restatement_matches_dependency(case):
    g, info = _fixture()
    c = info[case]
    cls, m = _inputs(g, c["inputs"])
    res = panoptic_reference(cls, m, c["threshold"], c["mask_threshold"], c["overlap_mask_area_threshold"],
                             set(c["label_ids_to_fuse"]), c["target_sizes"])
    for i, r in enumerate(res):
        assert r["segments_info"] == c["segments_info"][i]
        assert str(r["segmentation"].dtype) == str(g[f"{case}_segdtype_{i}"])
        assert torch.equal(r["segmentation"].to(torch.int16), torch.from_numpy(g[f"{case}_seg_{i}"]))


def test_fixture_pins_the_quirks():
    """The fixture holds what the docstrings promise: duplicate ids of a fused label, an image without kept queries
    (float -1 map at the target size), a threshold sitting on a score (dropped by the strict `>`), C = 1."""
    g, info = _fixture()
    assert [s["id"] for s in info["pan_mixed"]["segments_info"][0]] == [1, 2, 1, 2]
    assert all(s["was_fused"] == (s["label_id"] == 0) for s in info["pan_mixed"]["segments_info"][0])
    assert info["pan_mixed"]["segments_info"][1] == [] and str(g["pan_mixed_segdtype_1"]) == "torch.float32"
    assert g["pan_mixed_seg_1"].shape == (400, 500) and (g["pan_mixed_seg_1"] == -1).all()
    assert g["pan_none_seg_0"].shape == GRID and str(g["pan_none_segdtype_0"]) == "torch.int32"
    assert info["pan_thr"]["margins"]["scores_on_threshold"] >= 1
    kept_thr = {s["score"] for s in info["pan_thr"]["segments_info"][2]}
    assert round(info["pan_thr"]["threshold"], 6) not in kept_thr
    assert g["sem_c1_class_logits"].shape[-1] == 2 and (g["sem_c1_seg_0"] == 0).all()


# ------------------------------------------------------------------ host segment-id assignment
def _assign(labels, above, owned, overlap=0.8, fuse=()):
    from weed_instance_segmentation_amd.postprocess import assign_segment_ids
    return assign_segment_ids(labels, [0.9] * len(labels), above, owned, overlap, set(fuse))


def test_assign_fused_label_resets_counter_to_duplicate_ids():
    ids, segs = _assign([5, 7, 5, 9], [10] * 4, [10] * 4, fuse={5})
    assert ids == [1, 2, 1, 2]
    assert [(s["id"], s["label_id"], s["was_fused"]) for s in segs] == [(1, 5, True), (2, 7, False), (1, 5, True), (2, 9, False)]


def test_assign_without_fusion_numbers_survivors_in_query_order():
    ids, segs = _assign([5, 7, 5, 9], [10, 10, 10, 10], [10, 0, 10, 10])
    assert ids == [1, 0, 2, 3] and [s["id"] for s in segs] == [1, 2, 3]


def test_assign_exact_four_fifths_passes_at_point_eight():
    """float32(4 / 5) > 0.8 as a double: the dependency keeps an exact 0.8 ratio."""
    ids, _ = _assign([1, 1, 1], [5, 10, 1000], [4, 8, 799])
    assert ids == [1, 2, 0]
    ids, _ = _assign([1], [5], [4], overlap=0.81)
    assert ids == [0]


def test_assign_zero_areas_reject():
    ids, segs = _assign([1, 2, 3], [0, 7, 0], [0, 0, 3])
    assert ids == [0, 0, 0] and segs == []


def test_assign_score_rounding():
    from weed_instance_segmentation_amd.postprocess import assign_segment_ids
    s = float(torch.tensor(0.123456789, dtype=torch.float32))
    _, segs = assign_segment_ids([0], [s], [3], [3], 0.8, set())
    assert segs[0]["score"] == round(s, 6)


# ------------------------------------------------------------------ argument handling without a GPU
def _cpu_outputs():
    return SimpleNamespace(class_queries_logits=torch.randn(1, 4, 3), masks_queries_logits=torch.randn(1, 4, 8, 8))


@pytest.mark.parametrize("method", ["post_process_semantic_segmentation", "post_process_panoptic_segmentation"])
def test_cpu_logits_raise(method):
    from weed_instance_segmentation_amd._lib import Wm2fError
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    with pytest.raises(Wm2fError):
        getattr(Mask2FormerInstancePostProcessor(), method)(_cpu_outputs())


def test_processor_signatures_match_dependency():
    import inspect
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    p = Mask2FormerInstancePostProcessor
    sem = inspect.signature(p.post_process_semantic_segmentation).parameters
    assert list(sem) == ["self", "outputs", "target_sizes", "return_segmentation_scores"]
    assert sem["target_sizes"].default is None and sem["return_segmentation_scores"].default is False
    pan = inspect.signature(p.post_process_panoptic_segmentation).parameters
    assert list(pan) == ["self", "outputs", "threshold", "mask_threshold", "overlap_mask_area_threshold", "label_ids_to_fuse",
                         "target_sizes"]
    assert [pan[k].default for k in list(pan)[2:]] == [0.5, 0.5, 0.8, None, None]
    try:
        from weed_instance_segmentation_amd import Mask2FormerImageProcessor
    except ImportError:
        return
    assert hasattr(Mask2FormerImageProcessor, "post_process_panoptic_segmentation")


def test_semantic_output_has_key_and_attribute_access():
    from weed_instance_segmentation_amd.postprocess import SemanticSegmentationPostProcessorOutput
    a, b = torch.zeros(2, 2, dtype=torch.int64), torch.zeros(3, 2, 2)
    o = SemanticSegmentationPostProcessorOutput(a, b)
    assert o.segmentation is a and o["segmentation_scores"] is b
    with pytest.raises(AttributeError):
        o.missing
