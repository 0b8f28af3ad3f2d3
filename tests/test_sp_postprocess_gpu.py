"""Semantic and panoptic post-processing on the GPU: the HIP path against the dependency's own
outputs (tests/golden/postprocess_semantic_panoptic.npz) and against the plain-torch restatement of
tests/test_sp_postprocess_cpu.py run on the same GPU tensors at the reference's eval shape.  Needs an MI355X (-m gpu).

Agreement rules: segments_info identical (ids, labels, was_fused; scores within 2e-6); semantic scores within
rtol 1e-5 / atol 1e-6; a map pixel may differ only where the reference's top-two values are within 1e-5 relative,
and such pixels are at most 1e-4 of the map."""
import json
import logging
from types import SimpleNamespace

import pytest
import torch

from conftest import load_golden
from test_sp_postprocess_cpu import panoptic_reference, rel_top2_gap, semantic_reference, semantic_scores_at

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    return Mask2FormerInstancePostProcessor()


def _fixture():
    g = load_golden("postprocess_semantic_panoptic.npz")
    return g, json.loads(str(g["info_json"]))


def _inputs(g, name):
    return torch.from_numpy(g[f"{name}_class_logits"]), torch.from_numpy(g[f"{name}_mask_logits"])


def _outputs(cls, masks):
    return SimpleNamespace(class_queries_logits=cls.cuda(), masks_queries_logits=masks.cuda())


def _same_info(a, b, tol=2e-6):
    assert len(a) == len(b), (a, b)
    for x, y in zip(a, b):
        assert (x["id"], x["label_id"], x["was_fused"]) == (y["id"], y["label_id"], y["was_fused"]), (a, b)
        assert abs(x["score"] - y["score"]) <= tol


def _close_map(got, exp, gap, max_frac=1e-4):
    """got == exp except where the reference's top-two values are within 1e-5 relative (gap: that relative gap)."""
    assert got.shape == exp.shape
    diff = got.to(exp.device).to(torch.int64) != exp.to(torch.int64)
    if gap is None:
        assert not diff.any()
        return
    gap = gap.to(diff.device)
    assert not (diff & (gap >= 1e-5)).any(), f"{int((diff & (gap >= 1e-5)).sum())} pixels differ away from a near-tie"
    assert diff.float().mean().item() <= max_frac


# ------------------------------------------------------------------ against the dependency's outputs
@pytest.mark.parametrize("case", ["sem_none", "sem_mixed", "sem_c1"])
@pytest.mark.parametrize("scores", [False, True])
def test_semantic_matches_dependency(P, case, scores):
    g, info = _fixture()
    c = info[case]
    cls, m = _inputs(g, c["inputs"])
    ts, st = c["target_sizes"], c["score_stride"]
    res = P.post_process_semantic_segmentation(_outputs(cls, m), target_sizes=ts, return_segmentation_scores=scores)
    assert len(res) == cls.shape[0]
    for i, r in enumerate(res):
        seg = r.segmentation if scores else r
        assert seg.is_cuda and seg.dtype == torch.int64
        assert tuple(seg.shape) == (tuple(ts[i]) if ts else (384, 384))
        gap = rel_top2_gap(semantic_scores_at(cls[i], m[i], ts[i] if ts else None))
        _close_map(seg.cpu(), torch.from_numpy(g[f"{case}_seg_{i}"]), gap)
        if scores:
            assert r["segmentation_scores"].is_cuda and r.segmentation_scores.dtype == torch.float32
            assert r.segmentation_scores.shape == (cls.shape[-1] - 1, *seg.shape)
            torch.testing.assert_close(r.segmentation_scores[:, ::st, ::st].cpu(), torch.from_numpy(g[f"{case}_scores_{i}"]),
                                       rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", ["pan_mixed", "pan_none", "pan_nofuse", "pan_thr", "pan_c1"])
def test_panoptic_matches_dependency(P, case):
    g, info = _fixture()
    c = info[case]
    cls, m = _inputs(g, c["inputs"])
    res = P.post_process_panoptic_segmentation(_outputs(cls, m), threshold=c["threshold"], mask_threshold=c["mask_threshold"],
                                               overlap_mask_area_threshold=c["overlap_mask_area_threshold"],
                                               label_ids_to_fuse=set(c["label_ids_to_fuse"]), target_sizes=c["target_sizes"])
    _, gaps = panoptic_reference(cls, m, c["threshold"], c["mask_threshold"], c["overlap_mask_area_threshold"],
                                 set(c["label_ids_to_fuse"]), c["target_sizes"], with_gaps=True)
    for i, r in enumerate(res):
        _same_info(r["segments_info"], c["segments_info"][i])
        seg = r["segmentation"]
        assert seg.is_cuda and str(seg.dtype) == str(g[f"{case}_segdtype_{i}"])
        _close_map(seg.cpu(), torch.from_numpy(g[f"{case}_seg_{i}"]), gaps[i])


# ------------------------------------------------------------------ against the restatement at the eval shape
def _eval_inputs(B, Q, C, h=256, w=256, seed=0):
    """Mask logits that tile the image: a 16 x 16 grid of cells, each owned by one random query (logit about +6 there,
    -6 elsewhere, bicubic-upsampled, plus noise), so queries own 0, 1 or a few blobs; class logits where about a fifth
    of the queries name a class strongly and the rest lean to the null class."""
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


EVAL = [(2, 100, 3, [(1024, 1024), (683, 1024)]), (2, 200, 133, [(683, 1024), (1024, 1024)])]


@pytest.mark.parametrize("B,Q,C,ts", EVAL)
def test_semantic_matches_restatement_eval_shape(P, B, Q, C, ts):
    cls, m = _eval_inputs(B, Q, C)
    for sizes in (ts, None):
        res = P.post_process_semantic_segmentation(_outputs(cls, m), target_sizes=sizes, return_segmentation_scores=True)
        ref = semantic_reference(cls, m, sizes)
        for r, (seg, S) in zip(res, ref):
            torch.testing.assert_close(r.segmentation_scores, S, rtol=1e-5, atol=1e-6)
            _close_map(r.segmentation, seg, rel_top2_gap(S))
        plain = P.post_process_semantic_segmentation(_outputs(cls, m), target_sizes=sizes)
        assert all(torch.equal(a, b.segmentation) for a, b in zip(plain, res))


@pytest.mark.parametrize("B,Q,C,ts", EVAL)
@pytest.mark.parametrize("fuse", [set(), {0, 2}])
def test_panoptic_matches_restatement_eval_shape(P, B, Q, C, ts, fuse):
    cls, m = _eval_inputs(B, Q, C, seed=1)
    for sizes in (ts, None):
        res = P.post_process_panoptic_segmentation(_outputs(cls, m), label_ids_to_fuse=fuse, target_sizes=sizes)
        ref, gaps = panoptic_reference(cls, m, label_ids_to_fuse=fuse, target_sizes=sizes, with_gaps=True)
        assert sum(len(r["segments_info"]) for r in ref) >= 3  # the case exercises the area test and the painting
        for r, e, gap in zip(res, ref, gaps):
            _same_info(r["segments_info"], e["segments_info"])
            assert r["segmentation"].dtype == e["segmentation"].dtype == torch.int32
            _close_map(r["segmentation"], e["segmentation"], gap)


def test_panoptic_keeps_up_to_all_queries(P):
    """K = Q = 200: every query kept (strong labels everywhere), small odd target."""
    cls, m = _eval_inputs(1, 200, 3, 64, 48, seed=2)
    cls[..., :3] = -4.0
    cls[..., 1] = 8.0 + torch.rand(1, 200, device="cuda")
    res = P.post_process_panoptic_segmentation(_outputs(cls, m), label_ids_to_fuse=set(), target_sizes=[(97, 131)])
    ref, gaps = panoptic_reference(cls, m, target_sizes=[(97, 131)], with_gaps=True)
    _same_info(res[0]["segments_info"], ref[0]["segments_info"])
    _close_map(res[0]["segmentation"], ref[0]["segmentation"], gaps[0])


def test_bf16_logits(P):
    cls, m = _eval_inputs(2, 100, 3, 64, 64, seed=3)
    cls, m = cls.bfloat16(), m.bfloat16()
    ts = [(200, 150), (200, 150)]
    sem = P.post_process_semantic_segmentation(_outputs(cls, m), target_sizes=ts, return_segmentation_scores=True)
    for r, (seg, S) in zip(sem, semantic_reference(cls.float(), m.float(), ts)):
        torch.testing.assert_close(r.segmentation_scores, S, rtol=1e-5, atol=1e-6)
        _close_map(r.segmentation, seg, rel_top2_gap(S))
    pan = P.post_process_panoptic_segmentation(_outputs(cls, m), label_ids_to_fuse=set(), target_sizes=ts)
    ref, gaps = panoptic_reference(cls.float(), m.float(), target_sizes=ts, with_gaps=True)
    for r, e, gap in zip(pan, ref, gaps):
        _same_info(r["segments_info"], e["segments_info"])
        _close_map(r["segmentation"], e["segmentation"], gap)


def test_panoptic_empty(P):
    cls, m = _eval_inputs(2, 20, 3, 32, 32, seed=4)
    cls[..., 3] = 10.0  # every query predicts the null class
    for sizes, shapes in (([(50, 61), (7, 9)], [(50, 61), (7, 9)]), (None, [(384, 384)] * 2)):
        res = P.post_process_panoptic_segmentation(_outputs(cls, m), label_ids_to_fuse=set(), target_sizes=sizes)
        for r, shp in zip(res, shapes):
            assert r["segments_info"] == []
            s = r["segmentation"]
            assert s.is_cuda and s.dtype == torch.float32 and tuple(s.shape) == shp and bool((s == -1).all())


def test_panoptic_mixed_empty_and_kept(P):
    cls, m = _eval_inputs(3, 30, 3, 32, 32, seed=5)
    cls[1, :, 3] = 10.0
    ts = [(40, 40), (40, 40), (33, 21)]
    res = P.post_process_panoptic_segmentation(_outputs(cls, m), label_ids_to_fuse={1}, target_sizes=ts)
    ref, gaps = panoptic_reference(cls, m, label_ids_to_fuse={1}, target_sizes=ts, with_gaps=True)
    assert res[1]["segmentation"].dtype == torch.float32 and res[1]["segments_info"] == []
    for i in (0, 2):
        _same_info(res[i]["segments_info"], ref[i]["segments_info"])
        _close_map(res[i]["segmentation"], ref[i]["segmentation"], gaps[i])


def test_argument_errors(P, caplog):
    cls, m = _eval_inputs(2, 10, 3, 16, 16, seed=6)
    with pytest.raises(ValueError):
        P.post_process_semantic_segmentation(_outputs(cls, m), target_sizes=[(10, 10)])
    with pytest.raises(ValueError):
        P.post_process_panoptic_segmentation(_outputs(cls, m), label_ids_to_fuse=set(), target_sizes=[(10, 10)] * 3)
    with caplog.at_level(logging.WARNING):
        P.post_process_panoptic_segmentation(_outputs(cls, m))
    assert "label_ids_to_fuse" in caplog.text
