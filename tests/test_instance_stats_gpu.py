"""Per-instance statistics and box mAP on the GPU: the kernel against the numpy restatement with
torch.equal (all integer), the post-processor's `return_instance_stats`, `instance_statistics`, and
MeanAveragePrecision("bbox", boxes_from_masks=True) through update_from_maps against the CPU route of test_instance_stats_cpu.py."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from instance_stats_reference import (bbox_records_cpu, boxes_reference, images_from_maps, instance_stats_reference)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LDS_CAP = 1024  # kIsLdsMaxIds of csrc/instance_stats.hip: above it the kernel accumulates in global memory
NP_DT = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}


def _scene(rng, shape, N, dtype, noise=0.02):
    """Rectangles of ids 0 .. N-1 (later ones paint over earlier ones, tall ones span row strips), noise pixels of valid
    and of ignored values, background -1 (fp32 / int32) or 200 (uint8)."""
    H, W = shape
    bg = 200 if dtype == torch.uint8 else -1
    m = np.full(shape, bg, np.int64)
    for i in range(min(N, 40)):
        k = int(rng.integers(0, N))
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[y0:y0 + int(rng.integers(1, H)), x0:x0 + int(rng.integers(1, W))] = k
    hit = rng.random(shape) < noise
    m[hit] = rng.integers(0, min(N + 3, 250), int(hit.sum()))  # N .. N+2 are outside [0, N)
    m = m.astype(NP_DT[dtype])
    if dtype == torch.float32:
        m[rng.random(shape) < 0.005] = 1.5  # a fractional value is no id
    return m


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8])
@pytest.mark.parametrize("B,shape", [(3, (37, 53)), (3, (130, 257)), (1, (64, 64))])
@pytest.mark.parametrize("N", [1, 5, LDS_CAP + 76])
def test_stats_equal_the_restatement(dtype, B, shape, N):
    from weed_instance_segmentation_amd import ops
    rng = np.random.default_rng(N + shape[0] + B)
    maps = np.stack([_scene(rng, shape, min(N, 240), dtype) for _ in range(B)])
    t = torch.from_numpy(maps).to(DEV)
    got = ops.labelmap_instance_stats(t, N=N)
    assert got.shape == (B, N, 8) and got.dtype == torch.int64 and got.is_cuda
    ref = np.stack([instance_stats_reference(maps[b], N=N) for b in range(B)])
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
    assert int(ref[:, :, 0].sum()) > 0
    # the GT form: ascending raw ids, a different number per image, values the list omits
    pool = np.setdiff1d(np.arange(0, min(N + 3, 250)), [4])
    ids_l = [np.sort(rng.choice(pool, max(1, min(len(pool), N) - b), replace=False)) for b in range(B)]
    G = N
    ids_t = torch.zeros(B, G, dtype=torch.int32)
    for b in range(B):
        ids_t[b, :len(ids_l[b])] = torch.from_numpy(ids_l[b].astype(np.int32))
    n_ids = torch.tensor([len(x) for x in ids_l], dtype=torch.int32)
    got = ops.labelmap_instance_stats(t, ids_t.to(DEV), n_ids.to(DEV))
    ref = np.stack([instance_stats_reference(maps[b], ids=list(ids_l[b]), N=G) for b in range(B)])
    assert torch.equal(got.cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_all_background_and_single_instance(dtype):
    from weed_instance_segmentation_amd import ops
    H, W = 70, 260
    bg = np.full((H, W), 200 if dtype == torch.uint8 else -1, NP_DT[dtype])
    one = np.full((H, W), 2, NP_DT[dtype])
    t = torch.from_numpy(np.stack([bg, one])).to(DEV)
    got = ops.labelmap_instance_stats(t, N=4).cpu()
    empty = [0, W, H, -1, -1, 0, 0, 0]
    assert got[0].tolist() == [empty] * 4
    assert got[1].tolist() == [empty, empty, [H * W, 0, 0, W - 1, H - 1, H * W * (W - 1) // 2, W * H * (H - 1) // 2, 0], empty]


def test_full_size_property_and_run_to_run():
    from weed_instance_segmentation_amd import ops
    rng = np.random.default_rng(11)
    B, H, W, N = 2, 1024, 1024, 100
    maps = np.full((B, H, W), -1, np.float32)
    for b in range(B):
        for k in range(N):
            y0, x0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
            maps[b, y0:y0 + int(rng.integers(4, 300)), x0:x0 + int(rng.integers(4, 300))] = k
        hit = rng.random((H, W)) < 0.003
        maps[b][hit] = rng.integers(0, N + 2, int(hit.sum()))
    t = torch.from_numpy(maps).to(DEV)
    a = ops.labelmap_instance_stats(t, N=N)
    b2 = ops.labelmap_instance_stats(t, N=N)
    assert torch.equal(a, b2)
    ref = np.stack([instance_stats_reference(maps[b], N=N) for b in range(B)])
    assert int((ref[:, :, 0] > 0).sum()) > 150
    assert torch.equal(a.cpu(), torch.from_numpy(ref))


def test_instance_statistics_host_device_and_stack():
    from weed_instance_segmentation_amd import instance_statistics, ops
    rng = np.random.default_rng(3)
    maps = np.stack([_scene(rng, (45, 61), 5, torch.float32) for _ in range(2)])
    maps[maps == 3] = -1  # id 3 has no pixel
    dev_stack = torch.from_numpy(maps).to(DEV)
    stats = ops.labelmap_instance_stats(dev_stack, N=6)
    for arg, sel in ((maps[0], 0), (torch.from_numpy(maps[0]), 0), (dev_stack[1], 1), (dev_stack, slice(None))):
        area, bbox, cen = instance_statistics(arg, n=6)
        assert area.is_cuda and bbox.is_cuda and cen.is_cuda and cen.dtype == torch.float64 and bbox.dtype == torch.int64
        s = stats[sel]
        assert torch.equal(area, s[..., 0])
        ra, rb, rc = zip(*[boxes_reference(x) for x in s.cpu().numpy().reshape(-1, 6, 8)])
        assert torch.equal(bbox.cpu().reshape(-1, 6, 4), torch.from_numpy(np.stack(rb)))
        assert np.array_equal(cen.cpu().numpy().reshape(-1, 6, 2), np.stack(rc), equal_nan=True)
        assert torch.isnan(cen[..., 3, :]).all() and bbox[..., 3, :].eq(0).all() and area[..., 3].eq(0).all()
    # a raw-id list in the caller's order
    area, bbox, _ = instance_statistics(dev_stack, ids=[4, 0, 77])
    assert torch.equal(area[:, :2], stats[:, [4, 0], 0]) and area[:, 2].eq(0).all() and bbox[:, 2].eq(0).all()


# ------------------------------------------------------------------------------------------------ the post-processor
def _outputs(g):
    T = torch.from_numpy
    return SimpleNamespace(class_queries_logits=T(g["class_logits"]).cuda(), masks_queries_logits=T(g["mask_logits"]).cuda())


@pytest.mark.parametrize("tag,kw", [("mixed", {}), ("maps", {"return_binary_maps": True}), ("rle", {"return_coco_annotation": True})])
def test_postprocess_return_instance_stats(tag, kw):
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    g = load_golden("postprocess_instances.npz")
    ts = json.loads(str(g["info_json"]))[tag]["target_sizes"]
    if tag == "mixed":
        assert len({tuple(t) for t in ts}) >= 2  # two target sizes in one batch
    p = Mask2FormerInstancePostProcessor()
    plain = p.post_process_instance_segmentation(_outputs(g), threshold=0.5, target_sizes=ts, **kw)
    maps = p.post_process_instance_segmentation(_outputs(g), threshold=0.5, target_sizes=ts)  # the id maps themselves
    res = p.post_process_instance_segmentation(_outputs(g), threshold=0.5, target_sizes=ts, return_instance_stats=True, **kw)
    assert sum(len(r["segments_info"]) for r in res) > 0
    for r, q, m in zip(res, plain, maps):
        if isinstance(q["segmentation"], torch.Tensor):
            assert torch.equal(r["segmentation"], q["segmentation"])
        else:
            assert r["segmentation"] == q["segmentation"]
        assert [{k: s[k] for k in ("id", "label_id", "was_fused", "score")} for s in r["segments_info"]] == q["segments_info"]
        n = len(r["segments_info"])
        area, bbox, cen = boxes_reference(instance_stats_reference(m["segmentation"].cpu().numpy(), N=n))
        for s in r["segments_info"]:
            i = s["id"]
            assert type(s["area"]) is int and s["area"] == area[i]
            assert s["bbox"] == bbox[i].tolist() and all(type(v) is int for v in s["bbox"])
            assert s["centroid"] == (None if area[i] == 0 else (float(cen[i, 0]), float(cen[i, 1])))


# ------------------------------------------------------------------------------------------------------- box mAP
def _map_images(seed, n_images=3):
    """96 x 96 maps: about 6 predictions (one painted over completely) and 5 GT instances per image, one GT id of the
    mapping absent from the map, and a 255 region."""
    rng = np.random.default_rng(seed)
    H = W = 96
    segs, infos, gts, mappings = [], [], [], []
    for i in range(n_images):
        gt = np.zeros((H, W), np.uint8)
        boxes = [(4, 40, 4, 44), (50, 90, 6, 30), (8, 30, 52, 92), (40, 80, 40, 70), (84, 94, 60, 94)]
        for k, (y0, y1, x0, x1) in enumerate(boxes):
            gt[y0:y1, x0:x1] = k + 1
            gt[y0:(y0 + y1) // 2, x0 + 2:(x0 + x1) // 2] = 0  # not a rectangle
        gt[0:3, 70:96] = 255
        mappings.append({0: 0, 1: 1, 2: 2, 3: 1, 4: 2, 5: 1, 9: 2, 255: 0} if i else {1: 1, 2: 2, 3: 1, 4: 2, 5: 1, 9: 2})
        seg = np.full((H, W), -1, np.float32)
        info = []
        seg[60:70, 60:70] = 0  # painted over below: area 0
        for k, (y0, y1, x0, x1) in enumerate(boxes + [(60, 75, 55, 80)]):
            d = rng.integers(-6, 7, 4)
            seg[max(0, y0 + d[0]):min(H, y1 + d[1]), max(0, x0 + d[2]):min(W, x1 + d[3])] = k if k else 6
        seg[seg == 6] = 0 if i == 1 else 6
        n = 7 if i != 1 else 6
        for k in range(n):
            info.append({"id": k, "label_id": int(rng.integers(1, 3)), "was_fused": False,
                         "score": round(float(rng.choice([0.9, 0.8, 0.8, 0.6])), 6)})
        segs.append(seg)
        infos.append(info)
        gts.append(gt)
    return segs, infos, gts, mappings


def _eq(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (k, a[k], b[k])


def test_box_map_from_maps_equals_the_cpu_route():
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    segs, infos, gts, mappings = _map_images(0)
    cpu = MeanAveragePrecision("bbox", class_metrics=True, boxes_from_masks=True)
    ref = cpu._compute(bbox_records_cpu(images_from_maps(segs, infos, gts, mappings)))
    assert 0.0 < float(ref["map"]) < 1.0
    m = MeanAveragePrecision("bbox", class_metrics=True, boxes_from_masks=True)
    m.update_from_maps([torch.from_numpy(s).to(DEV) for s in segs[:2]], infos[:2], gts[:2], mappings[:2])
    m.update_from_maps([torch.from_numpy(segs[2])], infos[2:], [torch.from_numpy(gts[2]).to(torch.int32)], mappings[2:])
    _eq(m.compute(), ref)
    # both types at once: the bbox half is the same, the segm half is the plain segm metric
    both = MeanAveragePrecision(("bbox", "segm"), class_metrics=True, boxes_from_masks=True)
    segm = MeanAveragePrecision("segm", class_metrics=True)
    for mm in (both, segm):
        mm.update_from_maps([torch.from_numpy(s).to(DEV) for s in segs], infos, gts, mappings)
    res, plain = both.compute(), segm.compute()
    _eq({k[5:]: v for k, v in res.items() if k.startswith("bbox_")}, {k: v for k, v in ref.items() if k != "classes"})
    _eq({k[5:]: v for k, v in res.items() if k.startswith("segm_")}, {k: v for k, v in plain.items() if k != "classes"})
    assert torch.equal(res["classes"], ref["classes"]) and len(res) == 2 * 14 + 1
    # per-image ranking: one fresh metric per image
    for kind in ("bbox", "segm"):
        per = both.compute_per_image(kind)
        for i in range(len(segs)):
            fresh = MeanAveragePrecision(kind, boxes_from_masks=True)
            fresh.update_from_maps([torch.from_numpy(segs[i]).to(DEV)], [infos[i]], [gts[i]], [mappings[i]])
            assert torch.equal(per[i], fresh.compute()["map"]), (kind, i)
    assert torch.equal(m.compute_per_image(), both.compute_per_image("bbox"))
    with pytest.raises(ValueError):
        both.compute_per_image()
