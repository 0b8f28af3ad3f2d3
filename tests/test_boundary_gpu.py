"""Boundary bands and Boundary AP on the GPU: `ops.labelmap_boundary` bit for bit against the
brute-force restatement at the sizes where the two kernels change path, `ops.coco_match_min` against the reference's
matching on the smaller of two IoUs, and `MeanAveragePrecision(iou_type="boundary")` through `update_from_maps`
against the reference subclass of the oracle's COCOeval (tests/boundary_reference.py, pinned on the host by
tests/test_boundary_cpu.py)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import boundary_reference as R
from oracle import coco_eval as C

pytestmark = pytest.mark.gpu
DEV = "cuda"

# rows that are no multiple of 4 (53, 257, 1: the one-pixel-per-lane path), rows below one wave step, straddling one and
# several (70, 257, 300, 516 at 64 or 256 pixels per step), single rows and columns.  The vertical pass gives a chunk at
# least 64 rows (and at least 2d): H = 65 is the height just above one chunk, 130 and 200 span three and four, and at
# d = 31 a chunk's warm-up of 31 rows on either side is clipped at the image edges or reaches into both neighbours.
SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (65, 257), (200, 300), (130, 516)]
DTYPES = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8}


def _dilations(H, W):
    return sorted({1, 2, 7, 31, max(1, (min(H, W) - 1) // 2), max(H, W), max(H, W) + 3})


def _maps(kind, dtype, H, W, B=3):
    """B different (H, W) maps.  "rects": a few large rectangles, so interiors exist; "blocks": random 4 x 4 blocks, so
    almost none do.  Background -1 (uint8: 0, an id like any other)."""
    rng = np.random.default_rng(H * 1000 + W + (kind == "blocks"))
    out = []
    for b in range(B):
        if kind == "rects":
            m = np.full((H, W), -1, np.int64)
            for k in range(5):
                y, x = int(rng.integers(0, max(1, H // 2))), int(rng.integers(0, max(1, W // 2)))
                h, w = int(rng.integers(H // 3 + 1, H + 1)), int(rng.integers(W // 3 + 1, W + 1))
                m[y:y + h, x:x + w] = k
            m[:, W - W // 5:] = 9 + b  # a stripe to the right edge: the row test at the image border
        else:
            blocks = rng.integers(-1, 6, ((H + 3) // 4, (W + 3) // 4))
            m = np.kron(blocks, np.ones((4, 4), np.int64))[:H, :W]
        if dtype == torch.uint8:
            m = np.where(m < 0, 0, m + 1)
            if H * W > 8:
                m[H // 2, W // 2] = 255
            out.append(m.astype(np.uint8))
        elif dtype == torch.int32:
            if H * W > 8:
                m[H // 2, W // 2] = 70000  # an id beyond 2^16
                m[H // 3, W // 3] = -7     # a negative int is no id
            out.append(m.astype(np.int32))
        else:
            f = m.astype(np.float32)
            if H * W > 8:
                f[H // 2, W // 2] = 2.5       # no id: ends the runs through it
                f[H // 3, W // 3] = np.nan
                zeros = np.argwhere(m == 0)
                if len(zeros):                # -0.0 is id 0: inside a region of 0 it changes nothing
                    f[tuple(zeros[len(zeros) // 2])] = -0.0
                else:
                    f[0, 0] = -0.0
            out.append(f)
    return np.stack(out)


@pytest.mark.parametrize("kind", ["rects", "blocks"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelmap_boundary_equals_restatement(shape, dtype, kind):
    from weed_instance_segmentation_amd import ops
    H, W = shape
    maps = _maps(kind, DTYPES[dtype], H, W)
    dev = torch.from_numpy(maps).to(DEV)
    n_interior = 0
    for d in _dilations(H, W):
        want = torch.from_numpy(np.stack([R.boundary_map(m, d) for m in maps]))
        got = ops.labelmap_boundary(dev, d)
        assert got.dtype == torch.int32 and got.shape == dev.shape
        assert torch.equal(got.cpu(), want), (shape, dtype, kind, d, int((got.cpu() != want).sum()))
        assert torch.equal(ops.labelmap_boundary(dev, d), got), "a second call differs"
        n_interior += int(((want == -1) & torch.from_numpy(R.id_keys(maps) >= 0)).sum())
        if d >= max(H, W):
            assert torch.equal(got.cpu(), torch.from_numpy(R.id_keys(maps).astype(np.int32)))  # no interior at all
    if kind == "rects" and min(H, W) >= 37:
        assert n_interior > 0  # the comparison is not one of maps without interiors


def test_labelmap_boundary_unaligned_view_and_arguments():
    """A map whose storage starts 4 bytes into an allocation (W % 4 == 0, but no 16-byte alignment) takes the
    one-pixel path and gives the same result; sizes and dtypes outside the contract raise."""
    from weed_instance_segmentation_amd import _lib, ops
    m = _maps("rects", torch.float32, 64, 64)
    flat = torch.zeros(m.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = torch.from_numpy(m).to(DEV).reshape(-1)
    view = flat[1:].view(3, 64, 64)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    assert torch.equal(ops.labelmap_boundary(view, 3), ops.labelmap_boundary(torch.from_numpy(m).to(DEV), 3))
    with pytest.raises(TypeError):
        ops.labelmap_boundary(torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV), 1)
    with pytest.raises(ValueError):
        ops.labelmap_boundary(torch.zeros(4, 4, device=DEV), 1)
    with pytest.raises(ValueError):
        ops.labelmap_boundary(torch.zeros(1, 4, 4, device=DEV), 0)
    with pytest.raises(_lib.Wm2fError):
        ops.labelmap_boundary(torch.zeros(1, 4, 4, device=DEV), 16385)
    with pytest.raises(_lib.Wm2fError):
        ops.labelmap_boundary(torch.zeros(1, 4, 4), 1)


def test_boundary_maps_public_interface():
    from weed_instance_segmentation_amd import boundary_maps, instance_statistics
    m = _maps("rects", torch.float32, 200, 300)
    want5 = np.stack([R.boundary_map(x, 5) for x in m])
    got = boundary_maps(torch.from_numpy(m).to(DEV), dilation=5)
    assert got.dtype == torch.int32 and got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(want5))
    one = boundary_maps(m[1], dilation=5)  # a host numpy map, 2-D in and out
    assert one.shape == (200, 300) and torch.equal(one.cpu(), torch.from_numpy(want5[1]))
    d = R.boundary_dilation(200, 300)  # 0.02 x 360.6 = 7
    assert d == 7 and torch.equal(boundary_maps(m[0]).cpu(), torch.from_numpy(R.boundary_map(m[0], 7)))
    assert torch.equal(boundary_maps(m[0], dilation_ratio=0.01).cpu(), torch.from_numpy(R.boundary_map(m[0], 4)))
    # the result is an id map: the statistics kernel takes it as it is, and counts the bands
    area, _, _ = instance_statistics(one, n=12)
    assert area.cpu().tolist() == [int((want5[1] == k).sum()) for k in range(12)]


# ------------------------------------------------------------------------------------------------ coco_match_min
def _match_case(seed, B, D, G):
    """Two count triples per image.  Image 1 has no detection, image 2 no GT, image 3 an ABSENT GT column; areas around
    the range bounds, intersections giving equal and exactly-threshold IoUs, and a second triple that is zero where the
    first is not and the other way round."""
    from weed_instance_segmentation_amd.metrics import ABSENT
    rng = np.random.default_rng(seed)
    areas = np.array([10, 1024, 1025, 7000, 9216, 9217, 12000])
    da, ga = rng.choice(areas, (B, D)).astype(np.int32), rng.choice(areas, (B, G)).astype(np.int32)
    da2, ga2 = rng.choice([8, 300, 304, 600], (B, D)).astype(np.int32), rng.choice([8, 300, 304, 600], (B, G)).astype(np.int32)

    def inter_of(a, g):
        m = np.minimum(a[:, :, None], g[:, None, :])
        pick = rng.choice(4, m.shape, p=[0.45, 0.2, 0.2, 0.15])
        return np.select([pick == 0, pick == 1, pick == 2], [0, m, (2 * m) // 3], m // 2).astype(np.int32)

    inter, inter2 = inter_of(da, ga), inter_of(da2, ga2)
    dl = rng.integers(0, 3, (B, D)).astype(np.int32)
    gl = rng.integers(0, 3, (B, G)).astype(np.int32)
    sc = rng.choice(np.array([0.9, 0.8, 0.8, 0.55, 0.3], np.float32), (B, D))
    nd = np.full(B, D, np.int32)
    ng = np.full(B, G, np.int32)
    nd[1], ng[2] = 0, 0
    nd[3], ng[3] = max(1, D - 2), max(1, G - 1)
    gl[3, 0] = ABSENT
    return inter, da, ga, inter2, da2, ga2, dl, gl, sc, nd, ng


def _run_min(case, second=None):
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd.metrics import AREA_RANGES, IOU_THRESHOLDS
    inter, da, ga, inter2, da2, ga2, dl, gl, sc, nd, ng = case
    D = inter.shape[1]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    sc_pad = np.where(np.arange(D)[None] < nd[:, None], sc, -np.inf).astype(np.float32)
    order = torch.sort(t(sc_pad), dim=1, descending=True, stable=True).indices.to(torch.int32)
    tail = (t(dl), t(gl), order, t(nd), t(ng), t(IOU_THRESHOLDS), t(AREA_RANGES), 100)
    if second == "plain":
        return ops.coco_match(t(inter), t(da), t(ga), *tail)
    trip2 = (inter2, da2, ga2) if second is None else second
    return ops.coco_match_min(t(inter), t(da), t(ga), *(t(x) for x in trip2), *tail)


@pytest.mark.parametrize("D,G", [(5, 3), (70, 65)])
def test_coco_match_min_equals_reference(D, G):
    """The reference subclass's matching -- COCOeval.evaluateImg on min(mask IoU, boundary IoU), the area ranges on the
    first triple's areas -- per (image, category, area range)."""
    B = 4
    case = _match_case(D * 100 + G, B, D, G)
    inter, da, ga, inter2, da2, ga2, dl, gl, sc, nd, ng = case
    rank, dm, di, gi = (x.cpu().numpy() for x in _run_min(case))
    n_checked = n_differs = 0
    for b in range(B):
        for c in range(3):
            dsel = [d for d in range(nd[b]) if dl[b, d] == c]
            gsel = [g for g in range(ng[b]) if gl[b, g] == c]
            srt = sorted(range(len(dsel)), key=lambda i: -float(sc[b, dsel[i]]))
            for r, i in enumerate(srt):
                assert rank[b, dsel[i]] == r
            ious = R.min_iou(inter[b][np.ix_(dsel, gsel)], da[b, dsel], ga[b, gsel],
                             inter2[b][np.ix_(dsel, gsel)], da2[b, dsel], ga2[b, gsel])
            plain = R.iou_from_counts(inter[b][np.ix_(dsel, gsel)], da[b, dsel], ga[b, gsel])
            for a, rng_a in enumerate(C.AREA_RNG):
                dt = [(float(sc[b, d]), int(da[b, d]), ious[j]) for j, d in enumerate(dsel)]
                e = C.evaluate_img(dt, [int(ga[b, g]) for g in gsel], rng_a, 100)
                if e is None:
                    continue
                e1 = C.evaluate_img([(s, ar, plain[j]) for j, (s, ar, _) in enumerate(dt)], [int(ga[b, g]) for g in gsel], rng_a, 100)
                n_differs += not np.array_equal(e["dtMatches"], e1["dtMatches"])
                for r, i in enumerate(srt):
                    d = dsel[i]
                    assert np.array_equal(dm[b, a, :, d], e["dtMatches"][:, r].astype(np.uint8)), (b, c, a, d)
                    assert np.array_equal(di[b, a, :, d], e["dtIgnore"][:, r].astype(np.uint8)), (b, c, a, d)
                    n_checked += 1
                assert sorted(gi[b, a, gsel].tolist()) == sorted(e["gtIgnore"].tolist())
    assert n_checked >= 4 * (D - 2) and n_differs > 0  # the second triple does change matches
    assert (rank[1] == -1).all() and not dm[1].any() and not dm[2].any()
    # the second triple equal to the first: wm2f_coco_match's outputs, bit for bit
    for x, y in zip(_run_min(case, second=(inter, da, ga)), _run_min(case, second="plain")):
        assert torch.equal(x, y)


def test_coco_match_min_at_the_documented_bounds():
    """D = 1024, G = 512, A x T = 40: the launch with the largest LDS request the contract allows (52 KiB)."""
    B, D, G = 2, 1024, 512
    case = list(_match_case(7, 4, D, G))
    case = [x[:B] for x in case]
    case[9][:], case[10][:] = D, G  # every slot in use
    inter, da, ga = case[0], case[1], case[2]
    same, plain = _run_min(case, second=(inter, da, ga)), _run_min(case, second="plain")
    for x, y in zip(same, plain):
        assert torch.equal(x, y)
    assert plain[1].any()
    # bands that never meet: nothing matches, and a detection is ignored iff its (mask) area is outside the range
    rank, dm, di, gi = _run_min(case, second=(np.zeros_like(inter), case[4], case[5]))
    assert not dm.any() and torch.equal(rank, plain[0]) and torch.equal(gi, plain[3])
    lo, hi = (torch.tensor(np.asarray(C.AREA_RNG, np.float64)[:, k]) for k in (0, 1))
    a = torch.from_numpy(da.astype(np.float64))
    out = (a[:, None, :] < lo[None, :, None]) | (a[:, None, :] > hi[None, :, None])  # (B, A, D)
    counted = (rank.cpu() < 100)[:, None, None, :]
    assert torch.equal(di.cpu().bool(), (out[:, :, None, :] & counted).expand(-1, -1, 10, -1))


# ---------------------------------------------------------------------------------------------- Boundary AP
@functools.lru_cache(maxsize=None)
def _ap_case():
    """The fixtures and the reference's results on them, computed once."""
    segs, infos, maps, mappings = R.ap_fixtures()
    preds, target = R.fixtures_as_stacks(segs, infos, maps, mappings)
    ref_b, ref_s = R.BoundaryCocoEval(), C.CocoSegmEval()
    ref_b.update(preds, target)
    ref_s.update(preds, target)
    per = []
    for p, t in zip(preds, target):
        o = R.BoundaryCocoEval()
        o.update([p], [t])
        per.append(float(o.compute()["map"]))
    return (segs, infos, maps, mappings), ref_b.compute(), ref_s.compute(), torch.tensor(per, dtype=torch.float32)


def _update(metric, fixtures, rows=None):
    segs, infos, maps, mappings = fixtures
    rows = range(len(segs)) if rows is None else rows
    metric.update_from_maps([torch.from_numpy(segs[i]).to(DEV) for i in rows], [infos[i] for i in rows],
                            [maps[i] for i in rows], [mappings[i] for i in rows])
    return metric


def test_boundary_ap_equals_reference():
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    fixtures, ref_b, ref_s, _ = _ap_case()
    res = _update(MeanAveragePrecision(iou_type="boundary"), fixtures).compute()
    assert set(res) == set(ref_b)
    for k in ref_b:
        assert torch.equal(res[k], ref_b[k]), (k, res[k], ref_b[k])
    assert not torch.equal(ref_b["map"], ref_s["map"])  # (also asserted on the host) not plain mask AP
    # one image per update: the records do not depend on the batching; then a wider band, given by its ratio
    one = MeanAveragePrecision(iou_type="boundary")
    for i in range(3):
        _update(one, fixtures, [i])
    r1 = one.compute()
    for k in ref_b:
        assert torch.equal(r1[k], ref_b[k]), k
    wide = _update(MeanAveragePrecision(iou_type="boundary", dilation_ratio=0.05), fixtures).compute()
    preds, target = R.fixtures_as_stacks(*fixtures)
    ref_w = R.BoundaryCocoEval(dilation_ratio=0.05)
    ref_w.update(preds, target)
    ref_w = ref_w.compute()
    for k in ref_w:
        assert torch.equal(wide[k], ref_w[k]), k


def test_segm_and_boundary_together():
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    fixtures, ref_b, ref_s, _ = _ap_case()
    both = _update(MeanAveragePrecision(iou_type=("segm", "boundary")), fixtures).compute()
    plain = _update(MeanAveragePrecision(iou_type="segm"), fixtures).compute()
    assert set(both) == {f"{p}_{k}" for p in ("segm", "boundary") for k in plain if k != "classes"} | {"classes"}
    for k in plain:
        if k != "classes":
            assert torch.equal(both[f"segm_{k}"], plain[k]), k
            assert torch.equal(both[f"segm_{k}"], ref_s[k]), k
            assert torch.equal(both[f"boundary_{k}"], ref_b[k]), k
    assert torch.equal(both["classes"], plain["classes"])
    three = _update(MeanAveragePrecision(iou_type=("bbox", "boundary", "segm"), boxes_from_masks=True), fixtures).compute()
    box = _update(MeanAveragePrecision(iou_type="bbox", boxes_from_masks=True), fixtures).compute()
    for k in plain:
        if k != "classes":
            assert torch.equal(three[f"boundary_{k}"], ref_b[k]) and torch.equal(three[f"bbox_{k}"], box[k]), k


def test_compute_per_image_and_update_raises():
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    fixtures, _, _, per_ref = _ap_case()
    m = _update(MeanAveragePrecision(iou_type=("segm", "boundary")), fixtures)
    per = m.compute_per_image("boundary")
    fresh = torch.stack([_update(MeanAveragePrecision(iou_type="boundary"), fixtures, [i]).compute()["map"] for i in range(3)])
    assert torch.equal(per, fresh) and torch.equal(per, per_ref)
    assert not torch.equal(per, m.compute_per_image("segm"))
    assert torch.equal(_update(MeanAveragePrecision(iou_type="boundary"), fixtures).compute_per_image(), per_ref)
    preds, target = R.fixtures_as_stacks(*fixtures)
    with pytest.raises(ValueError, match="update_from_maps"):
        MeanAveragePrecision(iou_type="boundary").update(preds, target)


def test_test_with_metrics_boundary():
    """One pass of the tiny model over two of tests/golden/ref_samples: the twelve COCO names, finite, and the segm half
    of a ("segm", "boundary") call equal to the plain call."""
    from conftest import load_golden
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation, data
    from weed_instance_segmentation_amd.metrics import test_with_metrics
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    g = load_golden("full_tiny.npz")
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}
    sd["class_predictor.bias"] = sd["class_predictor.bias"].clone()
    sd["class_predictor.bias"][1] += 8.0  # instances of class 1 pass the score threshold (tests/test_metrics_gpu.py)
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig.from_dict(json.loads(str(g["config_json"]))))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    ds = data.PreprocessedDataset(os.path.join(os.path.dirname(__file__), "golden", "ref_samples"))
    loader = [data.collate_fn([ds[0], ds[1]])]
    names = {"map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100",
             "mar_small", "mar_medium", "mar_large"}
    res = test_with_metrics(model, Mask2FormerInstancePostProcessor(), loader, DEV, iou_type="boundary")
    assert names <= set(res) and all(bool(torch.isfinite(res[k])) for k in names)
    both = test_with_metrics(model, Mask2FormerInstancePostProcessor(), loader, DEV, iou_type=("segm", "boundary"))
    segm = test_with_metrics(model, Mask2FormerInstancePostProcessor(), loader, DEV)
    for k in names:
        assert torch.equal(both[f"segm_{k}"], segm[k]) and torch.equal(both[f"boundary_{k}"], res[k]), k
