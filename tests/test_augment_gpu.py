"""Training augmentation on the GPU: csrc/augment.hip through the processor, bit for bit against the
Pillow fixture and against the composed route -- the host-flipped image through the un-augmented call at the full
(h, w) frame, then a slice and a pad in torch -- and, at the smallest shapes that reach every branch of the two
kernels, against the numpy restatement (augment_reference.restate).  Every comparison is torch.equal.  Needs an MI355X
(-m gpu)."""
import json

import numpy as np
import pytest
import torch

import augment_reference as R
from conftest import load_golden
from test_augment_cpu import golden_cases
from weed_instance_segmentation_amd import preprocess as P
from weed_instance_segmentation_amd.augment import AugmentParams, TrainAugmentation

pytestmark = pytest.mark.gpu
EDGES = tuple(range(640, 801, 32))
IG = 255


@pytest.fixture(scope="module")
def proc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from weed_instance_segmentation_amd import Mask2FormerImageProcessor
    return Mask2FormerImageProcessor()


def _flip(a):
    if isinstance(a, torch.Tensor):
        return torch.flip(a, dims=[1]).contiguous()
    return np.ascontiguousarray(a[:, ::-1])


def composed(proc, images, maps, id2sem, params, pad_size=None, mask_dtype=torch.float32):
    """The route without the feature: flip on the host, today's call at the whole (h, w) frame, slice, pad."""
    wins = [p.window for p in params]
    Hp, Wp = (pad_size["height"], pad_size["width"]) if pad_size else (max(c for c, _ in wins), max(c for _, c in wins))
    pv = torch.zeros(len(images), 3, Hp, Wp, device="cuda")
    pm = torch.zeros(len(images), Hp, Wp, device="cuda", dtype=torch.int64)
    ml, cl = [], []
    for b, (im, p) in enumerate(zip(images, params)):
        (h, w), (y0, x0), (ch, cw) = p.size, p.origin, p.window
        kw = dict(size={"height": h, "width": w}, size_divisor=0, ignore_index=IG, mask_dtype=mask_dtype)
        src = _flip(im) if p.flip else im
        if maps is None:
            r = proc.preprocess([src], **kw)
        else:
            d = id2sem[b] if isinstance(id2sem, list) else id2sem
            r = proc.preprocess([src], [_flip(maps[b]) if p.flip else maps[b]], d, **kw)
        pv[b, :, :ch, :cw] = r["pixel_values"][0, :, y0:y0 + ch, x0:x0 + cw]
        pm[b, :ch, :cw] = r["pixel_mask"][0, y0:y0 + ch, x0:x0 + cw]
        if maps is None:
            continue
        cut = r["mask_labels"][0][:, y0:y0 + ch, x0:x0 + cw]
        keep = (cut != 0).flatten(1).any(1)  # an instance the crop removes entirely is absent
        masks = torch.full((int(keep.sum()), Hp, Wp), IG, device="cuda", dtype=mask_dtype)
        masks[:, :ch, :cw] = cut[keep]
        ml.append(masks)
        cl.append(r["class_labels"][0][keep])
    return pv, pm, ml, cl


def _assert_equal(out, exp, with_maps=True):
    pv, pm, ml, cl = exp
    assert out["pixel_values"].dtype == torch.float32 and torch.equal(out["pixel_values"], pv)
    assert out["pixel_mask"].dtype == torch.int64 and torch.equal(out["pixel_mask"], pm)
    if not with_maps:
        assert "mask_labels" not in out
        return
    assert len(out["mask_labels"]) == len(ml)
    for b in range(len(ml)):
        assert out["mask_labels"][b].shape == ml[b].shape and out["mask_labels"][b].dtype == ml[b].dtype
        assert torch.equal(out["mask_labels"][b], ml[b])
        assert out["class_labels"][b].dtype == torch.int64 and torch.equal(out["class_labels"][b], cl[b])


def _jitter(H, W, f, crop, flip, frac=(0.5, 0.5)):
    """The jitter rule of TrainAugmentation at an explicit f, the origin at `frac` of the positions that fit."""
    r = min(crop[0] * f / H, crop[1] * f / W)
    h, w = max(1, round(H * r)), max(1, round(W * r))
    ch, cw = min(crop[0], h), min(crop[1], w)
    return AugmentParams(flip, (h, w), (int((h - ch) * frac[0]), int((w - cw) * frac[1])), (ch, cw))


def _inputs(seed, H, W, n_ids=12):
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    m = R.blocky_map(rng, H, W, n_ids)
    return im, m, {int(i): int(i) % 3 for i in np.unique(m)}


# ------------------------------------------------------------------------------------------------ the Pillow fixture
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_pillow_fixture_through_the_processor(proc, case):
    out = proc.preprocess(case["images"], case["maps"], case["id2sem"], augment=case["params"],
                          pad_size=case["pad_size"], ignore_index=IG)
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    _assert_equal(out, (T(case["pixel_values"]), T(case["pixel_mask"]), [T(a) for a in case["mask_labels"]],
                        [T(a) for a in case["class_labels"]]))


# ------------------------------------------------------------------------------------------------ the composed route
@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("f", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("hw", [(1024, 1024), (966, 1296)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_jitter_equals_composed_route(proc, hw, f, mask_dtype):
    crop, pad = (1024, 1024), {"height": 1024, "width": 1024}
    im, m, d = _inputs(31 + int(f * 10), *hw)
    for flip, frac in [(0, (0.3, 0.7)), (1, (1.0, 0.0))]:
        p = [_jitter(*hw, f, crop, flip, frac)]
        out = proc.preprocess([im], [m], d, augment=p, pad_size=pad, ignore_index=IG, mask_dtype=mask_dtype)
        _assert_equal(out, composed(proc, [im], [m], d, p, pad, mask_dtype))


def test_short_edge_list_equals_composed_route(proc):
    """Every entry of the COCO-style list at 800 x 1333, as one batch of mixed sizes padded to the largest."""
    im, m, d = _inputs(41, 800, 1333)
    params = [AugmentParams(i % 2, P.output_size(800, 1333, {"shortest_edge": e, "longest_edge": 1333}, 32))
              for i, e in enumerate(EDGES)]
    assert len({p.size for p in params}) > 1
    B = len(params)
    out = proc.preprocess([im] * B, [m] * B, d, augment=params, ignore_index=IG)
    _assert_equal(out, composed(proc, [im] * B, [m] * B, d, params))


@pytest.mark.parametrize("B", [1, 8])
def test_mixed_batches_equal_composed_route(proc, B):
    sizes = [(1024, 1024), (966, 1296), (480, 640), (333, 1000), (700, 1500), (61, 75), (1024, 819), (512, 513)][:B]
    aug = TrainAugmentation(scale=(0.3, 2.0), crop_size=(640, 768))
    g = torch.Generator().manual_seed(11)
    ims, maps, ds, params = [], [], [], []
    for i, (H, W) in enumerate(sizes):
        im, m, d = _inputs(50 + i, H, W)
        ims.append(im), maps.append(m), ds.append(d), params.append(aug.sample(H, W, g))
    for mask_dtype in (torch.float32, torch.uint8):
        out = proc.preprocess(ims, maps, ds, augment=params, pad_size=aug.pad_size, ignore_index=IG, mask_dtype=mask_dtype)
        assert out["pixel_values"].shape == (B, 3, 640, 768)
        _assert_equal(out, composed(proc, ims, maps, ds, params, aug.pad_size, mask_dtype))
    out = proc.preprocess(ims, augment=params, pad_size=aug.pad_size)  # images only
    _assert_equal(out, composed(proc, ims, None, None, params, aug.pad_size), with_maps=False)


def test_heavy_downscale_takes_several_row_rounds(proc):
    """1 / 12: a 16-row tile reaches more than 64 source rows, so the kernel's row loop runs more than once."""
    im, m, d = _inputs(61, 1500, 1400)
    p = [AugmentParams(1, (125, 117), (20, 10), (100, 101))]
    _assert_equal(proc.preprocess([im], [m], d, augment=p, ignore_index=IG), composed(proc, [im], [m], d, p))


def test_crop_removes_an_instance_and_can_leave_none(proc):
    im = np.random.default_rng(71).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    m = np.full((256, 256), IG, np.uint8)
    m[10:40, 10:40] = 1      # left of the window after the flip: removed
    m[100:200, 180:250] = 2  # cut by the window: stays one instance
    d = {1: 0, 2: 1, IG: 2}
    # flipped and doubled, instance 2 covers rows 200..399 and columns 12..151 of the frame: the window cuts it at 100
    p = [AugmentParams(1, (512, 512), (100, 0), (300, 100))]
    out = proc.preprocess([im], [m], d, augment=p, ignore_index=IG)
    assert out["class_labels"][0].tolist() == [1] and out["mask_labels"][0].shape == (1, 300, 100)
    assert float(out["mask_labels"][0].sum()) == 200 * 88 < 4 * 100 * 70
    _assert_equal(out, composed(proc, [im], [m], d, p))
    pad = {"height": 64, "width": 96}
    q = [AugmentParams(0, (256, 256), (60, 60), (30, 90))]  # between the two instances
    out = proc.preprocess([im], [m], d, augment=q, pad_size=pad, ignore_index=IG, mask_dtype=torch.uint8)
    assert out["mask_labels"][0].shape == (0, 64, 96) and out["mask_labels"][0].dtype == torch.uint8
    assert out["class_labels"][0].shape == (0,)
    _assert_equal(out, composed(proc, [im], [m], d, q, pad, torch.uint8))
    with pytest.raises(ValueError):  # padding mask_labels without ignore_index, as in the un-augmented call
        proc.preprocess([im], [m], d, augment=q, pad_size=pad)


def test_device_tensors_as_inputs(proc):
    im, m, d = _inputs(81, 300, 401)
    p = [_jitter(300, 401, 1.3, (256, 256), 1)]
    pad = {"height": 256, "width": 256}
    exp = composed(proc, [im], [m], d, p, pad)
    out = proc.preprocess([torch.from_numpy(im).cuda()], [torch.from_numpy(m).cuda()], d, augment=p, pad_size=pad,
                          ignore_index=IG)
    _assert_equal(out, exp)


def _restated(images, maps, id2sem, params, pad_size=None):
    """The numpy restatement of the contract (augment_reference.restate) as device tensors."""
    pv, pm, ml, cl = R.restate(images, maps, id2sem, params, pad_size, IG)
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return T(pv), T(pm), [T(a) for a in ml], [T(a) for a in cl]


def test_identity_parameters_equal_the_unaugmented_call(proc):
    """The two routes share their host rows and differ in the kernels the dispatch picks; the numpy restatement is the
    expectation both are held to, so the equalities do not rest on either kernel."""
    im, m, d = _inputs(91, 333, 500)
    kw = dict(size={"height": 416, "width": 640}, size_divisor=0, ignore_index=IG)
    base = proc.preprocess([im], [m], d, **kw)
    _assert_equal(base, _restated([im], [m], d, [AugmentParams.identity(416, 640)]))
    out = proc.preprocess([im], [m], d, augment=AugmentParams.identity(416, 640), ignore_index=IG)
    _assert_equal(out, (base["pixel_values"], base["pixel_mask"], base["mask_labels"], base["class_labels"]))
    none = proc.preprocess([im], [m], d, augment=None, **kw)  # bit-identical to a call without the keyword
    _assert_equal(none, (base["pixel_values"], base["pixel_mask"], base["mask_labels"], base["class_labels"]))


# ------------------------------------------------------------------------------------------------ every kernel branch
# source (H, W), flip, frame, origin, window, pad: the smallest shapes that reach each branch of the two kernels
BRANCH_CASES = [
    # upscale, 3 row tiles x 3 column tiles, Wp % 4 = 2 (scalar stores), padding rows and columns
    ("upscale_scalar_stores", (37, 150), 0, (61, 391), (3, 5), (45, 263), {"height": 48, "width": 270}),
    ("upscale_mirrored_vector_stores", (37, 150), 1, (61, 391), (3, 5), (45, 263), {"height": 48, "width": 272}),
    # 7 column taps (coefficients read from the table), a 16-row tile reaching 297 source rows (5 rounds of 64), and
    # a last tile of one round
    ("table_taps_five_rounds_mirrored", (700, 520), 1, (40, 150), (5, 7), (33, 140), None),
    ("identity_window", (700, 520), 0, (40, 150), (0, 0), (40, 150), None),  # what a plain call fills in
]


@pytest.mark.parametrize("case", BRANCH_CASES, ids=lambda c: c[0])
def test_every_kernel_branch_equals_the_restatement(proc, case):
    _, hw, flip, frame, origin, window, pad = case
    im, m, d = _inputs(95, *hw)
    p = [AugmentParams(flip, frame, origin, window)]
    out = proc.preprocess([im], [m], d, augment=p, pad_size=pad, ignore_index=IG)
    _assert_equal(out, _restated([im], [m], d, p, pad))


def test_plain_call_with_several_row_rounds_equals_its_own_restatement(proc):
    """The identity case above without `augment`, against the restatement of DESIGN section 12."""
    from test_preprocess_cpu import restate
    im, m, d = _inputs(95, 700, 520)
    kw = dict(size={"height": 40, "width": 150}, size_divisor=0, ignore_index=IG)
    pv, pm, ml, cl = restate([im], [m], d, **kw)
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    _assert_equal(proc.preprocess([im], [m], d, **kw), (T(pv), T(pm), [T(a) for a in ml], [T(a) for a in cl]))


def test_kernel_rejects_what_it_does_not_build(proc):
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    img = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device="cuda")
    tab = torch.zeros(64, dtype=torch.int32, device="cuda")
    lut = torch.zeros(768, device="cuda")
    row = [0, 8, 8, 8, 8, 0, 0, 1, 0, 0, 1, 0, 0, 0, 8, 8]
    with pytest.raises(Wm2fError, match="outside"):  # window outside its frame
        ops.augment_resize_normalize_u8(img, np.array([row[:12] + [4, 0, 8, 8]]), tab, lut, 8, 8)
    with pytest.raises(Wm2fError, match="exceeds"):  # virtual frame above WM2F_AUG_MAX_VIRTUAL
        ops.augment_resize_normalize_u8(img, np.array([row[:3] + [70000, 8] + row[5:]]), tab, lut, 8, 8)
    with pytest.raises(Wm2fError, match="flip"):
        ops.augment_nearest_labels(img[:64], np.array([[0, 8, 8, 8, 8, 0, 0, 2, 0, 0, 8, 8]]), tab, 8, 8, IG)


# ------------------------------------------------------------------------------------------------ datasets
def _pheno_folder(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(21)
    (tmp_path / "img").mkdir()
    (tmp_path / "ann").mkdir()
    for i, (H, W) in enumerate([(200, 260), (231, 180)]):
        Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(str(tmp_path / "img" / f"t{i}.png"))
        coarse = (rng.random((H // 24 + 1, W // 24 + 1)) < 0.35) * rng.integers(1, 3, (H // 24 + 1, W // 24 + 1))
        sem = np.ascontiguousarray(np.kron(coarse, np.ones((24, 24)))[:H, :W].astype(np.uint16))
        Image.fromarray(sem).save(str(tmp_path / "ann" / f"t{i}.png"))
    return str(tmp_path / "img"), str(tmp_path / "ann")


def test_pheno_bench_dataset_with_augmentation(proc, tmp_path):
    from PIL import Image
    from weed_instance_segmentation_amd.annotations import PhenoBenchDataset
    img_dir, ann_dir = _pheno_folder(tmp_path)
    aug = TrainAugmentation(scale=(0.5, 2.0), crop_size=(128, 160))
    gen = lambda s: torch.Generator().manual_seed(s)  # noqa: E731
    plain = PhenoBenchDataset(img_dir, ann_dir, proc, {})
    a = PhenoBenchDataset(img_dir, ann_dir, proc, {}, augment=aug, generator=gen(3))
    b = PhenoBenchDataset(img_dir, ann_dir, proc, {}, augment=aug, generator=gen(3))
    c = PhenoBenchDataset(img_dir, ann_dir, proc, {}, augment=aug, generator=gen(4))
    replay = gen(3)
    differs = False
    for i in range(2):
        base, ia, ib, ic = plain[i], a[i], b[i], c[i]
        assert "augment" not in base and base["target_size"] == base["original_map"].shape
        p = ia["augment"]
        assert p == aug.sample(*base["original_map"].shape, replay) == ib["augment"]
        differs |= ic["augment"] != p
        assert ia["target_size"] == p.window and ia["pixel_values"].shape == (3, 128, 160)
        assert np.array_equal(ia["original_map"], base["original_map"]) and ia["id_to_semantic"] == base["id_to_semantic"]
        for k in ("pixel_values", "mask_labels", "class_labels"):
            assert torch.equal(ia[k], ib[k])
        image = np.asarray(Image.open(a.valid_files[i][0]).convert("RGB"))
        pv, pm, ml, cl = composed(proc, [image], [base["original_map"]], base["id_to_semantic"], [p], aug.pad_size)
        assert torch.equal(ia["pixel_values"], pv[0]) and torch.equal(ia["mask_labels"], ml[0])
        assert torch.equal(ia["class_labels"], cl[0])
    assert differs, "another seed draws another window"


# ------------------------------------------------------------------------------------------------ a train step
def test_tiny_model_trains_on_an_augmented_batch(proc):
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    g = load_golden("full_tiny.npz")
    cfg = Mask2FormerConfig.from_dict(json.loads(str(g["config_json"])))
    torch.manual_seed(0)
    model = Mask2FormerForUniversalSegmentation(cfg).cuda().train()
    aug = TrainAugmentation(scale=(0.5, 2.0), crop_size=(64, 96))
    gen = torch.Generator().manual_seed(5)
    ims, maps, ds = [], [], []
    for i, (H, W) in enumerate([(80, 100), (70, 131)]):
        im, m, _ = _inputs(100 + i, H, W, n_ids=4)
        ims.append(im), maps.append(m), ds.append({int(k): int(k) % cfg.num_labels for k in np.unique(m)})
    params = [aug.sample(im.shape[0], im.shape[1], gen) for im in ims]

    def step(batch):
        model.zero_grad(set_to_none=True)
        out = model(pixel_values=batch["pixel_values"], mask_labels=batch["mask_labels"],
                    class_labels=batch["class_labels"])
        out.loss.backward()
        return out.loss, {n for n, q in model.named_parameters() if q.grad is not None}

    _, plain = step(proc.preprocess(ims, maps, ds, size={"height": 64, "width": 96}, size_divisor=0, ignore_index=IG))
    loss, augmented = step(proc.preprocess(ims, maps, ds, augment=params, pad_size=aug.pad_size, ignore_index=IG))
    assert torch.isfinite(loss).item()
    assert len(plain) > 100 and plain <= augmented
    assert all(torch.isfinite(q.grad).all() for q in model.parameters() if q.grad is not None)
