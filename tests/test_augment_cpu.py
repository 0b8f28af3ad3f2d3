"""Host side of the training augmentation, no GPU: the parameter draws, the value object, and the
numpy restatement of the contract (tests/augment_reference.py) held to Pillow itself and to the dependency's fixture."""
import json

import numpy as np
import pytest
import torch

import augment_reference as R
from conftest import load_golden
from weed_instance_segmentation_amd import preprocess as P
from weed_instance_segmentation_amd.augment import AugmentParams, TrainAugmentation

SIZES = [(1024, 1024), (966, 1296), (480, 640), (333, 1000), (1500, 700)]
EDGES = tuple(range(640, 801, 32))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_package_exports():
    import weed_instance_segmentation_amd as pkg
    assert pkg.AugmentParams is AugmentParams and pkg.TrainAugmentation is TrainAugmentation


@pytest.mark.parametrize("aug", [TrainAugmentation(short_edge=EDGES, max_size=1333),
                                 TrainAugmentation(scale=(0.1, 2.0), crop_size=(1024, 1024))], ids=["edge", "jitter"])
def test_same_seed_same_parameters(aug):
    a = [aug.sample(966, 1296, g) for g in [_gen(7)] for _ in range(20)]
    b = [aug.sample(966, 1296, g) for g in [_gen(7)] for _ in range(20)]
    c = [aug.sample(966, 1296, g) for g in [_gen(8)] for _ in range(20)]
    assert a == b and a != c


def test_draws_are_pinned():
    """The documented order (flip, scale or edge, y0, x0) on torch's CPU Mersenne twister: fixed values for a seed."""
    g = _gen(0)
    flip = int(torch.rand(1, generator=g).item() < 0.5)
    f = 0.5 + 1.5 * float(torch.rand(1, dtype=torch.float64, generator=g).item())
    r = min(64 * f / 100, 64 * f / 80)
    h, w = max(1, round(100 * r)), max(1, round(80 * r))
    ch, cw = min(64, h), min(64, w)
    y0 = int(torch.randint(h - ch + 1, (1,), generator=g).item())
    x0 = int(torch.randint(w - cw + 1, (1,), generator=g).item())
    p = TrainAugmentation(scale=(0.5, 2.0), crop_size=(64, 64)).sample(100, 80, _gen(0))
    assert p == AugmentParams(flip, (h, w), (y0, x0), (ch, cw))


def test_short_edge_draws():
    aug = TrainAugmentation(short_edge=EDGES, max_size=1333, size_divisor=32)
    g = _gen(1)
    flips, seen = set(), set()
    for H, W in SIZES:
        allowed = {P.output_size(H, W, {"shortest_edge": e, "longest_edge": 1333}, 32) for e in EDGES}
        for _ in range(200):
            p = aug.sample(H, W, g)
            assert p.size in allowed and p.window == p.size and p.origin == (0, 0)
            flips.add(p.flip)
            if (H, W) == (480, 640):
                seen.add(p.size)
    assert flips == {0, 1}
    # both ends of the edge list are reached (480 x 640 keeps its aspect below max_size, so the edge shows in h)
    assert P.output_size(480, 640, {"shortest_edge": 640, "longest_edge": 1333}, 32) in seen
    assert P.output_size(480, 640, {"shortest_edge": 800, "longest_edge": 1333}, 32) in seen
    assert aug.pad_size is None


def test_jitter_draws():
    lo, hi, C = 0.1, 2.0, (1024, 1024)
    aug = TrainAugmentation(scale=(lo, hi), crop_size=C)
    g = _gen(2)
    flips, fs = set(), []
    for H, W in SIZES:
        for _ in range(200):
            p = aug.sample(H, W, g)
            (h, w), (y0, x0), (ch, cw) = p.size, p.origin, p.window
            assert 0 <= y0 and 0 <= x0 and y0 + ch <= h and x0 + cw <= w
            assert (ch, cw) == (min(C[0], h), min(C[1], w))
            flips.add(p.flip)
            fs.append(max(h / C[0], w / C[1]))  # = f up to the rounding of one pixel
    assert flips == {0, 1}
    hist, _ = np.histogram(fs, bins=20, range=(lo - 1e-3, hi + 1e-3))
    assert hist[0] > 0 and hist[-1] > 0, "the extreme scales are reached within one of 20 bins of the ends"
    assert min(fs) >= lo - 1e-3 and max(fs) <= hi + 1e-3
    assert aug.pad_size == {"height": 1024, "width": 1024}


def test_flip_probability_ends():
    assert {TrainAugmentation(short_edge=(64,), flip_prob=0.0).sample(50, 60, _gen(s)).flip for s in range(30)} == {0}
    assert {TrainAugmentation(short_edge=(64,), flip_prob=1.0).sample(50, 60, _gen(s)).flip for s in range(30)} == {1}


@pytest.mark.parametrize("kw", [dict(flip=0, size=(10, 10), origin=(0, 0), window=(11, 10)),
                                dict(flip=0, size=(10, 10), origin=(5, 0), window=(6, 10)),
                                dict(flip=0, size=(10, 10), origin=(0, -1), window=(5, 5)),
                                dict(flip=0, size=(0, 10)), dict(flip=0, size=(10, -3)),
                                dict(flip=0, size=(10, 10), window=(0, 5)), dict(flip=2, size=(10, 10)),
                                dict(flip=0, size=(10.5, 10))])
def test_params_validation(kw):
    with pytest.raises(ValueError):
        AugmentParams(**kw)


def test_params_defaults_and_recipe_validation():
    p = AugmentParams(True, (10, 12))
    assert (p.flip, p.size, p.origin, p.window) == (1, (10, 12), (0, 0), (10, 12))
    assert AugmentParams.identity(10, 12) == AugmentParams(0, (10, 12), (0, 0), (10, 12))
    for bad in (dict(), dict(short_edge=(640,), scale=(0.5, 1.0), crop_size=(8, 8)), dict(scale=(0.5, 1.0)),
                dict(scale=(1.0, 0.5), crop_size=(8, 8)), dict(short_edge=(640,), crop_size=(8, 8)),
                dict(short_edge=(), max_size=100), dict(short_edge=(640,), flip_prob=1.5)):
        with pytest.raises(ValueError):
            TrainAugmentation(**bad)


def test_nearest_table_is_not_mirror_symmetric():
    """Why the flip is applied to the source: mirroring the output of Pillow's nearest resize is another function."""
    for a, b in [(1000, 333), (1024, 819), (966, 1333), (1024, 1331)]:
        t = P.nearest_table(a, b)
        assert not np.array_equal((a - 1 - t)[::-1], t)


def _grid():
    """Both flips x ratios about 0.3, 0.8, 1.3, 2.0 x odd and even sides x windows at the four corners and inside."""
    out = []
    for H, W in [(64, 90), (61, 75)]:
        for ratio in (0.3, 0.8, 1.3, 2.0):
            h, w = max(2, int(round(H * ratio))), max(2, int(round(W * ratio)) + 1)
            ch, cw = max(1, h // 2), max(1, w // 2 + 1)
            for flip in (0, 1):
                for y0, x0 in [(0, 0), (0, w - cw), (h - ch, 0), (h - ch, w - cw), ((h - ch) // 2, (w - cw) // 3)]:
                    out.append((H, W, AugmentParams(flip, (h, w), (y0, x0), (ch, cw))))
    return out


@pytest.mark.parametrize("H,W,p", _grid(), ids=lambda v: None if isinstance(v, int) else f"f{v.flip}-{v.size}-{v.origin}")
def test_restatement_equals_pillow(H, W, p):
    rng = np.random.default_rng(H * 1000 + W + p.size[0])
    im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    m = R.blocky_map(rng, H, W, 6)
    assert np.array_equal(R.image_window(im, p), R.pil_image_window(im, p))
    assert np.array_equal(R.map_window(m, p), R.pil_map_window(m, p))


def test_restatement_equals_pillow_at_an_asymmetric_nearest_size():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 200, (7, 1000), dtype=np.uint8)
    p = AugmentParams(1, (7, 333), (0, 100), (7, 233))
    assert np.array_equal(R.map_window(m, p), R.pil_map_window(m, p))
    im = rng.integers(0, 256, (5, 1000, 3), dtype=np.uint8)
    q = AugmentParams(1, (5, 333), (0, 3), (5, 330))
    assert np.array_equal(R.image_window(im, q), R.pil_image_window(im, q))


def test_identity_parameters_equal_the_dependency_fixture():
    """flip = 0 and a whole-frame window through the restatement give the dependency's PIL processor outputs."""
    g = load_golden("preprocess_pil.npz")
    for name in ("downscale_3x_lost_id", "upscale_stretch"):
        kw = json.loads(str(g[f"{name}.kwargs"]))
        im, m = g[f"{name}.img0"], g[f"{name}.map0"]
        id2sem = [{int(k): v for k, v in d.items()} for d in json.loads(str(g[f"{name}.id2sem"]))]
        h, w = P.output_size(im.shape[0], im.shape[1], kw["size"], kw.get("size_divisor", 32))
        pv, pm, ml, cl = R.restate([im], [m], id2sem, [AugmentParams.identity(h, w)], None, kw["ignore_index"])
        assert np.array_equal(pv, g[f"{name}.pixel_values"]) and pv.dtype == np.float32
        assert np.array_equal(pm, g[f"{name}.pixel_mask"])
        assert np.array_equal(ml[0], g[f"{name}.mask_labels0"]) and np.array_equal(cl[0], g[f"{name}.class_labels0"])


def golden_cases():
    g = load_golden("augment_pil.npz")
    out = []
    for name in json.loads(str(g["cases"])):
        rows = json.loads(str(g[f"{name}.params"]))
        B = len(rows)
        out.append(dict(
            name=name, images=[g[f"{name}.img{b}"] for b in range(B)], maps=[g[f"{name}.map{b}"] for b in range(B)],
            params=[AugmentParams(r[0], (r[1], r[2]), (r[3], r[4]), (r[5], r[6])) for r in rows],
            pad_size=json.loads(str(g[f"{name}.pad_size"])),
            id2sem=[{int(k): v for k, v in d.items()} for d in json.loads(str(g[f"{name}.id2sem"]))],
            pixel_values=g[f"{name}.pixel_values"], pixel_mask=g[f"{name}.pixel_mask"],
            mask_labels=[g[f"{name}.mask_labels{b}"] for b in range(B)],
            class_labels=[g[f"{name}.class_labels{b}"] for b in range(B)]))
    return out


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_equals_the_pillow_fixture(case):
    pv, pm, ml, cl = R.restate(case["images"], case["maps"], case["id2sem"], case["params"], case["pad_size"], 255)
    assert np.array_equal(pv, case["pixel_values"]) and np.array_equal(pm, case["pixel_mask"])
    for b in range(len(case["images"])):
        assert ml[b].shape == case["mask_labels"][b].shape and np.array_equal(ml[b], case["mask_labels"][b])
        assert np.array_equal(cl[b], case["class_labels"][b])


def test_fixture_covers_the_grid():
    cases = golden_cases()
    assert len(cases) >= 12
    assert {p.flip for c in cases for p in c["params"]} == {0, 1}
    assert any(len(c["class_labels"][0]) == 0 for c in cases), "a window that leaves no instance"
    assert any(len(np.unique(c["maps"][0])) - 1 > len(c["class_labels"][0]) > 0 for c in cases), "a crop loses an instance"
    assert any(c["pad_size"] for c in cases)


def test_processor_rejects_bad_augment_arguments():
    from weed_instance_segmentation_amd.preprocess import Mask2FormerImageProcessor
    proc = Mask2FormerImageProcessor()
    im = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="augment"):
        proc.preprocess([im, im], augment=[AugmentParams.identity(8, 8)])
    with pytest.raises(ValueError, match="augment"):
        proc.preprocess([im], augment=[(0, 8, 8)])
    with pytest.raises(ValueError, match="do_resize"):
        proc.preprocess([im], augment=AugmentParams.identity(8, 8), do_resize=False)
