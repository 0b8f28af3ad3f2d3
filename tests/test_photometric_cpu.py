"""Host side of the colour jitter, no GPU: the numpy restatement of the contract
(tests/photometric_reference.py) held to Pillow itself and to the fixture, the value objects, the draws."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import photometric_reference as R
from conftest import load_golden
from weed_instance_segmentation_amd.augment import AugmentParams, PhotometricParams, TrainAugmentation

B, C, S, H = R.KINDS
GRID_D, GRID_V = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def all_colours() -> np.ndarray:
    """Every RGB triple once, as a 4096 x 4096 image."""
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def golden_cases():
    g = load_golden("photometric_pil.npz")
    out = []
    for name in json.loads(str(g["cases"])):
        chains = [tuple((k, v) for k, v in ops) for ops in json.loads(str(g[f"{name}.ops"]))]
        n = len(chains)
        out.append(dict(name=name, chains=chains, images=[g[f"{name}.img{b}"] for b in range(n)],
                        outs=[g[f"{name}.out{b}"] for b in range(n)], raw=g))
    return out


def test_package_exports():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import augment, ops
    assert pkg.PhotometricParams is PhotometricParams and pkg.adjust_colors is augment.adjust_colors
    assert callable(ops.photometric_u8)


# ------------------------------------------------------------------------------------------------ the blend
def test_blend_grid_equals_pillow():
    """All 65 536 (d, v) pairs at the factors where a fused multiply-add gives other bytes, at 0, 1, 0.5, 2 and at random
    factors.  At every discriminating factor the fused variant must differ from Pillow, or the list is wrong."""
    d_im, v_im = Image.fromarray(GRID_D), Image.fromarray(GRID_V)
    rng = np.random.default_rng(3)
    factors = list(R.DISCRIMINATING) + [0.0, 1.0, 0.5, 2.0] + [float(f) for f in rng.uniform(0.02, 2.5, 40)]
    for f in factors:
        pil = np.asarray(Image.blend(d_im, v_im, f))
        assert np.array_equal(R.blend(GRID_D, GRID_V, f), pil), f
        if f in R.DISCRIMINATING:
            assert (R.blend(GRID_D, GRID_V, f, fused=True) != pil).any(), f


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (5, 7), (33, 47), (31, 130)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("kind", [B, C, S])
def test_enhancers_equal_pillow(kind, hw):
    rng = np.random.default_rng(hw[0] * 131 + hw[1])
    im = rng.integers(0, 256, (*hw, 3), dtype=np.uint8)
    for f in (0.0, 0.3, 0.6, 1.0, 1.2, 1.7, 2.5):
        assert np.array_equal(R.apply(im, ((kind, f),)), R.pil_apply(im, ((kind, f),))), f


def test_contrast_mean_rounds_a_half_up():
    """Two grey pixels 10 and 11: L is 10 and 11, the mean 10.5, and int(10.5 + 0.5) = 11."""
    im = np.array([[[10, 10, 10], [11, 11, 11]]], dtype=np.uint8)
    assert R.luma(im).tolist() == [[10, 11]] and R.contrast_mean(im) == 11
    for f in (0.0, 0.6, 1.7):
        assert np.array_equal(R.contrast(im, f), R.pil_apply(im, ((C, f),)))
    assert R.contrast(im, 0.0).tolist() == [[[11] * 3, [11] * 3]]


CHAIN = ((B, 1.2), (S, 0.6), (H, -0.1), (C, 1.6))


def contrast_positions():
    """The four-step chain with contrast at each position: the mean is the one of the image the steps before it made."""
    rest = [s for s in CHAIN if s[0] != C]
    return [tuple(rest[:i] + [CHAIN[3]] + rest[i:]) for i in range(4)]


@pytest.mark.parametrize("ops", contrast_positions(), ids=lambda o: "-".join(k[0] for k, _ in o))
def test_contrast_at_each_position_of_a_chain(ops):
    im = np.random.default_rng(17).integers(0, 200, (23, 41, 3), dtype=np.uint8)
    assert np.array_equal(R.apply(im, ops), R.pil_apply(im, ops))
    at = [k for k, _ in ops].index(C)
    if at:
        assert R.contrast_mean(R.apply(im, ops[:at])) != R.contrast_mean(im), "the prefix moves the mean"


# ------------------------------------------------------------------------------------------------ hsv
def test_hsv_conversions_equal_pillow_over_all_colours():
    """Both conversions over all 2^24 inputs as one 4096 x 4096 image (a few seconds each in numpy)."""
    rgb = all_colours()
    assert np.array_equal(R.rgb_to_hsv(rgb), np.asarray(Image.fromarray(rgb).convert("HSV")))
    hsv = Image.frombuffer("HSV", (4096, 4096), rgb.tobytes(), "raw", "HSV", 0, 1)
    assert np.array_equal(R.hsv_to_rgb(rgb), np.asarray(hsv.convert("RGB")))


def _pil_hue(im, dh):
    h, s, v = Image.fromarray(im).convert("HSV").split()
    return np.asarray(Image.merge("HSV", (h.point(lambda x: (x + dh) % 256), s, v)).convert("RGB"))


def test_hue_step():
    im = np.random.default_rng(23).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for dh in (0, 1, 127, 128, 255):
        assert np.array_equal(R.hue(im, dh), _pil_hue(im, dh)), dh
    assert not np.array_equal(R.hue(im, 0), im), "dh = 0 still goes through HSV and changes pixels"
    for s, dh in [(0.0, 0), (0.004, 1), (0.5, 127), (-0.004, 255), (-0.03, 249), (-0.5, 129)]:
        assert R.hue_dh(s) == dh == PhotometricParams(((H, s),)).hue_byte()
        assert np.array_equal(R.apply(im, ((H, s),)), _pil_hue(im, dh))
        assert np.array_equal(R.apply(im, ((H, s),)), R.pil_apply(im, ((H, s),)))


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_equals_the_pillow_fixture(case):
    for im, ops, out in zip(case["images"], case["chains"], case["outs"]):
        assert np.array_equal(R.apply(im, ops), out)


def test_fixture_covers_the_ground():
    cases = golden_cases()
    assert len(cases) >= 12
    chains = [ops for c in cases for ops in c["chains"]]
    assert {len(ops) for ops in chains} == {0, 1, 2, 3, 4}
    assert {k for ops in chains for k, _ in ops} == set(R.KINDS)
    assert set(R.DISCRIMINATING) <= {v for ops in chains for k, v in ops if k != H}
    orders = {tuple(k for k, _ in ops) for ops in chains if len(ops) == 4}
    assert len(orders) >= 2
    assert any(im.shape[1] % 2 for c in cases for im in c["images"])
    assert all(max(im.shape[:2]) <= 96 for c in cases for im in c["images"])
    assert any(f"{c['name']}.pixel_values" in c["raw"] for c in cases), "one case composed with the geometry"
    fused = [not np.array_equal(R.apply(im, ops, fused=True), out)
             for c in cases for im, ops, out in zip(c["images"], c["chains"], c["outs"])]
    assert sum(fused) >= 6, "most cases tell a fused blend from Pillow's"


# ------------------------------------------------------------------------------------------------ value objects
def test_params_normalise_and_expose_float32():
    p = PhotometricParams([[B, 1.2], [H, -0.03]])
    assert p.ops == ((B, 1.2), (H, -0.03)) and p == PhotometricParams(((B, 1.2), (H, -0.03)))
    assert p.factor32(B) == float(np.float32(1.2)) != 1.2
    assert p.hue_byte() == 249
    assert p.desc_row(9, 4, 5) == [9, 4, 5, 2, 0, int(np.float32(1.2).view(np.uint32)), 3, 249, 0, 0, 0, 0]
    assert PhotometricParams().ops == () and PhotometricParams().desc_row(0, 1, 1)[3] == 0
    with pytest.raises(KeyError):
        p.factor32(C)
    with pytest.raises(ValueError):
        p.factor32(H)


@pytest.mark.parametrize("ops", [((B, -0.1),), ((B, float("nan")),), ((C, float("inf")),), ((S, 1e39),), ((H, 0.51),),
                                 ((H, -0.6),), ((B, 1.0), (B, 1.1)), (("gamma", 1.0),), ((B,),), 5, ((B, "1"),),
                                 ((B, True),), ((B, 1), (C, 1), (S, 1), (H, 0), (B, 2))])
def test_params_validation(ops):
    with pytest.raises(ValueError):
        PhotometricParams(ops)


def test_augment_params_keep_their_meaning():
    assert AugmentParams(1, (8, 9)).photometric is None
    assert AugmentParams(1, (8, 9)) == AugmentParams(1, (8, 9), (0, 0), (8, 9), None)
    assert AugmentParams.identity(8, 9) == AugmentParams(0, (8, 9))
    p = PhotometricParams(((B, 1.1),))
    assert AugmentParams(0, (8, 9), photometric=p) != AugmentParams(0, (8, 9))
    assert AugmentParams(0, (8, 9), photometric=p).photometric is p
    with pytest.raises(ValueError):
        AugmentParams(0, (8, 9), photometric=((B, 1.1),))


@pytest.mark.parametrize("kw", [dict(brightness=-0.1), dict(contrast=(1.2, 0.8)), dict(saturation=(-0.1, 1.0)),
                                dict(hue=0.6), dict(hue=(-0.6, 0.1)), dict(brightness="x"), dict(contrast=(1, 2, 3)),
                                dict(brightness=float("nan"))])
def test_recipe_validation(kw):
    with pytest.raises(ValueError):
        TrainAugmentation(short_edge=(64,), **kw)


def test_colour_ranges():
    aug = TrainAugmentation(short_edge=(64,), brightness=0.2, contrast=1.5, saturation=(0.5, 3.0), hue=0.05)
    assert aug.color_ranges == ((0.8, 1.2), (0.0, 2.5), (0.5, 3.0), (-0.05, 0.05))
    assert TrainAugmentation(short_edge=(64,), hue=(-0.5, 0.25)).color_ranges == (None, None, None, (-0.5, 0.25))
    assert TrainAugmentation(short_edge=(64,)).color_ranges == (None,) * 4


# ------------------------------------------------------------------------------------------------ draws
RECIPES = [dict(short_edge=tuple(range(640, 801, 32)), max_size=1333), dict(scale=(0.1, 2.0), crop_size=(1024, 1024))]
COLOURS = dict(brightness=0.4, contrast=(0.5, 1.5), saturation=0.3, hue=0.1)


@pytest.mark.parametrize("recipe", RECIPES, ids=["edge", "jitter"])
def test_same_seed_same_geometry_with_and_without_colour(recipe):
    plain, colour = TrainAugmentation(**recipe), TrainAugmentation(**recipe, **COLOURS)
    for seed in range(20):
        a, b = plain.sample(966, 1296, _gen(seed)), colour.sample(966, 1296, _gen(seed))
        assert a.photometric is None and b.photometric is not None
        assert (a.flip, a.size, a.origin, a.window) == (b.flip, b.size, b.origin, b.window)
        assert b == colour.sample(966, 1296, _gen(seed))


def test_draw_count_and_order_are_fixed():
    """Without colour arguments: the four draws of section 20 and no more.  With any: one randperm(4) and four float64
    uniforms after them, whichever kinds are on -- the generator ends in the same state, and the values are pinned."""
    recipe = dict(scale=(0.5, 2.0), crop_size=(64, 64))

    g, ref = _gen(5), _gen(5)
    p = TrainAugmentation(**recipe).sample(100, 80, g)
    torch.rand(1, generator=ref)  # flip, f, y0, x0
    torch.rand(1, dtype=torch.float64, generator=ref)
    torch.randint(p.size[0] - p.window[0] + 1, (1,), generator=ref)
    torch.randint(p.size[1] - p.window[1] + 1, (1,), generator=ref)
    assert torch.equal(g.get_state(), ref.get_state())

    order = torch.randperm(4, generator=ref).tolist()
    u = [float(torch.rand(1, dtype=torch.float64, generator=ref).item()) for _ in range(4)]
    ranges = dict(zip(R.KINDS, ((0.6, 1.4), (0.5, 1.5), (0.7, 1.3), (-0.1, 0.1))))
    states = []
    for on in [R.KINDS, (C,), (H, B), (S, C, B)]:
        g = _gen(5)
        p = TrainAugmentation(**recipe, **{k: COLOURS[k] for k in on}).sample(100, 80, g).photometric
        states.append(g.get_state())
        want = [(R.KINDS[k], ranges[R.KINDS[k]][0] + (ranges[R.KINDS[k]][1] - ranges[R.KINDS[k]][0]) * u[k])
                for k in order if R.KINDS[k] in on]
        assert p.ops == tuple(want), "a disabled kind is absent; the others keep the permutation's order"
    assert all(torch.equal(s, ref.get_state()) for s in states)


def test_factors_lie_in_their_ranges_and_orders_vary():
    aug = TrainAugmentation(short_edge=(64,), **COLOURS)
    g = _gen(9)
    lo_hi = dict(zip(R.KINDS, aug.color_ranges))
    orders, seen = set(), {k: [] for k in R.KINDS}
    for _ in range(300):
        p = aug.sample(50, 60, g).photometric
        orders.add(tuple(k for k, _ in p.ops))
        assert sorted(k for k, _ in p.ops) == sorted(R.KINDS)
        for k, v in p.ops:
            assert lo_hi[k][0] <= v <= lo_hi[k][1]
            seen[k].append(v)
    assert len(orders) == 24
    for k, (lo, hi) in lo_hi.items():
        assert min(seen[k]) < lo + 0.1 * (hi - lo) and max(seen[k]) > hi - 0.1 * (hi - lo)


# ------------------------------------------------------------------------------------------------ refusals
def test_no_gpu_no_result(monkeypatch):
    from weed_instance_segmentation_amd import adjust_colors
    from weed_instance_segmentation_amd._lib import Wm2fError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(Wm2fError):
        adjust_colors(torch.zeros(4, 4, 3, dtype=torch.uint8), PhotometricParams(((B, 1.2),)))


def test_adjust_colors_rejects_bad_arguments():
    from weed_instance_segmentation_amd import adjust_colors
    im = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="params"):
        adjust_colors([im, im], [PhotometricParams()])
    with pytest.raises(ValueError, match="params"):
        adjust_colors(im, ((B, 1.2),))
    with pytest.raises(ValueError, match="images"):
        adjust_colors(np.zeros((4, 4), np.uint8), PhotometricParams())


def test_processor_rejects_photometric_without_geometry():
    """The chain travels inside AugmentParams; a bare PhotometricParams is not an augment argument."""
    from weed_instance_segmentation_amd.preprocess import Mask2FormerImageProcessor
    with pytest.raises(ValueError, match="augment"):
        Mask2FormerImageProcessor().preprocess([np.zeros((8, 8, 3), np.uint8)], augment=PhotometricParams())
