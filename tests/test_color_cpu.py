"""Colour traits and vegetation indices, the parts that need no GPU: the numpy restatement on hand
pictures, Otsu's threshold, `color_from_sums` on the host, the options' refusals and the declared symbols."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import color_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXG = R.PRESETS["exg"]


def _one(pixels, coef=EXG, threshold=0, dark=32, bright=250, K=12, min_chroma=16):
    """The reference on a one-row picture whose pixels all carry id 0."""
    img = np.array(pixels, np.uint8).reshape(1, -1, 3)
    return R.color_stats(img, np.zeros(img.shape[:2], np.int32), 1, coef, threshold, dark, bright, K, min_chroma)


# ------------------------------------------------------------------------------------------------- the reference
def test_reference_all_black_and_all_white():
    s, h = _one([(0, 0, 0)] * 5)
    assert s[0].tolist() == [5] + [0] * 11 + [5, 0] and h.sum() == 0  # q = 0 where R + G + B = 0; dark, no hue
    s, h = _one([(255, 255, 255)] * 3)
    assert s[0].tolist() == [3, 765, 765, 765] + [3 * 65025] * 6 + [0, 0, 0, 3] and h.sum() == 0


def test_reference_floor_not_truncation():
    assert R.pixel_q(200, 1, 0, EXG) == -4035          # 4096 x -198 / 201 = -4034.87...
    assert int(4096 * -198 / 201) == -4034             # what truncation would give
    assert R.pixel_hue(255, 0, 1) == (359, 255)        # 60 x -1 / 255 floors to -1
    s, h = _one([(200, 1, 0), (255, 0, 1)], K=36)
    assert s[0, 11] == -4035 + R.pixel_q(255, 0, 1, EXG) and h[0, 35] == 1 and h[0, 0] == 1  # (200, 1, 0): h = 0


def test_reference_primary_hues_and_grey():
    for px, want in (((255, 0, 0), 0), ((0, 255, 0), 120), ((0, 0, 255), 240), ((255, 255, 0), 60)):
        assert R.pixel_hue(*px) == (want, 255)
    assert R.pixel_hue(90, 90, 90) == (None, 0)
    s, h = _one([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (90, 90, 90), (100, 110, 105)], K=6)
    assert h[0].tolist() == [1, 1, 1, 0, 1, 0]  # the two greyish pixels (chroma 0 and 10 < 16) land nowhere
    assert s[0, 0] == 6


def test_reference_thresholded_count_and_presets():
    for name, (bins, imin) in (("exg", (1021, -510)), ("exr5", (3061, -1275)), ("exgr5", (8161, -4335))):
        assert R.index_range(R.PRESETS[name]) == (bins, imin)
    s, _ = _one([(10, 200, 10), (200, 10, 10), (50, 60, 50)], threshold=20)
    assert s[0, 10] == 1  # ExG = 380, -190, 20: strictly above 20 only the first


# ------------------------------------------------------------------------------------------------------- Otsu
def test_otsu_two_spikes():
    from weed_instance_segmentation_amd import otsu_threshold
    h = np.zeros(1021, np.int64)
    h[100], h[700] = 40, 60
    # every t in [100, 699] separates the spikes equally well: the smallest wins
    assert R.otsu(h, -510) == 100 - 510 == R.otsu_fast(h, -510) == otsu_threshold(h, -510)


def test_otsu_tie_resolves_to_the_smaller_bin():
    from weed_instance_segmentation_amd import otsu_threshold
    h = [5, 0, 0, 5]  # t = 0, 1, 2 tie
    assert R.otsu(h, 0) == 0 == otsu_threshold(h, 0)
    h = [3, 1, 3]     # symmetric: t = 0 and t = 1 tie
    assert R.otsu(h, 7) == 7 == otsu_threshold(h, 7)


def test_otsu_matches_the_reference_on_random_histograms():
    from weed_instance_segmentation_amd import otsu_threshold
    rng = np.random.default_rng(0)
    for trial in range(40):
        h = rng.integers(0, 50, rng.integers(2, 60)) * (rng.random() < 0.9)
        h = np.where(rng.random(h.shape) < 0.3, 0, h)
        assert R.otsu(h, -3) == R.otsu_fast(h, -3) == otsu_threshold(h, -3), h


def test_otsu_one_value_picture():
    from weed_instance_segmentation_amd import otsu_threshold
    img = np.full((4, 5, 3), 77, np.uint8)
    hist = R.index_hist(img, EXG)
    assert hist.sum() == 20 and hist[0 + 510] == 20
    assert R.otsu(hist, -510) is None and otsu_threshold(hist, -510) is None
    t = R.threshold_of(img, EXG)
    assert t == 510 and R.index_mask(img, EXG, t)[1] == 0  # the index's largest value: nothing is on


# ---------------------------------------------------------------------------------------------- color_from_sums
def test_color_from_sums_against_numpy():
    from weed_instance_segmentation_amd import color_from_sums
    rng = np.random.default_rng(5)
    img, m = R.scene(rng, (40, 57), 6)
    coef = R.PRESETS["exgr5"]
    sums, _ = R.color_stats(img, m, 7, coef, 30, 32, 250)  # id 6 has no pixel
    got = color_from_sums(torch.from_numpy(sums), coef)
    worst = 0.0
    for i in range(7):
        px = img[m == i].astype(np.float64)
        if len(px) == 0:
            assert all(torch.isnan(got[k][i]).all() for k in got if k != "area") and int(got["area"][i]) == 0
            continue
        I = px @ np.array(coef, np.float64)
        q = np.array([R.pixel_q(int(a), int(b), int(c), coef) for a, b, c in img[m == i]], np.float64)
        want = {"mean_rgb": px.mean(0), "std_rgb": np.sqrt(px.var(0)), "index_mean": I.mean(), "index_std": np.sqrt(I.var()),
                "index_normalised_mean": q.mean() / 4096.0, "vegetation_fraction": (I > 30).mean(),
                "dark_fraction": (px.max(1) < 32).mean(), "bright_fraction": (px.max(1) >= 250).mean()}
        for k, w in want.items():
            g = got[k][i].numpy()
            np.testing.assert_allclose(g, w, rtol=1e-9, atol=0)
            worst = max(worst, float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))))
    print("largest relative difference to numpy", worst)


def test_color_from_sums_one_colour_is_exactly_zero():
    from weed_instance_segmentation_amd import color_from_sums
    img = np.tile(np.array([201, 17, 98], np.uint8), (9, 11, 1))
    sums, _ = R.color_stats(img, np.zeros((9, 11), np.int32), 1, EXG, 0, 32, 250)
    got = color_from_sums(torch.from_numpy(sums), "exg")
    assert got["std_rgb"][0].tolist() == [0.0, 0.0, 0.0] and float(got["index_std"][0]) == 0.0
    assert got["mean_rgb"][0].tolist() == [201.0, 17.0, 98.0] and float(got["index_mean"][0]) == -201.0 + 34.0 - 98.0


def test_color_from_sums_large_area_without_cancellation():
    """2^24 pixels, half (200, 100, 50) and half (201, 100, 50): the naive E[x^2] - E[x]^2 works on 4 x 10^4 +- 0.25 and
    the sums on 7 x 10^11; the centred form gives the variance 0.25 exactly."""
    from weed_instance_segmentation_amd import color_from_sums
    half = 2 ** 23
    pix = [(200, 100, 50), (201, 100, 50)]
    row = np.zeros(14, np.int64)
    row[0] = 2 * half
    for R_, G_, B_ in pix:
        row[1:10] += half * np.array([R_, G_, B_, R_ * R_, G_ * G_, B_ * B_, R_ * G_, R_ * B_, G_ * B_], np.int64)
    got = color_from_sums(torch.from_numpy(row[None]), (1, 0, 0))
    assert got["mean_rgb"][0].tolist() == [200.5, 100.0, 50.0]
    assert got["std_rgb"][0].tolist() == [0.5, 0.0, 0.0] and float(got["index_std"][0]) == 0.5
    got = color_from_sums(torch.from_numpy(row[None]), "exg")
    assert float(got["index_mean"][0]) == -200.5 + 200.0 - 50.0 and float(got["index_std"][0]) == 0.5


def test_dominant_hue():
    from weed_instance_segmentation_amd.color import dominant_hue
    h = torch.tensor([[0, 3, 3, 1], [0, 0, 0, 0], [9, 0, 0, 9]])
    got = dominant_hue(h)
    assert got[0] == 135.0 and torch.isnan(got[1]) and got[2] == 45.0  # the first of the largest bins, centre of 90-degree bins


# ------------------------------------------------------------------------------------------------------ refusals
def test_color_options_refusals_and_presets():
    from weed_instance_segmentation_amd import ColorOptions
    o = ColorOptions()
    assert (o.coefficients, o.bins, o.index_min, o.hue_bins, o.min_chroma, o.dark, o.bright) == ((-1, 2, -1), 1021, -510, 12, 16, 32, 250)
    assert (ColorOptions(index="exr5").bins, ColorOptions(index="exr5").index_min) == (3061, -1275)
    assert (ColorOptions(index="exgr5").bins, ColorOptions(index="exgr5").index_min) == (8161, -4335)
    assert ColorOptions(index=(1, 1, 1), threshold=-5).bins == 766
    for bad in (dict(index="ndvi"), dict(index=(0, 0, 0)), dict(index=(20, -10, 3)), dict(index=(1, 2)), dict(index=(1.0, 2, 3)),
                dict(index=(True, 0, 0)), dict(threshold="mean"), dict(threshold=1.5), dict(threshold=True),
                dict(threshold=2 ** 31), dict(hue_bins=0), dict(hue_bins=7), dict(hue_bins=40), dict(hue_bins=12.0),
                dict(min_chroma=0), dict(min_chroma=256), dict(dark=-1), dict(dark=256), dict(bright=256), dict(bright=None)):
        with pytest.raises(ValueError):
            ColorOptions(**bad)


def test_annotate_colors_refusals_need_no_device():
    from weed_instance_segmentation_amd import annotate_colors, color_statistics
    seg = np.zeros((4, 6), np.int32)
    image = np.zeros((4, 6, 3), np.uint8)
    result = {"segmentation": seg, "segments_info": [{"id": 0}]}
    with pytest.raises(TypeError):
        annotate_colors(result, image, options="exg")
    with pytest.raises(ValueError):
        annotate_colors({"segmentation": seg}, image)
    with pytest.raises(ValueError):
        annotate_colors(dict(result, segmentation=np.zeros((2, 4, 6), np.int32)), image)
    with pytest.raises(ValueError):
        annotate_colors(result, np.zeros((4, 7, 3), np.uint8))     # a picture of another size
    with pytest.raises(TypeError):
        annotate_colors(result, np.zeros((4, 6, 3), np.float32))   # the renderers' coercion refuses it
    with pytest.raises(ValueError):
        annotate_colors(dict(result, segments_info=[{"id": 0}, {"id": 0}]), image)
    with pytest.raises(ValueError):
        annotate_colors([result, result], [image])
    with pytest.raises(ValueError):
        color_statistics(seg, image)                                # neither n nor ids
    with pytest.raises(ValueError):
        color_statistics(seg, image[:, :5], n=1)
    empty = annotate_colors(dict(result, segments_info=[]), image)  # nothing to annotate: no device needed
    assert empty["segments_info"] == [] and result["segments_info"] == [{"id": 0}]


def test_declared_symbols_and_constants():
    from weed_instance_segmentation_amd import _build, _lib, ops
    header = open(os.path.join(ROOT, "include", "wm2f.h")).read()
    for name in ("wm2f_labelmap_color_stats", "wm2f_image_index_hist", "wm2f_image_index_mask"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
    assert "color.hip" in _build.SOURCES
    src = open(os.path.join(ROOT, "weed_instance_segmentation_amd", "csrc", "color.hip")).read()
    cap = re.search(r"constexpr int kCoLdsMaxIds = (\d+);", src)
    assert cap is not None and int(cap.group(1)) == ops.color.COLOR_LDS_MAX_IDS
    assert ops.color.INDEX_PRESETS == R.PRESETS and ops.color.COLOR_COLUMNS == 14
    assert ops.index_range("exgr5") == (8161, -4335)
    limits = open(os.path.join(ROOT, "weed_instance_segmentation_amd", "csrc", "labelmap.h")).read()
    assert int(re.search(r"constexpr int kMapMaxIds = (\d+);", limits).group(1)) == ops.color.MAX_IDS


def test_segment_tiled_options_are_keyword_only():
    import inspect
    from weed_instance_segmentation_amd import segment_tiled
    p = inspect.signature(segment_tiled).parameters
    assert p["colors"].default is None and p["colors"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["return_shape_stats"].kind is inspect.Parameter.KEYWORD_ONLY and p["split"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
