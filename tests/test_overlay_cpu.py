"""Overlays and contours, the host side: the two numpy restatements of the kernel's contract against
each other and against hand-written pictures, the blend, `build_overlay_tables` against plot_segmentation's rules, the
shipped palette against the matplotlib fixture, and that no renderer computes without a GPU."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from overlay_reference import blend_fill, entries_of, overlay_painter, overlay_reference

RED, GREEN, BLUE = (255, 0, 0, 0), (0, 255, 0, 0), (0, 0, 255, 0)  # alpha 0: the fill is the picture itself


def _grey(shape, v=100):
    return np.full((*shape, 3), v, np.uint8)


def _both(image, seg, ids, rgba, order, default=(0, 0, 0, 0), inner=1, outer=1):
    a = overlay_reference(image, seg, ids, rgba, order, default, inner, outer)
    b = overlay_painter(image, seg, ids, rgba, order, default, inner, outer)
    assert np.array_equal(a, b)
    return a


def _is(out, colour):
    return np.all(out == np.asarray(colour[:3], np.uint8), axis=-1)


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.uint8])
def test_the_two_forms_agree_on_random_maps(dtype):
    rng = np.random.default_rng(5)
    for trial in range(40):
        H, W = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        n = int(rng.integers(0, 7))
        ids = np.sort(rng.choice(12, n, replace=False))
        seg = rng.integers(0, 12, (H, W))
        if trial % 2:  # blobs instead of noise
            seg = np.repeat(np.repeat(rng.integers(0, 12, ((H + 3) // 4, (W + 3) // 4)), 4, 0), 4, 1)[:H, :W]
        seg = seg.astype(dtype)
        if dtype == np.float32:
            seg[rng.random((H, W)) < 0.1] = rng.choice(np.asarray([-1.0, 1.5, np.nan, np.inf, 2.0 ** 24], np.float32))
        rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
        order = rng.integers(-1, 4, n)  # ties and fill-only entries
        image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        default = tuple(int(v) for v in rng.integers(0, 256, 4))
        _both(image, seg, ids, rgba, order, default, int(rng.integers(0, 5)), int(rng.integers(0, 5)))


def test_entries_of_a_float_map():
    seg = np.asarray([[0.0, -0.0, 3.0, 3.5, -1.0, np.nan, np.inf, 2.0 ** 24, 2.0 ** 24 - 1, 7.0]], np.float32)
    assert entries_of(seg, [0, 3, 2 ** 24 - 1, 2 ** 24]).tolist() == [[0, 0, 1, -1, -1, -1, -1, -1, 2, -1]]
    assert entries_of(np.asarray([[255, 0, 4]], np.uint8), [4, 255]).tolist() == [[1, -1, 0]]
    assert entries_of(np.asarray([[-5, 6]], np.int32), [-5]).tolist() == [[0, -1]]
    assert entries_of(np.asarray([[1, 2]], np.int32), []).tolist() == [[-1, -1]]


def test_one_pixel_segment():
    seg = np.zeros((5, 5), np.int32)
    seg[2, 2] = 7
    img = _grey((5, 5))
    # width 1 inside: the pixel itself
    out = _both(img, seg, [7], [RED], [0], inner=1, outer=0)
    assert _is(out, RED).astype(int).tolist() == [[0] * 5, [0] * 5, [0, 0, 1, 0, 0], [0] * 5, [0] * 5]
    # width 1 outside: its four neighbours, the pixel keeps its fill
    out = _both(img, seg, [7], [RED], [0], inner=0, outer=1)
    assert _is(out, RED).astype(int).tolist() == [[0] * 5, [0, 0, 1, 0, 0], [0, 1, 0, 1, 0], [0, 0, 1, 0, 0], [0] * 5]
    # outer 2: the diamond of radius 2 without its centre
    out = _both(img, seg, [7], [RED], [0], inner=0, outer=2)
    assert _is(out, RED).astype(int).tolist() == [[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 0, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]]
    assert np.all(out[~_is(out, RED)] == 100)


def test_two_touching_segments_painters_order_decides():
    seg = np.asarray([[1, 1, 1, 2, 2, 2]] * 3, np.int32)
    img = _grey((3, 6))
    for order, winner in (([0, 1], GREEN), ([1, 0], RED)):
        out = _both(img, seg, [1, 2], [RED, GREEN], order, inner=1, outer=1)
        # columns 2 and 3 carry both contours (own inner, the other's outer): the later one is on top
        assert _is(out, winner)[:, 2:4].all() and np.all(out[:, :2] == 100) and np.all(out[:, 4:] == 100)
    # inner only: each keeps its own edge column
    out = _both(img, seg, [1, 2], [RED, GREEN], [0, 1], inner=1, outer=0)
    assert _is(out, RED)[:, 2].all() and _is(out, GREEN)[:, 3].all()
    # equal orders: the later entry
    out = _both(img, seg, [1, 2], [RED, GREEN], [5, 5], inner=1, outer=1)
    assert _is(out, GREEN)[:, 2:4].all()
    # order -1: filled (here at alpha 255), never outlined, and its neighbour's contour still crosses into it
    out = _both(img, seg, [1, 2], [(255, 0, 0, 255), GREEN], [-1, 0], inner=1, outer=1)
    assert _is(out, RED)[:, :2].all() and _is(out, GREEN)[:, 2:4].all() and np.all(out[:, 4:] == 100)


def test_segment_on_the_border_gets_no_contour_along_it():
    seg = np.zeros((4, 5), np.int32)
    seg[:3, :3] = 9  # touches the top and the left border
    out = _both(_grey((4, 5)), seg, [9], [BLUE], [0], inner=1, outer=0)
    assert _is(out, BLUE).astype(int).tolist() == [[0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [1, 1, 1, 0, 0], [0, 0, 0, 0, 0]]
    # a segment that is the whole picture has no contour at all
    out = _both(_grey((4, 5)), np.full((4, 5), 9, np.int32), [9], [BLUE], [0], inner=4, outer=4)
    assert np.all(out == 100)


def test_inner_and_outer_zero():
    seg = np.zeros((5, 6), np.uint8)
    seg[1:4, 1:5] = 3
    img = _grey((5, 6))
    none = _both(img, seg, [3], [(10, 20, 30, 255)], [0], inner=0, outer=0)
    assert np.array_equal(none, blend_fill(img, entries_of(seg, [3]), [(10, 20, 30, 255)], (0, 0, 0, 0)))
    inner = _both(img, seg, [3], [RED], [0], inner=1, outer=0)
    assert _is(inner, RED).astype(int).tolist() == [[0] * 6, [0, 1, 1, 1, 1, 0], [0, 1, 0, 0, 1, 0], [0, 1, 1, 1, 1, 0], [0] * 6]
    outer = _both(img, seg, [3], [RED], [0], inner=0, outer=1)
    assert _is(outer, RED).astype(int).tolist() == [[0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1],
                                                    [0, 1, 1, 1, 1, 0]]


def test_blend():
    img = np.asarray([[[0, 100, 255], [37, 200, 1]]], np.uint8)
    seg = np.zeros((1, 2), np.int32)
    col = (255, 10, 77)
    for a, expect in ((0, img), (255, np.broadcast_to(np.asarray(col, np.uint8), img.shape)),
                      (102, [[[102, 64, 184], [124, 124, 31]]]), (128, [[[128, 55, 166], [146, 105, 39]]])):
        out = _both(img, seg, [0], [(*col, a)], [-1])
        assert np.array_equal(out, np.asarray(expect, np.uint8)), a
        assert np.array_equal(out, (img.astype(np.int64) * (255 - a) + np.asarray(col) * a + 127) // 255)
    # the default colour paints what is not listed
    out = _both(img, seg, [], np.zeros((0, 4)), [], default=(*col, 102))
    assert out.tolist() == [[[102, 64, 184], [124, 124, 31]]]


# ------------------------------------------------------------------------------------------------ build_overlay_tables
class _Config:
    id2label = {1: "crop", 2: "weed"}


def _result(n, labels=(1, 2, 3)):
    return {"segmentation": None,
            "segments_info": [{"id": i, "label_id": labels[i % len(labels)], "score": 0.5 + 0.4 * (i % 2)} for i in range(n)]}


def test_tables_instance_mode_score_filter_and_label_text():
    from weed_instance_segmentation_amd.visualize import build_overlay_tables, palette
    res = _result(6)
    res["segments_info"][4].pop("score")  # a missing score counts as 1.0
    ids, rgba, order, legend = build_overlay_tables(res, id2label={2: "NOT USED", 3: "soil"}, config=_Config(), score_threshold=0.6)
    assert ids.dtype == np.int32 and rgba.dtype == np.uint8 and order.dtype == np.int32
    assert ids.tolist() == [1, 3, 4, 5] and order.tolist() == [0, 1, 2, 3]
    assert np.array_equal(rgba[:, :3], palette(4)) and set(rgba[:, 3]) == {102}  # round(0.4 * 255)
    # labels of ids 1, 3, 4, 5: 2, 1, 2, 3 -> config, config, config, id2label
    assert [t for t, _ in legend] == ["weed 1", "crop 1", "weed 2", "soil 1"]
    assert [c for _, c in legend] == [tuple(int(v) for v in c) for c in palette(4)]
    # the third source of the text
    _, _, _, legend = build_overlay_tables(_result(3), id2label=None, config=None)
    assert [t for t, _ in legend] == ["Class 1 1", "Class 2 1", "Class 3 1"]
    # nothing kept
    ids, rgba, order, legend = build_overlay_tables(_result(3), score_threshold=2.0)
    assert ids.shape == (0,) and rgba.shape == (0, 4) and order.shape == (0,) and legend == []


def test_tables_class_mode():
    from weed_instance_segmentation_amd.visualize import build_overlay_tables, palette
    res = {"segments_info": [{"id": 10, "label_id": 7}, {"id": 4, "label_id": 2}, {"id": 6, "label_id": 7}, {"id": 5, "label_id": 5}]}
    ids, rgba, order, legend = build_overlay_tables(res, id2label={7: "seven"}, instance_mode=False, alpha=0.5)
    pal = palette(3)  # classes 2, 5, 7 in sorted order
    assert ids.tolist() == [4, 5, 6, 10] and order.tolist() == [1, 3, 2, 0]
    assert np.array_equal(rgba[:, :3], pal[[0, 1, 2, 2]]) and set(rgba[:, 3]) == {128}
    assert legend == [("seven", tuple(pal[2])), ("Class 2", tuple(pal[0])), ("Class 5", tuple(pal[1]))]


def test_tables_switch_palettes_between_20_and_21_colours():
    from weed_instance_segmentation_amd.visualize import build_overlay_tables
    g = load_golden("overlay_palette.npz")
    for n in (20, 21):
        ids, rgba, order, _ = build_overlay_tables(_result(n))
        assert np.array_equal(rgba[:, :3], g[f"palette_{n}"])
    assert np.array_equal(g["palette_20"], g["tab20"]) and np.array_equal(g["palette_21"][0], g["nipy_spectral"][0])
    # class mode counts classes, not segments: 21 segments of 3 classes stay on tab20
    res = _result(21)
    _, rgba, _, _ = build_overlay_tables(res, instance_mode=False)
    assert np.array_equal(rgba[:3, :3], g["tab20"][:3])


def test_tables_duplicate_id_keeps_its_last_entry():
    from weed_instance_segmentation_amd.visualize import build_overlay_tables, palette
    res = {"segments_info": [{"id": 3, "label_id": 1}, {"id": 8, "label_id": 1}, {"id": 3, "label_id": 2}]}
    ids, rgba, order, legend = build_overlay_tables(res, config=_Config())
    assert ids.tolist() == [3, 8] and order.tolist() == [2, 1]
    assert np.array_equal(rgba[:, :3], palette(3)[[2, 1]])
    assert [t for t, _ in legend] == ["crop 1", "crop 2", "weed 1"]  # both entries of id 3 stay in the legend


def test_palette_equals_the_matplotlib_fixture():
    from weed_instance_segmentation_amd import _palette
    from weed_instance_segmentation_amd.visualize import palette
    g = load_golden("overlay_palette.npz")
    assert np.array_equal(_palette.tab20(), g["tab20"]) and np.array_equal(_palette.nipy_spectral(), g["nipy_spectral"])
    assert {20, 21} <= set(g["counts"].tolist())
    for n in g["counts"].tolist():
        got = palette(n)
        assert got.dtype == np.uint8 and np.array_equal(got, g[f"palette_{n}"]), n
    assert palette(0).shape == (1, 3)  # max(n, 1), as the reference builds it


def test_convert_gt_map_to_result():
    from weed_instance_segmentation_amd.visualize import convert_gt_map_to_result
    gt = np.asarray([[0, 3, 3, 255], [7, 7, 9, 0]], np.uint8)
    res = convert_gt_map_to_result(gt, {0: 0, 3: 1, 7: 2, 11: 1, 255: 0})
    assert res["segments_info"] == [{"id": 0, "label_id": 0, "score": 1.0}, {"id": 3, "label_id": 1, "score": 1.0},
                                    {"id": 7, "label_id": 2, "score": 1.0}]
    assert torch.equal(res["segmentation"], torch.from_numpy(gt))


def test_renderers_refuse_to_run_without_a_gpu(tmp_path):
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    img, seg = _grey((4, 4)), np.zeros((4, 4), np.int32)
    res = {"segmentation": torch.from_numpy(seg), "segments_info": [{"id": 0, "label_id": 1}]}
    # the op never takes host tensors; the renderers move theirs to a device, so they refuse where there is none
    calls = [lambda: ops.labelmap_overlay(torch.from_numpy(img)[None], torch.from_numpy(seg)[None], None, None, None, None)]
    if not torch.cuda.is_available():
        calls += [lambda: pkg.render_segmentation(img, res), lambda: pkg.render_segmentations([img], [res]),
                  lambda: pkg.render_label_overlay(img, seg.astype(np.uint8), {1: (0, 255, 0)}),
                  lambda: pkg.save_comparison(str(tmp_path / "x.png"), img, res, res)]
    for call in calls:
        with pytest.raises(Wm2fError):
            call()
    assert not (tmp_path / "x.png").exists()
