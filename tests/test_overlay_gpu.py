"""Overlays and contours on the GPU: csrc/overlay.hip against the numpy restatement of its contract
(tests/overlay_reference.py) with torch.equal -- the contract is all integer -- and the renderers of visualize.py end to
end against their tables plus that restatement."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from overlay_reference import overlay_batch, overlay_painter, overlay_reference
from weed_instance_segmentation_amd import (build_overlay_tables, ops, render_label_overlay, render_segmentation,
                                            render_segmentations)
from weed_instance_segmentation_amd._lib import Wm2fError

pytestmark = pytest.mark.gpu
DEV = "cuda"
LDS_CAP = 1024  # kOvLdsMaxIds of csrc/overlay.hip: above it the tables are read from global memory
MAX_IDS = 4096  # kOvMaxIds
NP_DT = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}
SHAPES = [(2, 37, 53), (1, 64, 64), (1, 130, 260)]  # W % 4 != 0; one tile; tile seams both ways with W % 4 == 0
NOT_AN_ID = np.asarray([-1.0, 2.5, np.nan, 2.0 ** 24, -np.inf], np.float32)


def _scene(rng, B, H, W, n_vals, dtype, noise=0.03):
    """Blobs of the values 0 .. n_vals-1 (4 x 4 to 16 x 16 cells, so that contours of width 4 meet), noise pixels, and
    in a float map the values that are no id."""
    maps = np.empty((B, H, W), np.int64)
    for b in range(B):
        c = int(rng.choice([4, 7, 16]))
        cells = rng.integers(0, n_vals, ((H + c - 1) // c, (W + c - 1) // c))
        maps[b] = np.repeat(np.repeat(cells, c, 0), c, 1)[:H, :W]
        hit = rng.random((H, W)) < noise
        maps[b][hit] = rng.integers(0, n_vals, int(hit.sum()))
    maps = maps.astype(NP_DT[dtype])
    if dtype == torch.float32:
        hit = rng.random(maps.shape) < 0.02
        maps[hit] = rng.choice(NOT_AN_ID, int(hit.sum()))
    return maps


def _tables(rng, B, N, pool, counts, fill_only=0.2):
    """ids (B, N) ascending draws from `pool` with counts[b] of them valid, random colours and alphas, orders a
    permutation with some entries at -1 (filled, never outlined)."""
    ids, rgba = np.zeros((B, N), np.int32), rng.integers(0, 256, (B, N, 4)).astype(np.uint8)
    order = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int32) if N else np.zeros((B, 0), np.int32)
    order[rng.random((B, N)) < fill_only] = -1
    for b in range(B):
        ids[b, :counts[b]] = np.sort(rng.choice(pool, counts[b], replace=False))
    return ids, np.asarray(counts, np.int32), rgba, order


def _check(images, maps, ids, n_ids, rgba, order, default, inner, outer, ref=overlay_reference):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    N = ids.shape[1]
    got = ops.labelmap_overlay(T(images), T(maps), *((T(ids), T(n_ids), T(rgba), T(order)) if N else (None,) * 4),
                               default_rgba=default, inner=inner, outer=outer)
    assert got.shape == images.shape and got.dtype == torch.uint8 and got.is_cuda
    want = overlay_batch(ref, images, maps, ids, n_ids, rgba, order, default, inner, outer)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    return got, want


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_overlay_equals_the_restatement(dtype, B, H, W):
    rng = np.random.default_rng(H + W)
    maps = _scene(rng, B, H, W, 9, dtype)
    if dtype == torch.float32:
        assert all(np.any(maps == v) for v in NOT_AN_ID[[0, 1, 3]]) and np.isnan(maps).any()
    images = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    ids, n_ids, rgba, order = _tables(rng, B, 6, 9, [6 - b for b in range(B)])  # n_ids differs per image
    got, want = _check(images, maps, ids, n_ids, rgba, order, (12, 200, 77, 60), 1, 1)
    assert (want != images).any()
    _check(images, maps, ids, n_ids, rgba, order, (0, 0, 0, 0), 2, 1)
    if (H, W) == (37, 53):  # and the second form of the contract, where it is cheap
        _check(images, maps, ids, n_ids, rgba, order, (0, 0, 0, 0), 2, 1, ref=overlay_painter)


@pytest.mark.parametrize("inner", [0, 1, 2, 4])
@pytest.mark.parametrize("outer", [0, 1, 2, 4])
def test_every_inner_and_outer(inner, outer):
    rng = np.random.default_rng(17)
    B, H, W = 2, 45, 150  # two tiles wide, two high, W % 4 != 0
    maps = _scene(rng, B, H, W, 6, torch.float32)
    images = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    ids, n_ids, rgba, order = _tables(rng, B, 5, 6, [5, 3])
    _, want = _check(images, maps, ids, n_ids, rgba, order, (0, 0, 0, 0), inner, outer)
    if inner == outer == 0:  # no contours: the fill alone
        assert np.array_equal(want, overlay_batch(overlay_reference, images, maps, ids, n_ids, rgba,
                                                  np.full_like(order, -1), (0, 0, 0, 0), 4, 4))


def test_three_is_a_width_too():
    rng = np.random.default_rng(3)
    maps, images = _scene(rng, 1, 50, 64, 5, torch.int32), rng.integers(0, 256, (1, 50, 64, 3)).astype(np.uint8)
    ids, n_ids, rgba, order = _tables(rng, 1, 5, 5, [5], fill_only=0.0)
    _check(images, maps, ids, n_ids, rgba, order, (0, 0, 0, 0), 3, 1)
    _check(images, maps, ids, n_ids, rgba, order, (0, 0, 0, 0), 0, 3)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("H,W", [(64, 64), (130, 260), (37, 53)])
def test_checkerboard_every_pixel_is_a_boundary(dtype, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    maps = (3 + 4 * ((yy + xx) % 2)).astype(NP_DT[dtype])[None]
    images = np.random.default_rng(0).integers(0, 256, (1, H, W, 3)).astype(np.uint8)
    ids, n_ids = np.asarray([[3, 7]], np.int32), np.asarray([2], np.int32)
    rgba = np.asarray([[[255, 0, 0, 100], [0, 0, 255, 100]]], np.uint8)
    for order, top in (([0, 1], (0, 0, 255)), ([1, 0], (255, 0, 0))):
        got, _ = _check(images, maps, ids, n_ids, rgba, np.asarray([order], np.int32), (0, 0, 0, 0), 1, 1)
        assert (got.cpu() == torch.tensor(top, dtype=torch.uint8)).all()  # the later contour covers everything
    got, _ = _check(images, maps, ids, n_ids, rgba, np.asarray([[0, 1]], np.int32), (0, 0, 0, 0), 1, 0)
    assert (got[0, 0, 0].cpu() == torch.tensor((255, 0, 0), dtype=torch.uint8)).all()  # own contours only


def test_no_ids_and_one_id():
    rng = np.random.default_rng(8)
    B, H, W = 2, 40, 132
    maps, images = _scene(rng, B, H, W, 3, torch.int32), rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    none = (np.zeros((B, 0), np.int32), np.zeros(B, np.int32), np.zeros((B, 0, 4), np.uint8), np.zeros((B, 0), np.int32))
    got, _ = _check(images, maps, *none, (0, 0, 0, 0), 2, 2)
    assert torch.equal(got.cpu(), torch.from_numpy(images))  # alpha 0 everywhere: the pictures themselves
    _, want = _check(images, maps, *none, (10, 250, 30, 128), 1, 1)
    assert np.array_equal(want, (images.astype(np.int64) * 127 + np.asarray([10, 250, 30]) * 128 + 127) // 255)
    # N = 1, and an image whose one entry is switched off by n_ids = 0
    one = (np.asarray([[1], [1]], np.int32), np.asarray([1, 0], np.int32),
           np.asarray([[[200, 100, 0, 102]]] * 2, np.uint8), np.zeros((B, 1), np.int32))
    got, _ = _check(images, maps, *one, (0, 0, 0, 0), 1, 1)
    assert torch.equal(got[1].cpu(), torch.from_numpy(images[1])) and not torch.equal(got[0].cpu(), torch.from_numpy(images[0]))


@pytest.mark.parametrize("N", [LDS_CAP, LDS_CAP + 1, MAX_IDS])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_id_counts_on_both_sides_of_the_lookup_cap(N, dtype):
    rng = np.random.default_rng(N)
    B, H, W = 2, 70, 136
    pool = N + N // 4  # a fifth of the values in the maps is not listed
    maps = _scene(rng, B, H, W, pool, dtype, noise=0.3)
    images = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    ids, n_ids, rgba, order = _tables(rng, B, N, pool, [N, N - 3])
    _, want = _check(images, maps, ids, n_ids, rgba, order, (9, 9, 9, 30), 1, 1)
    assert (want != images).any()


def test_limits_and_misuse():
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    seg = torch.zeros(1, 8, 8, dtype=torch.int32, device=DEV)
    N = MAX_IDS + 1
    big = (torch.arange(N, dtype=torch.int32, device=DEV)[None], torch.tensor([N], dtype=torch.int32, device=DEV),
           torch.zeros(1, N, 4, dtype=torch.uint8, device=DEV), torch.zeros(1, N, dtype=torch.int32, device=DEV))
    with pytest.raises(Wm2fError, match="code -2"):
        ops.labelmap_overlay(img, seg, *big)
    for kw in ({"inner": 5}, {"outer": -1}):
        with pytest.raises(Wm2fError, match="code -1"):
            ops.labelmap_overlay(img, seg, None, None, None, None, **kw)
    with pytest.raises(TypeError):
        ops.labelmap_overlay(img, seg.to(torch.int64), None, None, None, None)
    with pytest.raises(ValueError):
        ops.labelmap_overlay(img, seg[:, :4], None, None, None, None)
    # out == image: neighbours are read, so the library refuses (the wrapper always hands it a fresh tensor)
    from weed_instance_segmentation_amd import _lib
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
    rc = _lib.load().wm2f_labelmap_overlay(p(img), p(seg), _lib.WM2F_I32, p(None), p(None), p(None), p(None), 0, 1, 1, p(img),
                                           1, 8, 8, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.WM2F_EINVAL and b"overlap" in _lib.load().wm2f_last_error()


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_unaligned_maps_take_the_pixel_by_pixel_path(dtype):
    rng = np.random.default_rng(21)
    B, H, W = 1, 40, 136  # W % 4 == 0, but the tensors start one element into their storage
    maps, images = _scene(rng, B, H, W, 6, dtype), rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    ids, n_ids, rgba, order = _tables(rng, B, 5, 6, [5])
    T = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    m = torch.empty(maps.size + 1, dtype=dtype, device=DEV)[1:].view(B, H, W).copy_(T(maps))
    i = torch.empty(images.size + 1, dtype=torch.uint8, device=DEV)[1:].view(B, H, W, 3).copy_(T(images))
    assert m.is_contiguous() and m.data_ptr() % (4 * m.element_size()) != 0 and i.data_ptr() % 4 != 0
    want = overlay_batch(overlay_reference, images, maps, ids, n_ids, rgba, order, (1, 2, 3, 40), 2, 2)
    for pic, mp in ((i, m), (T(images), m), (i, T(maps))):
        got = ops.labelmap_overlay(pic, mp, T(ids), T(n_ids), T(rgba), T(order), default_rgba=(1, 2, 3, 40), inner=2, outer=2)
        assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_two_runs_give_identical_bytes():
    rng = np.random.default_rng(1)
    B, H, W = 2, 256, 384
    maps, images = _scene(rng, B, H, W, 40, torch.float32), rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    ids, n_ids, rgba, order = _tables(rng, B, 32, 40, [32, 20])
    T = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    args = (T(images), T(maps), T(ids), T(n_ids), T(rgba), T(order))
    a = ops.labelmap_overlay(*args, default_rgba=(0, 0, 0, 0), inner=1, outer=1)
    b = ops.labelmap_overlay(*args, default_rgba=(0, 0, 0, 0), inner=1, outer=1)
    assert torch.equal(a, b) and torch.equal(args[0].cpu(), torch.from_numpy(images))  # and the picture is left alone
    assert torch.equal(a.cpu(), torch.from_numpy(overlay_batch(overlay_reference, images, maps, ids, n_ids, rgba, order,
                                                               (0, 0, 0, 0), 1, 1)))


# ------------------------------------------------------------------------------------------------------ renderers
def _fixture_results(tag):
    g = load_golden("postprocess_instances.npz")
    info = json.loads(str(g["info_json"]))[tag]["segments_info"]
    return [{"segmentation": torch.from_numpy(g[f"seg_{tag}_{i}"].astype(np.float32)), "segments_info": info[i]}
            for i in range(len(info))]


def _expected(image, result, width, **kw):
    ids, rgba, order, legend = build_overlay_tables(result, **kw)
    seg = result["segmentation"].cpu().numpy()
    return overlay_reference(image, seg, ids, rgba, order, (0, 0, 0, 0), (width + 1) // 2, width // 2), legend


@pytest.mark.parametrize("instance_mode", [True, False])
def test_render_segmentation_end_to_end(instance_mode):
    results = _fixture_results("small")  # the post-processor's maps: fp32 ids, -1 background, three of one size
    assert sum(len(r["segments_info"]) for r in results) > 3
    rng = np.random.default_rng(2)
    H, W = results[0]["segmentation"].shape
    images = rng.integers(0, 256, (len(results), H, W, 3)).astype(np.uint8)
    kw = dict(instance_mode=instance_mode, score_threshold=0.7, id2label={0: "crop", 1: "weed", 2: "soil"})
    out, legends = render_segmentations(list(images), results, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == images.shape
    for b, r in enumerate(results):
        want, legend = _expected(images[b], r, 2, **kw)
        assert torch.equal(out[b].cpu(), torch.from_numpy(want)) and legends[b] == legend
    # one picture, from a device tensor and a device map, another width, an int64 map
    r = dict(results[0], segmentation=results[0]["segmentation"].to(torch.int64).to(DEV))
    one, legend = render_segmentation(torch.from_numpy(images[0]).to(DEV), r, contour_width=5, **kw)
    want, wl = _expected(images[0], r, 5, **kw)
    assert one.shape == (H, W, 3) and torch.equal(one.cpu(), torch.from_numpy(want)) and legend == wl
    assert (want != images[0]).any()
    with pytest.raises(ValueError):
        render_segmentation(images[0], r, contour_width=9)


def test_render_from_a_pil_image_and_save_comparison(tmp_path):
    from PIL import Image
    from weed_instance_segmentation_amd import convert_gt_map_to_result, save_comparison
    res = _fixture_results("mixed")[0]
    H, W = res["segmentation"].shape
    arr = np.random.default_rng(4).integers(0, 256, (H, W, 3)).astype(np.uint8)
    out, _ = render_segmentation(Image.fromarray(arr), res)
    assert torch.equal(out.cpu(), torch.from_numpy(_expected(arr, res, 2)[0]))
    gt = np.zeros((H, W), np.uint8)
    gt[5:30, 10:40], gt[0:4, :] = 2, 255
    truth = convert_gt_map_to_result(gt, {2: 1})
    path = save_comparison(str(tmp_path / "cmp.png"), arr, res, truth, id2label={1: "weed"})
    with Image.open(path) as sheet:
        assert sheet.size == (2 * W, H) and sheet.mode == "RGB"


def test_render_label_overlay():
    rng = np.random.default_rng(6)
    H, W = 60, 90
    mask = _scene(rng, 1, H, W, 5, torch.uint8)[0]
    mask[mask == 3] = 9  # a label that has no colour
    image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    colors = {0: [0, 0, 0], 1: [0, 255, 0], 2: [255, 0, 0], 4: [255, 0, 255], 7: [1, 2, 3]}
    out, legend = render_label_overlay(image, mask, colors, names={1: "crop", 2: "weed"})
    ids = np.asarray(sorted(colors))
    rgba = np.asarray([[*colors[k], 128] for k in ids], np.uint8)
    want = overlay_reference(image, mask, ids, rgba, np.full(len(ids), -1), (255, 255, 0, 128), 0, 0)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    # the same picture the visualiser composes: a colour mask at alpha 0.5 over everything
    colour_mask = np.zeros((H, W, 3), np.int64)
    for lbl in np.unique(mask):
        if lbl != 0:
            colour_mask[mask == lbl] = colors.get(int(lbl), [255, 255, 0])
    assert np.array_equal(want, (image.astype(np.int64) * 127 + colour_mask * 128 + 127) // 255)
    assert legend == [("crop", (0, 255, 0)), ("weed", (255, 0, 0)), ("Class 4", (255, 0, 255)), ("Class 9", (255, 255, 0))]
    # an int32 mask gives the same picture
    out32, legend32 = render_label_overlay(image, mask.astype(np.int32), colors, names={1: "crop", 2: "weed"})
    assert torch.equal(out32, out) and legend32 == legend
