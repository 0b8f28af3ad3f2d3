"""Colour traits and vegetation indices on the GPU: csrc/color.hip against the numpy restatement of
tests/color_reference.py, every integer compared for equality; the float traits against the host at rtol 1e-9."""
import copy
import functools

import numpy as np
import pytest
import torch

import color_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (7, 9): scalar loads at the border, one partial wave; (33, 65): W % 4 != 0; (40, 257): a row across the 256-pixel wave
# segment, W % 4 != 0; (64, 260): the vector path, two segments per row; (130, 70): three strips of 59 rows
SCENES = [((7, 9), 3), ((33, 65), 6), ((40, 257), 12), ((64, 260), 12), ((130, 70), 9)]
BATCHES = (1, 3)
DTYPES = {"f32": np.float32, "i32": np.int32, "u8": np.uint8}
HUE_BINS = (6, 12, 36)
EXG = R.PRESETS["exg"]
DARK, BRIGHT, MIN_CHROMA = 125, 150, 16  # a plant's largest byte is its green, 115 .. 165: both counts see something
THRESHOLD = 70


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ids(case):
    (H, W), N = case
    return f"{H}x{W}-N{N}"


@functools.lru_cache(maxsize=None)
def _scene(case, B):
    """B pictures and int64 maps (-1 background) of one scene, picture b from default_rng(1000 H + W + b).  (In a
    63-pixel picture one soil pixel above Otsu's threshold is 1.6 %: the (7, 9) pictures have to separate perfectly to
    meet the 99 % condition on the input, and these three do.)"""
    (H, W), N = case
    pairs = [R.scene(np.random.default_rng(1000 * H + W + b), (H, W), N, dtype=np.int64) for b in range(B)]
    imgs, maps = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    imgs.setflags(write=False)
    maps.setflags(write=False)
    return imgs, maps


@functools.lru_cache(maxsize=None)
def _reference(case, B, coef=EXG):
    """sums and {K: hue} of the scene, computed once and shared; the map's dtype does not change them."""
    imgs, maps = _scene(case, B)
    N = case[1]
    thr = [THRESHOLD + 3 * b for b in range(B)]
    out = {K: R.color_stats_batch(imgs, maps, N, coef, thr, DARK, BRIGHT, K, MIN_CHROMA) for K in HUE_BINS}
    sums = out[HUE_BINS[0]][0]
    assert all(np.array_equal(out[K][0], sums) for K in HUE_BINS)
    sums.setflags(write=False)
    return sums, {K: out[K][1] for K in HUE_BINS}, np.array(thr, np.int32)


def _typed_map(maps, dt, N, seed=0):
    """The int64 scene maps as a kernel dtype: a uint8 map has background 200; in an fp32 map some background becomes
    1.5 and N + 1, which are no ids."""
    m = maps.copy()
    if dt == "u8":
        return np.where(m < 0, 200, m).astype(np.uint8)
    if dt == "i32":
        return m.astype(np.int32)
    f = m.astype(np.float32)
    rng = np.random.default_rng(seed)
    bg = np.flatnonzero(m.ravel() < 0)
    pick = rng.permutation(bg)[:max(2, len(bg) // 5)]
    f.ravel()[pick[::2]] = 1.5
    f.ravel()[pick[1::2]] = N + 1
    return f


def _stats(imgs, maps, thr, N=None, K=12, **kw):
    from weed_instance_segmentation_amd import ops
    kw.setdefault("index", EXG)
    return ops.labelmap_color_stats(imgs, maps, thr, N=N, dark=DARK, bright=BRIGHT, hue_bins=K, min_chroma=MIN_CHROMA, **kw)


def _same(t, a):
    return t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), a)


# ------------------------------------------------------------------------------------------------- color_stats
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", SCENES, ids=_ids)
def test_color_stats_equals_the_reference(case, B, dt):
    imgs, maps = _scene(case, B)
    N = case[1]
    want, want_hue, thr = _reference(case, B)
    assert (want[..., 0] > 0).sum() >= 2 and want[..., 10].sum() > 0 and want[..., 12].sum() > 0 and want[..., 13].sum() > 0
    di, dm, dthr = _dev(imgs), _dev(_typed_map(maps, dt, N)), _dev(thr)
    for K in HUE_BINS:
        sums, hue = _stats(di, dm, dthr, N=N, K=K)
        assert _same(sums, want), (K, np.argwhere(sums.cpu().numpy() != want)[:5])
        assert _same(hue, want_hue[K]) and want_hue[K].sum() > 0
        again = _stats(di, dm, dthr, N=N, K=K)
        assert torch.equal(again[0], sums) and torch.equal(again[1], hue)
    sums, hue = _stats(di, dm, dthr, N=N, K=None)
    assert hue is None and _same(sums, want)


@pytest.mark.parametrize("B", BATCHES)
def test_color_stats_with_id_lists(B):
    """Ascending lists of different lengths per image, ids that own no pixel and listed ids above the scene's."""
    case = SCENES[2]
    imgs, maps = _scene(case, B)
    lists = [[1, 4, 5, 9, 11, 40], [0, 2, 3, 2000], [7]][:B]
    R_ = 7
    ids = np.zeros((B, R_), np.int32)
    for b, l in enumerate(lists):
        ids[b, :len(l)] = l
        ids[b, len(l):] = 3  # past n_ids: not looked at
    n_ids = np.array([len(l) for l in lists], np.int32)
    thr = np.full(B, THRESHOLD, np.int32)
    want, want_hue = R.color_stats_batch(imgs, maps, R_, EXG, thr, DARK, BRIGHT, 12, MIN_CHROMA, ids, n_ids)
    assert (want[..., 0] > 0).sum() >= 3
    for dt in sorted(DTYPES):
        sums, hue = _stats(_dev(imgs), _dev(_typed_map(maps, dt, 2001)), _dev(thr), ids=_dev(ids), n_ids=_dev(n_ids))
        assert _same(sums, want) and _same(hue, want_hue), dt


def test_color_statistics_keeps_the_callers_order():
    """Every trait, not only the integers, comes back in the caller's order: each against `color_from_sums` of the
    reference rows taken in that order."""
    from weed_instance_segmentation_amd import ColorOptions, color_from_sums, color_statistics
    from weed_instance_segmentation_amd.color import dominant_hue
    case = SCENES[3]
    imgs, maps = _scene(case, 1)
    order = [5, 2, 30, 7, 0]
    opt = ColorOptions(threshold=THRESHOLD, dark=DARK, bright=BRIGHT, hue_bins=36)
    got = color_statistics(maps[0].astype(np.int32), imgs[0], ids=order, options=opt)
    want, want_hue, _ = _reference(case, 1)
    rows = [want[0, i] if i < case[1] else np.zeros(14, np.int64) for i in order]
    hues = [want_hue[36][0, i] if i < case[1] else np.zeros(36, np.int64) for i in order]
    assert _same(got["area"], np.array([r[0] for r in rows])) and _same(got["hue_histogram"], np.stack(hues))
    assert got["mean_rgb"].shape == (5, 3) and bool(torch.isnan(got["index_mean"][2])) and got["area"].is_cuda
    host = color_from_sums(torch.from_numpy(np.stack(rows)), "exg")
    host["dominant_hue"] = dominant_hue(torch.from_numpy(np.stack(hues)))
    assert set(got) == set(host) | {"hue_histogram"}
    for k, h in host.items():
        if k != "area":  # compared exactly above
            torch.testing.assert_close(got[k].cpu(), h, rtol=1e-9, atol=0, equal_nan=True, msg=k)
    means = host["mean_rgb"][[0, 1, 3, 4]]
    assert len({tuple(r.tolist()) for r in means}) == 4  # the four present instances differ: a wrong order would show


@pytest.mark.parametrize("extra", (0, 76))
def test_color_stats_on_both_sides_of_the_lds_cap(extra):
    """N = 12 (accumulators in LDS) and N = COLOR_LDS_MAX_IDS + 76 (straight into the result): the same rows, the ids
    from 12 on empty and all zero."""
    from weed_instance_segmentation_amd import ops
    case = SCENES[2]
    N = case[1] if not extra else ops.color.COLOR_LDS_MAX_IDS + extra
    imgs, maps = _scene(case, 3)
    want, want_hue, thr = _reference(case, 3)
    for dt in ("f32", "i32") if extra else ("f32", "u8"):  # a uint8 map's background 200 is an id once N > 200
        sums, hue = _stats(_dev(imgs), _dev(_typed_map(maps, dt, N)), _dev(thr), N=N, K=36)
        assert _same(sums[:, :12], want) and _same(hue[:, :12], want_hue[36])
        assert int(sums[:, 12:].abs().sum()) == 0 and int(hue[:, 12:].abs().sum()) == 0
    ids = np.tile(np.arange(N, dtype=np.int32), (3, 1))
    sums, hue = _stats(_dev(imgs), _dev(maps.astype(np.int32)), _dev(thr), K=36, ids=_dev(ids), n_ids=_dev(np.full(3, N, np.int32)))
    assert _same(sums[:, :12], want) and _same(hue[:, :12], want_hue[36]) and int(sums[:, 12:].abs().sum()) == 0


@pytest.mark.parametrize("case", (SCENES[1], SCENES[3]), ids=_ids)
def test_color_stats_of_a_picture_at_an_odd_address(case):
    """The picture as a view at storage offset 1 of a flat byte buffer: the byte path, also where W % 4 == 0."""
    imgs, maps = _scene(case, 3)
    want, want_hue, thr = _reference(case, 3)
    flat = torch.zeros(imgs.size + 8, dtype=torch.uint8, device=DEV)
    view = flat[1:1 + imgs.size].view(imgs.shape)
    view.copy_(_dev(imgs))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    sums, hue = _stats(view, _dev(maps.astype(np.int32)), _dev(thr), N=case[1], K=12)
    assert _same(sums, want) and _same(hue, want_hue[12])


@pytest.mark.parametrize("shape", ((20, 512), (9, 301)))
def test_color_stats_uniform_and_checkerboard(shape):
    """One instance end to end: every wave is uniform and its partial sums leave the registers at the end of the strip
    (a wave has 4 or 5 items here; the 16-item flush is `test_color_stats_flushes_every_16_items`).  A checkerboard of
    two ids: every wave is mixed and every run is one pixel."""
    from weed_instance_segmentation_amd import ops
    H, W = shape
    rng = np.random.default_rng(H * W)
    img = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    thr = np.array([0, 40], np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for m in (np.zeros((2, H, W), np.int32), np.broadcast_to((yy + xx) % 2, (2, H, W)).astype(np.int32)):
        want, want_hue = R.color_stats_batch(img, m, 2, EXG, thr, 32, 250, 12, 16)
        sums, hue = ops.labelmap_color_stats(_dev(img), _dev(m), _dev(thr), N=2)
        assert _same(sums, want) and _same(hue, want_hue)
        big = ops.labelmap_color_stats(_dev(img), _dev(m), _dev(thr), N=ops.color.COLOR_LDS_MAX_IDS + 1)
        assert _same(big[0][:, :2], want) and _same(big[1][:, :2], want_hue)


@pytest.mark.parametrize("B", BATCHES)
def test_color_stats_flushes_every_16_items(B):
    """A one-id map of (256, 16): min_rows = 4096 / 16 = 256, so the image is one strip of 256 one-segment rows and each
    of the four waves meets 64 uniform items of the same id -- the partial sums and the hue counters are flushed after
    every 16th item, four times per wave, and start again from zero.  A second map changes its id every 80 rows (20 items of a wave), so a
    flush by the count (after 16 items) and a flush by an id change (after 4 more) alternate.  With hue, on both sides of the LDS cap, on the vector
    path and (the picture at storage offset 1) on the byte path."""
    from weed_instance_segmentation_amd import ops
    H, W = 256, 16
    rng = np.random.default_rng(256016 + B)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    thr = np.arange(B, dtype=np.int32) * 50 - 20
    flat = torch.zeros(img.size + 8, dtype=torch.uint8, device=DEV)
    odd = flat[1:1 + img.size].view(img.shape)
    odd.copy_(_dev(img))
    assert odd.data_ptr() % 4 == 1
    bands = np.broadcast_to((np.arange(H) // 80 % 3)[None, :, None], (B, H, W)).astype(np.int32)
    for m in (np.zeros((B, H, W), np.int32), bands):
        n = int(m.max()) + 1
        want, want_hue = R.color_stats_batch(img, m, n, EXG, thr, 32, 250, 36, 16)
        assert want[..., 0].sum() == B * H * W and want_hue.sum() > 0
        for N in (n, ops.color.COLOR_LDS_MAX_IDS + 1):
            for pictures in (_dev(img), odd):
                sums, hue = ops.labelmap_color_stats(pictures, _dev(m), _dev(thr), N=N, hue_bins=36)
                assert _same(sums[:, :n], want) and _same(hue[:, :n], want_hue), (N, pictures is odd)
                assert int(sums[:, n:].abs().sum()) == 0 and int(hue[:, n:].abs().sum()) == 0
                assert _same(ops.labelmap_color_stats(pictures, _dev(m), _dev(thr), N=N, hue_bins=None)[0][:, :n], want)


def test_color_stats_hand_pixels():
    from weed_instance_segmentation_amd import ops
    px = [(0, 0, 0), (255, 255, 255), (200, 1, 0), (255, 0, 1), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0),
          (90, 90, 90), (100, 110, 105), (1, 0, 0)]
    img = np.array(px, np.uint8).reshape(1, 1, -1, 3)
    m = np.arange(len(px), dtype=np.int32).reshape(1, 1, -1)  # every pixel its own instance
    thr = np.array([0], np.int32)
    for coef in ("exg", "exr5", "exgr5", (32, 0, 0), (0, 0, -32)):
        c = R.PRESETS.get(coef, coef)
        want, want_hue = R.color_stats_batch(img, m, len(px), c, thr, 32, 250, 36, 1)
        sums, hue = ops.labelmap_color_stats(_dev(img), _dev(m), _dev(thr), N=len(px), index=coef, hue_bins=36, min_chroma=1)
        assert _same(sums, want) and _same(hue, want_hue), coef
    assert want[0, 2, 11] == R.pixel_q(200, 1, 0, (0, 0, -32)) == 0
    want, _ = R.color_stats_batch(img, m, len(px), EXG, thr, 32, 250, 36, 1)
    assert want[0, 2, 11] == -4035 and want_hue[0, 3, 35] == 1  # floor, not truncation


# ------------------------------------------------------------------------------------- histogram, Otsu, mask
@pytest.mark.parametrize("case", SCENES, ids=_ids)
def test_index_hist_equals_bincount(case):
    from weed_instance_segmentation_amd import ops
    imgs, _ = _scene(case, 3)
    for coef in ("exg", "exr5", "exgr5", (1, 1, 1)):
        c = R.PRESETS.get(coef, coef)
        want = np.stack([R.index_hist(im, c) for im in imgs])
        got = ops.image_index_hist(_dev(imgs), coef)
        assert _same(got, want) and torch.equal(ops.image_index_hist(_dev(imgs), coef), got), coef
    flat = torch.zeros(imgs.size + 8, dtype=torch.uint8, device=DEV)
    view = flat[3:3 + imgs.size].view(imgs.shape)
    view.copy_(_dev(imgs))
    assert _same(ops.image_index_hist(view, (1, 1, 1)), want)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", SCENES, ids=_ids)
def test_otsu_mask_and_counts_equal_the_reference(case, B):
    from weed_instance_segmentation_amd import ColorOptions, ops, vegetation_masks, vegetation_threshold
    imgs, maps = _scene(case, B)
    thr = np.array([R.threshold_of(im, EXG) for im in imgs], np.int32)
    ref = [R.index_mask(im, EXG, t) for im, t in zip(imgs, thr)]
    for b in range(B):  # a condition on the input, asserted on the reference
        agree = float((ref[b][0].astype(bool) == (maps[b] >= 0)).mean())
        print(case, b, "otsu", int(thr[b]), "agreement", agree)
        assert agree >= 0.99
    got = vegetation_threshold(_dev(imgs))
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), thr)
    mask, counts = ops.image_index_mask(_dev(imgs), got)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), np.stack([r[0] for r in ref]))
    assert _same(counts, np.array([r[1] for r in ref]))
    again = ops.image_index_mask(_dev(imgs), got)
    assert torch.equal(again[0], mask) and torch.equal(again[1], counts)
    masks, cover = vegetation_masks(_dev(imgs), ColorOptions(), return_cover=True)
    assert torch.equal(masks, mask) and cover.dtype == torch.float64
    # one float64 division of two exact integers: two units in the last place at the most
    np.testing.assert_allclose(cover.cpu().numpy(), np.array([r[1] for r in ref], np.float64) / (case[0][0] * case[0][1]),
                               rtol=4.5e-16, atol=0)
    fixed = vegetation_masks(imgs[0], ColorOptions(threshold=int(thr[0])))
    assert tuple(fixed.shape) == case[0] and torch.equal(fixed, mask[0])


def test_vegetation_mask_to_connected_components():
    from weed_instance_segmentation_amd import vegetation_masks
    from weed_instance_segmentation_amd.annotations import connected_components
    imgs, maps = _scene(SCENES[3], 1)
    mask = vegetation_masks(_dev(imgs[0]))
    num, labels = connected_components(mask)
    assert num - 1 >= 1 and tuple(labels.shape) == SCENES[3][0]
    assert torch.equal(labels > 0, mask > 0)


def test_one_value_picture_warns_and_turns_nothing_on():
    from weed_instance_segmentation_amd import vegetation_masks, vegetation_threshold
    imgs, _ = _scene(SCENES[1], 1)
    stack = np.concatenate([imgs, np.full_like(imgs, 77)])
    with pytest.warns(RuntimeWarning, match=r"\[1\]"):
        thr = vegetation_threshold(stack)
    assert thr.tolist() == [R.threshold_of(imgs[0], EXG), 510]
    with pytest.warns(RuntimeWarning):
        masks, cover = vegetation_masks(stack, return_cover=True)
    assert int(masks[1].sum()) == 0 and float(cover[1]) == 0.0 and int(masks[0].sum()) > 0
    # the warning points at the caller's line, whichever public function met the picture
    from weed_instance_segmentation_amd import annotate_colors, color_statistics
    flat = np.full((8, 8, 3), 77, np.uint8)
    seg = np.zeros((8, 8), np.int32)
    calls = (lambda: vegetation_threshold(flat), lambda: vegetation_masks(flat), lambda: color_statistics(seg, flat, n=1),
             lambda: annotate_colors({"segmentation": seg, "segments_info": [{"id": 0}]}, flat),
             lambda: annotate_colors([{"segmentation": seg, "segments_info": [{"id": 0}]}], [flat]))
    for call in calls:
        with pytest.warns(RuntimeWarning) as record:
            call()
        assert [w.filename for w in record if issubclass(w.category, RuntimeWarning)] == [__file__]


# ------------------------------------------------------------------------------------------------- the host layer
def test_color_statistics_against_the_host():
    from weed_instance_segmentation_amd import ColorOptions, color_from_sums, color_statistics
    from weed_instance_segmentation_amd.color import dominant_hue
    case = SCENES[4]
    imgs, maps = _scene(case, 3)
    want, want_hue, _ = _reference(case, 3)
    opt = ColorOptions(threshold=THRESHOLD, dark=DARK, bright=BRIGHT, hue_bins=12)
    thr = np.full(3, THRESHOLD, np.int32)
    want = R.color_stats_batch(imgs, maps, case[1], EXG, thr, DARK, BRIGHT)[0]
    got = color_statistics(_dev(maps.astype(np.int32)), _dev(imgs), n=case[1], options=opt)
    host = color_from_sums(torch.from_numpy(want), "exg")
    assert _same(got["area"], want[..., 0]) and _same(got["hue_histogram"], want_hue[12])
    for k, h in host.items():
        if k == "area":
            continue
        g = got[k].cpu()
        assert g.dtype == torch.float64 and g.shape == h.shape
        both = ~torch.isnan(h)
        assert torch.equal(torch.isnan(g), torch.isnan(h))
        diff = ((g[both] - h[both]).abs() / h[both].abs().clamp_min(1e-300)).max().item() if both.any() else 0.0
        print(k, "largest relative difference device / host", diff)
        torch.testing.assert_close(g[both], h[both], rtol=1e-9, atol=0)
    torch.testing.assert_close(got["dominant_hue"].cpu(), dominant_hue(torch.from_numpy(want_hue[12])), rtol=0, atol=0,
                               equal_nan=True)
    # against numpy directly, for one instance
    i = int(np.argmax(want[0, :, 0]))
    px = imgs[0][maps[0] == i].astype(np.float64)
    np.testing.assert_allclose(got["mean_rgb"][0, i].cpu().numpy(), px.mean(0), rtol=1e-9)
    np.testing.assert_allclose(got["std_rgb"][0, i].cpu().numpy() ** 2, px.var(0), rtol=1e-9)
    np.testing.assert_allclose(float(got["index_std"][0, i]) ** 2, (px @ np.array(EXG, np.float64)).var(), rtol=1e-9)


def _result(case):
    imgs, maps = _scene(case, 1)
    seg = torch.from_numpy(maps[0].astype(np.float32))
    infos = [{"id": i, "label_id": i % 2, "score": 0.5} for i in (3, 0, 5, 40)]  # 40 owns no pixel
    return imgs[0], {"segmentation": seg, "segments_info": infos}


def test_annotate_colors_on_a_dict_and_a_list():
    from weed_instance_segmentation_amd import COLOR_TRAITS, ColorOptions, annotate_colors, color_statistics
    image, result = _result(SCENES[3])
    before = copy.deepcopy(result["segments_info"])
    opt = ColorOptions(index="exgr5", hue_bins=6)
    out = annotate_colors(result, image, opt)
    assert result["segments_info"] == before and out is not result and out["segmentation"] is result["segmentation"]
    traits = color_statistics(result["segmentation"], image, ids=[3, 0, 5, 40], options=opt)
    for k, (info, old) in enumerate(zip(out["segments_info"], before)):
        assert set(info) - set(old) == set(COLOR_TRAITS) and all(info[key] == old[key] for key in old)
        assert isinstance(info["index_mean"], float) and isinstance(info["mean_rgb"], list) and len(info["mean_rgb"]) == 3
        assert all(isinstance(v, int) for v in info["hue_histogram"]) and len(info["hue_histogram"]) == 6
        assert info["hue_histogram"] == traits["hue_histogram"][k].tolist()
        if old["id"] == 40:
            assert np.isnan(info["index_mean"]) and np.isnan(info["dominant_hue"]) and sum(info["hue_histogram"]) == 0
        else:
            assert info["mean_rgb"] == traits["mean_rgb"][k].tolist() and 0.0 <= info["vegetation_fraction"] <= 1.0
    both = annotate_colors([result, result], [image, torch.from_numpy(image.copy()).to(DEV)], opt)
    assert isinstance(both, list) and len(both) == 2
    for one in both:  # NaN is not equal to itself: compare the printed entries
        assert [str(s) for s in one["segments_info"]] == [str(s) for s in out["segments_info"]]
    with pytest.raises(ValueError):
        annotate_colors(result, image[:, :-1], opt)


class _StubProcessor:
    """One instance per tile: the pixels whose green byte exceeds the red one."""

    def __call__(self, images):
        return {"pixel_values": torch.stack(list(images))}

    def post_process_instance_segmentation(self, outputs, target_sizes, **kw):
        out = []
        for t in outputs:
            seg = torch.where(t[..., 1] > t[..., 0], 0.0, -1.0).to(torch.float32)
            out.append({"segmentation": seg, "segments_info": [{"id": 0, "label_id": 1, "score": 0.9}] if bool((seg == 0).any()) else []})
        return out


def test_segment_tiled_with_colors():
    from weed_instance_segmentation_amd import COLOR_TRAITS, ColorOptions, segment_tiled
    (H, W), N = (96, 160), 10
    image, _ = R.scene(np.random.default_rng(3), (H, W), N)

    def model(pixel_values):
        return pixel_values

    plain = segment_tiled(image, model, _StubProcessor(), tile=64, overlap=16, batch_size=2)
    again = segment_tiled(image, model, _StubProcessor(), tile=64, overlap=16, batch_size=2, colors=None)
    assert torch.equal(plain["segmentation"], again["segmentation"]) and plain["segments_info"] == again["segments_info"]
    assert plain["segments_info"] and not set(COLOR_TRAITS) & set(plain["segments_info"][0])
    got = segment_tiled(image, model, _StubProcessor(), tile=64, overlap=16, batch_size=2, colors=ColorOptions(threshold=70))
    assert torch.equal(got["segmentation"], plain["segmentation"]) and len(got["segments_info"]) == len(plain["segments_info"])
    seg = plain["segmentation"].cpu().numpy()
    for info, old in zip(got["segments_info"], plain["segments_info"]):
        assert set(info) - set(old) == set(COLOR_TRAITS)
        px = image[seg == old["id"]].astype(np.float64)
        np.testing.assert_allclose(info["mean_rgb"], px.mean(0), rtol=1e-9)
        assert info["mean_rgb"][1] > info["mean_rgb"][0]  # green above red, as the stub segmented
    with pytest.raises(TypeError):
        segment_tiled(image, model, _StubProcessor(), tile=64, overlap=16, colors="exg")


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        img = torch.zeros(2, 8, 12, 3, dtype=torch.uint8, device=DEV)
        m = torch.zeros(2, 8, 12, dtype=torch.int32, device=DEV)
        thr = torch.zeros(2, dtype=torch.int32, device=DEV)
        bad = [
            lambda: ops.labelmap_color_stats(img.float(), m, thr, N=2),                     # dtypes
            lambda: ops.labelmap_color_stats(img, m.to(torch.int64), thr, N=2),
            lambda: ops.labelmap_color_stats(img, m, thr.to(torch.int64), N=2),
            lambda: ops.labelmap_color_stats(img, m[:, :7], thr, N=2),                      # shapes that disagree
            lambda: ops.labelmap_color_stats(img[..., :2], m, thr, N=2),
            lambda: ops.labelmap_color_stats(img, m, thr, N=2, index=(0, 0, 0)),            # coefficient bounds
            lambda: ops.labelmap_color_stats(img, m, thr, N=2, index=(16, -16, 1)),
            lambda: ops.labelmap_color_stats(img, m, thr, N=2, index="ndvi"),
            lambda: ops.labelmap_color_stats(img, m, thr, N=2, hue_bins=7),                 # K
            lambda: ops.labelmap_color_stats(img, m, thr, N=2, hue_bins=72),
            lambda: ops.labelmap_color_stats(img, m, thr, N=2, min_chroma=0),               # min_chroma
            lambda: ops.labelmap_color_stats(img, m, thr, N=2, min_chroma=256),
            lambda: ops.labelmap_color_stats(img, m, thr[:1], N=2),                         # thresholds shape
            lambda: ops.labelmap_color_stats(img, m, thr, N=2, dark=256),
            lambda: ops.labelmap_color_stats(img, m, thr),                                  # neither N nor ids
            lambda: ops.labelmap_color_stats(img.cpu(), m, thr, N=2),                       # not on the GPU
            lambda: ops.image_index_hist(img[0]),
            lambda: ops.image_index_hist(img, (33, 0, 0)),
            lambda: ops.image_index_hist(img.cpu()),
            lambda: ops.image_index_mask(img, thr.view(2, 1)),
            lambda: ops.image_index_mask(img, thr.float()),
            lambda: ops.image_index_mask(img, thr, (0, 0, 0)),
        ]
        for call in bad:
            with pytest.raises((Wm2fError, ValueError)):
                call()
        assert timer.records == {}  # the wrappers refused before the one launch path was entered
        with pytest.raises(Wm2fError, match="N <= 4096"):
            ops.labelmap_color_stats(img, m, thr, N=5000)  # the library's own limit, checked before anything is enqueued
        ops.labelmap_color_stats(img, m, thr, N=2)  # and the timer does see a launch
        assert len(timer.records["color_stats"]) == 2
    finally:
        ops.set_kernel_timer(None)
