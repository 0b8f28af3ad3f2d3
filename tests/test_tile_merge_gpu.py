"""Tiled inference on the GPU: the four kernels of csrc/tiles.hip one by one and merge_tile_results /
segment_tiled end to end, every comparison exact equality against the numpy restatement of tests/tile_merge_reference.py."""
import functools
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
import tile_merge_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
# widths that are no multiple of 4, rectangles narrower than a wave and wider than several wave steps, local x offsets
# aligned in one tile and not in the other (150 x 150: 28 against 0, 29 against 0)
SMALL = R.GEOMETRIES + [(1, 70, 32, 8), (70, 1, 32, 8), (37, 53, 32, 8)]
# several workgroups per rectangle and per cell: pixel by pixel (cuts and origins not multiples of 4), and four pixels per
# lane (everything a multiple of 128; a 512 x 256 rectangle is two workgroups)
BIG = [(700, 900, 384, 96), (768, 768, 512, 256)]
DTYPES = {"f32": np.float32, "i32": np.int32}
CASES = ([(g, fill, dt, 64) for g in SMALL for fill in ("scene", "blocks") for dt in DTYPES]
         + [(g, fill, dt, N) for g in ((150, 150, 64, 31), (37, 53, 32, 8)) for fill, dt in (("scene", "f32"), ("blocks", "i32"))
            for N in (100, 200, 256)]      # N = 100: the largest LDS histogram in use; 200, 256: global bins
         # ids up to N - 1 with n_ids = N: the far corner of the (N+1)^2 bins, areas and labels indexed up to N - 1
         + [(g, "scene_full", dt, N) for g in ((150, 150, 64, 31), (37, 53, 32, 8)) for dt in DTYPES for N in (100, 200, 256)]
         + [(g, "blocks", dt, 64) for g in BIG for dt in DTYPES])


def _ids(case):
    (H, W, tile, overlap), fill, dt, N = case
    return f"{H}x{W}-t{tile}-o{overlap}-{fill}-{dt}-N{N}"


@functools.lru_cache(maxsize=None)
def _case(case):
    """The inputs of one case as numpy arrays, with values that are no id sprinkled in, and the reference's results."""
    from weed_instance_segmentation_amd import tile_windows
    (H, W, tile, overlap), fill, dt, N = case
    seed = abs(hash((H, W, tile, overlap, ("scene", "blocks", "scene_full").index(fill), dt == "f32", N))) % (2 ** 31)
    g = tile_windows(H, W, tile, overlap)
    T = len(g.windows)
    if fill in ("scene", "scene_full"):
        truth, obj_labels = R.scene(H, W, seed)
        tiles, n_ids, labels = R.cut_scene(truth, obj_labels, g.windows, 64 if fill == "scene" else N, N, seed + 1)
    else:
        tiles, n_ids, labels = R.random_blocks(T, g.th, g.tw, N, seed)
        n_ids[0] = 4  # ids 4 and 5 of the first tile are beyond its n_ids
    rng = np.random.default_rng(seed + 2)
    tiles = tiles.astype(DTYPES[dt])
    where = rng.random(tiles.shape) < 0.02
    junk = np.array([2.5, np.nan, -0.0, np.inf, -7.0], np.float32) if dt == "f32" else np.array([N, N + 5, 2 ** 30, -5], np.int32)
    tiles[where] = junk[rng.integers(0, len(junk), int(where.sum()))]
    ref = R.merge(tiles, n_ids, labels, g.geom_table(), g.pair_table(), H, W, 1, 2)
    return SimpleNamespace(grid=g, tiles=tiles, n_ids=n_ids, labels=labels, N=N, ref=ref, H=H, W=W)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _eq(t, a):
    return np.array_equal(t.cpu().numpy(), a)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_four_ops_one_by_one(case):
    from weed_instance_segmentation_amd import ops
    c = _case(case)
    tiles, n_ids, labels = _dev(c.tiles), _dev(c.n_ids), _dev(c.labels)
    geom, pairs = _dev(c.grid.geom_table()), _dev(c.grid.pair_table())
    hist = ops.tile_pair_counts(tiles, n_ids, pairs, c.N)
    owned = ops.tile_owned_counts(tiles, n_ids, geom, c.N)
    assert _eq(hist, c.ref["hist"])
    assert _eq(owned, c.ref["owned"])
    # each later step from the reference's inputs, so one wrong kernel fails its own line
    remap, n_merged = ops.tile_link(_dev(c.ref["hist"]), pairs, labels, n_ids, _dev(c.ref["owned"]), (1, 2))
    assert int(n_merged) == c.ref["n_merged"]
    assert _eq(remap, c.ref["remap"])
    out = ops.tile_compose(tiles, n_ids, geom, _dev(c.ref["remap"]), (c.H, c.W))
    assert out.dtype == torch.int32 and _eq(out, c.ref["out"])
    # a second call returns identical tensors
    assert torch.equal(ops.tile_pair_counts(tiles, n_ids, pairs, c.N), hist)
    assert torch.equal(ops.tile_owned_counts(tiles, n_ids, geom, c.N), owned)
    remap2, n2 = ops.tile_link(hist, pairs, labels, n_ids, owned, (1, 2))
    assert torch.equal(remap2, remap) and torch.equal(n2, n_merged)
    assert torch.equal(ops.tile_compose(tiles, n_ids, geom, remap, (c.H, c.W)), out)


def test_other_thresholds():
    from weed_instance_segmentation_amd import ops
    c = _case(((150, 150, 64, 31), "blocks", "i32", 64))
    pairs, labels, n_ids = _dev(c.grid.pair_table()), _dev(c.labels), _dev(c.n_ids)
    hist, owned = _dev(c.ref["hist"]), _dev(c.ref["owned"])
    counts = []
    for num, den in ((0, 1), (1, 3), (2, 3), (1, 1), (3, 2)):
        want, n = R.link(c.ref["hist"], c.grid.pair_table(), c.labels, c.n_ids, c.ref["owned"], num, den)
        remap, n_merged = ops.tile_link(hist, pairs, labels, n_ids, owned, (num, den))
        assert int(n_merged) == n and _eq(remap, want)
        counts.append(n)
    assert counts == sorted(counts) and counts[0] < counts[-1]  # a higher bar links less


def _results(c, dtype):
    """Per-tile results as the post-processor gives them: n_ids[t] instances each."""
    rng = np.random.default_rng(7)
    out = []
    for t in range(len(c.tiles)):
        info = [{"id": i, "label_id": int(c.labels[t, i]), "was_fused": False, "score": round(float(rng.random()), 6)}
                for i in range(int(c.n_ids[t]))]
        out.append({"segmentation": _dev(c.tiles[t].astype(dtype)), "segments_info": info})
    return out


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == 64 and c[0] not in BIG], ids=_ids)
def test_merge_tile_results_end_to_end(case):
    from weed_instance_segmentation_amd import merge_tile_results
    c = _case(case)
    results = _results(c, c.tiles.dtype)
    N = int(c.n_ids.max())  # merge_tile_results sizes its tables by the tiles' instance counts
    ref = R.merge(c.tiles, c.n_ids, c.labels[:, :N], c.grid.geom_table(), c.grid.pair_table(), c.H, c.W, 1, 2)
    got = merge_tile_results(results, c.grid, return_instance_stats=True)
    seg = got["segmentation"]
    assert seg.is_cuda and seg.dtype == torch.int32 and _eq(seg, ref["out"])
    want = R.expected_segments(ref["remap"], ref["n_merged"], [r["segments_info"] for r in results])
    area = np.bincount(ref["out"][ref["out"] >= 0], minlength=ref["n_merged"])
    assert len(got["segments_info"]) == ref["n_merged"]
    for k, (g, w) in enumerate(zip(got["segments_info"], want)):
        assert {key: g[key] for key in w} == w
        assert g["area"] == area[k] > 0
        ys, xs = np.nonzero(ref["out"] == k)
        assert g["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
        assert g["centroid"] == (xs.sum() / area[k], ys.sum() / area[k])
    plain = merge_tile_results(results, c.grid)
    assert torch.equal(plain["segmentation"], seg) and plain["segments_info"] == want


def test_no_instances_and_single_tile():
    from weed_instance_segmentation_amd import merge_tile_results, tile_windows
    g = tile_windows(97, 131, 64, 16)
    empty = [{"segmentation": torch.full((64, 64), -1.0, device=DEV), "segments_info": []} for _ in g.windows]
    got = merge_tile_results(empty, g, return_instance_stats=True)
    assert got["segments_info"] == [] and bool((got["segmentation"] == -1).all()) and tuple(got["segmentation"].shape) == (97, 131)
    g1 = tile_windows(40, 50, 64, 16)
    m = np.full((40, 50), -1, np.int32)
    m[3:9, 4:30] = 1  # id 0 owns nothing: it is not reported, and id 1 becomes 0
    one = [{"segmentation": _dev(m), "segments_info": [{"id": 0, "label_id": 1, "score": 0.5, "was_fused": False},
                                                       {"id": 1, "label_id": 0, "score": 0.75, "was_fused": False}]}]
    got = merge_tile_results(one, g1)
    assert got["segments_info"] == [{"id": 0, "label_id": 0, "score": 0.75, "was_fused": False, "members": [(0, 1)]}]
    assert _eq(got["segmentation"], np.where(m == 1, 0, -1))


def test_downstream_consumers_take_the_merged_map():
    from weed_instance_segmentation_amd import (MeanAveragePrecision, encode_label_maps, instance_statistics,
                                                merge_tile_results, render_segmentation, tile_windows, trace_label_maps)
    H, W = 97, 131
    g = tile_windows(H, W, 64, 16)
    truth, obj_labels = R.scene(H, W, 5)
    tiles, n_ids, labels = R.cut_scene(truth, obj_labels, g.windows, 64, 64, 6)
    c = SimpleNamespace(tiles=tiles, n_ids=n_ids, labels=labels)
    ref = R.merge(tiles, n_ids, labels, g.geom_table(), g.pair_table(), H, W)
    got = merge_tile_results(_results(c, np.float32), g)
    seg, n = got["segmentation"], len(got["segments_info"])
    assert _eq(seg, ref["out"]) and n == len(obj_labels) and R.same_up_to_bijection(ref["out"], truth)
    area, bbox, centroid = instance_statistics(seg, n=n)
    assert np.array_equal(area.cpu().numpy(), np.bincount(ref["out"][ref["out"] >= 0], minlength=n))
    rles = encode_label_maps(seg, n=n)
    assert sorted(k for k in rles if k >= 0) == list(range(n))
    loops = trace_label_maps(seg, n=n)
    assert sorted(loops) == list(range(n))
    image = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    picture, legend = render_segmentation(image, got, id2label={0: "crop", 1: "weed"})
    assert tuple(picture.shape) == (H, W, 3) and picture.dtype == torch.uint8
    metric = MeanAveragePrecision()
    metric.update_from_maps([seg], [got["segments_info"]], [(truth + 1).astype(np.int32)],
                            [{k + 1: int(v) for k, v in enumerate(obj_labels)}])
    assert float(metric.compute()["map"]) == 1.0  # the scene, recovered exactly, with its own labels


# ------------------------------------------------------------------------------------------------ the model route
THRESHOLD = 0.1  # the tiny model's instance scores lie between 0.1 and 0.2


@functools.lru_cache(maxsize=None)
def _tiny_model():
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    g = load_golden("full_tiny.npz")
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig.from_dict(json.loads(str(g["config_json"]))))
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    return model.cuda().eval()


def test_segment_tiled_equals_the_hand_composition():
    from weed_instance_segmentation_amd import Mask2FormerImageProcessor, segment_tiled, tile_windows
    model = _tiny_model()
    proc = Mask2FormerImageProcessor(do_resize=False)  # a 64 x 64 tile is fed as 64 x 64
    image = np.random.default_rng(11).integers(0, 256, (96, 160, 3), dtype=np.uint8)
    got = segment_tiled(image, model, proc, tile=64, overlap=16, batch_size=2, threshold=THRESHOLD)
    # by hand: the same public calls with the same batching, then the numpy reference
    g = tile_windows(96, 160, 64, 16)
    dev_image = torch.from_numpy(image).cuda()
    crops = [dev_image[y0:y1, x0:x1] for y0, x0, y1, x1 in g.windows]
    results = []
    with torch.no_grad():
        for s in range(0, len(crops), 2):
            inputs = proc(images=crops[s:s + 2])
            assert tuple(inputs["pixel_values"].shape[-2:]) == (64, 64)
            outputs = model(pixel_values=inputs["pixel_values"])
            results += proc.post_process_instance_segmentation(outputs, threshold=THRESHOLD,
                                                               target_sizes=[(64, 64)] * len(crops[s:s + 2]))
    T = len(results)
    n_ids = np.array([len(r["segments_info"]) for r in results], np.int32)
    N = int(n_ids.max())
    labels = np.full((T, N), -1, np.int32)
    for t, r in enumerate(results):
        labels[t, :n_ids[t]] = [s["label_id"] for s in r["segments_info"]]
    tiles = np.stack([r["segmentation"].cpu().numpy() for r in results])
    ref = R.merge(tiles, n_ids, labels, g.geom_table(), g.pair_table(), 96, 160, 1, 2)
    want = R.expected_segments(ref["remap"], ref["n_merged"], [r["segments_info"] for r in results])
    print("instances per tile", n_ids.tolist(), "merged", ref["n_merged"], "members", [len(w["members"]) for w in want])
    assert n_ids.max() >= 2, "no tile keeps two instances: the test would pass on next to nothing"
    assert any(len({t for t, _ in w["members"]}) >= 2 for w in want), "no pair links"
    assert _eq(got["segmentation"], ref["out"])
    assert got["segments_info"] == want


def test_segment_tiled_on_an_image_smaller_than_a_tile():
    from weed_instance_segmentation_amd import Mask2FormerImageProcessor, segment_tiled
    model = _tiny_model()
    proc = Mask2FormerImageProcessor(size={"height": 64, "width": 64})
    image = torch.from_numpy(np.random.default_rng(12).integers(0, 256, (48, 48, 3), dtype=np.uint8))
    got = segment_tiled(image, model, proc, tile=64, overlap=16, threshold=THRESHOLD, return_instance_stats=True)
    with torch.no_grad():
        outputs = model(pixel_values=proc(images=image)["pixel_values"])
    plain = proc.post_process_instance_segmentation(outputs, threshold=THRESHOLD, target_sizes=[(48, 48)],
                                                    return_instance_stats=True)[0]
    seg = plain["segmentation"].cpu().numpy().astype(np.int32)
    alive = [s for s in plain["segments_info"] if s["area"] > 0]  # an instance painted over entirely is not reported
    assert len(alive) >= 1
    table = np.full(len(plain["segments_info"]) + 1, -1, np.int32)
    table[[s["id"] for s in alive]] = np.arange(len(alive))
    assert _eq(got["segmentation"], table[seg])  # ids kept in order; dense when every instance owns a pixel
    for k, (g, s) in enumerate(zip(got["segments_info"], alive)):
        assert g["members"] == [(0, s["id"])] and g["id"] == k
        assert all(g[key] == s[key] for key in ("label_id", "score", "area", "bbox", "centroid"))
    assert len(got["segments_info"]) == len(alive)


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    from weed_instance_segmentation_amd import _lib, merge_tile_results, ops, tile_windows
    g = tile_windows(4, 12, 8, 4)
    tiles = torch.full((2, 4, 8), -1, dtype=torch.int32)
    n_ids = torch.zeros(2, dtype=torch.int32)
    geom, pairs = torch.from_numpy(g.geom_table()), torch.from_numpy(g.pair_table())
    with pytest.raises(_lib.Wm2fError):
        ops.tile_pair_counts(tiles, n_ids, pairs, 4)
    with pytest.raises(_lib.Wm2fError):
        ops.tile_compose(tiles.cuda(), n_ids.cuda(), geom, torch.zeros(2, 4, dtype=torch.int32).cuda(), (4, 12))
    with pytest.raises(_lib.Wm2fError):
        merge_tile_results([{"segmentation": tiles[0], "segments_info": []}] * 2, g)
    d = lambda t: t.cuda()
    with pytest.raises(_lib.Wm2fError, match="at most"):  # N beyond the cap: the library's own answer
        ops.tile_pair_counts(d(tiles), d(n_ids), d(pairs), 257)
    with pytest.raises(_lib.Wm2fError, match="at most"):
        ops.tile_owned_counts(d(tiles), d(n_ids), d(geom), 300)
    with pytest.raises(_lib.Wm2fError, match="at most"):
        ops.tile_link(torch.zeros(1, 258, 258, dtype=torch.int32).cuda(), d(pairs), torch.zeros(2, 257, dtype=torch.int32).cuda(),
                      d(n_ids), torch.zeros(2, 257, dtype=torch.int32).cuda())
    with pytest.raises(_lib.Wm2fError, match="threshold"):
        ops.tile_link(torch.zeros(1, 5, 5, dtype=torch.int32).cuda(), d(pairs), torch.zeros(2, 4, dtype=torch.int32).cuda(),
                      d(n_ids), torch.zeros(2, 4, dtype=torch.int32).cuda(), (1, 0))
    with pytest.raises(TypeError):
        ops.tile_owned_counts(d(tiles).to(torch.uint8), d(n_ids), d(geom), 4)
