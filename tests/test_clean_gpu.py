"""Repair of id maps on the GPU: `ops.labelmap_clean` bit for bit against the scipy restatement
(tests/clean_reference.py, pinned on the host by tests/test_clean_cpu.py) at the sizes where the kernels change path and
on long chains across tiles, its fixed launch count, and the layers built on it: `clean_label_maps`, the post-processor's
`clean=`, the VIA export and the tiled route."""
import itertools

import numpy as np
import pytest
import torch

import clean_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# single pixel, row and column; one pixel past a 32 x 32 tile; W % 4 != 0 (the one-pixel paint path); several tiles both
# ways with W % 4 == 0 (the 16-byte paint path)
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 33), (37, 53), (64, 64), (65, 257), (130, 516)]
DTYPES = {"f32": np.float32, "i32": np.int32, "u8": np.uint8}
OPTIONS = list(itertools.product(("all", "largest"), (0, 10), (False, True), (None, 4), (False, True)))
N = 6


def _check(got, want, what):
    out, stats, n_out = got
    w_out, w_stats, w_n = want
    assert out.shape == w_out.shape and stats.shape == w_stats.shape
    o = out.cpu().numpy()
    assert np.array_equal(o.astype(np.int64), w_out), (what, int((o != w_out).sum()))
    assert stats.dtype == torch.int64 and np.array_equal(stats.cpu().numpy(), w_stats), what
    assert n_out.dtype == torch.int32 and np.array_equal(n_out.cpu().numpy(), w_n), what


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelmap_clean_equals_restatement(shape, dtype):
    from weed_instance_segmentation_amd import ops
    H, W = shape
    maps = R.typed_maps(DTYPES[dtype], H, W)
    dev = torch.from_numpy(maps).to(DEV)
    ref = R.Cleaner(maps, N)
    for keep, min_area, fill, limit, relabel in OPTIONS:
        want = ref.run(keep, min_area, fill, limit, relabel)
        for out_dtype in (torch.int32, torch.float32):
            got = ops.labelmap_clean(dev, N, keep=keep, min_area=min_area, fill_holes=fill, max_hole_area=limit,
                                     relabel=relabel, out_dtype=out_dtype)
            assert got[0].dtype == out_dtype
            _check(got, want, (shape, dtype, keep, min_area, fill, limit, relabel, out_dtype))
        again = ops.labelmap_clean(dev, N, keep=keep, min_area=min_area, fill_holes=fill, max_hole_area=limit,
                                   relabel=relabel, out_dtype=torch.float32)
        assert all(torch.equal(a, b) for a, b in zip(again, got)), "a second call differs"
    # the no-op call gives the ids of the map back
    out, _, _ = ops.labelmap_clean(dev, N, keep="all", min_area=1)
    assert np.array_equal(out.cpu().numpy(), R.id_keys(maps, N))


@pytest.mark.parametrize("kind", ["serpentine", "spiral"])
def test_long_chains_across_tiles(kind):
    """A one-pixel wall that crosses every tile many times and the one corridor it encloses: the wall is one piece, the
    corridor one hole; opened to the border by one pixel, nothing is filled."""
    from weed_instance_segmentation_amd import ops
    make = getattr(R, kind)
    H, W = 130, 516
    closed, opened = make(H, W), make(H, W, open_to_border=True)
    maps = np.stack([closed, opened]).astype(np.int32)
    want = R.clean(maps, 1, keep="largest", fill_holes=True)
    got = ops.labelmap_clean(torch.from_numpy(maps).to(DEV), 1, keep="largest", fill_holes=True)
    _check(got, want, kind)
    stats = got[1].cpu().numpy()
    assert stats[0, 0, 1] == 1 and stats[0, 0, 2] == 1 and stats[0, 0, 4] == 1 and stats[0, 0, 5] > 40000
    assert stats[1, 0, 4] == 0 and stats[1, 0, 5] == 0 and stats[1, 0, 6] == stats[1, 0, 3]
    # inside the ring everything is the plant now
    assert bool((got[0][0, 1:H - 1, 1:W - 1] == 0).all())


@pytest.mark.parametrize("c,o", [(1, 2), (2, 0), (0, 1)])
def test_every_case_of_the_border_merge_rule(c, o):
    """3 x 3 tiles on which border pixels of value c meet all 16 combinations of the four neighbour facts the merge rule
    reads, on a top border and on a left border.  The map minus one has the ids 0 and 1 and free pixels: (1, 2) and
    (2, 0) put the pieces of an id there (next to another id, next to free pixels), (0, 1) the free components, whose
    4-connected rule reads three of the four facts."""
    from weed_instance_segmentation_amd import ops
    m = R.border_rule_map(c, o)
    top, left = R.border_rule_cases(m, c)
    assert len(top) == 16 and len(left) == 16  # a condition on the input
    maps = (m - 1).astype(np.int32)[None]
    got = ops.labelmap_clean(torch.from_numpy(maps).to(DEV), 2, keep="all", fill_holes=True)
    _check(got, R.clean(maps, 2, keep="all", fill_holes=True), ("border rule", c, o))


def test_checkerboards():
    """Two ids on a checkerboard are one piece each under 8-connectivity.  On a checkerboard of one id and free pixels
    the id is one piece as well, and under 4-connectivity the free pixels do not join into a component that reaches the
    border through the diagonal gaps: each is a component of its own, so those off the border are holes of one pixel
    and those on it stay free."""
    from weed_instance_segmentation_amd import ops
    H, W = 70, 100
    yy, xx = np.mgrid[:H, :W]
    two = ((yy + xx) % 2).astype(np.int32)
    out, stats, n_out = ops.labelmap_clean(torch.from_numpy(two[None]).to(DEV), 2, keep="largest", min_area=2, fill_holes=True)
    assert np.array_equal(out.cpu().numpy()[0], two)
    assert stats.cpu().numpy()[0, :, :4].tolist() == [[H * W // 2, 1, 1, H * W // 2]] * 2 and n_out.tolist() == [2]
    one = np.where((yy + xx) % 2 == 0, 0, -1).astype(np.int32)
    got = ops.labelmap_clean(torch.from_numpy(one[None]).to(DEV), 1, keep="largest", fill_holes=True)
    _check(got, R.clean(one[None], 1, keep="largest", fill_holes=True), "id / free checkerboard")
    s = got[1].cpu().numpy()[0, 0]
    # the id is one 8-connected piece; its diagonal gaps do not leak: every free pixel off the border is a hole of it
    interior_free = int((one[1:-1, 1:-1] < 0).sum())
    assert s[1] == 1 and s[4] == interior_free and s[5] == interior_free
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert np.array_equal(got[0].cpu().numpy()[0] < 0, (one < 0) & border)


@pytest.mark.parametrize("n", [1, 300, 1100])
def test_id_count_bounds(n):
    """Every id present as a 2 x 2 block on a 64 x 600 map (one id: the whole call with N = 1).  Up to 1024 ids the
    pieces are gathered per workgroup in LDS before they reach the result; 1100 ids take the direct path."""
    from weed_instance_segmentation_amd import ops
    m = np.full((64, 600), -1, np.int32)
    for k in range(n):
        y, x = 3 * (k // 150), 4 * (k % 150)
        m[y:y + 2, x:x + 2] = k
    m[40, 7] = 0  # a second, smaller piece of id 0
    for kw in (dict(keep="largest", min_area=2, fill_holes=True, relabel=True), dict(keep="all", min_area=5)):
        got = ops.labelmap_clean(torch.from_numpy(m[None]).to(DEV), n, **kw)
        _check(got, R.clean(m[None], n, **kw), (n, kw))
    assert got[2].tolist() == [0]  # min_area=5 leaves nothing


def test_launch_count_is_fixed():
    from weed_instance_segmentation_amd import ops
    counts = {}
    for B, n in ((1, 1), (1, 300), (3, 1), (3, 300)):
        m = torch.from_numpy(np.stack([R.block_map(64, 600, b) for b in range(B)]).astype(np.int32)).to(DEV)
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        try:
            ops.labelmap_clean(m, n, keep="largest", min_area=4, fill_holes=True, relabel=True)
        finally:
            ops.set_kernel_timer(None)
        torch.cuda.synchronize()
        counts[(B, n)] = {k: v[0] for k, v in timer.summary().items()}
    first = counts[(1, 1)]
    assert set(first) == {"clean_pieces", "clean_choose", "clean_holes", "clean_paint"} and all(v == 1 for v in first.values())
    assert all(c == first for c in counts.values()), counts


def test_arguments():
    from weed_instance_segmentation_amd import _lib, ops
    z = torch.zeros(1, 4, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError):
        ops.labelmap_clean(z.long(), 1)
    with pytest.raises(TypeError):
        ops.labelmap_clean(z, 1, out_dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.labelmap_clean(z[0], 1)
    with pytest.raises(ValueError):
        ops.labelmap_clean(z, 1, keep="biggest")
    with pytest.raises(ValueError):
        ops.labelmap_clean(z, 1, min_area=-1)
    with pytest.raises(_lib.Wm2fError):
        ops.labelmap_clean(z, 4097)
    with pytest.raises(_lib.Wm2fError):
        ops.labelmap_clean(z.cpu(), 1)
    out, stats, n_out = ops.labelmap_clean(z, 0, fill_holes=True)  # no instance at all: everything is free
    assert bool((out == -1).all()) and stats.shape == (1, 0, 8) and n_out.tolist() == [0]
    # a map whose storage is not 16-byte aligned gives the same result
    m = R.typed_maps(np.float32, 64, 64)
    flat = torch.zeros(m.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = torch.from_numpy(m).to(DEV).reshape(-1)
    a = ops.labelmap_clean(flat[1:].view(3, 64, 64), N, keep="largest", fill_holes=True)
    b = ops.labelmap_clean(torch.from_numpy(m).to(DEV), N, keep="largest", fill_holes=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the public layer
def _plants():
    """(60, 90): four plants made of overlapping rectangles (4-connected, so each traces as one outer loop), each with
    pinholes, plus detached specks of their ids; the reference's cleaned map of it."""
    m = np.full((60, 90), -1, np.int32)
    for k, (y, x) in enumerate([(4, 5), (6, 50), (34, 8), (32, 52)]):
        m[y:y + 18, x:x + 22] = k
        m[y + 6:y + 24, x + 10:x + 30] = k
        m[y + 3, x + 4] = -1                 # pinholes: free, and a pixel of another id
        m[y + 10, x + 14:x + 16] = -1
        m[y + 14, x + 20] = (k + 1) % 4
    for k, (y, x) in enumerate([(0, 40), (29, 2), (58, 45), (30, 88)]):
        m[y:y + 2, x:x + 2] = k              # specks away from their plants
    want, stats, n_out = R.clean_one(m, 4, keep="largest", min_area=4, fill_holes=True)
    return m, want, stats


def test_clean_label_maps_public_interface():
    from weed_instance_segmentation_amd import CleanOptions, clean_label_maps, instance_statistics
    m, want, stats = _plants()
    opts = CleanOptions(min_area=4, keep="largest", fill_holes=True)
    got, got_stats = clean_label_maps(torch.from_numpy(m).to(DEV), 4, opts, return_stats=True)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(got_stats.cpu().numpy(), stats) and (stats[:, 1] >= 3).all() and (stats[:, 4] >= 3).all()
    host = clean_label_maps(m.astype(np.float32), 4, keep="largest", min_area=4, fill_holes=True)  # a host map, keywords
    assert host.shape == (60, 90) and host.dtype == torch.int32 and torch.equal(host, got)
    stack = clean_label_maps(np.stack([m, m[::-1].copy()]), 4, opts, fill_holes=False, relabel=True)  # a field replaced
    assert np.array_equal(stack[0].cpu().numpy(), R.clean_one(m, 4, keep="largest", min_area=4, relabel=True)[0])
    assert np.array_equal(stack[1].cpu().numpy(), R.clean_one(m[::-1], 4, keep="largest", min_area=4, relabel=True)[0])
    # the result is an id map: the statistics kernel takes it as it is
    area, _, _ = instance_statistics(got, n=4)
    assert area.cpu().tolist() == stats[:, 6].tolist()


def _outputs():
    from types import SimpleNamespace
    from conftest import load_golden
    g = load_golden("postprocess_instances.npz")
    T = torch.from_numpy
    return SimpleNamespace(class_queries_logits=T(g["class_logits"]).to(DEV), masks_queries_logits=T(g["mask_logits"]).to(DEV))


SIZES = [[50, 70], [33, 47], [50, 70]]  # two target sizes in one batch


@pytest.mark.parametrize("min_area", [6, 40])
def test_post_processor_clean_equals_reference_on_the_uncleaned_map(min_area):
    import trace_reference as TR
    from weed_instance_segmentation_amd import CleanOptions
    from weed_instance_segmentation_amd.instances import cleaned_segments_info
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    p = Mask2FormerInstancePostProcessor()
    kw = dict(threshold=0.5, target_sizes=SIZES, return_instance_stats=True, return_polygons=True)
    plain = p.post_process_instance_segmentation(_outputs(), **kw)
    none = p.post_process_instance_segmentation(_outputs(), clean=None, **kw)
    opts = CleanOptions(min_area=min_area, keep="largest", fill_holes=True)
    res = p.post_process_instance_segmentation(_outputs(), clean=opts, **kw)
    changed = dropped = 0
    for a, z, b in zip(plain, none, res):
        assert torch.equal(a["segmentation"], z["segmentation"]) and len(a["segments_info"]) == len(z["segments_info"])
        for s, t in zip(a["segments_info"], z["segments_info"]):
            assert {k: v for k, v in s.items() if k != "polygons"} == {k: v for k, v in t.items() if k != "polygons"}
        m = a["segmentation"].cpu().numpy()
        n = len(a["segments_info"])
        want, stats, n_out = R.clean_one(m, n, keep="largest", min_area=min_area, fill_holes=True, relabel=True)
        seg = b["segmentation"]
        assert seg.dtype == a["segmentation"].dtype and np.array_equal(seg.cpu().numpy().astype(np.int64), want)
        changed += int((want != R.id_keys(m, n)).sum())
        dropped += n - n_out
        bare = [{k: v for k, v in s.items() if k in ("id", "label_id", "was_fused", "score")} for s in a["segments_info"]]
        expect = cleaned_segments_info(bare, stats[:, 7])
        assert len(b["segments_info"]) == n_out == len(expect)
        assert [s["id"] for s in b["segments_info"]] == list(range(n_out))
        loops = {}
        for k, pts, a2 in TR.trace(want, n_out, 1, True):
            loops.setdefault(k, []).append((pts, a2 < 0))
        for s, e in zip(b["segments_info"], expect):
            assert {k: s[k] for k in e} == e
            ys, xs = np.nonzero(want == s["id"])
            assert s["area"] == len(ys) > 0
            assert s["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
            assert [([tuple(q) for q in l["points"].tolist()], l["hole"]) for l in s["polygons"]] == loops[s["id"]]
            assert sum(not hole for _, hole in loops[s["id"]]) >= 1
    assert changed > 0 and (dropped > 0 or min_area < 40)
    # the run-length form and the binary stack describe the cleaned map as well
    rle = p.post_process_instance_segmentation(_outputs(), threshold=0.5, target_sizes=SIZES, clean=opts, return_coco_annotation=True)
    stack = p.post_process_instance_segmentation(_outputs(), threshold=0.5, target_sizes=SIZES, clean=opts, return_binary_maps=True)
    from weed_instance_segmentation_amd.postprocess import convert_segmentation_to_rle
    for b, r, s in zip(res, rle, stack):
        assert r["segmentation"] == convert_segmentation_to_rle(b["segmentation"].cpu())
        assert [x["id"] for x in r["segments_info"]] == [x["id"] for x in s["segments_info"]] == [x["id"] for x in b["segments_info"]]
        if b["segments_info"]:
            ids = torch.arange(len(b["segments_info"]), device=DEV).view(-1, 1, 1)
            assert torch.equal(s["segmentation"], (b["segmentation"].unsqueeze(0) == ids).float())
    with pytest.raises(TypeError):
        p.post_process_instance_segmentation(_outputs(), clean={"keep": "largest"})


def test_via_export_round_trip():
    from weed_instance_segmentation_amd import CleanOptions, clean_label_maps, via_annotations
    from weed_instance_segmentation_amd.annotations import _via_polygons, polygons_to_instance_map
    m, want, stats = _plants()
    info = [{"id": k, "label_id": k % 2, "was_fused": False, "score": 0.9} for k in range(4)]
    names = {0: "sorghum", 1: "weed"}
    raw = via_annotations([{"segmentation": torch.from_numpy(m).to(DEV), "segments_info": info}], ["a.png"], names)
    (entry,) = raw.values()
    assert len(entry["regions"]) > 4  # every speck is a region of its own: more plants than there are
    fixed = clean_label_maps(m, 4, CleanOptions(min_area=4, keep="largest", fill_holes=True))
    (entry,) = via_annotations([{"segmentation": fixed, "segments_info": info}], ["a.png"], names).values()
    assert len(entry["regions"]) == 4  # one region per instance
    polygons, ids, id_to_semantic = _via_polygons(entry, {"sorghum": 0, "weed": 1}, 1.0, 1.0, skip_255=False)
    assert ids == [1, 2, 3, 4] and id_to_semantic == {k + 1: k % 2 for k in range(4)}
    painted = polygons_to_instance_map(polygons, ids, m.shape, 0, DEV)
    assert np.array_equal(painted.cpu().numpy(), want + 1)  # the annotation tool's file repaints the cleaned map


def test_merge_tile_results_clean():
    """The fabricated two-tile case of the tile tests (a scene cut into tiles), with specks and pinholes added to the
    tiles: the cleaned merge equals the reference on the composed map."""
    import tile_merge_reference as TM
    from weed_instance_segmentation_amd import CleanOptions, merge_tile_results, tile_windows
    H, W = 64, 100
    g = tile_windows(H, W, 64, 28)
    assert g.n_tiles == 2
    truth, obj_labels = TM.scene(H, W, 5)
    tiles, n_ids, labels = TM.cut_scene(truth, obj_labels, g.windows, 64, 64, 6)
    rng = np.random.default_rng(3)
    tiles = tiles.astype(np.int32)
    for t in range(2):
        free = np.argwhere(tiles[t] < 0)
        own = np.argwhere(tiles[t] >= 0)
        for y, x in free[rng.choice(len(free), min(25, len(free)), replace=False)]:
            tiles[t, y, x] = rng.integers(0, max(1, n_ids[t]))  # specks
        for y, x in own[rng.choice(len(own), min(25, len(own)), replace=False)]:
            tiles[t, y, x] = -1                                    # pinholes
    results = [{"segmentation": torch.from_numpy(tiles[t]).to(DEV),
                "segments_info": [{"id": i, "label_id": int(labels[t, i]), "was_fused": False, "score": 0.5 + 0.01 * i}
                                  for i in range(int(n_ids[t]))]} for t in range(2)]
    plain = merge_tile_results(results, g, return_instance_stats=True)
    n = len(plain["segments_info"])
    composed = plain["segmentation"].cpu().numpy()
    opts = CleanOptions(min_area=5, keep="largest", fill_holes=True)
    want, stats, n_out = R.clean_one(composed, n, keep="largest", min_area=5, fill_holes=True, relabel=True)
    assert (want != composed).any() and stats[:, 4].sum() > 0 and (stats[:, 1] > stats[:, 2]).any()
    got = merge_tile_results(results, g, return_instance_stats=True, clean=opts)
    assert got["segmentation"].dtype == torch.int32 and np.array_equal(got["segmentation"].cpu().numpy(), want)
    assert len(got["segments_info"]) == n_out
    survivors = [s for s in plain["segments_info"] if stats[s["id"], 7] >= 0]
    for s, old in zip(got["segments_info"], survivors):
        assert s["id"] == stats[old["id"], 7] and s["members"] == old["members"] and s["label_id"] == old["label_id"]
        assert s["score"] == old["score"] and s["area"] == int((want == s["id"]).sum()) > 0
        ys, xs = np.nonzero(want == s["id"])
        assert s["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
    again = merge_tile_results(results, g)  # clean=None: as before
    assert torch.equal(again["segmentation"], plain["segmentation"])
