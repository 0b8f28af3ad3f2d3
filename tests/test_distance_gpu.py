"""Interior distance maps and aim points on the device against tests/distance_reference.py: d2 and
the points bit for bit, the bounds of the C ABI, and `return_aim_points=True` of the post-processor and the tile merge."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import distance_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# W of 1, W % 4 != 0 (7, 3, 65, 257, 9: the pixel-by-pixel staging) and W % 4 == 0 (256, 300, 700, 20); rows below a wave,
# across one (65) and across a 256-pixel step (257, 300, 700); rows below 1024 pixels share a workgroup: three of 300,
# one of 700, all of the small maps.
# The columns pass gives a chunk at least 32 rows, and exactly 32 at every size here: H = 31, 32, 33 sit around one chunk,
# 64 is two whole chunks, 67, 130 and 515 are three, five and seventeen with a short last one.  (515, 700) holds discs of
# radius 100, so walks cross more than a wave's width.
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (31, 9), (32, 20), (33, 65), (64, 256), (67, 257), (130, 300), (515, 700)]
KINDS = ["random", "discs", "stripes_h", "stripes_v", "checker", "full", "none", "frame"]
DTYPES = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8}


def _keys(kind, H, W, seed=0):
    """(H, W) int64 ids with -1 for no id."""
    rng = np.random.default_rng(H * 1000 + W + 7 * seed)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "random":
        return rng.integers(-1, 5, (H, W))
    if kind == "discs":  # overlapping discs painted one over the other, the first as large as the map allows
        m = np.full((H, W), -1, np.int64)
        for k in range(6):
            r = max(1, min(H, W, 202) // 2 - 1) if k == 0 else int(rng.integers(1, max(2, min(H, W) // 3)))
            cy, cx = (H // 2, W // 2) if k == 0 else (int(rng.integers(0, H)), int(rng.integers(0, W)))
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
        return m
    if kind == "stripes_h":
        return (yy % 3).astype(np.int64)
    if kind == "stripes_v":
        return (xx % 3).astype(np.int64) - 1  # every third column carries no id
    if kind == "checker":
        return ((yy + xx) % 2).astype(np.int64)
    if kind == "full":
        return np.full((H, W), 2, np.int64)
    if kind == "none":
        return np.full((H, W), -1, np.int64)
    m = np.full((H, W), 1, np.int64)  # "frame": one instance that touches all four borders, around a hole
    m[H // 4:H - H // 4, W // 4:W - W // 4] = -1
    m[H // 2, W // 2] = 4
    return m


def _typed(keys, dtype):
    """The key map in a map dtype: uint8 has no "no id" (its background 0 is an id like any other); the wider types get
    values that are no id and, for floats, a -0.0."""
    H, W = keys.shape
    if dtype == torch.uint8:
        return (keys + 1).astype(np.uint8)
    if dtype == torch.int32:
        m = keys.astype(np.int32)
        if H * W > 8:
            m[H // 3, W // 3] = -7
            m[H // 2, W // 3] = 70000
        return m
    f = keys.astype(np.float32)
    if H * W > 8:
        f[H // 3, W // 3] = np.nan
        f[H // 2, W // 3] = 2.5
        f[H // 3, W // 2] = 2.0 ** 24
        zeros = np.argwhere(keys == 0)
        if len(zeros):
            f[tuple(zeros[len(zeros) // 2])] = -0.0
    return f


@functools.lru_cache(maxsize=None)
def _case(kind, shape, dtype, outside, seed=0):
    """(map, reference d2), computed once and shared; neither is written to."""
    m = _typed(_keys(kind, *shape, seed), DTYPES[dtype])
    want = R.squared_distance(m, outside)
    m.setflags(write=False)
    want.setflags(write=False)
    return m, want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelmap_distance_equals_restatement(shape, kind):
    from weed_instance_segmentation_amd import ops
    for dtype in sorted(DTYPES):
        for outside in (True, False):
            m, want = _case(kind, shape, dtype, outside)
            dev = torch.from_numpy(m.copy()).to(DEV).unsqueeze(0)
            got = ops.labelmap_distance(dev, outside)
            assert got.dtype == torch.int32 and got.shape == dev.shape
            bad = int((got[0].cpu().numpy() != want).sum())
            assert bad == 0, (shape, kind, dtype, outside, bad)
            assert torch.equal(ops.labelmap_distance(dev, outside), got), "a second call differs"
    if kind == "full":  # one id fills the image: nothing to be far from unless the border counts
        assert (_case(kind, shape, "u8", False)[1] == R.INT32_MAX).all()  # the uint8 map has no other value in it
    if kind == "discs" and shape == (515, 700):
        assert _case(kind, shape, "i32", True)[1].max() > 64 ** 2


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_labelmap_distance_stack(dtype):
    """B = 3 with different content per image, also where a workgroup's rows cross from one image into the next."""
    from weed_instance_segmentation_amd import ops
    for shape in [(5, 3), (67, 257), (130, 300)]:
        for outside in (True, False):
            cases = [_case(k, shape, dtype, outside) for k in ("discs", "random", "frame")]
            got = ops.labelmap_distance(torch.from_numpy(np.stack([c[0] for c in cases])).to(DEV), outside)
            assert np.array_equal(got.cpu().numpy(), np.stack([c[1] for c in cases])), (shape, outside)


def test_labelmap_distance_wide_rows():
    """Rows beyond 4096 pixels take a workgroup of 1024 threads each, and beyond 8192 more than 64 KiB of LDS."""
    from weed_instance_segmentation_amd import ops
    rng = np.random.default_rng(5)
    for H, W in [(3, 4100), (2, 11004), (2, 11003)]:
        m = np.repeat(rng.integers(-1, 3, (H, W // 37 + 1)), 37, axis=1)[:, :W].astype(np.int32)
        m[:, 5000:9000] = 7  # whole columns of one id: in border-inside mode g says nothing and the walks are long
        for outside in (True, False):
            got = ops.labelmap_distance(torch.from_numpy(m).to(DEV).unsqueeze(0), outside)
            assert np.array_equal(got[0].cpu().numpy(), R.d2_scipy(m, outside)), (H, W, outside)


def test_labelmap_distance_unaligned_view_and_arguments():
    """A map whose storage starts one element into an allocation (W % 4 == 0, but no 16-byte alignment) is staged pixel by
    pixel and gives the same result; sizes and dtypes outside the contract raise."""
    from weed_instance_segmentation_amd import _lib, ops
    for dtype in ("f32", "u8"):
        m, want = _case("discs", (64, 256), dtype, True)
        flat = torch.zeros(m.size + 1, dtype=DTYPES[dtype], device=DEV)
        flat[1:] = torch.from_numpy(m.copy()).to(DEV).reshape(-1)
        view = flat[1:].view(1, 64, 256)
        assert view.data_ptr() % (4 * flat.element_size()) != 0 and view.is_contiguous()
        aligned = ops.labelmap_distance(torch.from_numpy(m.copy()).to(DEV).unsqueeze(0))
        assert torch.equal(ops.labelmap_distance(view), aligned) and np.array_equal(aligned[0].cpu().numpy(), want)
        d2 = aligned
        pts = ops.labelmap_aim_points(view, d2, N=8)
        assert torch.equal(pts, ops.labelmap_aim_points(torch.from_numpy(m.copy()).to(DEV).unsqueeze(0), d2, N=8))
    with pytest.raises(TypeError):
        ops.labelmap_distance(torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.labelmap_distance(torch.zeros(4, 4, device=DEV))
    with pytest.raises(ValueError):
        ops.labelmap_distance(torch.zeros(1, 0, 4, device=DEV))
    with pytest.raises(_lib.Wm2fError):
        ops.labelmap_distance(torch.zeros(1, 4, 4))
    z = torch.zeros(1, 4, 4, device=DEV)
    with pytest.raises(TypeError):
        ops.labelmap_aim_points(z, z, N=2)  # d2 must be int32
    with pytest.raises(ValueError):
        ops.labelmap_aim_points(z, z.int())  # N or ids
    with pytest.raises(ValueError):
        ops.labelmap_aim_points(z, z.int(), N=2, stats=torch.zeros(1, 3, 8, dtype=torch.int64, device=DEV))


def test_bounds_of_the_c_abi():
    """Sizes alone decide: nothing of that size is allocated, the pointers are never looked at."""
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)

    def dist(B, H, W):
        return lib.wm2f_labelmap_distance(null, _lib.WM2F_I32, null, null, B, H, W, 1, null)

    def aim(B, H, W, N):
        return lib.wm2f_labelmap_aim_points(null, _lib.WM2F_I32, null, null, null, null, null, null, B, H, W, N, null)

    for B, H, W in [(1, 16385, 4), (1, 4, 16385), (33, 4, 4)]:
        assert dist(B, H, W) == _lib.WM2F_EUNSUPPORTED and lib.wm2f_labelmap_distance_workspace(B, H, W) == -1
        assert aim(B, H, W, 4) == _lib.WM2F_EUNSUPPORTED
    assert aim(1, 4, 4, 4097) == _lib.WM2F_EUNSUPPORTED and lib.wm2f_labelmap_aim_points_workspace(1, 4097) == -1
    for B, H, W in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (1, -1, 4)]:
        assert dist(B, H, W) == _lib.WM2F_EINVAL and aim(B, H, W, 4) == _lib.WM2F_EINVAL
    assert aim(1, 4, 4, 0) == _lib.WM2F_EINVAL
    assert lib.wm2f_labelmap_distance_workspace(32, 16384, 16384) >= 2 * 32 * 16384 * 16384
    assert lib.wm2f_labelmap_aim_points_workspace(32, 4096) == 20 * 32 * 4096
    with pytest.raises(_lib.Wm2fError):  # through ops: the launch reports the unsupported size
        from weed_instance_segmentation_amd import ops
        ops.labelmap_aim_points(torch.zeros(1, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int32, device=DEV), N=4097)


# ------------------------------------------------------------------------------------------------------ aim points
def _check_points(maps, d2, ids_per_image, got, centred):
    """got (B, N, 4) against the restatement, and the properties that make a point an aim point."""
    for b, ids in enumerate(ids_per_image):
        want = R.aim_points(maps[b], d2[b], ids, centred=centred)
        assert np.array_equal(got[b, :len(ids)], want), (b, centred, np.argwhere(got[b, :len(ids)] != want)[:4])
        assert (got[b, len(ids):] == np.array([-1, -1, 0, 0])).all()  # rows beyond n_ids are empty
        key = R.id_keys(maps[b])
        for r, k in enumerate(ids):
            x, y, dmax, zero = got[b, r]
            if x >= 0:
                assert key[y, x] == k and d2[b][y, x] == dmax == d2[b][key == k].max() and zero == 0
            else:
                assert not (key == k).any() or k < 0


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_aim_points_n_form(dtype):
    from weed_instance_segmentation_amd import ops
    shape = (67, 257)
    cases = [_case(k, shape, dtype, True) for k in ("discs", "random", "stripes_h", "frame")]
    maps, d2 = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    dev, dd = torch.from_numpy(maps).to(DEV), torch.from_numpy(d2).to(DEV)
    for N in (1, 9):  # ids up to 8: some without a pixel in every image
        stats = ops.labelmap_instance_stats(dev, N=N)
        for st in (stats, None):
            got = ops.labelmap_aim_points(dev, dd, N=N, stats=st)
            assert got.dtype == torch.int32 and got.shape == (4, N, 4)
            _check_points(maps, d2, [list(range(N))] * 4, got.cpu().numpy(), st is not None)
            assert torch.equal(ops.labelmap_aim_points(dev, dd, N=N, stats=st), got), "a second call differs"


def test_aim_points_bar_and_c_shape_on_the_device():
    from weed_instance_segmentation_amd import aim_points, distance_maps, instance_statistics
    bar = np.full((9, 46), -1, np.int32)
    bar[2:7, 3:43] = 1
    point, clearance = aim_points(bar, ids=[1, 7])
    assert point.dtype == torch.int64 and clearance.dtype == torch.float64 and point.is_cuda
    assert point.cpu().tolist() == [[23, 4], [-1, -1]]  # the middle of the medial line; an id without a pixel
    assert clearance[0].item() == 3.0 and bool(torch.isnan(clearance[1]))
    c = np.full((16, 16), -1.0, np.float32)
    c[2:14, 2:14] = 0
    c[5:11, 5:14] = -1
    _, _, centroid = instance_statistics(c, n=1)
    cx, cy = (int(v) for v in centroid[0].cpu().tolist())
    (x, y), = aim_points(c, n=1)[0].cpu().tolist()
    assert c[cy, cx] == -1 and c[y, x] == 0  # the centroid lies on bare soil, the aim point on the plant
    d2 = distance_maps(c)
    assert d2.dtype == torch.int32 and d2.shape == (16, 16) and np.array_equal(d2.cpu().numpy(), R.squared_distance(c, True))
    assert d2[y, x] == d2.max()
    root = distance_maps(torch.from_numpy(c).to(DEV), squared=False)
    assert root.dtype == torch.float32 and np.array_equal(root.cpu().numpy(), np.sqrt(R.squared_distance(c, True).astype(np.float64)).astype(np.float32))
    stack = np.stack([c, np.zeros_like(c)])
    inside = distance_maps(stack, border="inside")
    assert np.array_equal(inside[0].cpu().numpy(), R.squared_distance(c, False)) and (inside[1] == R.INT32_MAX).all()
    p2, cl2 = aim_points(stack, ids=[5, 0], border="inside")  # the caller's order; one id fills image 1
    assert p2.shape == (2, 2, 2) and p2[:, 0].cpu().tolist() == [[-1, -1], [-1, -1]]
    assert p2[1, 1].cpu().tolist() == [8, 8] and cl2[1, 1].item() == np.sqrt(np.float64(R.INT32_MAX))  # the rounded centroid


def test_aim_points_ids_form():
    from weed_instance_segmentation_amd import ops
    H, W = 67, 257
    keys = _keys("discs", H, W)
    table = np.array([3, 200, 70000, 5, 12, 70001])
    a = np.where(keys >= 0, table[np.clip(keys, 0, 5)], -1).astype(np.int32)
    b = np.where(_keys("random", H, W) >= 2, 200, 3).astype(np.int32)
    maps = np.stack([a, b])
    d2 = np.stack([R.squared_distance(m, True) for m in maps])
    dev, dd = torch.from_numpy(maps).to(DEV), torch.from_numpy(d2).to(DEV)
    listed = [[3, 5, 9, 200, 70000, 70001], [3, 4, 200]]  # ascending, 9 and 4 without a pixel, 12 not listed
    N = 7
    ids = torch.tensor([l + [0] * (N - len(l)) for l in listed], dtype=torch.int32, device=DEV)
    n_ids = torch.tensor([len(l) for l in listed], dtype=torch.int32, device=DEV)
    stats = ops.labelmap_instance_stats(dev, ids, n_ids)
    assert np.array_equal(stats[0, :6].cpu().numpy(), R.instance_stats(a, listed[0]))
    for st in (stats, None):
        got = ops.labelmap_aim_points(dev, dd, ids, n_ids, stats=st)
        _check_points(maps, d2, listed, got.cpu().numpy(), st is not None)


def test_aim_points_many_ids():
    """N = 1500: beyond the 1024 ids whose accumulators live in LDS."""
    from weed_instance_segmentation_amd import ops
    H, W, N = 130, 300, 1500
    rng = np.random.default_rng(15)
    blocks = rng.integers(-1, N - 20, ((H + 3) // 4, (W + 5) // 6))  # repeated ids: instances of several pieces
    m = np.kron(blocks, np.ones((4, 6), np.int64))[:H, :W].astype(np.int32)
    m[40:90, 100:220] = 17  # one instance with a real interior and a tie along its medial line
    d2 = R.squared_distance(m, True)
    dev, dd = torch.from_numpy(m).to(DEV).unsqueeze(0), torch.from_numpy(d2).to(DEV).unsqueeze(0)
    assert torch.equal(ops.labelmap_distance(dev), dd)
    stats = ops.labelmap_instance_stats(dev, N=N)
    for st in (stats, None):
        got = ops.labelmap_aim_points(dev, dd, N=N, stats=st)
        _check_points(m[None], d2[None], [list(range(N))], got.cpu().numpy(), st is not None)
    assert got[0, 17, 2].item() == 25 ** 2 and got[0, N - 1, 0].item() == -1


# ---------------------------------------------------------------------------------------- the post-processor
def _outputs():
    from types import SimpleNamespace
    from conftest import load_golden
    g = load_golden("postprocess_instances.npz")
    T = torch.from_numpy
    return SimpleNamespace(class_queries_logits=T(g["class_logits"]).to(DEV), masks_queries_logits=T(g["mask_logits"]).to(DEV))


def _check_segments(result):
    """aim_point / clearance of every entry against the restatement on the returned map."""
    m = result["segmentation"].cpu().numpy()
    n = len(result["segments_info"])
    assert [s["id"] for s in result["segments_info"]] == list(range(n))
    want = R.aim_points(m, R.squared_distance(m, True), list(range(n)))
    seen = 0
    for s, (x, y, d2max, _) in zip(result["segments_info"], want.tolist()):
        if x < 0:
            assert s["aim_point"] is None and np.isnan(s["clearance"])
            continue
        assert s["aim_point"] == (x, y) and all(type(v) is int for v in s["aim_point"])
        assert type(s["clearance"]) is float and s["clearance"] == float(np.sqrt(np.float64(d2max)))
        assert m[y, x] == s["id"]
        seen += 1
    return seen


@pytest.mark.parametrize("sizes", [None, [[50, 70], [33, 47], [50, 70]]], ids=["grid", "two-sizes"])
@pytest.mark.parametrize("cleaned", [False, True], ids=["plain", "clean"])
def test_post_processor_aim_points(cleaned, sizes):
    from weed_instance_segmentation_amd import CleanOptions
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    p = Mask2FormerInstancePostProcessor()
    kw = dict(threshold=0.5, target_sizes=sizes, clean=CleanOptions(min_area=4, keep="largest") if cleaned else None)
    seen = 0
    for stats in (False, True):  # independent of return_instance_stats
        off = p.post_process_instance_segmentation(_outputs(), return_instance_stats=stats, **kw)
        on = p.post_process_instance_segmentation(_outputs(), return_instance_stats=stats, return_aim_points=True, **kw)
        assert len(on) == len(off)
        for a, b in zip(off, on):
            assert torch.equal(a["segmentation"], b["segmentation"]) and len(a["segments_info"]) == len(b["segments_info"])
            for s, t in zip(a["segments_info"], b["segments_info"]):
                assert "aim_point" not in s and "clearance" not in s
                assert {k: v for k, v in t.items() if k not in ("aim_point", "clearance")} == s
            seen += _check_segments(b)
    assert seen > 0


# --------------------------------------------------------------------------------------------------- the tile merge
def test_merge_tile_results_aim_points():
    """A 2 x 2 grid of 64 x 64 tiles with overlap 16: one instance spans both seams, so its aim point lies in the overlap
    of all four tiles; the points are those of the merged map."""
    import tile_merge_reference as TM
    from weed_instance_segmentation_amd import merge_tile_results, tile_windows
    H = W = 112
    g = tile_windows(H, W, 64, 16)
    assert g.n_tiles == 4 and (g.th, g.tw) == (64, 64)
    truth = np.full((H, W), -1, np.int32)
    truth[36:76, 30:82] = 0   # across both seams
    truth[4:20, 6:40] = 1     # inside tile 0
    truth[90:108, 70:100] = 2  # inside tile 3
    truth[60:100, 8:14] = 3   # across the horizontal seam on the left
    obj_labels = np.array([0, 1, 0, 1], np.int32)
    tiles, n_ids, labels = TM.cut_scene(truth, obj_labels, g.windows, 6, 6, 11)
    results = [{"segmentation": torch.from_numpy(tiles[t]).to(DEV),
                "segments_info": [{"id": i, "label_id": int(labels[t, i]), "was_fused": False, "score": 0.5 + 0.01 * i}
                                  for i in range(int(n_ids[t]))]} for t in range(4)]
    plain = merge_tile_results(results, g)
    for stats in (False, True):
        off = merge_tile_results(results, g, return_instance_stats=stats)
        on = merge_tile_results(results, g, return_instance_stats=stats, return_aim_points=True)
        assert torch.equal(on["segmentation"], plain["segmentation"]) and torch.equal(off["segmentation"], plain["segmentation"])
        assert TM.same_up_to_bijection(on["segmentation"].cpu().numpy(), truth)
        assert len(on["segments_info"]) == len(off["segments_info"]) == 4
        for s, t in zip(off["segments_info"], on["segments_info"]):
            assert "aim_point" not in s and {k: v for k, v in t.items() if k not in ("aim_point", "clearance")} == s
        assert _check_segments(on) == 4
    merged = on["segmentation"].cpu().numpy()
    big = next(s for s in on["segments_info"] if s["id"] == merged[56, 56])
    x, y = big["aim_point"]
    assert 48 <= x < 64 and 48 <= y < 64 and big["clearance"] == 20.0  # in the overlap of all four tiles
    assert off["segments_info"] == merge_tile_results(results, g, return_instance_stats=True)["segments_info"]
