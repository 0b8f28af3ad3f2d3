"""Nearest-instance maps, growth and cell counts on the device against tests/nearest_reference.py, bit
for bit, and the bounds of the C ABI."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nearest_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8}
N_IDS = 6

# W of 1, W % 4 != 0 (7, 3, 9, 65, 257: the pixel-by-pixel staging) and W % 4 == 0 (20, 300); rows below 1024 pixels
# share a workgroup.  The columns pass gives a chunk at least 32 rows, and exactly 32 at every size here: H = 31, 32, 33 sit
# around one chunk, 67 and 130 are three and five chunks with a short last one.
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (31, 9), (32, 20), (33, 65), (67, 257), (130, 300)]
KINDS = ["speckle", "discs", "checker", "full", "none", "single"]
# r = 0, 1, 2 (max_d2 = 5: not a square), 5, 37 -- larger than a chunk, so the warm-up spans two chunks above and below, and
# at least the width of the narrow maps
CAPS = [0, 1, 5, 25, 37 * 37 + 3]


def _keys(kind, H, W):
    """(H, W) int64 ids of [0, N_IDS) with -1 for a free pixel."""
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "speckle":
        return np.where(rng.random((H, W)) < 0.02, rng.integers(0, N_IDS, (H, W)), -1)
    if kind == "discs":
        m = np.full((H, W), -1, np.int64)
        for k in range(N_IDS):
            r = int(rng.integers(1, max(2, min(H, W) // 5 + 1)))
            cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
        return m
    if kind == "checker":  # single pixels of ids 1 and 4 alternating on the even lattice, free between them: ties everywhere
        return np.where((yy % 2 == 0) & (xx % 2 == 0), 1 + ((yy // 2 + xx // 2) % 2) * 3, -1)
    if kind == "full":
        return (yy + xx) % N_IDS
    if kind == "none":
        return np.full((H, W), -1, np.int64)
    m = np.full((H, W), -1, np.int64)  # "single"
    m[H // 2, W // 3] = 3
    return m


def _typed(keys, dtype):
    """The key map in a map dtype; free pixels as values that are no id of [0, N_IDS): 255 for uint8, a mix for the others."""
    H, W = keys.shape
    if dtype == torch.uint8:
        return np.where(keys < 0, 255, keys).astype(np.uint8)
    if dtype == torch.int32:
        m = keys.astype(np.int32)
        m[(keys < 0) & (np.arange(H * W).reshape(H, W) % 3 == 0)] = N_IDS + 1  # an id beyond N is free
        return m
    f = keys.astype(np.float32)
    free = keys < 0
    pick = np.arange(H * W).reshape(H, W) % 4
    f[free & (pick == 0)] = np.nan
    f[free & (pick == 1)] = 2.5
    f[free & (pick == 2)] = float(N_IDS)
    zeros = np.argwhere(keys == 0)
    if len(zeros):
        f[tuple(zeros[len(zeros) // 2])] = -0.0
    return f


SUBSET = np.array([0, 1, 0, 1, 1, 0], np.uint8)  # ids 1, 3 and 4 are sources


@functools.lru_cache(maxsize=None)
def _case(kind, shape, dtype, cap, subset, blocked):
    """(map, nearest, d2) computed once and shared; none is written to."""
    m = _typed(_keys(kind, *shape), DTYPES[dtype])
    near, d2 = R.nearest_separable(m, N_IDS, cap, SUBSET if subset else None, blocked)
    for a in (m, near, d2):
        a.setflags(write=False)
    return m, near, d2


def _run(ops, maps, cap, subset, blocked, **kw):
    source = torch.from_numpy(np.tile(SUBSET, (maps.shape[0], 1))).to(DEV) if subset else None
    return ops.labelmap_nearest(maps, N_IDS, cap, source, blocked, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelmap_nearest_equals_restatement(shape, kind):
    from weed_instance_segmentation_amd import ops
    assert ops.labelmaps.NEAREST_MIN_CHUNK_ROWS == 32
    claimed = 0
    for i, dtype in enumerate(sorted(DTYPES)):
        for cap in CAPS:
            for subset, blocked in ((False, False), (True, False), (True, True)) if i == 0 else ((True, bool(cap % 2)),):
                m, near, d2 = _case(kind, shape, dtype, cap, subset, blocked)
                dev = torch.from_numpy(m.copy()).to(DEV).unsqueeze(0)
                got_n, got_d = _run(ops, dev, cap, subset, blocked)
                assert got_n.dtype == got_d.dtype == torch.int32 and got_n.shape == got_d.shape == dev.shape
                bad = int((got_n[0].cpu().numpy() != near).sum()) + int((got_d[0].cpu().numpy() != d2).sum())
                assert bad == 0, (shape, kind, dtype, cap, subset, blocked, bad)
                again = _run(ops, dev, cap, subset, blocked)
                assert torch.equal(again[0], got_n) and torch.equal(again[1], got_d), "a second call differs"
                walked = _run(ops, dev, cap, subset, blocked, walk_all=True)
                assert torch.equal(walked[0], got_n) and torch.equal(walked[1], got_d), "the early none changes a result"
                claimed += int(((near >= 0) & (d2 > 0)).sum())
    if kind in ("speckle", "discs", "checker", "single") and shape[0] * shape[1] >= 200:
        assert claimed > 100  # the comparison is not one of maps where nothing is ever in range


def test_checkerboard_ties_take_the_smaller_id():
    """Single pixels of ids 1 and 4 alternate on the even lattice of an odd-sided map: every free pixel has two or four
    sources equally far, half of them of either id, and takes id 1."""
    from weed_instance_segmentation_amd import ops
    m, near, d2 = _case("checker", (33, 65), "i32", 25, False, False)
    key = R.id_keys(np.where(m == N_IDS + 1, -1, m))
    free = key < 0
    assert free.sum() > 1500 and (near[free] == 1).all() and set(d2[free].tolist()) == {1, 2}
    got_n, _ = ops.labelmap_nearest(torch.from_numpy(m.copy()).to(DEV).unsqueeze(0), N_IDS, 25, None, False)
    assert np.array_equal(got_n[0].cpu().numpy(), near)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_labelmap_nearest_stack(dtype):
    """B = 3 with different content and different sources per image, also where a workgroup's rows cross from one image
    into the next."""
    from weed_instance_segmentation_amd import ops
    sources = np.array([[1, 1, 1, 1, 1, 1], [0, 1, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0]], np.uint8)
    for shape in [(5, 3), (67, 257), (130, 300)]:
        maps = np.stack([_typed(_keys(k, *shape), DTYPES[dtype]) for k in ("discs", "speckle", "full")])
        for cap, blocked in ((25, True), (37 * 37 + 3, False)):
            want = [R.nearest_separable(maps[b], N_IDS, cap, sources[b], blocked) for b in range(3)]
            got_n, got_d = ops.labelmap_nearest(torch.from_numpy(maps).to(DEV), N_IDS, cap, torch.from_numpy(sources).to(DEV), blocked)
            assert np.array_equal(got_n.cpu().numpy(), np.stack([w[0] for w in want])), (shape, cap)
            assert np.array_equal(got_d.cpu().numpy(), np.stack([w[1] for w in want])), (shape, cap)


def test_labelmap_nearest_long_rows():
    """A row of 1024 pixels or more has a workgroup to itself; beyond 4096 it gets 1024 threads, beyond 8192 more than
    64 KiB of LDS.  W % 4 != 0 among them."""
    from weed_instance_segmentation_amd import ops
    assert (ops.labelmaps.NEAREST_ROW_PIXELS, ops.labelmaps.NEAREST_WIDE_ROW) == (1024, 4096)
    rng = np.random.default_rng(7)
    for H, W in [(3, 1100), (2, 4100), (2, 11003)]:
        m = np.where(rng.random((H, W)) < 0.004, rng.integers(0, N_IDS, (H, W)), -1).astype(np.int32)
        m[:, 2 * W // 3:] = -1  # a long stretch with nothing in range
        for cap in (25, 70 * 70):
            near, d2 = R.nearest_separable(m, N_IDS, cap)
            got_n, got_d = ops.labelmap_nearest(torch.from_numpy(m).to(DEV).unsqueeze(0), N_IDS, cap, None, True)
            assert np.array_equal(got_n[0].cpu().numpy(), near) and np.array_equal(got_d[0].cpu().numpy(), d2), (H, W, cap)


def test_labelmap_nearest_unaligned_view_and_arguments():
    from weed_instance_segmentation_amd import _lib, ops
    for dtype in ("f32", "u8"):
        m, near, d2 = _case("discs", (32, 20), dtype, 25, True, True)
        flat = torch.zeros(m.size + 1, dtype=DTYPES[dtype], device=DEV)
        flat[1:] = torch.from_numpy(m.copy()).to(DEV).reshape(-1)
        view = flat[1:].view(1, 32, 20)
        assert view.data_ptr() % (4 * flat.element_size()) != 0 and view.is_contiguous()
        got_n, got_d = _run(ops, view, 25, True, True)
        assert np.array_equal(got_n[0].cpu().numpy(), near) and np.array_equal(got_d[0].cpu().numpy(), d2)
    z = torch.zeros(1, 4, 4, device=DEV)
    with pytest.raises(TypeError):
        ops.labelmap_nearest(torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV), 2, 4)
    with pytest.raises(ValueError):
        ops.labelmap_nearest(torch.zeros(4, 4, device=DEV), 2, 4)
    with pytest.raises(ValueError):
        ops.labelmap_nearest(z, 0, 4)
    with pytest.raises(ValueError):
        ops.labelmap_nearest(z, 2, -1)
    with pytest.raises(ValueError):
        ops.labelmap_nearest(z, 2, 4, torch.zeros(1, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.Wm2fError):  # through ops: the launch reports the unsupported cap
        ops.labelmap_nearest(z, 2, 1024 * 1024 + 1)
    n_bool, _ = ops.labelmap_nearest(z, 2, 4, torch.tensor([[False, True]], device=DEV))  # a bool source list
    assert (n_bool == 0).all()  # blocked: id 0 is no source and keeps its pixels


def test_bounds_of_the_c_abi():
    """Sizes alone decide: nothing of that size is allocated, the pointers are never looked at."""
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)

    def near(B, H, W, N=4, cap=9, flags=0):
        return lib.wm2f_labelmap_nearest(null, _lib.WM2F_I32, null, null, null, null, B, H, W, N, cap, flags, null)

    def cells(B, H, W, N=4, G=1, ch=4, cw=4, oy=0, ox=0, veto_max=0):
        return lib.wm2f_labelmap_cell_counts(null, _lib.WM2F_I32, null, null, veto_max, null, B, H, W, N, G, ch, cw, oy, ox, null)

    for B, H, W in [(1, 16385, 4), (1, 4, 16385), (33, 4, 4)]:
        assert near(B, H, W) == _lib.WM2F_EUNSUPPORTED and lib.wm2f_labelmap_nearest_workspace(B, H, W) == -1
        assert cells(B, H, W) == _lib.WM2F_EUNSUPPORTED
    assert near(1, 4, 4, N=4097) == _lib.WM2F_EUNSUPPORTED and cells(1, 4, 4, N=4097) == _lib.WM2F_EUNSUPPORTED
    assert near(1, 4, 4, cap=1024 * 1024 + 1) == _lib.WM2F_EUNSUPPORTED
    assert cells(1, 4, 4, ch=16385) == _lib.WM2F_EUNSUPPORTED
    for B, H, W in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (1, -1, 4)]:
        assert near(B, H, W) == _lib.WM2F_EINVAL and cells(B, H, W) == _lib.WM2F_EINVAL
    assert near(1, 4, 4, N=0) == _lib.WM2F_EINVAL and near(1, 4, 4, cap=-1) == _lib.WM2F_EINVAL
    assert near(1, 4, 4, flags=4) == _lib.WM2F_EINVAL and near(1, 4, 4, flags=-1) == _lib.WM2F_EINVAL
    for kw in ({"G": 0}, {"G": 9}, {"ch": 0}, {"cw": 0}, {"oy": 4}, {"ox": -1}, {"veto_max": -1}):
        assert cells(1, 4, 4, **kw) == _lib.WM2F_EINVAL, kw
    assert near(1, 4, 4) == _lib.WM2F_EINVAL and cells(1, 4, 4) == _lib.WM2F_EINVAL  # in bounds: now the null pointers count
    assert lib.wm2f_labelmap_nearest_workspace(32, 16384, 16384) == 6 * 32 * 16384 * 16384
    assert lib.wm2f_labelmap_nearest_workspace(1, 3, 3) == 32 + 36  # 18 bytes of g rounded up to 16s, then 9 ids


# ----------------------------------------------------------------------------------------------------------- growth
def test_grow_label_maps_on_the_golden_instance_maps():
    from conftest import load_golden
    from weed_instance_segmentation_amd import grow_label_maps, nearest_instance_maps
    g = load_golden("postprocess_instances.npz")
    for name in ("seg_mixed_0", "seg_small_0", "seg_small_2"):
        m = g[name].astype(np.int32)
        n = int(m.max()) + 1
        assert n >= 1
        for margin, sources in ((0, None), (2.5, None), (4, list(range(0, n, 2)))):
            want = R.grow(m, n, margin, sources)
            got = grow_label_maps(m, n, margin, sources)
            assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want), (name, margin)
            assert np.array_equal(got.cpu().numpy()[m >= 0], m[m >= 0])  # instance pixels never change
        # the device form, a stack, float distances
        stack = torch.from_numpy(np.stack([m, m[::-1].copy()])).to(DEV)
        near, dist = nearest_instance_maps(stack, n, 3, sources=np.arange(n) % 2 == 0, squared=False)
        want = [R.nearest_separable(a, n, 9, np.arange(n) % 2 == 0, False) for a in (m, m[::-1])]
        assert np.array_equal(near.cpu().numpy(), np.stack([w[0] for w in want]))
        d = dist.cpu().numpy()
        assert np.isinf(d[near.cpu().numpy() < 0]).all() and d.dtype == np.float32
        ok = near.cpu().numpy() >= 0
        assert np.array_equal(d[ok], np.sqrt(np.stack([w[1] for w in want])[ok].astype(np.float64)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------ cell counts
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_cell_counts_equal_restatement(dtype):
    from weed_instance_segmentation_amd import ops
    rng = np.random.default_rng(382)
    H, W = 37, 53
    m = _typed(np.where(rng.random((H, W)) < 0.6, rng.integers(0, N_IDS, (H, W)), -1), DTYPES[dtype])
    veto = rng.integers(0, 30, (H, W)).astype(np.int32)
    dev = torch.from_numpy(m).to(DEV).unsqueeze(0)
    groups = {1: np.array([0, 255, 0, 255, 0, 0], np.uint8), 8: np.array([7, 0, 255, 3, 5, 7], np.uint8)}
    # cells that do not divide H or W, offsets, 1 x 1, larger than the image, one pixel row / column per cell
    for cell, off in (((4, 5), (0, 0)), ((4, 5), (3, 4)), ((1, 1), (0, 0)), ((64, 80), (20, 33)), ((37, 53), (0, 0)),
                      ((1, 53), (0, 7)), ((37, 1), (5, 0)), ((16, 16), (15, 15))):
        for G, group in groups.items():
            for vd in (None, veto):
                want = R.cell_counts(m, group, G, cell, off, vd, 11)
                got = ops.labelmap_cell_counts(dev, torch.from_numpy(group).to(DEV).unsqueeze(0), G, cell, off,
                                               None if vd is None else torch.from_numpy(vd).to(DEV).unsqueeze(0), 11)
                assert got.dtype == torch.int32 and tuple(got.shape) == (1,) + want.shape
                assert np.array_equal(got[0].cpu().numpy(), want), (cell, off, G, vd is None)


def test_cell_counts_stack_of_many_tiles():
    """More cells than one workgroup's tile in both directions, B = 3 with a group row per image, twice the same."""
    from weed_instance_segmentation_amd import ops
    rng = np.random.default_rng(383)
    B, H, W = 3, 70, 600
    m = np.where(rng.random((B, H, W)) < 0.5, rng.integers(0, N_IDS, (B, H, W)), -1).astype(np.int32)
    group = rng.integers(0, 3, (B, N_IDS)).astype(np.uint8)
    group[1, 2] = 255
    veto = rng.integers(0, 30, (B, H, W)).astype(np.int32)
    for cell, off in (((3, 2), (1, 1)), ((8, 8), (0, 5))):
        want = np.stack([R.cell_counts(m[b], group[b], 3, cell, off, veto[b], 9) for b in range(B)])
        args = (torch.from_numpy(m).to(DEV), torch.from_numpy(group).to(DEV), 3, cell, off, torch.from_numpy(veto).to(DEV), 9)
        got = ops.labelmap_cell_counts(*args)
        assert np.array_equal(got.cpu().numpy(), want), (cell, off)
        assert torch.equal(ops.labelmap_cell_counts(*args), got)
    with pytest.raises(ValueError):
        ops.labelmap_cell_counts(args[0], args[1], 3, (4, 4), (4, 0))
    with pytest.raises(ValueError):
        ops.labelmap_cell_counts(args[0], args[1], 9, (4, 4))
    with pytest.raises(ValueError):
        ops.labelmap_cell_counts(args[0], args[1][:2], 3, (4, 4))
    with pytest.raises(TypeError):
        ops.labelmap_cell_counts(args[0], args[1], 3, (4, 4), veto_d2=args[5].float())
