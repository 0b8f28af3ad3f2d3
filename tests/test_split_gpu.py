"""Splitting touching instances on the device against tests/split_reference.py: out, info and
status bit for bit, the bounds of the C ABI, and `split=` of the post-processor, the tile merge and the PNG loader.

Every input is chosen so that the restatement settles (status[2] == 0) within the rounds under test; `_check` asserts
it.  The cases that test the cap on rounds say so."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import distance_reference as D
import split_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8}
RATIOS = [(0, 1), (1, 2), (3, 4), (1, 1)]


def _typed(m, dtype):
    """An int32 map with -1 background in a map dtype; uint8 has no -1: its background is 255, an id >= N."""
    if dtype == "u8":
        return np.where(m < 0, 255, m).astype(np.uint8)
    if dtype == "f32":
        return m.astype(np.float32)
    return m.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _blobs(H, W, seed=0):
    """Overlapping discs of the ids 0 .. 2 painted over one another on background: touching parts of one id, touching
    ids, specks.  Read-only."""
    rng = np.random.default_rng(1000 * H + W + seed)
    big = max(4, min(max(H, W), 48) // 4)
    spec = [(int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(2, big)), int(rng.integers(0, 3)))
            for _ in range(16)]
    m = S.discs((H, W), spec)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _ragged(side, seed):
    m, n = S.ragged(side, seed)
    m.setflags(write=False)
    return m, n


@functools.lru_cache(maxsize=None)
def _want(name, dtype, N, M, num, den, min_peak_d2, rounds, outside):
    """The restatement's (d2, out, info, status) of a named map, computed once and shared."""
    m = _typed(MAPS[name](), dtype)
    d2 = D.squared_distance(m, outside)
    return (d2,) + S.split(m, d2, N, M, num, den, min_peak_d2, rounds)


MAPS = {
    "31x31": lambda: _blobs(31, 31), "32x32": lambda: _blobs(32, 32), "33x33": lambda: _blobs(33, 33),
    "65x33": lambda: _blobs(65, 33), "40x1": lambda: _blobs(40, 1), "1x40": lambda: _blobs(1, 40),
    "70x90": lambda: _blobs(70, 90, 3),
    # a disc whose peak is the pixel at the corner of four 32 x 32 tiles: its basin lies in all four
    "corner_basin": lambda: S.discs((64, 64), [(32, 32, 11, 0), (12, 50, 6, 0)]),
    # a bar 8 thick around the tile corner: its two middle rows, 31 and 32, tie along the whole length
    "corner_plateau": lambda: _bar_at_corner(),
    "two_discs": S.two_discs, "dumbbell": S.dumbbell_with_bump, "bar": S.bar, "disc": S.disc, "bud": S.disc_with_bud,
    "three_discs": S.three_discs,
    "ragged128": lambda: _ragged(128, 1)[0], "ragged128b": lambda: _ragged(128, 2)[0], "ragged128c": lambda: _ragged(128, 3)[0],
    "ragged256": lambda: _ragged(256, 1)[0],
}
N_OF = {"ragged128": 8, "ragged128b": 5, "ragged128c": 7, "ragged256": 23}


def _bar_at_corner():
    m = np.full((64, 64), -1, np.int32)
    m[28:36, 10:54] = 0
    return m


def _n(name):
    return N_OF.get(name, 3 if "x" in name else 1)


def _run(m, N, M, num, den, min_peak_d2, rounds, outside):
    from weed_instance_segmentation_amd import ops
    dev = torch.from_numpy(np.ascontiguousarray(m)).to(DEV)
    dev = dev.unsqueeze(0) if dev.dim() == 2 else dev
    d2 = ops.labelmap_distance(dev, outside)
    got = ops.labelmap_split(dev, d2, N, M, num, den, min_peak_d2, rounds)
    again = ops.labelmap_split(dev, d2, N, M, num, den, min_peak_d2, rounds)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "a second call differs"
    return d2, got


def _check(name, dtype="i32", N=None, M=64, num=1, den=2, min_peak_d2=0, rounds=8, outside=True, settles=True):
    N = _n(name) if N is None else N
    d2, out, info, status = _want(name, dtype, N, M, num, den, min_peak_d2, rounds, outside)
    if settles:
        assert status[2] == 0, (name, "the restatement has not settled", status.tolist())
    gd2, (gout, ginfo, gstatus) = _run(_typed(MAPS[name](), dtype), N, M, num, den, min_peak_d2, rounds, outside)
    what = (name, dtype, N, M, num, den, min_peak_d2, rounds, outside)
    assert gout.dtype == ginfo.dtype == gstatus.dtype == torch.int32
    assert gout.shape == (1,) + out.shape and ginfo.shape == (1, M, 4) and gstatus.shape == (1, 4)
    assert np.array_equal(gd2[0].cpu().numpy(), d2), what
    assert gstatus[0].cpu().tolist() == status.tolist(), what
    assert int((gout[0].cpu().numpy() != out).sum()) == 0, what
    assert np.array_equal(ginfo[0].cpu().numpy(), info), what
    return out, info, status


@pytest.mark.parametrize("name", ["31x31", "32x32", "33x33", "65x33", "40x1", "1x40", "70x90"])
def test_sides_around_the_tile_dtypes_ratios_and_clearances(name):
    """Sides around the 32-pixel tile, W = 1 and H = 1; three dtypes, four ratios, min_clearance 0 and 3."""
    seen = set()
    for dtype in sorted(DTYPES):
        for num, den in RATIOS:
            for min_peak_d2 in (0, 9):
                out, _, status = _check(name, dtype, M=48, num=num, den=den, min_peak_d2=min_peak_d2)
                seen.add((int(status[0]), int(status[1])))
    if name == "70x90":
        assert len(seen) >= 4 and max(s[1] for s in seen) > 20  # the ratios and the clearance change what is split


@pytest.mark.parametrize("name", ["corner_basin", "corner_plateau"])
def test_basin_and_plateau_across_a_tile_corner(name):
    for num, den in RATIOS:
        out, info, status = _check(name, num=num, den=den, M=8)
    assert status[1] == (2 if name == "corner_basin" else 1)
    if name == "corner_basin":
        assert info[0].tolist() == [0, 32, 32, 122] and len({int(out[y, x]) for y in (28, 35) for x in (28, 35)}) == 1
    else:
        assert info[0].tolist() == [0, 13, 31, 16]  # the first pixel of the plateau, left of and above the corner


@pytest.mark.parametrize("name,ratio,pieces", [
    ("two_discs", (1, 2), 1), ("two_discs", (3, 4), 2), ("dumbbell", (1, 2), 2), ("dumbbell", (3, 4), 3), ("bar", (1, 2), 1),
    ("bar", (3, 4), 1), ("disc", (1, 2), 1), ("disc", (3, 4), 1), ("bud", (3, 4), 1), ("bud", (9, 10), 2)])
def test_hand_cases(name, ratio, pieces):
    out, info, status = _check(name, num=ratio[0], den=ratio[1], M=8)
    assert S.pieces(out) == pieces == status[0]


@pytest.mark.parametrize("rounds,pieces,links", [(1, 2, 1), (2, 1, 1), (8, 1, 0)])
def test_rounds_are_synchronous(rounds, pieces, links):
    """Three discs in a row: the cap on rounds is what is tested, so the restatement need not have settled."""
    out, _, status = _check("three_discs", rounds=rounds, M=8, settles=False)
    assert S.pieces(out) == pieces and status[2] == links and status[3] == rounds


@pytest.mark.parametrize("name", ["ragged128", "ragged256"])
@pytest.mark.parametrize("outside", [True, False], ids=["outside", "inside"])
def test_ragged_maps(name, outside):
    for num, den in RATIOS:
        for rounds in (8,) if (num, den) != (1, 2) else (8, 32):
            _, _, status = _check(name, num=num, den=den, M=256, rounds=rounds, outside=outside)
    assert status[1] >= (45 if name == "ragged128" else 150)
    for dtype in ("f32", "u8"):
        _check(name, dtype, num=3, den=4, min_peak_d2=9, M=256, outside=outside)


def test_stack_of_three_maps():
    from weed_instance_segmentation_amd import ops
    names, N, M = ["ragged128", "ragged128b", "ragged128c"], 8, 40
    maps = np.stack([MAPS[n]() for n in names])
    d2, (out, info, status) = _run(maps, N, M, 3, 4, 0, 8, True)
    assert out.shape == (3, 128, 128) and info.shape == (3, M, 4) and status.shape == (3, 4)
    for b, name in enumerate(names):
        _, wout, winfo, wstatus = _want(name, "i32", N, M, 3, 4, 0, 8, True)
        assert wstatus[2] == 0
        assert np.array_equal(out[b].cpu().numpy(), wout) and np.array_equal(info[b].cpu().numpy(), winfo), name
        assert status[b].cpu().tolist() == wstatus.tolist(), name
    assert len({tuple(s) for s in status.cpu().tolist()}) == 3


def test_no_instances_missing_ids_and_the_id_space():
    # N = 0: everything is background
    out, info, status = _check("70x90", N=0, M=0)
    assert (out == -1).all() and status.tolist() == [0, 0, 0, 8]
    out, info, status = _check("70x90", N=0, M=4)
    assert (info == [-1, -1, -1, 0]).all()
    # ids 3 .. 5 own no pixel; id 2 is background when N = 2
    out, info, status = _check("70x90", N=6, M=48, num=1, den=1)
    assert (info[3:6] == [-1, -1, -1, 0]).all() and info[6, 0] in (0, 1, 2) and status[0] > 7
    out2, _, _ = _check("70x90", N=2, M=48, num=1, den=1)
    assert (out2[MAPS["70x90"]() == 2] == -1).all() and (out[MAPS["70x90"]() == 2] >= 0).all()
    # M = N: nothing may split off, and the count is still reported; M = N + 1: exactly the first extra
    wanted = int(status[0])
    m = MAPS["70x90"]()
    out, info, status = _check("70x90", N=6, M=6, num=1, den=1)
    assert status[0] == wanted and np.array_equal(out, np.where(m >= 0, m, -1))
    out, info, status = _check("70x90", N=6, M=7, num=1, den=1)
    assert status[0] == wanted and sorted(np.unique(out).tolist()) == [-1, 0, 1, 2, 6] and info[6, 0] >= 0


def test_unaligned_view():
    from weed_instance_segmentation_amd import ops
    for dtype in ("f32", "u8"):
        m = _typed(MAPS["ragged128"](), dtype)
        flat = torch.zeros(m.size + 1, dtype=DTYPES[dtype], device=DEV)
        flat[1:] = torch.from_numpy(m.copy()).to(DEV).reshape(-1)
        view = flat[1:].view(1, 128, 128)
        assert view.data_ptr() % (4 * flat.element_size()) != 0 and view.is_contiguous()
        d2 = ops.labelmap_distance(view)
        got = ops.labelmap_split(view, d2, 8, 64, 3, 4)
        _, out, info, status = _want("ragged128", dtype, 8, 64, 3, 4, 0, 8, True)
        assert np.array_equal(got[0][0].cpu().numpy(), out) and np.array_equal(got[1][0].cpu().numpy(), info)
        assert got[2][0].cpu().tolist() == status.tolist()


def test_bounds_of_the_c_abi_and_arguments():
    """Sizes alone decide: nothing of that size is allocated, the pointers are never looked at."""
    from weed_instance_segmentation_amd import _lib, ops
    lib = _lib.load()
    null = ctypes.c_void_p(0)

    def split(B, H, W, N, M, num=1, den=2, min_peak=0, rounds=8):
        return lib.wm2f_labelmap_split(null, _lib.WM2F_I32, null, null, null, null, null, B, H, W, N, M, num, den, min_peak,
                                       rounds, null)

    for B, H, W in [(1, 16385, 4), (1, 4, 16385), (33, 4, 4)]:
        assert split(B, H, W, 2, 4) == _lib.WM2F_EUNSUPPORTED and lib.wm2f_labelmap_split_workspace(B, H, W, 4) == -1
    assert split(1, 4, 4, 2, 4097) == _lib.WM2F_EUNSUPPORTED and lib.wm2f_labelmap_split_workspace(1, 4, 4, 4097) == -1
    assert split(1, 4, 4, 5, 4) == _lib.WM2F_EUNSUPPORTED  # N > M
    for B, H, W in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (1, -1, 4)]:
        assert split(B, H, W, 2, 4) == _lib.WM2F_EINVAL and lib.wm2f_labelmap_split_workspace(B, H, W, 4) == -1
    assert split(1, 4, 4, -1, 4) == _lib.WM2F_EINVAL
    for kw in ({"rounds": 0}, {"rounds": 33}, {"den": 0}, {"den": 1025}, {"num": 3}, {"num": -1}, {"min_peak": -1}):
        assert split(1, 4, 4, 2, 4, **kw) == _lib.WM2F_EINVAL, kw
    assert split(1, 4, 4, 2, 4) == _lib.WM2F_EINVAL  # sizes in range: now the null pointers are what is wrong
    assert lib.wm2f_labelmap_split_workspace(32, 16384, 16384, 4096) >= 16 * 32 * 16384 * 16384
    z = torch.zeros(1, 4, 4, dtype=torch.int32, device=DEV)
    for kw in ({"N": 2, "M": 1}, {"N": 2, "M": 4, "rounds": 0}, {"N": 2, "M": 4, "num": 2, "den": 1},
               {"N": 2, "M": 4, "den": 2000}, {"N": 2, "M": 4, "min_peak_d2": -1}):
        with pytest.raises(ValueError):
            ops.labelmap_split(z, z, **{"num": 1, "den": 2, **kw})
    with pytest.raises(_lib.Wm2fError):
        ops.labelmap_split(z, z, 2, 5000, 1, 2)  # through ops: the launch reports the unsupported size
    with pytest.raises(TypeError):
        ops.labelmap_split(z, z.float(), 2, 4, 1, 2)
    with pytest.raises(ValueError):
        ops.labelmap_split(z, z[:, :2], 2, 4, 1, 2)


# ------------------------------------------------------------------------------------------- the public interface
def test_split_label_maps():
    from weed_instance_segmentation_amd import SplitOptions, split_label_maps
    m = S.two_discs()
    one = split_label_maps(m, 1)
    assert one.dtype == torch.int32 and one.shape == m.shape and np.array_equal(one.cpu().numpy(), np.where(m >= 0, 0, -1))
    out, parent, peaks, clearance, n_out = split_label_maps(torch.from_numpy(m).to(DEV), 1, SplitOptions(min_neck_ratio=0.75),
                                                            return_info=True, max_instances=5)
    want, info, status = S.split_map(m, 1, 5, 3, 4)
    assert np.array_equal(out.cpu().numpy(), want) and n_out.item() == 2 == status[0]
    assert parent.cpu().tolist() == [0, 0, -1, -1, -1] and peaks.cpu().tolist() == info[:, 1:3].tolist()
    assert clearance[:2].cpu().tolist() == np.sqrt(info[:2, 3].astype(np.float64)).tolist() and torch.isnan(clearance[2:]).all()
    stack = np.stack([m, np.where(m >= 0, 1, -1).astype(np.int32)]).astype(np.float32)
    out, parent, peaks, clearance, n_out = split_label_maps(stack, 2, min_neck_ratio=0.75, min_clearance=3.0, return_info=True,
                                                            border="inside", max_instances=4)
    assert out.shape == (2,) + m.shape and parent.cpu().tolist() == [[0, -1, 0, -1], [-1, 1, 1, -1]] and n_out.cpu().tolist() == [3, 3]
    for b, N in ((0, 2), (1, 2)):
        want, info, _ = S.split_map(stack[b], N, 4, 3, 4, 9, border_outside=False)
        assert np.array_equal(out[b].cpu().numpy(), want) and peaks[b].cpu().tolist() == info[:, 1:3].tolist()
    with pytest.raises(ValueError):
        split_label_maps(m, 3, max_instances=2)


# ---------------------------------------------------------------------------------------- the post-processor
def _outputs():
    from types import SimpleNamespace
    from conftest import load_golden
    g = load_golden("postprocess_instances.npz")
    T = torch.from_numpy
    return SimpleNamespace(class_queries_logits=T(g["class_logits"]).to(DEV), masks_queries_logits=T(g["mask_logits"]).to(DEV))


def _same_result(a, b):
    assert torch.equal(a["segmentation"], b["segmentation"]) and a["segmentation"].dtype == b["segmentation"].dtype
    assert a["segments_info"] == b["segments_info"]


def _check_split_result(off, on, options):
    """`on` is `off` with its map split: the map against the restatement, the entries, and what describes the map."""
    base = off["segmentation"].cpu().numpy()
    n = len(off["segments_info"])
    f = options.neck_fraction()
    want, info, status = S.split_map(base, n, n + 64, f.numerator, f.denominator, options.kernel_arguments()["min_peak_d2"])
    assert status[2] == 0
    got = on["segmentation"].cpu().numpy()
    assert on["segmentation"].dtype == off["segmentation"].dtype and np.array_equal(got, want)
    segs = on["segments_info"]
    assert [s["id"] for s in segs] == list(range(min(int(status[0]), n + 64)))
    plain = {"area", "bbox", "centroid", "aim_point", "clearance", "polygons"}
    for s, t in zip(off["segments_info"], segs):
        assert "split_from" not in t and {k: v for k, v in t.items() if k not in plain} == {k: v for k, v in s.items() if k not in plain}
    for t in segs[n:]:
        parent = segs[t["split_from"]]
        assert t["split_from"] == info[t["id"], 0] < n and (t["label_id"], t["score"]) == (parent["label_id"], parent["score"])
    ids = list(range(len(segs)))
    stats = D.instance_stats(got, ids)
    points = D.aim_points(got, D.squared_distance(got, True), ids)
    for t in segs:
        assert t["area"] == stats[t["id"], 0]
        if t["area"] == 0:  # painted over entirely by later instances: never a part that was split off
            assert t["aim_point"] is None and t["id"] < n
            continue
        assert t["bbox"][:2] == stats[t["id"], 1:3].tolist()
        assert t["aim_point"] == tuple(points[t["id"], :2].tolist()) and got[t["aim_point"][1], t["aim_point"][0]] == t["id"]
    return len(segs) - n


@pytest.mark.parametrize("sizes", [None, [[50, 70], [33, 47], [50, 70]]], ids=["grid", "two-sizes"])
def test_post_processor_split(sizes):
    from weed_instance_segmentation_amd import CleanOptions, SplitOptions
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    p = Mask2FormerInstancePostProcessor()
    kw = dict(threshold=0.5, target_sizes=sizes)
    today = p.post_process_instance_segmentation(_outputs(), **kw)
    for a, b in zip(today, p.post_process_instance_segmentation(_outputs(), split=None, **kw)):
        _same_result(a, b)
    Q = _outputs().class_queries_logits.shape[1]
    options = SplitOptions(min_neck_ratio=1.0, max_instances=Q + 64)  # room for 64 parts, as `_check_split_result` gives
    extras = 0
    for clean in (None, CleanOptions(min_area=4, keep="largest")):
        more = dict(kw, clean=clean, return_instance_stats=True, return_aim_points=True)
        off = p.post_process_instance_segmentation(_outputs(), **more)
        on = p.post_process_instance_segmentation(_outputs(), split=options, **more)
        extras += sum(_check_split_result(a, b, options) for a, b in zip(off, on))
    assert extras > 0
    stack = p.post_process_instance_segmentation(_outputs(), split=options, return_binary_maps=True, **kw)
    maps = p.post_process_instance_segmentation(_outputs(), split=options, **kw)
    for s, m in zip(stack, maps):
        assert s["segments_info"] == m["segments_info"]
        if m["segments_info"]:
            ids = torch.arange(len(m["segments_info"]), device=DEV).view(-1, 1, 1)
            assert torch.equal(s["segmentation"], (m["segmentation"].unsqueeze(0) == ids).float())
    with pytest.raises(TypeError):
        p.post_process_instance_segmentation(_outputs(), split={"min_neck_ratio": 0.5}, **kw)


# --------------------------------------------------------------------------------------------------- the tile merge
def test_merge_tile_results_split():
    """A 2 x 2 grid of 64 x 64 tiles with overlap 16: the spanning blob is two discs joined inside the overlap."""
    import tile_merge_reference as TM
    from weed_instance_segmentation_amd import SplitOptions, merge_tile_results, tile_windows
    H = W = 112
    g = tile_windows(H, W, 64, 16)
    assert g.n_tiles == 4 and (g.th, g.tw) == (64, 64)
    truth = S.discs((H, W), [(43, 56, 14, 0), (69, 56, 14, 0), (20, 14, 8, 1), (90, 96, 9, 2)])
    obj_labels = np.array([0, 1, 0], np.int32)
    tiles, n_ids, labels = TM.cut_scene(truth, obj_labels, g.windows, 6, 6, 11)
    results = [{"segmentation": torch.from_numpy(tiles[t]).to(DEV),
                "segments_info": [{"id": i, "label_id": int(labels[t, i]), "was_fused": False, "score": 0.5 + 0.01 * i}
                                  for i in range(int(n_ids[t]))]} for t in range(4)]
    more = dict(return_instance_stats=True, return_aim_points=True)
    plain = merge_tile_results(results, g, **more)
    _same_result(plain, merge_tile_results(results, g, split=None, **more))
    assert len(plain["segments_info"]) == 3
    same = merge_tile_results(results, g, split=SplitOptions(min_neck_ratio=0.25), **more)  # the neck is half a radius
    _same_result(plain, same)
    options = SplitOptions(min_neck_ratio=0.75)
    on = merge_tile_results(results, g, split=options, **more)
    assert _check_split_result(plain, on, options) == 1
    extra = on["segments_info"][3]
    merged = on["segmentation"].cpu().numpy()
    assert merged[56, 43] != merged[56, 69] and {int(merged[56, 43]), int(merged[56, 69])} == {extra["id"], extra["split_from"]}
    # the cut runs through the overlap of the tiles, columns 48 .. 63
    assert np.nonzero(merged == merged[56, 43])[1].max() < 64 and np.nonzero(merged == merged[56, 69])[1].min() >= 48


# ------------------------------------------------------------------------------------------------- the PNG loaders
def test_loaders_split_touching_discs():
    from weed_instance_segmentation_amd import SplitOptions
    from weed_instance_segmentation_amd.annotations import color_mask_to_instance_map, semantic_to_instance_map
    shape = (56, 120)
    sem = np.zeros(shape, np.uint8)
    sem[S.discs(shape, [(28, 28, 20, 0), (58, 28, 20, 0)]) == 0] = 1  # two touching discs of class 1
    sem[S.discs(shape, [(100, 28, 12, 0)]) == 0] = 2                   # one disc of class 2
    dev = torch.from_numpy(sem).to(DEV)
    one, ids_one = semantic_to_instance_map(dev)
    again, ids_again = semantic_to_instance_map(dev, split=None)
    assert torch.equal(one, again) and ids_one == ids_again == {1: 1, 2: 2}
    two, ids_two = semantic_to_instance_map(dev, split=SplitOptions(min_neck_ratio=0.75))
    assert ids_two == {1: 1, 2: 2, 3: 1} and two.dtype == torch.int32
    m = two.cpu().numpy()
    assert np.array_equal(m == 255, sem == 0) and np.array_equal(m == 2, sem == 2)
    assert {int(m[28, 28]), int(m[28, 58])} == {1, 3} and set(np.unique(m[sem == 1]).tolist()) == {1, 3}
    want, _, _ = S.split_map(np.where(one.cpu().numpy() == 255, -1, one.cpu().numpy() - 1), 2, 66, 3, 4)
    assert np.array_equal(np.where(m == 255, -1, m - 1), want)
    kept, ids_kept = semantic_to_instance_map(dev, split=SplitOptions(min_neck_ratio=0.5))
    assert torch.equal(kept, one) and ids_kept == ids_one
    rgb = np.zeros(shape + (3,), np.uint8)
    rgb[sem == 1] = (0, 255, 0)
    rgb[sem == 2] = (255, 0, 0)
    cmap = {"crop": {"color": [0, 255, 0], "id": 0}, "weed": {"color": [255, 0, 0], "id": 1}}
    c1, d1 = color_mask_to_instance_map(torch.from_numpy(rgb).to(DEV), cmap)
    c2, d2 = color_mask_to_instance_map(torch.from_numpy(rgb).to(DEV), cmap, split=SplitOptions(min_neck_ratio=0.75))
    assert d1 == {1: 0, 2: 1} and d2 == {1: 0, 2: 1, 3: 0} and torch.equal(c2, two) and torch.equal(c1, one)
