"""Skeleton graphs on the device against tests/skeleton_graph_reference.py: `out`, `status`, `labels`
and `sums` bit for bit, every call twice, at the labelling tile's edges, across tile corners, on hand cases and ragged
maps, and the host layer (`prune_skeleton_maps`, `skeleton_branch_maps`, `skeleton_graph_statistics`,
`annotate_skeletons` with `prune`).

A case is (the original id map or None, the skeleton map, d2, N).  The skeletons of ragged maps are the restatement's
thinning at 64 iterations, which settles all of them (asserted)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import distance_reference as D
import skeleton_graph_reference as G
import skeleton_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _thinned(m, N, rounds=64):
    sk, status = S.skeleton(m, N, rounds)
    assert (np.atleast_2d(status)[:, 2] == 0).all(), "the restatement's thinning has not settled"
    d2 = np.stack([D.squared_distance(x, True) for x in m]) if m.ndim == 3 else D.squared_distance(m, True)
    return sk, d2.astype(np.int32)


def _ragged(H, W, seed, n):
    m = S.ragged(H, W, seed, n)
    return (m, *_thinned(m, n), n)


def _hand(name):
    sk, d2, N = G.HAND[name]()
    return None, sk, d2.astype(np.int32), N


def _stack():
    """Three images: a ragged map (two busy rounds), an empty one, a T (one busy round)."""
    a, sk, d2, _ = _ragged(70, 90, 7, 9)
    t, td, _ = G.hand_t()
    tt, tdd = np.full((70, 90), -1, np.int32), np.ones((70, 90), np.int32)
    tt[20:32, 30:46], tdd[20:32, 30:46] = t, td
    empty = np.full((70, 90), -1, np.int32)
    return None, np.stack([sk, empty, tt]), np.stack([d2, np.zeros_like(d2), tdd]), 12  # ids 9 .. 11 own no pixel


def _unsettled():
    m = np.zeros((16, 16), np.int32)
    sk, status = S.skeleton(m, 1, 2)
    assert status[2] != 0  # a 12 x 12 block: the re-thinning has work of its own
    return m, sk, D.squared_distance(m, True).astype(np.int32), 1


def _corners():
    sk, d2, N = G.across_corners()
    return None, sk, d2.astype(np.int32), N


CASES = {
    "31x31": lambda: _ragged(31, 31, 31, 5), "32x32": lambda: _ragged(32, 32, 32, 5), "33x33": lambda: _ragged(33, 33, 33, 5),
    "65x33": lambda: _ragged(65, 33, 65, 6), "40x1": lambda: _ragged(40, 1, 4, 3), "1x40": lambda: _ragged(1, 40, 4, 3),
    "corners": _corners, "stack": _stack, "unsettled": _unsettled,
    "ragged128": lambda: _ragged(128, 128, 1, 23), "ragged256": lambda: _ragged(256, 256, 2, 23),
    **{f"hand_{k}": functools.partial(_hand, k) for k in G.HAND},
}


@functools.lru_cache(maxsize=None)
def _case(name):
    m, sk, d2, N = CASES[name]()
    for a in (m, sk, d2):
        if a is not None:
            a.setflags(write=False)
    return m, sk, d2, N


@functools.lru_cache(maxsize=None)
def _want(name, N=None, min_pixels=2, ratio_q=16, rounds=8, rethin=4):
    """The restatement's (out, status, labels and sums of the input, labels and sums of out), computed once."""
    _, sk, d2, n = _case(name)
    N = n if N is None else N
    out, status = G.prune(sk, d2, N, min_pixels, ratio_q, rounds, rethin)
    res = (out, status, *G.graph(sk, N), *G.graph(out, N))
    for a in res:
        a.setflags(write=False)
    return res


def _dev(a):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t.unsqueeze(0) if t.dim() == 2 else t


def _twice(fn, *args, **kw):
    got, again = fn(*args, **kw), fn(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "a second call differs"
    return got


def _same(got: torch.Tensor, want: np.ndarray, what):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype, (what, g.dtype)
    assert np.array_equal(g.reshape(want.shape), want), what


def _check(name, settles=True, **kw):
    from weed_instance_segmentation_amd import ops
    _, sk, d2, n = _case(name)
    N = kw.get("N", n)
    out, status, labels, sums, labels_out, sums_out = _want(name, **kw)
    if settles:
        assert (np.atleast_2d(status)[:, 2] == 0).all(), (name, "the restatement has not settled", status.tolist())
    args = {k: v for k, v in kw.items() if k != "N"}
    g_out, g_status = _twice(ops.labelmap_skeleton_prune, _dev(sk), _dev(d2), N, **args)
    _same(g_out, out, (name, kw, "out"))
    _same(g_status, status, (name, kw, "status"))
    g_labels, g_sums = _twice(ops.labelmap_skeleton_graph, _dev(sk), N=N)
    _same(g_labels, labels, (name, "labels"))
    _same(g_sums, sums, (name, "sums"))
    g_labels, g_sums = _twice(ops.labelmap_skeleton_graph, g_out, N=N)
    _same(g_labels, labels_out, (name, kw, "labels of out"))
    _same(g_sums, sums_out, (name, kw, "sums of out"))
    return status


@pytest.mark.parametrize("name", ["31x31", "32x32", "33x33", "65x33", "40x1", "1x40"])
def test_tile_edges(name):
    _check(name)
    _check(name, ratio_q=32)


def test_spurs_and_node_clusters_across_tile_corners_and_branches_along_borders():
    status = _check("corners")
    assert status.tolist() == [312, 1, 0, 17]
    _, _, labels, sums, _, sums_out = _want("corners")
    for c in (32, 64):  # the node cluster has a pixel in each of the four tiles around the corner
        assert len({labels[y, x] for y in (c - 1, c) for x in (c - 1, c)}) == 1 and labels[c, c] <= -2
    assert sums[:, 1].tolist() == [6, 6, 3] and sums_out[:, 1].tolist() == [4, 4, 0]


@pytest.mark.parametrize("name", sorted(G.HAND))
def test_hand_cases(name):
    _check("hand_" + name)


@pytest.mark.parametrize("ratio_q", [16, 24, 32])
@pytest.mark.parametrize("name", ["ragged128", "ragged256"])
def test_ragged_maps(name, ratio_q):
    status = _check(name, ratio_q=ratio_q)
    assert status[3] > 0 and 2 <= status[1] <= 3


def test_stack_with_an_empty_image_and_uneven_rounds():
    status = _check("stack")
    assert status[:, 1].tolist() == [2, 0, 1] and status[1].tolist() == [0, 0, 0, 0]
    _check("stack", rounds=3)  # the first round that confirms the slowest image
    assert _check("stack", rounds=2, settles=False)[:, 2].tolist()[1:] == [0, 0]  # one short of it: only that image says so
    assert _want("stack", rounds=2)[1][0, 2] != 0


def test_values_that_are_no_instance():
    from weed_instance_segmentation_amd import ops
    _check("ragged128", N=10)  # ids 10 .. 22 are dead
    _check("ragged128", N=30)  # ids 23 .. 29 own no pixel
    assert not _want("ragged128", N=30)[3][23:].any()
    _, sk, d2, _ = _case("ragged128")
    out, status = _twice(ops.labelmap_skeleton_prune, _dev(sk), _dev(d2), 0)
    assert (out == -1).all() and status.cpu().tolist() == [[0, 0, 0, 0]]
    labels, sums = _twice(ops.labelmap_skeleton_graph, _dev(sk), N=0)
    assert (labels == -1).all() and sums.shape == (1, 0, 8)
    odd = sk.copy()
    odd[0, :5], odd[1, :5], odd[2, :5] = -7, 23, 2 ** 31 - 1
    want = G.prune(odd, d2, 23)
    got = _twice(ops.labelmap_skeleton_prune, _dev(odd), _dev(d2), 23)
    _same(got[0], want[0], "odd values, out")
    _same(got[1], want[1], "odd values, status")
    _same(ops.labelmap_skeleton_graph(_dev(odd), N=23)[0], G.graph(odd, 23)[0], "odd values, labels")


def test_unsettled_input_is_thinned_by_the_round():
    status = _check("unsettled")
    assert status.tolist() == [1, 2, 0, 143]


def test_no_pruning_is_the_identity():
    status = _check("ragged128", min_pixels=0, ratio_q=0)
    assert status[1:].tolist() == [0, 0, 0] and np.array_equal(_want("ragged128", min_pixels=0, ratio_q=0)[0], _case("ragged128")[1])


def test_rounds_too_small_is_reported_and_defined():
    status = _check("ragged128", ratio_q=32, rounds=2, settles=False)
    assert status[2] != 0 and status[1] == 2
    assert _check("ragged128", ratio_q=32, rounds=1, rethin=1, settles=False)[2] != 0


def test_unaligned_view():
    from weed_instance_segmentation_amd import ops
    _, sk, d2, N = _case("ragged128")
    out, status, labels, sums, _, _ = _want("ragged128")
    views = []
    for a in (sk, d2):
        flat = torch.full((a.size + 1,), -1, dtype=torch.int32, device=DEV)
        flat[1:] = torch.from_numpy(a.copy()).to(DEV).reshape(-1)
        views.append(flat[1:].view(1, 128, 128))
        assert views[-1].data_ptr() % 16 != 0 and views[-1].is_contiguous()
    g_out, g_status = _twice(ops.labelmap_skeleton_prune, views[0], views[1], N)
    _same(g_out, out, "out")
    _same(g_status, status, "status")
    g_labels, g_sums = _twice(ops.labelmap_skeleton_graph, views[0], N=N)
    _same(g_labels, labels, "labels")
    _same(g_sums, sums, "sums")


def test_graph_rows_of_listed_ids():
    from weed_instance_segmentation_amd import ops
    _, sk, _, _ = _case("ragged128")
    ids = [3, 7, 8, 20, 22, 40]  # ascending; 40 owns nothing
    ids_t = torch.tensor([ids + [0, 0]], dtype=torch.int32, device=DEV)
    n_ids = torch.tensor([6], dtype=torch.int32, device=DEV)
    labels, sums = _twice(ops.labelmap_skeleton_graph, _dev(sk), ids_t, n_ids)
    want_labels, want = G.graph(sk, ids=ids + [-1, -1])
    _same(labels, want_labels, "labels")
    _same(sums, want, "sums")
    assert want[:5, 0].all() and not want[5:].any() and (want_labels[np.isin(sk, [0, 1, 2])] == -1).all()


def test_bounds_of_the_c_abi_and_arguments():
    import ctypes
    from weed_instance_segmentation_amd import _lib, ops
    z = torch.zeros(1, 4, 4, dtype=torch.int32, device=DEV)
    for kw in ({"N": -1}, {"N": 2, "min_pixels": -1}, {"N": 2, "ratio_q": 1025}, {"N": 2, "rounds": 0}, {"N": 2, "rounds": 65},
               {"N": 2, "rethin": 0}, {"N": 2, "rethin": 17}):
        with pytest.raises(ValueError):
            ops.labelmap_skeleton_prune(z, z, **kw)
    with pytest.raises(_lib.Wm2fError):
        ops.labelmap_skeleton_prune(z, z, 5000)  # through ops: the launch reports the unsupported size
    with pytest.raises(_lib.Wm2fError):
        ops.labelmap_skeleton_graph(z, N=5000)
    with pytest.raises(TypeError):
        ops.labelmap_skeleton_prune(z.float(), z, 2)
    with pytest.raises(ValueError):
        ops.labelmap_skeleton_prune(z, z[:, :2], 2)
    with pytest.raises(ValueError):
        ops.labelmap_skeleton_graph(z)
    lib = _lib.load()
    out = torch.empty_like(z)
    ws = torch.empty(lib.wm2f_labelmap_skeleton_prune_workspace(1, 4, 4), dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.wm2f_labelmap_skeleton_prune(p(z), p(z), p(z), p(out), p(ws), 1, 4, 4, 2, 2, 16, 8, 4, None) == _lib.WM2F_EINVAL
    assert b"overlaps" in lib.wm2f_last_error()


# ------------------------------------------------------------------------------------------- the public interface
def _same_floats(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(g[~np.isnan(g)], want[~np.isnan(want)])


def _public_want(m, ids, N, rounds=64, prune=(2, 16, 8, 4)):
    """The restatement's (pruned skeleton, thinning status, prune status, stats rows, graph rows, traits) of a map."""
    sk, st = S.skeleton(m, N, rounds)
    d2 = D.squared_distance(m, True)
    out, pst = G.prune(sk, d2, N, *prune)
    rows = S.skeleton_stats(out, ids=ids, d2=d2)
    return out, st, pst, rows, G.graph(out, ids=ids)[1], S.traits(rows, D.instance_stats(m, ids)[:, 0])


def test_public_maps_and_graph_statistics():
    from weed_instance_segmentation_amd import (PruneOptions, SkeletonOptions, prune_skeleton_maps, skeleton_branch_maps,
                                                skeleton_graph_statistics, skeleton_maps, skeleton_statistics)
    m, sk, d2, N = _case("ragged128")
    out, status, labels, _, labels_out, _ = _want("ragged128")
    got, st = prune_skeleton_maps(sk, m, N, return_status=True)
    assert got.shape == sk.shape and np.array_equal(got.cpu().numpy(), out) and st.cpu().tolist() == status.tolist()
    assert np.array_equal(prune_skeleton_maps(torch.from_numpy(sk.copy()).to(DEV), m.astype(np.float32), N).cpu().numpy(), out)
    wide = G.prune(sk, d2, N, 3, 24, 4, 2)[0]
    assert np.array_equal(prune_skeleton_maps(sk, m, N, PruneOptions(3, 1.5, 4, 2)).cpu().numpy(), wide)
    assert np.array_equal(skeleton_branch_maps(sk, N).cpu().numpy(), labels)
    opts = SkeletonOptions(prune=PruneOptions())
    assert np.array_equal(skeleton_maps(m, N, opts).cpu().numpy(), out)
    assert np.array_equal(skeleton_branch_maps(skeleton_maps(np.stack([m, m]), N, opts), N)[1].cpu().numpy(), labels_out)
    ids = list(range(25))  # 23 and 24 own nothing
    _, _, pst, rows, grows, want = _public_want(m, ids, 25)
    got = skeleton_graph_statistics(m.astype(np.float32), n=25)
    plain = skeleton_statistics(m, n=25, options=opts)
    for k, col in (("skeleton_pixels", 0), ("tips", 3), ("junction_pixels", 4)):
        assert got[k].dtype == torch.int64 and got[k].cpu().tolist() == rows[:, col].tolist() and torch.equal(plain[k], got[k])
    for k in ("skeleton_length", "mean_width", "max_width", "length_per_area"):
        _same_floats(got[k], want[k])
        _same_floats(plain[k], want[k])
    for k, v in G.traits(grows).items():
        assert got[k].dtype == torch.int64 and got[k].cpu().tolist() == v.tolist(), k
    assert got["pruned_pixels"].cpu().tolist() == [int(pst[3])] * 25 and got["prune_settled"].all() and got["settled"].all()
    assert set(plain) | set(G.traits(grows)) | {"pruned_pixels", "prune_settled"} == set(got)
    assert got["tips"].sum() < skeleton_statistics(m, n=25)["tips"].sum()  # the pruning is what the traits see
    order = [20, 3, 22, 7, 40, 8]
    stack = np.stack([m, m[::-1].copy()])
    sel = skeleton_graph_statistics(torch.from_numpy(stack).to(DEV), ids=order, options=SkeletonOptions(widths=False))
    assert "mean_width" not in sel and sel["branches"].shape == (2, 6)
    for b in range(2):
        _, _, pst, rows, grows, want = _public_want(stack[b], order, 41)
        assert sel["tips"][b].cpu().tolist() == rows[:, 3].tolist() and sel["pruned_pixels"][b, 0].item() == pst[3]
        for k, v in G.traits(grows).items():
            assert sel[k][b].cpu().tolist() == v.tolist(), (k, b)
        _same_floats(sel["skeleton_length"][b], want["skeleton_length"])
    few = skeleton_graph_statistics(m, n=23, options=SkeletonOptions(prune=PruneOptions(ratio=2.0, max_rounds=1)))
    assert not few["prune_settled"].any() and few["settled"].all()


def test_plants_report_their_leaves_through_the_public_path():
    from weed_instance_segmentation_amd import SkeletonOptions, skeleton_graph_statistics, skeleton_statistics
    maps = np.stack([G.plant_map(*spec, seed) for spec in G.PLANTS for seed in (1, 2, 3)])
    leaves = [spec[0] for spec in G.PLANTS for _ in range(3)]
    opts = SkeletonOptions(max_iterations=256)
    raw = skeleton_statistics(maps, n=1, options=opts)["tips"][:, 0].cpu().tolist()
    got = skeleton_graph_statistics(maps, n=1, options=opts)
    assert raw == [7, 8, 6, 3, 7, 3, 10, 11, 11, 3, 3, 2]
    assert got["tips"][:, 0].cpu().tolist() == leaves and got["prune_settled"].all() and got["settled"].all()


def _outputs():
    from types import SimpleNamespace
    from conftest import load_golden
    g = load_golden("postprocess_instances.npz")
    T = torch.from_numpy
    return SimpleNamespace(class_queries_logits=T(g["class_logits"]).to(DEV), masks_queries_logits=T(g["mask_logits"]).to(DEV))


def _check_annotated(plain, noted):
    from weed_instance_segmentation_amd import SKELETON_GRAPH_TRAITS, SKELETON_TRAITS
    base = plain["segmentation"].cpu().numpy()
    ids = [int(s["id"]) for s in plain["segments_info"]]
    assert torch.equal(noted["segmentation"], plain["segmentation"]) and len(noted["segments_info"]) == len(ids)
    if not ids:
        return 0
    added = SKELETON_TRAITS + SKELETON_GRAPH_TRAITS
    _, st, pst, rows, grows, want = _public_want(base, ids, max(ids) + 1)
    assert st[2] == 0 and pst[2] == 0
    graph = G.traits(grows)
    for j, (s, t) in enumerate(zip(plain["segments_info"], noted["segments_info"])):
        assert {k: v for k, v in t.items() if k not in added} == s and set(added) <= set(t)
        assert (t["skeleton_pixels"], t["tips"], t["junction_pixels"]) == (rows[j, 0], rows[j, 3], rows[j, 4])
        assert t["settled"] is True and t["prune_settled"] is True and t["pruned_pixels"] == pst[3]
        for k, v in graph.items():
            assert isinstance(t[k], int) and t[k] == v[j], (k, j)
        for k in ("skeleton_length", "mean_width", "max_width", "length_per_area"):
            assert isinstance(t[k], float) and (t[k] == want[k][j] or (np.isnan(t[k]) and np.isnan(want[k][j]))), (k, j)
    return int(rows[:, 0].sum())


def test_annotate_skeletons_with_prune_on_the_post_processor_and_the_tile_merge():
    import split_reference as SP
    import tile_merge_reference as TM
    from weed_instance_segmentation_amd import (PruneOptions, SkeletonOptions, annotate_skeletons, merge_tile_results,
                                                tile_windows)
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    opts = SkeletonOptions(prune=PruneOptions())
    results = Mask2FormerInstancePostProcessor().post_process_instance_segmentation(
        _outputs(), threshold=0.5, target_sizes=[[50, 70], [33, 47], [50, 70]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        noted = annotate_skeletons(results, opts)
    assert sum(_check_annotated(a, b) for a, b in zip(results, noted)) > 0
    H = W = 112
    g = tile_windows(H, W, 64, 16)
    truth = SP.discs((H, W), [(43, 56, 14, 0), (69, 56, 14, 0), (20, 14, 8, 1), (90, 96, 9, 2)])
    tiles, n_ids, labels = TM.cut_scene(truth, np.array([0, 1, 0], np.int32), g.windows, 6, 6, 11)
    parts = [{"segmentation": torch.from_numpy(tiles[t]).to(DEV),
              "segments_info": [{"id": i, "label_id": int(labels[t, i]), "was_fused": False, "score": 0.5 + 0.01 * i}
                                for i in range(int(n_ids[t]))]} for t in range(4)]
    merged = merge_tile_results(parts, g)
    assert _check_annotated(merged, annotate_skeletons(merged, opts)) > 0
