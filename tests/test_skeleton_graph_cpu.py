"""Skeleton graphs without a GPU: the numpy restatement against a literal flood-fill reading, the
hand cases with pinned literals, the plants' leaf counts, what pruning must keep (pieces, holes, idempotence), the
meaning of `status`, the options, the C ABI's declarations and the errors that need no device."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import distance_reference as D
import skeleton_graph_reference as G
import skeleton_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W, seed) of the ragged maps (23 ids), the ratios they are pruned at, and at ratio 1.0 (tips, pixels) before -> after
RAGGED = {(128, 128, 1): ((1.0, 1.5, 2.0), (149, 121, 1278, 1179)), (256, 256, 2): ((1.0, 1.5, 2.0), (150, 129, 2625, 2519)),
          (64, 64, 3): ((1.0,), (103, 75, 555, 475)), (96, 80, 4): ((1.0,), (136, 99, 891, 768))}


@functools.lru_cache(maxsize=None)
def _ragged(H, W, seed):
    """(map, skeleton at 256 iterations, d2) of a ragged map, computed once, shared and read-only."""
    m = S.ragged(H, W, seed)
    sk, status = S.skeleton(m, 23, 256)
    assert status[2] == 0
    d2 = D.squared_distance(m, True)
    for a in (m, sk, d2):
        a.setflags(write=False)
    return m, sk, d2


# ------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_against_the_literal_reading(seed):
    m = S.ragged(24 + seed, 28 - seed, seed, n=4)
    m[0, :] = 1  # live pixels on the image border
    m[:, -1] = 2
    d2 = D.squared_distance(m, True)
    for thin in (1, 64):  # an unsettled input (thick parts: big node clusters) and a skeleton
        sk, _ = S.skeleton(m, 4, thin)
        labels, sums = G.graph(sk, 4)
        lit, rec, clusters = G.graph_literal(sk, 4)
        assert np.array_equal(labels, lit)
        for k in range(4):
            mine = [r for r in rec.values() if r["id"] == k]
            ends = [r for r in mine if r["T"] >= 1 and r["clusters"]]
            closed = [r for r in mine if r["T"] == 0 and len({c for c, _ in r["clusters"]}) <= 1]
            assert sums[k].tolist() == [len(mine), len(ends), sum(1 for i, _ in clusters if i == k), int((lit[sk == k] <= -2).sum()),
                                        sum(r["T"] for r in mine), max([r["P"] for r in ends], default=0),
                                        max([r["P"] for r in mine], default=0), len(closed)], (seed, thin, k)
        for min_pixels, ratio_q, rounds, rethin in ((2, 16, 1, 1), (2, 32, 3, 2), (0, 24, 2, 4), (5, 0, 2, 1)):
            want = G.prune_literal(sk, d2, 4, min_pixels, ratio_q, rounds, rethin)
            assert np.array_equal(G.prune(sk, d2, 4, min_pixels, ratio_q, rounds, rethin)[0], want), (seed, thin, ratio_q)
    assert np.array_equal(G.graph(sk, ids=[2, 0])[1], sums[[2, 0]])


def test_listed_ids_make_every_other_value_dead():
    sk = _ragged(64, 64, 3)[1]
    labels, sums = G.graph(sk, 23)
    l2, s2 = G.graph(sk, ids=[7, 2, 30])
    assert np.array_equal(s2, np.stack([sums[7], sums[2], np.zeros(8, np.int64)]))
    keep = (sk == 7) | (sk == 2)
    assert np.array_equal(l2[keep], labels[keep]) and (l2[~keep] == -1).all()


# ------------------------------------------------------------------------------------------------------ hand cases
def _pruned(name):
    sk, d2, N = G.HAND[name]()
    out, status = G.prune(sk, d2, N)
    assert ((out == sk) | (out == -1)).all()
    return sk, out, status, G.graph(sk, N)[1], G.graph(out, N)[1]


def test_t_with_a_two_pixel_stem():
    sk, out, status, before, after = _pruned("t")
    assert status.tolist() == [12, 1, 0, 2] and before.tolist() == [[3, 3, 1, 4, 3, 5, 5, 0]]
    assert np.argwhere(out >= 0).tolist() == [[4, x] for x in range(2, 14)]  # the bar, one thin line
    assert after.tolist() == [[1, 0, 0, 0, 2, 0, 12, 0]] and G.tips(sk, 1) == 3 and G.tips(out, 1) == 2


def test_plus_keeps_its_four_arms():
    sk, out, status, before, after = _pruned("plus")
    assert np.array_equal(out, sk) and status.tolist() == [29, 0, 0, 0]
    assert before.tolist() == after.tolist() == [[4, 4, 1, 5, 4, 6, 6, 0]]
    labels = G.graph(sk, 1)[0]
    assert labels[8, 8] == -2 - (7 * 17 + 8) and (labels[7:10, 7:10] <= -2).sum() == 5  # the cluster's first pixel is (7, 8)
    assert sorted(set(labels[labels >= 0].tolist())) == [1 * 17 + 8, 8 * 17 + 1, 8 * 17 + 10, 10 * 17 + 8]


def test_isolated_line_and_single_pixel_are_untouched():
    sk, out, status, before, after = _pruned("line_and_pixel")
    assert np.array_equal(out, sk) and status.tolist() == [8, 0, 0, 0]
    assert before.tolist() == [[1, 0, 0, 0, 2, 0, 7, 0], [1, 0, 0, 0, 1, 0, 1, 0]]
    far, _ = G.prune(sk, np.full_like(sk, 2 ** 31 - 1), 2, 1 << 20, 1024, 3, 1)  # no contact: no setting makes a spur of them
    assert np.array_equal(far, sk)


def test_ring_loses_its_spur_and_keeps_its_hole():
    sk, out, status, before, after = _pruned("ring")
    assert status.tolist() == [68, 1, 0, 2] and before.tolist() == [[2, 1, 1, 4, 1, 1, 65, 1]]
    assert after.tolist() == [[1, 0, 0, 0, 0, 0, 68, 1]]  # one closed branch, no node, no free end
    assert S.holes(sk >= 0) == S.holes(out >= 0) == 1 and G.tips(out, 1) == 0
    again, st = G.prune(out, np.full_like(sk, 2 ** 31 - 1), 1, 1 << 20, 1024, 2, 1)  # a ring is never touched
    assert np.array_equal(again, out) and st.tolist() == [68, 0, 0, 0]


def test_two_ids_sharing_a_border_prune_as_they_would_alone():
    sk, out, status, before, after = _pruned("two_ids")
    assert status.tolist() == [24, 1, 0, 4] and after.tolist() == [[1, 0, 0, 0, 2, 0, 12, 0]] * 2
    d2 = np.ones_like(sk)
    for k in (0, 1):
        alone, _ = G.prune(np.where(sk == k, k, -1).astype(np.int32), d2, 2)
        assert np.array_equal(out == k, alone == k)
        assert np.array_equal(G.graph(sk, 2)[1][k], G.graph(np.where(sk == k, k, -1), 2)[1][k])


# --------------------------------------------------------------------------------------------------------- the plants
@pytest.mark.parametrize("spec,raw", zip(G.PLANTS, ([7, 8, 6], [3, 7, 3], [10, 11, 11], [3, 3, 2])))
def test_plants_report_their_leaves(spec, raw):
    for seed, raw_tips in zip((1, 2, 3), raw):
        m = G.plant_map(*spec, seed)
        sk, st = S.skeleton(m, 1, 256)
        out, status = G.prune(sk, D.squared_distance(m, True), 1)
        assert st[2] == 0 and G.tips(sk, 1) == raw_tips, (spec, seed)
        assert G.tips(out, 1) == spec[0] and status[1] <= 2 and status[2] == 0, (spec, seed, status.tolist())
        assert S.pieces(out == 0, True) == 1 and ((out == sk) | (out == -1)).all()


# ------------------------------------------------------------------------------------------------------ ragged maps
@pytest.mark.parametrize("shape", sorted(RAGGED))
def test_ragged_maps_keep_pieces_and_holes_and_settle(shape):
    ratios, (tips_in, tips_out, px_in, px_out) = RAGGED[shape]
    m, sk, d2 = _ragged(*shape)
    assert (G.tips(sk, 23), int((sk >= 0).sum())) == (tips_in, px_in)
    for ratio in ratios:
        q = round(16 * ratio)
        out, status = G.prune(sk, d2, 23, 2, q, 8, 4)
        assert ((out == sk) | (out == -1)).all()  # out is a part of in, with its ids
        for k in range(23):
            assert S.pieces(out == k, True) == S.pieces(sk == k, True), (ratio, k)
            assert S.holes(out == k) == S.holes(sk == k), (ratio, k)
        assert status[2] == 0 and 1 <= status[1] <= 3 and status[0] == (out >= 0).sum() and status[3] == px_in - status[0]
        again, st = G.prune(out, d2, 23, 2, q, 3, 4)  # pruning a pruned, settled map is the identity
        assert np.array_equal(again, out) and st.tolist() == [int(status[0]), 0, 0, 0]
        if ratio == 1.0:
            assert (G.tips(out, 23), int(status[0])) == (tips_out, px_out)
        # status one round short of settling and at it
        busy = G.settles_in(sk, d2, 23, 2, q, 4)
        assert busy == status[1]
        short, s = G.prune(sk, d2, 23, 2, q, busy, 4)
        assert s[2] != 0 and s[1] == busy and np.array_equal(short, out)  # the last busy round gave the result
        at, s = G.prune(sk, d2, 23, 2, q, busy + 1, 4)
        assert np.array_equal(at, out) and s.tolist() == status.tolist()


def test_no_pruning_is_the_identity():
    m, sk, d2 = _ragged(64, 64, 3)
    out, status = G.prune(sk, d2, 23, 0, 0, 4, 4)
    assert np.array_equal(out, sk) and status.tolist() == [555, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------- the host layer
def test_options_validation():
    from weed_instance_segmentation_amd import PruneOptions, SkeletonOptions
    o = PruneOptions()
    assert (o.min_pixels, o.ratio, o.max_rounds, o.rethin, o.ratio_q) == (2, 1.0, 8, 4, 16)
    with pytest.raises(Exception):
        o.ratio = 2.0  # frozen
    for bad in ({"min_pixels": -1}, {"min_pixels": (1 << 20) + 1}, {"min_pixels": 2.0}, {"min_pixels": True}, {"ratio": -0.5},
                {"ratio": 64.5}, {"ratio": float("nan")}, {"ratio": "1"}, {"ratio": True}, {"max_rounds": 0}, {"max_rounds": 65},
                {"max_rounds": 1.0}, {"rethin": 0}, {"rethin": 17}, {"rethin": False}):
        with pytest.raises(ValueError):
            PruneOptions(**bad)
    assert PruneOptions(ratio=1.5).ratio_q == 24 and PruneOptions(ratio=64).ratio_q == 1024 and PruneOptions(ratio=0).ratio_q == 0
    assert PruneOptions(min_pixels=np.int64(0), ratio=np.float32(2.0), max_rounds=np.int32(64), rethin=16).ratio_q == 32
    s = SkeletonOptions()
    assert s.prune is None and [f.name for f in s.__dataclass_fields__.values()][-1] == "prune"
    assert SkeletonOptions(prune=o).prune is o
    for bad in ({"ratio": 1.0}, 1.0, True):
        with pytest.raises(ValueError):
            SkeletonOptions(prune=bad)


def test_header_declares_and_lib_binds_the_entry_points():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    want = {
        "int64_t wm2f_labelmap_skeleton_prune_workspace": ["int B", "int H", "int W"],
        "int wm2f_labelmap_skeleton_prune": ["const int32_t* skel", "const int32_t* d2", "int32_t* out", "int32_t* status",
                                             "void* workspace", "int B", "int H", "int W", "int N", "int min_pixels",
                                             "int ratio_q", "int rounds", "int rethin", "void* stream"],
        "int64_t wm2f_labelmap_skeleton_graph_workspace": ["int B", "int H", "int W"],
        "int wm2f_labelmap_skeleton_graph": ["const int32_t* skel", "const int32_t* ids", "const int32_t* n_ids",
                                             "int32_t* labels", "int64_t* sums", "void* workspace", "int B", "int H", "int W",
                                             "int N", "void* stream"],
    }
    for decl, args in want.items():
        proto = re.search(re.escape(decl) + r"\(([^;]*)\);", header)
        assert proto is not None, decl
        assert [a.strip() for a in " ".join(proto.group(1).split()).split(",")] == args
        res, argtypes = _lib.SIGNATURES[decl.split()[1]]
        assert len(argtypes) == len(args)
    assert "skeleton_graph.hip" in _build.SOURCES
    for rule in ("node pixel: b >= 3", "256 P'^2 <= ratio_q^2 D", "key = 2 k + [node]", "cmin = cmax"):
        assert rule in header, rule  # the contract is there in full
    with open(os.path.join(ROOT, "profiles", "skeleton_graph_resources.txt")) as f:
        record = f.read()
    rows = [[c.strip() for c in line.split("|")] for line in record.splitlines()[4:] if "|" in line]
    assert len(rows) == 7 and {r[4] for r in rows} == {"0"}  # local, merge, flatten, record, labels, delete, status: no scratch
    with open(os.path.join(ROOT, "weed_instance_segmentation_amd", "csrc", "skeleton_graph.hip")) as f:
        source = f.read()
    assert {r[0] for r in rows} == set(re.findall(r"void (\w+_kernel)\(", source))


def test_public_interface_and_errors_without_a_device():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import ops, skeleton
    from weed_instance_segmentation_amd._lib import Wm2fError
    for name in ("PruneOptions", "prune_skeleton_maps", "skeleton_branch_maps", "skeleton_graph_statistics", "SKELETON_GRAPH_TRAITS"):
        assert getattr(pkg, name) is getattr(skeleton, name), name
    assert pkg.SKELETON_GRAPH_TRAITS == ("branches", "end_branches", "nodes", "longest_end_branch", "longest_branch",
                                         "closed_branches", "pruned_pixels", "prune_settled")
    sig = inspect.signature(ops.labelmap_skeleton_prune).parameters
    assert list(sig) == ["skel", "d2", "N", "min_pixels", "ratio_q", "rounds", "rethin"]
    assert [sig[k].default for k in ("min_pixels", "ratio_q", "rounds", "rethin")] == [2, 16, 8, 4]
    sig = inspect.signature(ops.labelmap_skeleton_graph).parameters
    assert list(sig) == ["skel", "ids", "n_ids", "N"] and all(p.default is None for p in list(sig.values())[1:])
    sig = inspect.signature(pkg.prune_skeleton_maps).parameters
    assert list(sig) == ["skeletons", "maps", "n", "options", "border", "return_status"]
    assert sig["border"].kind is inspect.Parameter.KEYWORD_ONLY and sig["border"].default == "outside"
    assert list(inspect.signature(pkg.skeleton_branch_maps).parameters) == ["skeletons", "n"]
    assert list(inspect.signature(pkg.skeleton_graph_statistics).parameters) == ["segmentation", "n", "ids", "options"]
    assert "spurs are not pruned" not in skeleton.__doc__
    m = np.zeros((4, 4), np.int32)
    with pytest.raises(ValueError):
        pkg.skeleton_graph_statistics(m)
    with pytest.raises(ValueError):
        pkg.skeleton_graph_statistics(m, n=1, ids=[0])
    with pytest.raises(ValueError):
        pkg.skeleton_graph_statistics(m, ids=[1, 1])
    with pytest.raises(TypeError):
        pkg.skeleton_graph_statistics(m, n=1, options=pkg.PruneOptions())
    with pytest.raises(TypeError):
        pkg.prune_skeleton_maps(m, m, 1, pkg.SkeletonOptions())
    with pytest.raises(TypeError):
        pkg.prune_skeleton_maps(m.astype(np.float32), m, 1)
    with pytest.raises(ValueError):
        pkg.prune_skeleton_maps(m, m[:2], 1)
    with pytest.raises(ValueError):
        pkg.prune_skeleton_maps(m, m, 4097)
    with pytest.raises(ValueError):
        pkg.prune_skeleton_maps(m, m, 1, border="edge")
    with pytest.raises(TypeError):
        pkg.skeleton_branch_maps(m.astype(np.uint8), 1)
    with pytest.raises(ValueError):
        pkg.skeleton_branch_maps(m, -1)
    z = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(Wm2fError):  # no CPU fallback
        ops.labelmap_skeleton_prune(z, z, 1)
    with pytest.raises(Wm2fError):
        ops.labelmap_skeleton_graph(z, N=1)
    with pytest.raises(TypeError):
        ops.labelmap_skeleton_prune(z.numpy(), z, 1)
    with pytest.raises(TypeError):
        ops.labelmap_skeleton_graph(z.numpy(), N=1)
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            pkg.prune_skeleton_maps(m, m, 1)
        with pytest.raises(Wm2fError):
            pkg.skeleton_branch_maps(m, 1)
        with pytest.raises(Wm2fError):
            pkg.skeleton_graph_statistics(m, n=1)
        with pytest.raises(Wm2fError):
            pkg.skeleton_maps(m, 1, pkg.SkeletonOptions(prune=pkg.PruneOptions()))


def test_without_prune_the_entry_points_keep_their_keys(monkeypatch):
    """`prune=None` is today's path: the same ops calls in the same order, the same keys, SKELETON_TRAITS unchanged."""
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import ops, skeleton
    assert pkg.SKELETON_TRAITS == ("skeleton_pixels", "skeleton_length", "tips", "junction_pixels", "mean_width", "max_width",
                                   "length_per_area", "settled")
    calls = []

    def fake(name, result):
        def op(*a, **kw):
            calls.append(name)
            return result(*a, **kw)
        monkeypatch.setattr(ops, name, op)

    B, N = 1, 3
    fake("labelmap_skeleton", lambda maps, n, rounds=64: (torch.full(maps.shape, -1, dtype=torch.int32), torch.tensor([[0, 0, 0, rounds]] * B, dtype=torch.int32)))
    fake("labelmap_distance", lambda maps, outside: torch.zeros(maps.shape, dtype=torch.int32))
    fake("labelmap_skeleton_stats", lambda skel, ids, n_ids, N=None, d2=None: torch.zeros(B, N, 8, dtype=torch.int64))
    fake("labelmap_instance_stats", lambda maps, ids, n_ids, N=None: torch.zeros(B, N, 8, dtype=torch.int64))
    fake("labelmap_skeleton_prune", lambda skel, d2, n, **kw: (skel, torch.tensor([[0, 0, 0, 0]] * B, dtype=torch.int32)))
    fake("labelmap_skeleton_graph", lambda skel, ids, n_ids, N=None: (skel, torch.zeros(B, N, 8, dtype=torch.int64)))
    monkeypatch.setattr(skeleton, "_device_stack", lambda seg, who: seg.unsqueeze(0) if seg.dim() == 2 else seg)
    m = np.zeros((4, 4), np.int32)
    plain = ["skeleton_pixels", "tips", "junction_pixels", "skeleton_length", "mean_width", "max_width", "length_per_area", "settled"]
    got = pkg.skeleton_statistics(m, n=N)
    assert list(got) == plain and calls == ["labelmap_skeleton", "labelmap_distance", "labelmap_skeleton_stats", "labelmap_instance_stats"]
    del calls[:]
    assert pkg.skeleton_maps(m, N).shape == (4, 4) and calls == ["labelmap_skeleton"]
    del calls[:]
    result = {"segmentation": m, "segments_info": [{"id": 0, "score": 0.5}, {"id": 2, "score": 0.25}]}
    noted = pkg.annotate_skeletons(result)
    assert [list(s) for s in noted["segments_info"]] == [["id", "score"] + list(pkg.SKELETON_TRAITS)] * 2
    assert "labelmap_skeleton_prune" not in calls and "labelmap_skeleton_graph" not in calls
    del calls[:]
    opts = pkg.SkeletonOptions(prune=pkg.PruneOptions(), widths=False)
    assert list(pkg.skeleton_statistics(m, n=N, options=opts)) == [k for k in plain if "width" not in k]
    assert calls == ["labelmap_skeleton", "labelmap_distance", "labelmap_skeleton_prune", "labelmap_skeleton_stats", "labelmap_instance_stats"]
    noted = pkg.annotate_skeletons(result, opts)
    want = [k for k in pkg.SKELETON_TRAITS if "width" not in k] + list(pkg.SKELETON_GRAPH_TRAITS)
    assert [list(s) for s in noted["segments_info"]] == [["id", "score"] + want] * 2
    assert list(pkg.skeleton_graph_statistics(m, n=N)) == plain + list(pkg.SKELETON_GRAPH_TRAITS)


def test_c_abi_reports_sizes_before_pointers():
    """The library loads and answers without a device: limits and argument errors never touch the GPU."""
    import ctypes
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)

    def prune(B=1, H=4, W=4, N=2, min_pixels=2, ratio_q=16, rounds=8, rethin=4):
        return lib.wm2f_labelmap_skeleton_prune(null, null, null, null, null, B, H, W, N, min_pixels, ratio_q, rounds, rethin, null)

    def graph(B=1, H=4, W=4, N=2):
        return lib.wm2f_labelmap_skeleton_graph(null, null, null, null, null, null, B, H, W, N, null)

    for kw in ({"H": 16385}, {"W": 16385}, {"B": 33}, {"N": 4097}):
        assert prune(**kw) == _lib.WM2F_EUNSUPPORTED and graph(**kw) == _lib.WM2F_EUNSUPPORTED, kw
    for kw in ({"B": 0}, {"H": 0}, {"W": -1}, {"N": -1}):
        assert prune(**kw) == _lib.WM2F_EINVAL and graph(**kw) == _lib.WM2F_EINVAL, kw
    for kw in ({"min_pixels": -1}, {"min_pixels": (1 << 20) + 1}, {"ratio_q": -1}, {"ratio_q": 1025}, {"rounds": 0}, {"rounds": 65},
               {"rethin": 0}, {"rethin": 17}):
        assert prune(**kw) == _lib.WM2F_EINVAL and b"null pointer" not in lib.wm2f_last_error(), kw
    assert prune(min_pixels=1 << 20, ratio_q=1024, rounds=64, rethin=16) == _lib.WM2F_EINVAL and b"null pointer" in lib.wm2f_last_error()
    assert graph() == _lib.WM2F_EINVAL and b"null pointer" in lib.wm2f_last_error()
    for B, H, W in [(1, 16385, 4), (33, 4, 4), (0, 4, 4)]:
        assert lib.wm2f_labelmap_skeleton_prune_workspace(B, H, W) == -1 == lib.wm2f_labelmap_skeleton_graph_workspace(B, H, W)
    assert lib.wm2f_labelmap_skeleton_graph_workspace(1, 64, 64) == 7 * 64 * 64 * 4
    assert lib.wm2f_labelmap_skeleton_prune_workspace(1, 64, 64) == 8 * 64 * 64 * 4 + 65 * 16 + lib.wm2f_labelmap_skeleton_workspace(1, 64, 64)
