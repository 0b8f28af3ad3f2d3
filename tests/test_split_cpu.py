"""The watershed split of touching instances without a device: the numpy restatement on the hand
cases with their piece counts, against a literal pixel-by-pixel reading of the rule, the properties of the numbering,
`SplitOptions`, the C ABI, and the public interface's argument checks."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import distance_reference as D
import split_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def split_literal(id_map, d2, N, M, num, den, min_peak_d2, rounds):
    """The rule of include/wm2f.h read pixel by pixel, with nothing precomputed: (out, info, status)."""
    ids = S.instance_ids(id_map, N)
    H, W = ids.shape

    def key(p):
        return (int(d2[p // W, p % W]) << 32) | (S.LOW - p)

    def neighbours(p):
        y, x = divmod(p, W)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dy or dx) and 0 <= y + dy < H and 0 <= x + dx < W and ids[y + dy, x + dx] == ids[y, x]:
                    yield (y + dy) * W + x + dx

    pixels = [p for p in range(H * W) if ids[p // W, p % W] >= 0]
    up = {p: max([p] + list(neighbours(p)), key=key) for p in pixels}

    def peak_of(p):
        while up[p] != p:
            p = up[p]
        return p
    basin = {p: peak_of(p) for p in pixels}
    n_basins = len(set(basin.values()))
    group = dict(basin)  # pixel -> its group's peak
    links = 0
    for _ in range(rounds):
        best = {}
        for p in pixels:
            for q in neighbours(p):
                if group[p] != group[q]:
                    s = min(int(d2[p // W, p % W]), int(d2[q // W, q % W]))
                    best[group[p]] = max(best.get(group[p], 0), (s << 32) | (S.LOW - group[q]))
        parent = {}
        for g, b in best.items():
            s, o = b >> 32, S.LOW - (b & S.LOW)
            mine = int(d2[g // W, g % W])
            if key(o) > key(g) and (mine < min_peak_d2 or s * den * den >= num * num * mine):
                parent[g] = o
        links = len(parent)

        def root(g):
            while g in parent:
                g = parent[g]
            return g
        group = {p: root(g) for p, g in group.items()}
    roots = sorted(set(group.values()))
    keeper = {}
    for g in roots:
        k = int(ids[g // W, g % W])
        if k not in keeper or key(g) > key(keeper[k]):
            keeper[k] = g
    extras = [g for g in roots if keeper[int(ids[g // W, g % W])] != g]
    new_id = {g: int(ids[g // W, g % W]) for g in keeper.values()}
    new_id.update({g: N + j for j, g in enumerate(extras)})
    out = np.full((H, W), -1, np.int32)
    info = np.tile(np.array([-1, -1, -1, 0], np.int32), (M, 1))
    for p in pixels:
        j = new_id[group[p]]
        out[p // W, p % W] = j if j < M else ids[p // W, p % W]
    for g, j in new_id.items():
        if j < M:
            info[j] = (ids[g // W, g % W], g % W, g // W, d2[g // W, g % W])
    return out, info, np.array([N + len(extras), n_basins, links, rounds], np.int32)


def _small_maps():
    rng = np.random.default_rng(37)
    maps = []
    for i in range(24):
        H, W = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        spec = [(int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(1, 7)), int(rng.integers(0, 4)))
                for _ in range(int(rng.integers(1, 9)))]
        maps.append(S.discs((H, W), spec))
    maps += [np.full((6, 5), -1, np.int32), np.full((7, 9), 2, np.int32), S.bar(), S.three_discs()[::2, ::2].copy()]
    return maps


def test_restatement_equals_the_literal_reading():
    n_extra = n_rounds = 0
    for i, m in enumerate(_small_maps()):
        for outside in (True, False):
            d2 = D.squared_distance(m, outside)
            for N, M, num, den, mp, rounds in [(4, 12, 1, 2, 0, 8), (3, 5, 3, 4, 4, 8), (4, 40, 1, 1, 0, 1), (4, 4, 2, 3, 0, 2),
                                               (4, 40, 0, 1, 0, 3)]:
                want = split_literal(m, d2, N, M, num, den, mp, rounds)
                got = S.split(m, d2, N, M, num, den, mp, rounds)
                for a, b in zip(got, want):
                    assert a.dtype == np.int32 and np.array_equal(a, b), (i, outside, N, M, num, den, mp, rounds)
                n_extra += int(got[2][0]) - N
                n_rounds += int(got[2][2] > 0)
    assert n_extra > 100 and n_rounds > 0  # the comparison is not one of maps that never split or always settle


@pytest.mark.parametrize("name,ratio,pieces", [
    ("two_discs", (1, 2), 1), ("two_discs", (3, 4), 2), ("dumbbell_with_bump", (1, 2), 2), ("dumbbell_with_bump", (3, 4), 3),
    ("bar", (1, 2), 1), ("bar", (3, 4), 1), ("disc", (1, 2), 1), ("disc", (3, 4), 1), ("disc_with_bud", (3, 4), 1),
    ("disc_with_bud", (9, 10), 2)])
def test_hand_cases(name, ratio, pieces):
    m = getattr(S, name)()
    out, info, status = S.split_map(m, 1, 8, *ratio)
    assert S.pieces(out) == pieces == status[0] and status[2] == 0
    assert np.array_equal(out >= 0, m >= 0)
    if name == "bar":
        assert status[1] == 1 and info[0].tolist() == [0, 5, 4, 9]  # one basin from the start: the medial line ties
    if name == "dumbbell_with_bump":
        # the ends never merge through the bump: they are two pieces at either ratio, and at 1/2 the bump is the left one's
        assert out[36, 30] != out[36, 100] and (out[24, 65] == out[36, 30]) == (pieces == 2)


def test_rounds_are_synchronous():
    m = S.three_discs()
    one = S.split_map(m, 1, 8, 1, 2, rounds=1)
    two = S.split_map(m, 1, 8, 1, 2, rounds=2)
    assert one[2].tolist() == [2, 3, 1, 1] and S.pieces(one[0]) == 2  # both small discs decide on the round's start
    assert two[2].tolist() == [1, 3, 1, 2] and S.pieces(two[0]) == 1
    assert S.split_map(m, 1, 8, 1, 2, rounds=3)[2].tolist() == [1, 3, 0, 3]


def _touching():
    """Ids 0 and 1 side by side along a long straight border, each of them two overlapping discs."""
    m = S.discs((60, 100), [(25, 30, 18, 0), (50, 30, 18, 0), (60, 30, 18, 1), (85, 30, 18, 1)])
    m[:, 55:][m[:, 55:] == 0] = 1
    return m


def test_numbering_properties():
    m = _touching()
    ragged, n = S.ragged(128, 1)
    for ids, N in ((m, 2), (ragged, n)):
        d2 = D.squared_distance(ids, True)
        for num, den in ((1, 2), (3, 4), (1, 1)):
            out, info, status = S.split(ids, d2, N, 200, num, den)
            assert status[2] == 0 and status[0] <= 200
            # two different ids that touch never exchange pixels
            assert np.array_equal(np.where(out >= 0, info[np.maximum(out, 0), 0], -1), np.where(ids >= 0, ids, -1))
            keys = S.pixel_keys(d2)
            for k in range(N):
                # the keeping group holds the id's largest key
                top = np.argmax(np.where(ids == k, keys, 0))
                assert out.reshape(-1)[top] == k and info[k].tolist() == [k, top % ids.shape[1], top // ids.shape[1], d2.reshape(-1)[top]]
            # extras are in raster order of their peaks, and every peak is a pixel of its own id
            lin = info[N:status[0], 2].astype(np.int64) * ids.shape[1] + info[N:status[0], 1]
            assert (np.diff(lin) > 0).all() and (info[status[0]:] == [-1, -1, -1, 0]).all()
            assert (out[info[N:status[0], 2], info[N:status[0], 1]] == np.arange(N, status[0])).all()
        assert status[0] > N
    assert (S.split_map(m, 2, 8, 3, 4)[0][:, 55:][m[:, 55:] >= 0] != 0).all()


def test_the_id_space_caps_what_is_split_off():
    m, n = S.ragged(128, 1)
    free = S.split_map(m, n, 200, 1, 1)
    wanted = int(free[2][0])
    assert wanted > n + 3
    for M in (n, n + 1, n + 3):
        out, info, status = S.split_map(m, n, M, 1, 1)
        assert status.tolist() == free[2].tolist() and info.shape == (M, 4)  # the uncapped count is reported
        assert np.array_equal(info, free[1][:M])
        over = free[0] >= M
        assert over.any() and np.array_equal(out[~over], free[0][~over]) and np.array_equal(out[over], m[over])


# --------------------------------------------------------------------------------------------------- SplitOptions
def test_split_options():
    from weed_instance_segmentation_amd import SplitOptions
    d = SplitOptions()
    assert (d.min_neck_ratio, d.min_clearance, d.rounds, d.border, d.max_instances) == (0.5, 0.0, 8, "outside", None)
    assert d.kernel_arguments() == {"num": 1, "den": 2, "min_peak_d2": 0, "rounds": 8}
    for ratio, frac in ((0, (0, 1)), (1, (1, 1)), (0.75, (3, 4)), (0.9, (9, 10)), (1 / 3, (1, 3)), (0.3337, (303, 908)),
                        (np.float32(0.5), (1, 2))):
        a = SplitOptions(min_neck_ratio=ratio).kernel_arguments()
        assert (a["num"], a["den"]) == frac == tuple(Fraction(float(ratio)).limit_denominator(1024).as_integer_ratio())
        assert 0 <= a["num"] <= a["den"] <= 1024
    for c, want in ((0, 0), (3, 9), (2.5, 7), (1.5, 3), (0.1, 1), (3.0000001, 10)):
        assert SplitOptions(min_clearance=c).kernel_arguments()["min_peak_d2"] == want
    assert SplitOptions(rounds=32, border="inside", max_instances=7).id_space(7) == 7
    assert d.id_space(0) == 64 and d.id_space(10) == 74 and d.id_space(100) == 200 and d.id_space(4000) == 4096
    for bad in ({"min_neck_ratio": -0.1}, {"min_neck_ratio": 1.01}, {"min_neck_ratio": float("nan")}, {"min_neck_ratio": "0.5"},
                {"min_neck_ratio": True}, {"min_clearance": -1}, {"min_clearance": float("inf")}, {"min_clearance": 40000},
                {"rounds": 0}, {"rounds": 33}, {"rounds": 2.0}, {"border": "beyond"}, {"max_instances": 4097},
                {"max_instances": -1}, {"max_instances": 2.5}):
        with pytest.raises(ValueError):
            SplitOptions(**bad)
    with pytest.raises(ValueError):
        SplitOptions(max_instances=3).id_space(4)
    with pytest.raises(ValueError):
        d.id_space(5000)
    with pytest.raises(Exception):
        d.rounds = 3  # frozen


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_lib_binds_the_entry_points():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    want = {
        "int64_t wm2f_labelmap_split_workspace": ["int B", "int H", "int W", "int M"],
        "int wm2f_labelmap_split": ["const void* map", "int dtype", "const int32_t* d2", "int32_t* out", "int32_t* info",
                                    "int32_t* status", "void* workspace", "int B", "int H", "int W", "int N", "int M", "int num",
                                    "int den", "int min_peak_d2", "int rounds", "void* stream"],
    }
    for decl, args in want.items():
        proto = re.search(re.escape(decl) + r"\(([^;]*)\);", header)
        assert proto is not None, decl
        assert [a.strip() for a in " ".join(proto.group(1).split()).split(",")] == args
        res, argtypes = _lib.SIGNATURES[decl.split()[1]]
        assert len(argtypes) == len(args)
        assert [t is _lib.c_void_p for t in argtypes] == ["*" in a for a in args]
    assert "split.hip" in _build.SOURCES


# ------------------------------------------------------------------------------------------ the public interface
def test_public_interface_checks_arguments_before_it_needs_a_device():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import SplitOptions, ops, split_label_maps
    from weed_instance_segmentation_amd._lib import Wm2fError
    from weed_instance_segmentation_amd.annotations import semantic_to_instance_map
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    assert pkg.split_label_maps is split_label_maps and pkg.SplitOptions is SplitOptions
    m = torch.zeros(4, 4)
    with pytest.raises(TypeError):
        split_label_maps(m, 2, {"min_neck_ratio": 0.5})
    with pytest.raises(ValueError):
        split_label_maps(m, 2, min_neck_ratio=2)
    with pytest.raises(ValueError):
        split_label_maps(m, 2, SplitOptions(), rounds=0)
    with pytest.raises(TypeError):
        split_label_maps(m, 2, bogus=1)
    with pytest.raises(ValueError):
        split_label_maps(m, -1)
    with pytest.raises(ValueError):
        split_label_maps(m, 3, max_instances=2)
    with pytest.raises(ValueError):
        split_label_maps(m, 5000)
    with pytest.raises(TypeError):
        split_label_maps(torch.zeros(4, 4, dtype=torch.int64), 2)
    with pytest.raises(TypeError):
        split_label_maps(np.zeros((4, 4), np.float64), 2)
    with pytest.raises(ValueError):
        split_label_maps(torch.zeros(4), 2)
    with pytest.raises(ValueError):
        split_label_maps(torch.zeros(1, 1, 4, 4), 2)
    z = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(Wm2fError):  # the kernels take device tensors only
        ops.labelmap_split(z, z, 2, 4, 1, 2)
    with pytest.raises(TypeError):
        ops.labelmap_split(z.numpy(), z, 2, 4, 1, 2)
    with pytest.raises(TypeError):
        Mask2FormerInstancePostProcessor().post_process_instance_segmentation(None, split="yes")
    with pytest.raises(Wm2fError):
        semantic_to_instance_map(torch.zeros(4, 4, dtype=torch.uint8), split=SplitOptions())
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            split_label_maps(m, 2)
        with pytest.raises(Wm2fError):
            split_label_maps(m.numpy(), 2, min_neck_ratio=0.75, return_info=True)
