"""Crop rows on the GPU: the accumulator and the energies of wm2f_labelmap_row_votes and the counts
and the zone of wm2f_labelmap_row_bands against the numpy restatement, exactly; `crop_rows` against the restatement's
dict; `annotate_rows`; `treatment_grid` with a zone; the refusals; run-to-run identity."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest
import torch

from rows_reference import bands_reference, crop_rows_reference, n_bins, row_field, votes_reference
from shape_reference import ellipse_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
NP_DT = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}
# (H, W), ids: R tiny and scalar loads; one tile; W % 4 != 0 and a row across a 256-lane segment; the 16-byte load;
# more than one 64 x 64 tile each way
SCENES = [((7, 9), 3), ((33, 65), 6), ((40, 257), 12), ((64, 260), 12), ((130, 70), 9)]
ANGLES = (1, 8, 180, 256)   # 8 and 180 are no multiple of the band of 16 angles
SHIFTS = (14, 16)


@functools.lru_cache(maxsize=None)
def _scene(shape, N, B):
    """B maps of one scene (int64, background -1) and a vote row per image, each with a voter."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + B)
    maps = np.stack([ellipse_scene(rng, shape, N, np.int64) for _ in range(B)])
    vote = (rng.random((B, N)) < 0.5).astype(np.uint8)
    for b in range(B):
        vote[b, int(np.bincount(maps[b][maps[b] >= 0], minlength=N).argmax())] = 1
    return maps, vote


@functools.lru_cache(maxsize=None)
def _votes(shape, N, B, T, shift):
    maps, vote = _scene(shape, N, B)
    acc, energy = zip(*[votes_reference(maps[b], vote[b], T, shift) for b in range(B)])
    return np.stack(acc), np.array(energy, np.int64)


def _typed(maps, dtype, N):
    """The scene in a map dtype: background -1, or 200 in uint8; fp32 gets fractions and values >= N, which are no ids."""
    m = maps.copy()
    if dtype == torch.uint8:
        m[m < 0] = 200
    m = m.astype(NP_DT[dtype])
    if dtype == torch.float32:
        bg = maps[0] < 0
        m[0][bg] = np.where(np.arange(bg.sum()) % 2 == 0, 1.5, float(N + 1)).astype(np.float32)
    return m


def _cs(T):
    from weed_instance_segmentation_amd import ops
    return torch.from_numpy(ops.row_angle_table(T)).to(DEV)


# ------------------------------------------------------------------------------------------ votes
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape,N", SCENES)
def test_votes_equal_the_restatement(shape, N, B, dtype):
    from weed_instance_segmentation_amd import ops
    maps, vote = _scene(shape, N, B)
    t = torch.from_numpy(_typed(maps, dtype, N)).to(DEV)
    v = torch.from_numpy(vote).to(DEV)
    for T in ANGLES:
        for shift in SHIFTS:
            want_acc, want_e = _votes(shape, N, B, T, shift)
            acc, energy = ops.labelmap_row_votes(t, v, _cs(T), shift)
            assert acc.shape == (B, T, n_bins(*shape, shift)) and acc.dtype == torch.int32 and acc.is_cuda
            assert energy.shape == (B, T) and energy.dtype == torch.int64
            assert want_acc.sum() > 0
            assert np.array_equal(acc.cpu().numpy(), want_acc), (T, shift)
            assert np.array_equal(energy.cpu().numpy(), want_e), (T, shift)


def _hand_maps(H, W):
    none = np.zeros((H, W), np.int64)                 # id 0 everywhere, and nothing votes (see the vote rows)
    every = np.zeros((H, W), np.int64)                # the footprint
    one = np.full((H, W), -1, np.int64)
    one[H - 1, W - 1] = 0                             # a single pixel in the last corner
    row = np.full((H, W), -1, np.int64)
    row[H // 2, :] = 0
    col = np.full((H, W), -1, np.int64)
    col[:, W - 2] = 0
    return np.stack([none, every, one, row, col]), np.array([[0], [1], [1], [1], [1]], np.uint8)


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_votes_on_hand_maps(dtype):
    from weed_instance_segmentation_amd import ops
    H, W, T = 130, 70, 180
    maps, vote = _hand_maps(H, W)
    m = maps.copy()
    if dtype == torch.uint8:
        m[m < 0] = 255
    t = torch.from_numpy(m.astype(NP_DT[dtype])).to(DEV)
    for shift in SHIFTS:
        acc, energy = ops.labelmap_row_votes(t, torch.from_numpy(vote).to(DEV), _cs(T), shift)
        acc, energy = acc.cpu().numpy(), energy.cpu().numpy()
        for b in range(len(maps)):
            want_acc, want_e = votes_reference(maps[b], vote[b], T, shift)
            assert np.array_equal(acc[b], want_acc) and [int(e) for e in energy[b]] == want_e, (b, shift)
        assert not acc[0].any() and not energy[0].any()
        assert (acc[1].sum(1) == H * W).all() and (acc[2].sum(1) == 1).all() and (energy[2] == 1).all()
        if shift == 14:
            assert energy[3][T // 2] == W * W and energy[4][0] == H * H   # a row / a column in one bin of its normal


def test_votes_run_to_run_identity():
    """Two calls give equal bytes."""
    from weed_instance_segmentation_amd import ops
    maps, vote = _scene((130, 70), 9, 3)
    t, v = torch.from_numpy(maps.astype(np.int32)).to(DEV), torch.from_numpy(vote).to(DEV)
    a1, e1 = ops.labelmap_row_votes(t, v, _cs(180), 14)
    a2, e2 = ops.labelmap_row_votes(t, v, _cs(180), 14)
    assert a1.cpu().numpy().tobytes() == a2.cpu().numpy().tobytes() and e1.cpu().numpy().tobytes() == e2.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------ bands
def _lines(rng, shape, B, K, Kmax, negative_c=False):
    """A line per image (another direction each) and K ascending row positions within the image's span."""
    from weed_instance_segmentation_amd import ops
    H, W = shape
    table = ops.row_angle_table(180)
    line = np.zeros((B, 4), np.int32)
    rho = np.zeros((B, max(Kmax, 1)), np.int32)
    for b in range(B):
        t = int(rng.integers(91, 180)) if negative_c else int(rng.integers(0, 180))
        c, s = int(table[t, 0]), int(table[t, 1])
        line[b] = [c, s, ops.row_offset(c, W), K]
        span = (W + H - 2) << 14
        rho[b, :K] = np.sort(rng.choice(span, K, replace=False))
        rho[b, K:] = -7   # never looked at
    return line, rho[:, :Kmax] if Kmax else rho[:, :0]


def _check_bands(maps_np, t, line, rho, band, N, ids=None, n_ids=None, lists=None):
    from weed_instance_segmentation_amd import ops
    kw = dict(N=N) if ids is None else dict(ids=ids, n_ids=n_ids)
    counts, zone = ops.labelmap_row_bands(t, torch.from_numpy(line).to(DEV), torch.from_numpy(rho).to(DEV), band, zone=True, **kw)
    assert counts.dtype == torch.int64 and zone.dtype == torch.uint8 and zone.shape == t.shape
    only = ops.labelmap_row_bands(t, torch.from_numpy(line).to(DEV), torch.from_numpy(rho).to(DEV), band, **kw)
    assert torch.equal(only, counts)   # the same counts without a zone
    for b in range(maps_np.shape[0]):
        want, wzone = bands_reference(maps_np[b], line[b], rho[b], band, ids=None if lists is None else lists[b], N=N)
        assert np.array_equal(counts[b].cpu().numpy(), want), b
        assert np.array_equal(zone[b].cpu().numpy(), wzone), b
    return counts, zone


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8])
@pytest.mark.parametrize("shape,N", SCENES)
def test_bands_equal_the_restatement(shape, N, dtype):
    maps, _ = _scene(shape, N, 3)
    typed = _typed(maps, dtype, N)
    t = torch.from_numpy(typed).to(DEV)
    rng = np.random.default_rng(shape[0] + 17)
    spacing = 12 << 14
    for K, Kmax, band, neg in ((0, 4, 3 << 14, False), (0, 0, 3 << 14, False), (1, 1, 0, True), (5, 8, 2 * spacing, False),
                               (5, 5, (1 << 14) + 5, True), (300, 300, 1 << 12, True)):
        line, rho = _lines(rng, shape, 3, K, Kmax, neg)
        counts, zone = _check_bands(typed, t, line, rho, band, N)
        if K == 0:
            assert not zone.any() and not counts[..., 1].any() and counts[..., 0].sum() > 0
        if neg:
            assert (line[:, 0] < 0).all()


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_bands_with_id_lists(dtype):
    shape, N, B = (40, 257), 12, 3
    maps, _ = _scene(shape, N, B)
    raw = np.where(maps >= 0, 3 * maps + 7, -1)  # raw ids 7, 10, ..., 40
    lists = [[7, 10, 13, 14, 19, 40], [10, 22, 25, 28, 31, 34, 37, 39], [16]]
    G = 9
    ids = torch.zeros(B, G, dtype=torch.int32)
    for b, l in enumerate(lists):
        ids[b, :len(l)] = torch.tensor(l, dtype=torch.int32)
    n_ids = torch.tensor([len(l) for l in lists], dtype=torch.int32)
    m = raw.copy()
    if dtype == torch.uint8:
        m[m < 0] = 200
    typed = m.astype(NP_DT[dtype])
    line, rho = _lines(np.random.default_rng(5), shape, B, 5, 6)
    counts, _ = _check_bands(typed, torch.from_numpy(typed).to(DEV), line, rho, 4 << 14, G, ids.to(DEV), n_ids.to(DEV), lists)
    assert int((counts[..., 0] > 0).sum()) >= 8


def test_bands_with_more_ids_than_the_lds_cap():
    from weed_instance_segmentation_amd import ops
    N = ops.rows.ROW_LDS_MAX_IDS + 76
    assert N == 1100
    rng = np.random.default_rng(8)
    base = ellipse_scene(rng, (48, 64), 12, np.int64)
    present = np.sort(rng.choice(N, 12, replace=False))
    present[-1] = N - 1
    m = np.where(base >= 0, present[np.clip(base, 0, 11)], -1).astype(np.float32)[None]
    line, rho = _lines(rng, (48, 64), 1, 5, 5, True)
    counts, _ = _check_bands(m, torch.from_numpy(m).to(DEV), line, rho, 3 << 14, N)
    assert int((counts[0, :, 0] > 0).sum()) >= 8 and counts[0, N - 1, 0] > 0


def test_bands_run_to_run_identity():
    from weed_instance_segmentation_amd import ops
    maps, _ = _scene((130, 70), 9, 3)
    t = torch.from_numpy(maps.astype(np.int32)).to(DEV)
    line, rho = _lines(np.random.default_rng(2), (130, 70), 3, 5, 5)
    args = (t, torch.from_numpy(line).to(DEV), torch.from_numpy(rho).to(DEV), 2 << 14)
    c1, z1 = ops.labelmap_row_bands(*args, N=9, zone=True)
    c2, z2 = ops.labelmap_row_bands(*args, N=9, zone=True)
    assert c1.cpu().numpy().tobytes() == c2.cpu().numpy().tobytes() and z1.cpu().numpy().tobytes() == z2.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _field():
    m, labels, truth = row_field(np.random.default_rng(30), (192, 256), 30, 28)
    infos = [{"id": i, "label_id": int(l)} for i, l in enumerate(labels)]
    want = crop_rows_reference(m, (labels == 0).astype(np.uint8), infos=[(i, int(l)) for i, l in enumerate(labels)])
    return m, labels, infos, want


def _same(got, want, path=""):
    """Integers, bools, strings and None exactly; floats to rtol 1e-12 (NaN equals NaN)."""
    if isinstance(want, dict):
        assert set(got) == set(want), path
        for k in want:
            _same(got[k], want[k], f"{path}.{k}")
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{path}[{i}]")
    elif isinstance(want, (float, np.floating)):
        assert isinstance(got, float), path
        assert (math.isnan(got) and math.isnan(want)) or got == want or abs(got - want) <= 1e-12 * abs(want), (path, got, want)
    else:
        assert type(got) in (int, bool, str, type(None)) and got == want, (path, got, want)


@pytest.mark.parametrize("where", ["host", "device"])
def test_crop_rows_equals_the_restatement(where):
    from weed_instance_segmentation_amd import RowOptions, annotate_rows, crop_rows
    m, labels, infos, want = _field()
    seg = torch.from_numpy(m)
    result = {"segmentation": seg.to(DEV) if where == "device" else seg, "segments_info": infos}
    got = crop_rows(result, RowOptions(vote_labels=[0]), return_zone=True)
    zone = got.pop("zone")
    wz = want["zone"]
    assert zone.is_cuda and zone.dtype == torch.uint8 and np.array_equal(zone.cpu().numpy(), wz)
    assert got["found"] and len(got["rho"]) >= 4
    _same(got, {k: v for k, v in want.items() if k != "zone"})
    json.dumps(got)
    assert "zone" not in crop_rows(result, RowOptions(vote_labels=[0]))
    # a bare map with a vote table, another bin width and a fixed band
    flags = (labels == 0).astype(np.uint8)
    got = crop_rows(seg.to(DEV), RowOptions(vote_labels=[], bin=2, band=5.5, smooth=1), vote=flags)
    _same(got, {k: v for k, v in crop_rows_reference(m, flags, bin=2, band=5.5, smooth=1).items() if k != "zone"})
    # annotate_rows: every entry gets its row
    out = annotate_rows(result, crop_rows(result, RowOptions(vote_labels=[0])))
    assert "row" not in result["segments_info"][0]
    for seg_info, p in zip(out["segments_info"], want["per_instance"]):
        assert (seg_info["row"], seg_info["in_row"]) == (p["row"], p["in_row"])
        assert seg_info["row_offset"] == pytest.approx(p["offset"], rel=1e-12, nan_ok=True)


def test_crop_rows_without_rows():
    from weed_instance_segmentation_amd import RowOptions, crop_rows
    m, labels, infos, _ = _field()
    result = {"segmentation": torch.from_numpy(m).to(DEV), "segments_info": infos}
    got = crop_rows(result, RowOptions(vote_labels=[7]), return_zone=True)   # no such label: nothing votes
    assert not got["found"] and got["contrast"] == 0.0 and got["rho"] == [] and got["lines"] == [] and math.isnan(got["spacing"])
    assert not got["zone"].any() and all(p["row"] == -1 and not p["in_row"] and math.isnan(p["offset"]) for p in got["per_instance"])
    assert [p["area"] for p in got["per_instance"]] == [int((m == i).sum()) for i in range(len(labels))]
    _same({k: v for k, v in got.items() if k != "zone"},
          {k: v for k, v in crop_rows_reference(m, np.zeros(len(labels), np.uint8), infos=[(i, int(l)) for i, l in enumerate(labels)]).items()
           if k != "zone"})


def _cell_sums(mask, cell, offset):
    H, W = mask.shape
    cy, cx = (np.arange(H) + offset[0]) // cell[0], (np.arange(W) + offset[1]) // cell[1]
    out = np.zeros((cy.max() + 1, cx.max() + 1), np.int64)
    np.add.at(out, (cy[:, None].repeat(W, 1), cx[None, :].repeat(H, 0)), mask.astype(np.int64))
    return out


@pytest.mark.parametrize("zone", ["inter_row", "intra_row"])
def test_treatment_grid_with_a_zone(zone):
    from weed_instance_segmentation_amd import RowOptions, TreatmentOptions, crop_rows, ops, treatment_grid
    from weed_instance_segmentation_amd.instances import nearest_rows, squared_cap
    m, labels, infos, want = _field()
    result = {"segmentation": torch.from_numpy(m).to(DEV), "segments_info": infos}
    rows = crop_rows(result, RowOptions(vote_labels=[0]))
    keep = (want["zone"] != 0) if zone == "intra_row" else (want["zone"] == 0)
    target = labels == 1
    # no margin, no protection: the kept pixels of the weeds per cell, counted by numpy
    opts = TreatmentOptions(cell=(32, 24), offset=(3, 5), target_labels=[1], protect_labels=[0])
    grid = treatment_grid(result, opts, rows=rows, zone=zone)
    weeds = np.isin(m, np.nonzero(target)[0])
    assert np.array_equal(grid["coverage"], _cell_sums(weeds & keep, opts.cell, opts.offset))
    assert np.array_equal(grid["cells"], grid["coverage"] >= 1) and not grid["vetoed"].any()
    assert 0 < grid["coverage"].sum() < weeds.sum()
    # a margin and a protection distance: the same grid from the grown map masked on the host
    opts = TreatmentOptions(cell=(32, 24), offset=(3, 5), margin=4, protect=7, target_labels=[1], protect_labels=[0], min_pixels=3)
    grid = treatment_grid(result, opts, rows=rows, zone=zone)
    maps = result["segmentation"].unsqueeze(0)
    N = len(labels)
    grown, _ = nearest_rows(maps, N, squared_cap(4, "test"), target, True)
    _, veto_d2 = nearest_rows(maps, N, squared_cap(7, "test"), labels == 0, False)
    masked = torch.from_numpy(np.where(keep, grown[0].cpu().numpy(), -1).astype(np.int32)).to(DEV).unsqueeze(0)
    group = torch.from_numpy(np.where(target, 0, 255).astype(np.uint8)).to(DEV).unsqueeze(0)
    counts = ops.labelmap_cell_counts(masked, group, 1, opts.cell, opts.offset, veto_d2, squared_cap(7, "test"))[0].cpu().numpy()
    assert np.array_equal(grid["coverage"], counts[..., 0]) and np.array_equal(grid["vetoed"], counts[..., 1])
    assert np.array_equal(grid["cells"], counts[..., 0] >= 3) and grid["cells"].any()
    # without a zone nothing changes, whatever rows is
    plain = treatment_grid(result, opts)
    for other in (treatment_grid(result, opts, None, None), treatment_grid(result, opts, rows=rows)):
        assert set(other) == set(plain)
        for k in plain:
            if isinstance(plain[k], np.ndarray):
                assert np.array_equal(other[k], plain[k]), k
            elif k == "instances":
                assert json.dumps(other[k]) == json.dumps(plain[k])
            else:
                assert other[k] == plain[k], k
    assert not np.array_equal(plain["coverage"], grid["coverage"])


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from weed_instance_segmentation_amd import _lib, ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    m = torch.zeros(1, 8, 8, dtype=torch.int32, device=DEV)
    v = torch.ones(1, 1, dtype=torch.uint8, device=DEV)
    line = torch.tensor([[16384, 0, 0, 0]], dtype=torch.int32, device=DEV)
    rho = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(Wm2fError):
        ops.labelmap_row_votes(m.cpu(), v, _cs(8), 14)
    with pytest.raises(Wm2fError):
        ops.labelmap_row_bands(m.cpu(), line, rho, 0, N=1)
    with pytest.raises(Wm2fError, match="bad size"):
        ops.labelmap_row_votes(m, v, torch.zeros(0, 2, dtype=torch.int32, device=DEV), 14)           # T = 0
    with pytest.raises(Wm2fError, match="code -2"):
        ops.labelmap_row_votes(m, v, torch.zeros(1025, 2, dtype=torch.int32, device=DEV), 14)        # T = 1025
    with pytest.raises(Wm2fError, match="shift"):
        ops.labelmap_row_votes(m, v, _cs(8), 13)
    with pytest.raises(Wm2fError, match="shift"):
        ops.labelmap_row_votes(m, v, _cs(8), 21)
    with pytest.raises(Wm2fError, match="code -2"):
        ops.labelmap_row_bands(m, line, torch.zeros(1, 1025, dtype=torch.int32, device=DEV), 0, N=1)  # Kmax = 1025
    big = torch.zeros(33, 4, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(Wm2fError, match="code -2"):
        ops.labelmap_row_votes(big, torch.ones(33, 1, dtype=torch.uint8, device=DEV), _cs(8), 14)    # B = 33
    with pytest.raises(Wm2fError, match="code -2"):
        ops.labelmap_row_bands(big, line.expand(33, 4).contiguous(), rho.expand(33, 4).contiguous(), 0, N=1)
    with pytest.raises(ValueError):
        ops.labelmap_row_votes(m, v, torch.zeros(8, 3, dtype=torch.int32, device=DEV), 14)
    with pytest.raises(ValueError):
        ops.labelmap_row_bands(m, line, rho, -1, N=1)
    with pytest.raises(TypeError):
        ops.labelmap_row_votes(m.to(torch.int64), v, _cs(8), 14)
    # a side of 16385 through the C entries with null pointers: refused before a pointer is looked at
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    for H, W in ((16385, 8), (8, 16385)):
        assert lib.wm2f_labelmap_row_votes(null, _lib.WM2F_I32, null, null, null, null, 1, H, W, 1, 8, 14, null) == _lib.WM2F_EUNSUPPORTED
        assert lib.wm2f_labelmap_row_bands(null, _lib.WM2F_I32, null, null, null, null, null, null, 1, H, W, 1, 4, 0, null) == _lib.WM2F_EUNSUPPORTED
    assert lib.wm2f_labelmap_row_votes(null, _lib.WM2F_I32, null, null, null, null, 1, 8, 8, 1, 8, 13, null) == _lib.WM2F_EINVAL
    assert lib.wm2f_labelmap_row_votes(null, _lib.WM2F_I32, null, null, null, null, 1, 8, 8, 1, 8, 14, null) == _lib.WM2F_EINVAL  # null pointers
