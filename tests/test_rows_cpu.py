"""Crop rows without a GPU: the numpy restatement of tests/rows_reference.py finds the truth of
generated row fields and rejects clutter; the host steps of the package (direction, peaks, lines) agree with the
restatement's on hand-made inputs; options, `annotate_rows` and the refusals of `treatment_grid`'s `zone`.

Sweep of the restatement, 24 seeds a case, T = 180, discs of radius 5, jitter 1.5 px, 15 % of the plants missing, one weed
per 4096 pixels, lines shorter than 0.6 of the longest chord unplanted (`row_field` says why):

    image    normal spacing  contrast (crop votes / all vote)  direction error   worst row error
    192x256    0     32      2.46-2.77 / 2.19-2.58             0 / 1 step        1.08 / 1.55 px
    192x256   30     28      2.62-2.98 / 2.44-2.79             0                 0.64 / 0.69
    192x256  100     36      2.90-3.85 / 2.66-3.42             0                 0.65
    192x256  135     30      3.08-3.88 / 2.88-3.57             0                 1.50
    256x192   45     32      3.28-4.58 / 2.97-4.08             0                 1.51 / 1.57
     96x128   20     24      1.95-2.51 / 1.96-2.36             <= 2 steps        0.74 / 1.47
    130x70    60     26      1.97-2.58 / 1.89-2.33 (jitter 0.75)  <= 2 steps     0.76 / 0.98
    130x70    60     26      1.80-2.41 / 1.76-2.19 (jitter 1.5)   <= 3 / 4 steps 0.66 / 0.94

A row of 130x70 carries three to five plants: the direction's spread follows the jitter over the row length, and the
+-2 steps hold at jitter 0.75 only, which is what the test below uses at that size; without jitter every case is exact.
Clutter (60 discs, 9 % cover) gave 1.09-1.36 over 24 seeds at 192x256 and at 256x192, three of the 48 above 1.30 (1.31,
1.31, 1.36); a single blob 1.10.  On small images clutter is NOT told from rows: 12 discs on 130x70 reached 1.93, 15 on
96x128 1.71.  The default `min_contrast` is 1.5, between 1.36 and 1.76."""
import functools
import json
import math

import numpy as np
import pytest
import torch

from rows_reference import (angle_steps, angle_table, bands_reference, clutter_field, crop_rows_reference,
                            direction_reference, footprint_reference, line_reference, n_bins, peaks_reference, row_errors,
                            row_field, votes_reference)

# ((H, W), normal in degrees, spacing, jitter)
FIELDS = [((192, 256), 0, 32, 1.5), ((192, 256), 30, 28, 1.5), ((192, 256), 100, 36, 1.5), ((192, 256), 135, 30, 1.5),
          ((256, 192), 45, 32, 1.5), ((130, 70), 60, 26, 0.75), ((96, 128), 20, 24, 1.5)]
SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _field(shape, deg, spacing, jitter, seed):
    return row_field(np.random.default_rng(seed * 7 + deg), shape, deg, spacing, jitter=jitter)


# ------------------------------------------------------------------------------------------ the restatement finds the truth
@pytest.mark.parametrize("weeds_vote", [False, True])
@pytest.mark.parametrize("shape,deg,spacing,jitter", FIELDS)
def test_restatement_finds_the_rows(shape, deg, spacing, jitter, weeds_vote):
    """Direction within +-2 steps of 180, every row with at least three plants within +-3 px (at the mean of its plants),
    contrast >= 1.5; the spacing within 3 px of the truth."""
    for seed in SEEDS:
        m, labels, truth = _field(shape, deg, spacing, jitter, seed)
        flags = np.ones(len(labels), np.uint8) if weeds_vote else (labels == 0).astype(np.uint8)
        r = crop_rows_reference(m, flags)
        errs = row_errors(r, truth)
        print(shape, deg, seed, weeds_vote, "t", r["t"], "contrast %.3f" % r["contrast"], "row errors", np.round(errs, 2))
        assert r["found"] and r["contrast"] >= 1.5
        assert angle_steps(r["t"], truth["theta"], 180) <= 2
        assert len(errs) >= 2 and max(errs) <= 3
        assert abs(r["spacing"] - spacing) <= 3
        # the angle of the rows themselves: the normal turned back by a quarter, in (-pi/2, pi/2]
        assert -math.pi / 2 < r["angle"] <= math.pi / 2
        assert abs(math.cos(r["angle"]) * r["normal"][0] + math.sin(r["angle"]) * r["normal"][1]) < 1e-4


def test_restatement_assigns_plants_to_their_rows():
    m, labels, truth = _field((192, 256), 30, 28, 1.5, 0)
    r = crop_rows_reference(m, (labels == 0).astype(np.uint8))
    per = {p["id"]: p for p in r["per_instance"]}
    crop = [i for i in range(len(labels)) if labels[i] == 0 and per[i]["area"] > 0]
    rows_of = {}
    for i in crop:
        rows_of.setdefault(truth["plant_row"][i], set()).add(per[i]["row"])
        assert abs(per[i]["offset"]) <= 3 * 1.5 + 1 and per[i]["in_row"]
    assert all(len(v) == 1 for v in rows_of.values())                     # the plants of one true row share a found row
    assert len({next(iter(v)) for v in rows_of.values()}) == len(rows_of)   # and two true rows never do
    assert r["zone"].shape == m.shape and 0 < r["zone"].mean() < 1


def test_restatement_rejects_clutter_and_a_blob():
    for seed in range(4):
        m, labels = clutter_field(np.random.default_rng(1000 + seed), (192, 256), plants=60)
        r = crop_rows_reference(m, np.ones(len(labels), np.uint8))
        print("clutter", seed, "%.3f" % r["contrast"])
        assert r["contrast"] <= 1.3 and not r["found"] and r["rho"] == [] and all(p["row"] == -1 for p in r["per_instance"])
    m = np.full((192, 256), -1, np.int32)
    yy, xx = np.mgrid[0:192, 0:256]
    m[(xx - 100) ** 2 + (yy - 90) ** 2 <= 900] = 0
    r = crop_rows_reference(m, [1])
    assert r["contrast"] <= 1.3 and not r["found"]
    r = crop_rows_reference(np.full((40, 50), -1, np.int32), [1])  # nothing votes
    assert r["contrast"] == 0.0 and not r["found"] and r["t"] == 0


def test_votes_restatement_on_hand_maps():
    H, W, T = 9, 12, 8
    m = np.full((H, W), -1, np.int32)
    m[4, :] = 0                                      # one full row: all its pixels in one bin of the vertical normal
    acc, E = votes_reference(m, [1], T, 14)
    assert acc.shape == (T, n_bins(H, W, 14)) and n_bins(H, W, 14) == H + W - 1
    assert acc[T // 2, 4] == W and acc[T // 2].sum() == W and (acc.sum(1) == W).all()
    assert list(acc[0, :W]) == [1] * W and E[T // 2] == W * W and E[0] == W
    cos, sin = angle_table(T)
    assert cos[0] == 16384 and sin[0] == 0 and cos[T // 2] == 0 and sin[T // 2] == 16384 and (sin >= 0).all()
    acc16, _ = votes_reference(m, [1], T, 16)        # bins of 4 pixels
    assert acc16.shape[1] == ((H + W - 2) >> 2) + 1 and list(acc16[0, :3]) == [4, 4, 4]
    # a float map: fractions, values >= N, negatives and NaN vote nowhere; flags choose among the ids
    f = np.array([[0.0, 1.0, 1.5, 2.0], [np.nan, -1.0, 1.0, 7.0]], np.float32)
    acc, _ = votes_reference(f, [0, 1, 1], 1, 14)
    assert list(acc[0]) == [0, 1, 1, 1, 0]


# ------------------------------------------------------------------------------------------ the package's host steps
PROFILES = [
    ([0, 0, 5, 0, 0, 0, 0, 0, 5, 0, 0], 1, 3, 0.3),          # two equal peaks: the lower bin is taken first
    ([0, 4, 4, 4, 4, 4, 4, 4, 4, 0, 0, 0], 1, 3, 0.5),        # a plateau: min_spacing thins it out
    ([0, 0, 9, 1, 0, 0, 2, 0, 0, 0, 9, 0], 0, 2, 0.3),        # a peak below the fraction is left out
    ([3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7], 2, 4, 0.3),        # windows clipped at both ends
    ([0, 0, 0, 0], 2, 4, 0.3),                                # an empty profile
    ([], 2, 4, 0.3),
    ([0, 6, 0, 0, 6, 0, 0, 6, 0], 0, 3, 1.0),                 # exactly min_spacing apart: all kept
    ([0, 6, 0, 0, 6, 0, 0, 6, 0], 0, 3.5, 1.0),               # a little more: every other one
]


@pytest.mark.parametrize("shift", [14, 16])
@pytest.mark.parametrize("profile,smooth,min_spacing,fraction", PROFILES)
def test_peak_rule_on_hand_made_profiles(profile, smooth, min_spacing, fraction, shift):
    from weed_instance_segmentation_amd.rows import pick_peaks
    width = 1 << (shift - 14)
    bins, rho = pick_peaks(np.array(profile, np.int32), smooth, min_spacing * width, fraction, shift)
    assert rho == peaks_reference(profile, smooth, min_spacing * width, fraction, shift)
    assert rho == sorted(rho) and len(bins) == len(rho)
    if profile == PROFILES[0][0]:
        # the box sums are 5 at bins 1, 2, 3 and 7, 8, 9: the lowest bin of each is taken, the position is bin 2's / 8's centre
        assert bins == [1, 7] and rho == [(2 * 2 + 1) << (shift - 1), (2 * 8 + 1) << (shift - 1)]
    if profile == PROFILES[1][0]:
        assert bins == [2, 5, 8]     # sums 8 12 12 ... 12 8: bin 2 first, then the next ones three bins on
    if profile == PROFILES[2][0]:
        assert bins == [2, 10]
    if profile == PROFILES[3][0]:
        assert bins == [0, 9] and rho == [1 << (shift - 1), 23 << (shift - 1)]   # window 7..11 holds bin 11 alone
    if not any(profile):
        assert bins == [] and rho == []
    if profile == PROFILES[6][0]:
        assert bins == ([1, 4, 7] if min_spacing == 3 else [1, 7])


def test_direction_rule():
    from weed_instance_segmentation_amd.rows import pick_direction
    rng = np.random.default_rng(3)
    for _ in range(20):
        E = rng.integers(0, 2 ** 40, 37)
        FE = rng.integers(1, 2 ** 44, 37)
        assert pick_direction(E, FE) == direction_reference(E, FE)
    assert pick_direction([4, 8, 2, 8], [2, 4, 1, 4]) == (0, 1.0)          # all equal: the lowest t
    assert pick_direction([1, 6, 3], [1, 2, 1])[0] == 1 and pick_direction([1, 6, 3], [1, 2, 1])[1] == 1.0
    assert pick_direction([0, 0, 0], [5, 6, 7]) == (0, 0.0)
    assert pick_direction([0, 0, 9], [5, 6, 7]) == (2, float("inf"))
    # a product above 2^64: Python integers decide
    assert pick_direction([2 ** 43 + 1, 2 ** 43], [2 ** 43, 2 ** 43 - 1])[0] == 1
    with pytest.raises(ValueError):
        pick_direction([1, 2], [1, 0])


def test_row_lines_meet_the_border():
    from weed_instance_segmentation_amd.ops.rows import row_angle_table, row_bins, row_offset
    from weed_instance_segmentation_amd.rows import row_line
    H, W, T = 70, 130, 180
    table = row_angle_table(T)
    cos, sin = angle_table(T)
    assert np.array_equal(table[:, 0], cos) and np.array_equal(table[:, 1], sin) and table.dtype == np.int32
    assert row_bins(H, W, 14) == n_bins(H, W, 14) and row_bins(H, W, 17) == n_bins(H, W, 17)
    for t in (0, 1, 45, 90, 91, 135, 179):
        c, s = int(cos[t]), int(sin[t])
        off = row_offset(c, W)
        assert off == -min(0, c) * (W - 1)
        for rho in (0, 5 << 14, (40 << 14) + 77, (W + H) << 14):
            got = row_line(c, s, off, rho, H, W)
            assert got == line_reference(c, s, off, rho, H, W)
            if got is not None:
                for x, y in got:
                    assert 0 <= x <= W - 1 and 0 <= y <= H - 1 and abs(x * c + y * s + off - rho) < 1e-6 * (1 << 14)
    assert row_line(16384, 0, 0, 10 << 14, H, W) == [[10.0, 0.0], [10.0, float(H - 1)]]
    assert row_line(0, 16384, 0, 10 << 14, H, W) == [[0.0, 10.0], [float(W - 1), 10.0]]
    assert row_line(16384, 0, 0, (W + 5) << 14, H, W) is None


def test_bands_restatement_on_a_hand_map():
    m = np.array([[0, 0, 1, 1, -1, 2], [0, 0, 1, 1, -1, 2]], np.int32)
    counts, zone = bands_reference(m, [16384, 0, 0, 2], [1 << 14, 5 << 14], 1 << 14, N=3)   # rows at x = 1 and x = 5
    assert zone.tolist() == [[1, 1, 1, 0, 1, 1]] * 2
    assert counts.tolist() == [[4, 4, 2 << 14], [4, 2, 10 << 14], [2, 2, 10 << 14]]
    counts, zone = bands_reference(m, [16384, 0, 0, 0], [1 << 14, 5 << 14], 1 << 14, N=3)   # K = 0: nothing is in a band
    assert not zone.any() and counts[:, 1].tolist() == [0, 0, 0] and counts[:, 0].tolist() == [4, 4, 2]
    counts, _ = bands_reference(m + 10, [16384, 0, 0, 2], [1 << 14, 5 << 14], 0, ids=[10, 12, 15])
    assert counts.tolist() == [[4, 2, 2 << 14], [2, 2, 10 << 14], [0, 0, 0]]


# ------------------------------------------------------------------------------------------ options and the public interface
def test_row_options_validation():
    from weed_instance_segmentation_amd import RowOptions
    o = RowOptions(vote_labels=[0])
    assert (o.vote_labels, o.angles, o.bin, o.smooth, o.min_spacing, o.peak_fraction, o.band, o.min_contrast) == (
        (0,), 180, 1, 2, 16.0, 0.3, None, 1.5)
    assert o.shift == 14 and RowOptions(vote_labels=(1, 2), bin=4).shift == 16 and RowOptions(vote_labels=[], band=0).band == 0.0
    with pytest.raises(TypeError):
        RowOptions()
    bad = [dict(vote_labels=3), dict(vote_labels=[0.5]), dict(vote_labels=[True]), dict(vote_labels=[0], angles=0),
           dict(vote_labels=[0], angles=1025), dict(vote_labels=[0], angles=90.0), dict(vote_labels=[0], bin=3),
           dict(vote_labels=[0], bin=128), dict(vote_labels=[0], bin=0), dict(vote_labels=[0], smooth=-1),
           dict(vote_labels=[0], smooth=1.5), dict(vote_labels=[0], min_spacing=0), dict(vote_labels=[0], min_spacing="16"),
           dict(vote_labels=[0], peak_fraction=0), dict(vote_labels=[0], peak_fraction=1.5),
           dict(vote_labels=[0], band=-1), dict(vote_labels=[0], band=float("nan")), dict(vote_labels=[0], min_contrast=-0.1),
           dict(vote_labels=[0], min_contrast=None), dict(vote_labels=[0], angles=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            RowOptions(**kw)


def _fake_rows(found=True):
    return {"found": found, "line": [16384, 0, 0], "rho_fixed": [5 << 14] if found else [], "band_fixed": 1 << 14,
            "image_size": (8, 8),
            "per_instance": [{"id": 0, "label_id": 0, "area": 4, "row": 0, "offset": -0.5, "in_row": True},
                             {"id": 2, "label_id": 1, "area": 0, "row": -1, "offset": float("nan"), "in_row": False}]}


def test_annotate_rows_returns_a_new_result():
    from weed_instance_segmentation_amd import annotate_rows
    seg = torch.zeros(8, 8, dtype=torch.int32)
    result = {"segmentation": seg, "segments_info": [{"id": 0, "label_id": 0, "score": 0.9}, {"id": 1, "label_id": 1},
                                                     {"id": 2, "label_id": 1}]}
    before = json.dumps(result["segments_info"])
    out = annotate_rows(result, _fake_rows())
    assert json.dumps(result["segments_info"]) == before and out is not result and out["segmentation"] is seg
    assert out["segments_info"][0] == {"id": 0, "label_id": 0, "score": 0.9, "row": 0, "row_offset": -0.5, "in_row": True}
    assert out["segments_info"][1]["row"] == -1 and math.isnan(out["segments_info"][1]["row_offset"])   # not listed
    assert out["segments_info"][2]["row"] == -1 and out["segments_info"][2]["in_row"] is False
    with pytest.raises(ValueError):
        annotate_rows(result, {"found": True})
    with pytest.raises(ValueError):
        annotate_rows([], _fake_rows())


def test_zone_argument_refusals_and_no_gpu_behaviour():
    import inspect
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import RowOptions, TreatmentOptions, crop_rows, ops, rows, treatment_grid
    from weed_instance_segmentation_amd._lib import Wm2fError
    assert pkg.crop_rows is rows.crop_rows and pkg.annotate_rows is rows.annotate_rows and pkg.RowOptions is rows.RowOptions
    assert list(inspect.signature(treatment_grid).parameters) == ["result", "options", "rows", "zone"]
    assert list(inspect.signature(ops.labelmap_row_votes).parameters) == ["maps", "vote", "cs", "shift"]
    assert list(inspect.signature(ops.labelmap_row_bands).parameters) == ["maps", "line", "rho", "band", "ids", "n_ids", "N", "zone"]
    result = {"segmentation": torch.zeros(8, 8, dtype=torch.int32), "segments_info": [{"id": 0, "label_id": 1}]}
    opts = TreatmentOptions(cell=(4, 4))
    for kw in (dict(zone="inter_row"), dict(zone="intra_row", rows=_fake_rows(found=False)), dict(zone="between", rows=_fake_rows()),
               dict(zone="inter_row", rows=[1])):
        with pytest.raises(ValueError):
            treatment_grid(result, opts, **kw)
    with pytest.raises(TypeError):
        crop_rows(result, {"vote_labels": [0]})
    with pytest.raises(ValueError):
        crop_rows(result["segmentation"], RowOptions(vote_labels=[0]))              # a bare map without vote
    with pytest.raises(ValueError):
        crop_rows(result, RowOptions(vote_labels=[0]), vote=[1])                     # a result with vote
    with pytest.raises(ValueError):
        crop_rows(torch.zeros(2, 8, 8, dtype=torch.int32), RowOptions(vote_labels=[0]), vote=[1])
    with pytest.raises(TypeError):
        crop_rows(torch.zeros(8, 8, dtype=torch.int64), RowOptions(vote_labels=[0]), vote=[1])
    # every op refuses host tensors: there is no CPU fallback
    m = torch.zeros(1, 8, 8, dtype=torch.int32)
    cs = torch.from_numpy(ops.row_angle_table(4))
    with pytest.raises(Wm2fError):
        ops.labelmap_row_votes(m, torch.ones(1, 1, dtype=torch.uint8), cs, 14)
    with pytest.raises(Wm2fError):
        ops.labelmap_row_bands(m, torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), 0, N=1)
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            crop_rows(result, RowOptions(vote_labels=[1]))
        with pytest.raises(Wm2fError):
            treatment_grid(result, opts, rows=_fake_rows(), zone="inter_row")


def test_result_serialises_to_json():
    m, labels, _ = _field((96, 128), 20, 24, 1.5, 0)
    r = crop_rows_reference(m, (labels == 0).astype(np.uint8), infos=[(i, int(l)) for i, l in enumerate(labels)])
    r.pop("zone")
    back = json.loads(json.dumps(r))
    assert back["rho_fixed"] == r["rho_fixed"] and back["lines"] == r["lines"] and back["found"] is True
    assert len(back["per_instance"]) == len(labels) and back["per_instance"][0]["label_id"] == 0
