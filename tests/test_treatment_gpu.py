"""`treatment_grid` on the device: a hand case with its values written out, the numpy restatement on
a random map with an offset grid, the JSON round trip, and a `merge_tile_results` dict as input."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import nearest_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _same(grid, want, H, W):
    assert grid["cells"].dtype == np.bool_ and np.array_equal(grid["cells"], want["cells"])
    assert grid["coverage"].dtype == np.int32 and np.array_equal(grid["coverage"], want["coverage"])
    assert np.array_equal(grid["vetoed"], want["vetoed"])
    assert grid["treated_fraction_exact"] == want["treated_fraction_exact"]
    assert grid["treated_fraction"] == float(want["treated_fraction_exact"])
    assert grid["grid_size"] == tuple(want["grid_size"]) and grid["image_size"] == (H, W)
    assert len(grid["instances"]) == len(want["instances"])
    for a, b in zip(grid["instances"], want["instances"]):
        assert (a["id"], a["label_id"]) == (b["id"], b["label_id"])
        for k in ("treated", "vetoed_fraction"):
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (a, b)


def test_hand_case():
    """16 x 16: a 2 x 2 weed (id 0, label 1) at rows 5-6, columns 2-3 and a 2 x 2 crop plant (id 1, label 0) at columns
    7-8 of the same rows, three free pixels between them.  Margin 2 grows the weed to a disc of 24 pixels over rows 3 .. 8
    and columns 0 .. 5; protect 2 reaches column 5 in rows 5 and 6, so two grown pixels are vetoed.  Cells of 4 x 4."""
    from weed_instance_segmentation_amd import TreatmentOptions, treatment_grid
    m = np.full((16, 16), -1, np.int32)
    m[5:7, 2:4] = 0
    m[5:7, 7:9] = 1
    infos = [{"id": 0, "label_id": 1, "score": 0.9}, {"id": 1, "label_id": 0, "score": 0.8}]
    opt = TreatmentOptions(cell=(4, 4), margin=2, protect=2, target_labels=[1], protect_labels=[0])
    for seg in (torch.from_numpy(m).to(DEV), m, torch.from_numpy(m.astype(np.float32)).to(DEV)):
        grid = treatment_grid({"segmentation": seg, "segments_info": infos}, opt)
        assert grid["cells"].tolist() == [[True, False, False, False], [True, True, False, False],
                                          [True, False, False, False], [False, False, False, False]]
        assert grid["coverage"].tolist() == [[2, 0, 0, 0], [14, 4, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0]]
        assert grid["vetoed"].tolist() == [[0, 0, 0, 0], [0, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
        assert grid["treated_fraction_exact"] == Fraction(1, 4) and grid["treated_fraction"] == 0.25
        assert grid["instances"] == [{"id": 0, "label_id": 1, "treated": 1.0, "vetoed_fraction": 0.0}]
        assert (grid["cell"], grid["offset"], grid["image_size"], grid["grid_size"]) == ((4, 4), (0, 0), (16, 16), (4, 4))
        _same(grid, R.treatment(m, [(0, 1), (1, 0)], (4, 4), margin=2, protect=2, target_labels=[1], protect_labels=[0]), 16, 16)
    # five kept pixels are asked of a cell: the two edge cells and the corner of four go off
    grid = treatment_grid({"segmentation": m, "segments_info": infos}, TreatmentOptions(
        cell=(4, 4), margin=2, protect=2, target_labels=[1], protect_labels=[0], min_pixels=5))
    assert grid["cells"].sum() == 1 and grid["cells"][1, 0] and grid["treated_fraction_exact"] == Fraction(1, 16)
    assert grid["instances"][0]["treated"] == 1.0  # the weed itself lies in cell (1, 0): rows 4-7, columns 0-3
    # no protection: the vetoed pixels are kept
    grid = treatment_grid({"segmentation": m, "segments_info": infos}, TreatmentOptions(cell=(4, 4), margin=2, target_labels=[1]))
    assert grid["coverage"][1, 1] == 6 and grid["vetoed"].sum() == 0
    # nothing to treat, and no segment at all
    grid = treatment_grid({"segmentation": m, "segments_info": infos}, TreatmentOptions(cell=(4, 4), target_labels=[7]))
    assert not grid["cells"].any() and grid["instances"] == [] and grid["treated_fraction_exact"] == 0
    grid = treatment_grid({"segmentation": np.full((5, 9), -1, np.int32), "segments_info": []}, TreatmentOptions(cell=(4, 4)))
    assert grid["cells"].shape == (2, 3) and not grid["cells"].any() and grid["instances"] == []


def test_restatement_on_a_random_map_with_an_offset_grid():
    from weed_instance_segmentation_amd import TreatmentOptions, treatment_grid
    rng = np.random.default_rng(384)
    H, W = 61, 45
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.full((H, W), -1, np.int32)
    labels = []
    for k in range(9):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 5))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
        labels.append(int(k % 3))  # label 0: crop, 1 and 2: weeds
    infos = [{"id": k, "label_id": labels[k]} for k in range(9)] + [{"id": 9, "label_id": 1}]  # id 9 has no pixel
    pairs = [(s["id"], s["label_id"]) for s in infos]
    for kw in (dict(cell=(7, 5), offset=(3, 4), margin=2.5, protect=3, target_labels=(1, 2), protect_labels=(0,)),
               dict(cell=(7, 5), offset=(6, 0), margin=0, protect=6.5, protect_labels=(0,), min_pixels=3),
               dict(cell=(16, 16), offset=(5, 11), margin=4, target_labels=(2,))):
        grid = treatment_grid({"segmentation": torch.from_numpy(m).to(DEV), "segments_info": infos}, TreatmentOptions(**kw))
        want = R.treatment(m, pairs, **{**kw, "target_labels": kw.get("target_labels")})
        _same(grid, want, H, W)
        assert grid["cells"].any() and not grid["cells"].all()
        if kw.get("target_labels") == (1, 2):
            assert grid["instances"][-1]["id"] == 9 and np.isnan(grid["instances"][-1]["treated"])
            assert grid["vetoed"].sum() > 0


def test_json_round_trip(tmp_path):
    from weed_instance_segmentation_amd import TreatmentOptions, load_treatment_grid, save_treatment_grid, treatment_grid
    m = np.full((16, 20), -1, np.int32)
    m[5:7, 2:4] = 0
    m[9:12, 10:15] = 1
    infos = [{"id": 0, "label_id": 1}, {"id": 1, "label_id": 0}, {"id": 2, "label_id": 1}]  # id 2 has no pixel: NaN -> null
    grid = treatment_grid({"segmentation": m, "segments_info": infos},
                          TreatmentOptions(cell=(4, 6), offset=(1, 2), margin=1.5, protect=2, protect_labels=[0]))
    transform = (0.002, 0.0, 431200.0, 0.0, -0.002, 5032110.5)
    for t in (None, transform):
        path = tmp_path / "grid.json"
        save_treatment_grid(path, grid, transform=t)
        back = load_treatment_grid(path)
        assert np.array_equal(back["cells"], grid["cells"]) and back["cells"].dtype == np.bool_
        for k in ("cell", "offset", "image_size", "grid_size", "treated_fraction", "treated_fraction_exact"):
            assert back[k] == grid[k], k
        assert back["transform"] == t
        assert len(back["instances"]) == 2 and back["instances"][0] == grid["instances"][0]
        assert back["instances"][1]["id"] == 2 and np.isnan(back["instances"][1]["treated"])


def test_treatment_grid_of_a_tile_merge():
    """The dict `merge_tile_results` returns goes in as it is."""
    import tile_merge_reference as TM
    from weed_instance_segmentation_amd import TreatmentOptions, merge_tile_results, tile_windows, treatment_grid
    H = W = 112
    g = tile_windows(H, W, 64, 16)
    truth = np.full((H, W), -1, np.int32)
    truth[36:76, 30:82] = 0
    truth[4:20, 6:40] = 1
    truth[90:108, 70:100] = 2
    truth[60:100, 8:14] = 3
    obj_labels = np.array([0, 1, 0, 1], np.int32)
    tiles, n_ids, labels = TM.cut_scene(truth, obj_labels, g.windows, 6, 6, 11)
    results = [{"segmentation": torch.from_numpy(tiles[t]).to(DEV),
                "segments_info": [{"id": i, "label_id": int(labels[t, i]), "was_fused": False, "score": 0.5 + 0.01 * i}
                                  for i in range(int(n_ids[t]))]} for t in range(4)]
    merged = merge_tile_results(results, g)
    kw = dict(cell=(16, 16), offset=(0, 8), margin=10, protect=12, target_labels=(1,), protect_labels=(0,))
    grid = treatment_grid(merged, TreatmentOptions(**kw))
    pairs = [(int(s["id"]), int(s["label_id"])) for s in merged["segments_info"]]
    _same(grid, R.treatment(merged["segmentation"].cpu().numpy(), pairs, **kw), H, W)
    assert len(grid["instances"]) == 2 and grid["vetoed"].sum() > 0 and grid["cells"].sum() >= 6
