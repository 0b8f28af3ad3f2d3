"""Run-length encodings on the host: the COCO string codec pinned by hand-worked cases (pycocotools
is not installed), the host layer fed with the restatement's toggle lists, the results export, and the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import rle_reference as R
from weed_instance_segmentation_amd import rle as M


# ------------------------------------------------------------------------------------------------ the string codec
@pytest.mark.parametrize("counts,string", [([5], "5"), ([15], "?"), ([16], "`0"), ([0], "0"), ([], "")])
def test_codec_single_values(counts, string):
    # 5 -> group 5, nothing left: chr(48 + 5).  15 -> 0b01111: bit 4 clear and nothing left: chr(63).
    # 16 -> 0b10000: bit 4 is set and the rest (0) is not -1, so a continuation follows: chr(48 + 16 + 32), then "0".
    assert R.to_string(counts) == string and M.rle_to_string(counts) == string
    assert R.from_string(string) == counts and M.rle_from_string(string) == counts


def test_codec_delta_of_minus_one_is_O():
    # index 3 stores counts[3] - counts[1] = -1: group 31, the rest -1 with bit 4 set ends the number: chr(48 + 31)
    counts = [2, 7, 4, 6]
    assert M.rle_to_string(counts) == "274O" == R.to_string(counts)
    assert M.rle_from_string("274O") == counts


def test_codec_worked_example():
    # counts        3    20    1000   19    1030   20    430
    # stored        3    20    1000   -1    30     1     -600        (index > 2: minus counts[i - 2])
    #   3    -> "3"
    #   20   -> 0b10100: group 20, rest 0, bit 4 set and rest != -1 -> 20 + 32 + 48 = 100 "d", then group 0 -> "0"
    #   1000 -> 31 * 32 + 8: group 8, rest 31 -> 8 + 32 + 48 = 88 "X"; group 31, rest 0, bit 4 set and rest != -1 ->
    #           31 + 32 + 48 = 111 "o"; group 0 -> "0"                                          (three characters)
    #   -1   -> "O"
    #   30   -> group 30, rest 0, bit 4 set -> 30 + 32 + 48 = 110 "n"; then "0"
    #   1    -> "1"
    #   -600 -> -19 * 32 + 8: group 8, rest -19 -> "X"; -19 = -1 * 32 + 13: group 13, rest -1, bit 4 clear and rest != 0
    #           -> 13 + 32 + 48 = 93 "]"; group 31, rest -1, bit 4 set and rest == -1 -> 79 "O"  (a three-character delta)
    counts = [3, 20, 1000, 19, 1030, 20, 430]
    want = "3d0Xo0On01X]O"
    assert R.to_string(counts) == want and M.rle_to_string(counts) == want
    assert R.from_string(want) == counts and M.rle_from_string(want) == counts
    assert M.rle_from_string(want.encode()) == counts  # bytes, as some files carry them


def test_codec_round_trip_on_random_counts():
    rng = np.random.default_rng(0)
    for trial in range(40):
        n = int(rng.integers(1, 60))
        c = rng.integers(0, 50, n)
        c[rng.random(n) < 0.2] = 0
        big = rng.random(n) < 0.2
        c[big] = rng.integers(2 ** 20, 2 ** 28, int(big.sum()))
        c = c.tolist()
        s = M.rle_to_string(c)
        assert s == R.to_string(c), trial
        assert M.rle_from_string(s) == c and R.from_string(s) == c


def test_codec_refuses_a_truncated_string():
    with pytest.raises(ValueError):
        M.rle_from_string("`")  # a continuation bit on the last character


# ------------------------------------------------------------------------- the host layer on the restatement's toggles
def _fixture_maps():
    g = load_golden("postprocess_instances.npz")
    return [g[k].astype(np.int64) for k in sorted(g) if k.startswith("seg_")]


def _host_encode(m, N, fmt, compressed=True):
    counts, positions, offsets = R.csr([m], N, M.FORMATS[fmt])
    return M.encode_toggles(counts, positions, offsets, m.shape, fmt, compressed)[0]


def test_reference_toggles_by_hand():
    m = np.array([[0, 0, -1], [-1, 1, 1]])  # row-major 0 0 -1 -1 1 1; column-major 0 -1 0 1 -1 1
    assert R.toggle_lists(m, 2, 0) == ([[2, 4], [0, 2], [4, 6]], 0)
    assert R.toggle_lists(m, 2, 1) == ([[1, 2, 4, 5], [0, 1, 2, 3], [3, 4, 5, 6]], 0)
    assert R.toggle_lists(m, 1, 0)[1] == 2  # id 1 is outside [-1, 1)
    assert R.coco_counts(m == 1) == [3, 1, 1, 1] and R.coco_counts(m == 0) == [0, 1, 1, 1, 3]


def test_hf_equals_binary_mask_to_rle_on_the_fixture_maps():
    from weed_instance_segmentation_amd.postprocess import binary_mask_to_rle, convert_segmentation_to_rle
    maps = _fixture_maps()
    assert maps
    small = 0
    for m in maps:
        if m.size > 20000:  # the plain-loop restatement walks every pixel
            m = m[::4, ::4]
        small += 1
        N = int(m.max()) + 1
        got = _host_encode(m, N, "hf")
        ids = np.unique(m).tolist()
        assert list(got) == ids  # ascending, -1 first, ids without pixels absent
        for k in ids:
            assert got[k] == binary_mask_to_rle(torch.from_numpy((m == k).astype(np.int64))) == R.hf_rle(m == k)
        assert list(got.values()) == convert_segmentation_to_rle(torch.from_numpy(m))
    assert small


def test_coco_counts_sum_and_decode():
    rng = np.random.default_rng(1)
    for shape in [(1, 1), (3, 5), (7, 6), (12, 9)]:
        m = rng.integers(-1, 3, shape)
        m[-1, -1] = 2  # id 2 owns the last pixel: no trailing 0
        m[0, 0] = 0  # id 0 owns the first: a leading 0
        N = 5  # ids 3 and 4 have no pixel
        plain = _host_encode(m, N, "coco", compressed=False)
        packed = _host_encode(m, N, "coco")
        assert sorted(plain) == np.unique(m).tolist() and 3 not in plain and 4 not in plain
        for k, rle in plain.items():
            c = rle["counts"]
            assert rle["size"] == list(shape) and c == R.coco_counts(m == k)
            assert sum(c) == m.size and all(v > 0 for v in c[1:])
            assert np.array_equal(R.decode_coco(c, *shape), m == k)
            assert packed[k] == {"size": list(shape), "counts": R.to_string(c)}
            runs = M.rle_to_runs(packed[k])
            assert runs[:, 1].sum() == (m == k).sum() and np.array_equal(runs, M.rle_to_runs(rle))
        assert plain[0]["counts"][0] == 0
        if m.size > 1:
            assert len(plain[2]["counts"]) % 2 == 0  # it ends in a 1-run


def test_runs_of_an_hf_list():
    assert M.rle_to_runs([1, 2, 6, 1], "hf").tolist() == [[0, 2], [5, 1]]
    assert M.rle_to_runs({"size": [2, 3], "counts": [0, 2, 3, 1]}).tolist() == [[0, 2], [5, 1]]
    assert M.rle_to_runs({"size": [2, 3], "counts": [6]}).tolist() == []


# ------------------------------------------------------------------------------------------------- the results export
def test_coco_results_field_by_field(monkeypatch):
    seg_a, seg_b = torch.zeros(4, 6), torch.zeros(2, 3)
    calls = []

    def fake_encode(maps, n=None, format="coco", compressed=True):
        calls.append((tuple(maps[0].shape), len(maps), n, format, compressed))
        return [{-1: {"size": list(m.shape), "counts": "x"}, 0: {"size": list(m.shape), "counts": f"rle{i}"}}
                for i, m in enumerate(maps)]

    monkeypatch.setattr(M, "encode_label_maps", fake_encode)
    info = lambda i, label, score, **k: {"id": i, "label_id": label, "was_fused": False, "score": score, **k}
    results = [{"segmentation": seg_a, "segments_info": [info(0, 2, 0.75, area=7, bbox=[1, 0, 3, 4], centroid=(2.0, 1.5)),
                                                         info(1, 1, 0.5, area=0, bbox=[0, 0, 0, 0], centroid=None)]},
               {"segmentation": seg_b, "segments_info": []},
               {"segmentation": seg_a, "segments_info": [info(0, 1, 0.25, area=3, bbox=[0, 1, 2, 2], centroid=(0.5, 1.5))]}]
    out = M.coco_results(results, ["a.png", "b.png", "c.png"], category_of={1: 10, 2: 20})
    assert calls == [((4, 6), 2, 2, "coco", True), ((2, 3), 1, 0, "coco", True)]  # one encode per distinct size
    assert out == [{"image_id": "a.png", "category_id": 20, "segmentation": {"size": [4, 6], "counts": "rle0"},
                    "bbox": [1, 0, 3, 4], "area": 7, "score": 0.75},
                   {"image_id": "c.png", "category_id": 10, "segmentation": {"size": [4, 6], "counts": "rle1"},
                    "bbox": [0, 1, 2, 2], "area": 3, "score": 0.25}]  # id 1 of image a owns no pixel: no entry
    assert M.coco_results(results, [1, 2, 3], category_of=lambda l: l + 100)[0]["category_id"] == 102
    assert M.coco_results(results, [1, 2, 3])[1]["category_id"] == 1
    with pytest.raises(ValueError):
        M.coco_results(results, [1, 2])
    del results[0]["segments_info"][0]["bbox"]
    with pytest.raises(ValueError, match="return_instance_stats"):
        M.coco_results(results, [1, 2, 3])


def test_save_coco_results_writes_json(monkeypatch, tmp_path):
    import json
    monkeypatch.setattr(M, "encode_label_maps", lambda maps, **k: [{0: {"size": [2, 2], "counts": "04"}} for _ in maps])
    results = [{"segmentation": torch.zeros(2, 2), "segments_info": [{"id": 0, "label_id": 3, "score": 0.5, "area": 4,
                                                                        "bbox": [0, 0, 2, 2]}]}]
    path = tmp_path / "res.json"
    out = M.save_coco_results(str(path), results, [17])
    assert json.loads(path.read_text()) == out and out[0]["image_id"] == 17 and out[0]["category_id"] == 3


# ---------------------------------------------------------------------------------------- argument errors, the C ABI
def test_ops_refuse_host_tensors_and_bad_arguments():
    from weed_instance_segmentation_amd import _lib, ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    with pytest.raises(Wm2fError):
        ops.labelmap_toggles(torch.zeros(1, 4, 4), N=3)
    with pytest.raises(Wm2fError):
        ops.labelmap_toggle_counts(torch.zeros(1, 4, 4, dtype=torch.int32), N=3, order=1)
    with pytest.raises(TypeError):
        ops.labelmap_toggles(np.zeros((1, 4, 4), np.float32), N=3)
    with pytest.raises(Wm2fError):
        ops.rle_paint_(torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        M.encode_label_maps(torch.zeros(4, 4), format="png")
    with pytest.raises(ValueError):
        M.decode_rle([[1, 2]], format="hf")  # no size
    if not torch.cuda.is_available():
        with pytest.raises(Wm2fError):
            M.encode_label_maps(torch.zeros(4, 4), n=2)
    assert _lib.WM2F_RLE_MAX_IDS >= 256


def test_header_declares_and_lib_binds_the_entry_points():
    from weed_instance_segmentation_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "wm2f.h")) as f:
        header = f.read()
    want = {
        "wm2f_rle_workspace": ["int B", "int H", "int W", "int N", "int order"],
        "wm2f_labelmap_toggle_counts": ["const void* map", "int dtype", "int32_t* counts", "int32_t* out_of_range",
                                        "void* workspace", "int B", "int H", "int W", "int N", "int order", "void* stream"],
        "wm2f_labelmap_toggles": ["const void* map", "int dtype", "const int32_t* offsets", "int32_t* positions",
                                  "void* workspace", "int B", "int H", "int W", "int N", "int order", "void* stream"],
        "wm2f_rle_paint_workspace": ["int B", "int H", "int W"],
        "wm2f_rle_paint": ["int32_t* out", "const int32_t* runs", "int R", "int32_t* status", "void* workspace", "int B",
                           "int H", "int W", "int order", "void* stream"],
    }
    for name, args in want.items():
        proto = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*)\);", header, re.M)
        assert proto is not None, name
        assert [a.strip() for a in " ".join(proto.group(1).split()).split(",")] == args
        assert len(_lib.SIGNATURES[name][1]) == len(args)
    cap = re.search(r"#define WM2F_RLE_MAX_IDS (\d+)", header)
    assert cap is not None and int(cap.group(1)) == _lib.WM2F_RLE_MAX_IDS
    assert "rle.hip" in _build.SOURCES


def test_package_exports():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import annotations, ops
    for name in ("encode_label_maps", "decode_rle", "rle_to_string", "rle_from_string", "coco_results", "save_coco_results"):
        assert getattr(pkg, name) is getattr(M, name)
    for name in ("labelmap_toggle_counts", "labelmap_toggles", "rle_paint_"):
        assert callable(getattr(ops, name))
    assert callable(annotations.rle_to_instance_map)
    import inspect
    from weed_instance_segmentation_amd.metrics import test_with_metrics
    assert inspect.signature(test_with_metrics).parameters["results_json"].default is None
