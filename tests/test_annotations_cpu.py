"""Host side of the GPU instance-map builder: OpenCV's nearest index tables, a CPU restatement of
the reference loaders' steps 2-4 with OpenCV's component order (checked on hand cases), refusal of host tensors and the
dataset classes' file handling."""
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from weed_instance_segmentation_amd import annotations as A
from weed_instance_segmentation_amd._lib import Wm2fError

_EIGHT = np.ones((3, 3), dtype=bool)


# ------------------------------------------------------------------------------------------- CPU restatement
def nearest_formula(src: int, dst: int) -> np.ndarray:
    """OpenCV resizeNN, written out per index: ifx = 1.0 / (dst / src), sx = min(floor(x * ifx), src - 1)."""
    ifx = 1.0 / (dst / src)
    return np.array([min(int(np.floor(x * ifx)), src - 1) for x in range(dst)], dtype=np.int32)


def restate_resize(mask: np.ndarray, dsize) -> np.ndarray:
    w, h = dsize
    return mask[nearest_formula(mask.shape[0], h)][:, nearest_formula(mask.shape[1], w)]


def components_cv2_order(binary: np.ndarray):
    """(n, labels) of the 8-connected components of a binary map, numbered 1..n by their first 2 x 2 block in
    block-raster order (OpenCV's block-based labelling), starting from scipy's raster-order labels."""
    lab, n = ndimage.label(binary, structure=_EIGHT)
    if n == 0:
        return 0, lab.astype(np.int32)
    H, W = binary.shape
    blk = (np.arange(H)[:, None] >> 1) * ((W + 1) // 2) + (np.arange(W)[None, :] >> 1)
    first = np.full(n + 1, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, lab.ravel(), blk.ravel().astype(np.int64))
    order = np.argsort(first[1:], kind="stable")
    assert np.unique(first[1:]).size == n  # one component per (class, block): same-class pixels of a block touch
    relabel = np.zeros(n + 1, dtype=np.int32)
    relabel[order + 1] = np.arange(1, n + 1, dtype=np.int32)
    return n, relabel[lab]


def restate_instance_map(classes: np.ndarray, class_order, semantic_of=None):
    """Steps 3-4 of the loaders on a class map: per class in `class_order`, components in OpenCV order, ids 1, 2, ...
    skipping 255, 255 elsewhere.  semantic_of maps a class to the id recorded in the dict (default: the class)."""
    H, W = classes.shape
    inst = np.full((H, W), 255, dtype=np.int32)
    id_to_sem = {}
    cur = 1
    for c in class_order:
        n, lab = components_cv2_order(classes == c)
        ids = np.zeros(n + 1, dtype=np.int32)
        for k in range(1, n + 1):
            if cur == 255:
                cur += 1
            ids[k] = cur
            id_to_sem[cur] = int(c) if semantic_of is None else semantic_of[c]
            cur += 1
        inst = np.where(lab > 0, ids[lab], inst)
    return inst, id_to_sem


def restate_semantic(semantic: np.ndarray, dsize=None):
    """PhenoBench (dataset.py:85-116): classes in ascending value order, 0 skipped."""
    if dsize is not None:
        semantic = restate_resize(semantic, dsize)
    return restate_instance_map(semantic, [c for c in np.unique(semantic) if c != 0])


def restate_color(mask_rgb: np.ndarray, color_map: dict, dsize=None):
    """CropWeed PNG (dataset_from_png_annotations.py:80-116): colours in dict order, exact match."""
    if dsize is not None:
        mask_rgb = restate_resize(mask_rgb, dsize)
    inst = np.full(mask_rgb.shape[:2], 255, dtype=np.int32)
    id_to_sem, cur = {}, 1
    for info in color_map.values():
        n, lab = components_cv2_order(np.all(mask_rgb == np.array(info["color"]), axis=-1))
        ids = np.zeros(n + 1, dtype=np.int32)
        for k in range(1, n + 1):
            if cur == 255:
                cur += 1
            ids[k] = cur
            id_to_sem[cur] = info["id"]
            cur += 1
        inst = np.where(lab > 0, ids[lab], inst)
    return inst, id_to_sem


def restate_cc(mask: np.ndarray):
    """cv2.connectedComponents(mask): (num_labels counting the background, int32 labels)."""
    n, lab = components_cv2_order(mask != 0)
    return n + 1, lab


# ------------------------------------------------------------------------------------------- nearest tables
def test_nearest_table_pins_the_float64_formula():
    t = A.cv2_nearest_table(1488, 1024)
    assert t[64] == 92 and 64 * 1488 // 1024 == 93
    r = A.cv2_nearest_table(430, 426)
    assert r[213] == 214 and 213 * 430 // 426 == 215
    for src, dst in [(1488, 1024), (430, 426), (1296, 1024), (966, 1024), (1, 7), (7, 1), (1024, 1024), (3000, 17),
                     (17, 3000), (1365, 1023)]:
        np.testing.assert_array_equal(A.cv2_nearest_table(src, dst), nearest_formula(src, dst), err_msg=f"{src}->{dst}")


def test_nearest_table_differs_from_integer_formula_often():
    """The double rounding is not a corner case: across realistic sizes many entries differ from x * src // dst."""
    diff = 0
    for src in range(1025, 2049):
        t = A.cv2_nearest_table(src, 1024)
        diff += int((t != (np.arange(1024) * src // 1024)).sum())
    assert diff > 0


def test_nearest_table_rejects_empty_sizes():
    with pytest.raises(ValueError):
        A.cv2_nearest_table(0, 4)


# ------------------------------------------------------------------------------------------- ordering rule
def test_block_order_differs_from_pixel_order():
    m = np.array([[0, 0, 0, 0, 0, 1],
                  [1, 0, 0, 0, 0, 0]], dtype=np.uint8)
    n, lab = restate_cc(m)
    assert n == 3
    assert lab[1, 0] == 1 and lab[0, 5] == 2
    sc, _ = ndimage.label(m, structure=_EIGHT)
    assert sc[0, 5] == 1 and sc[1, 0] == 2  # scipy numbers by the first pixel instead


def test_eight_connectivity_joins_diagonals():
    m = np.eye(6, dtype=np.uint8)
    m[0, 5] = 1
    n, lab = restate_cc(m)
    assert n == 3 and lab[0, 0] == 1 and lab[5, 5] == 1 and lab[0, 5] == 2


def test_instance_map_class_order_and_ids():
    sem = np.array([[2, 2, 0, 1],
                    [0, 0, 0, 1],
                    [7, 0, 2, 0]], dtype=np.uint16)
    inst, d = restate_semantic(sem)
    # class 1 first (one component), then class 2 (two), then class 7
    assert d == {1: 1, 2: 2, 3: 2, 4: 7}
    np.testing.assert_array_equal(inst, [[2, 2, 255, 1], [255, 255, 255, 1], [4, 255, 3, 255]])


def test_instance_map_skips_255():
    sem = np.zeros((2, 2 * 300), dtype=np.uint16)
    sem[0, ::2] = 1  # 300 isolated pixels
    inst, d = restate_semantic(sem)
    assert len(d) == 300 and 255 not in d and max(d) == 301
    assert 255 not in set(np.unique(inst[0, ::2]).tolist())
    assert inst[0, 2 * 253] == 254 and inst[0, 2 * 254] == 256


def test_color_restatement_uses_dict_order_and_ids():
    cm = {"crop": {"color": [0, 255, 0], "id": 0}, "weed": {"color": [255, 0, 0], "id": 1}}
    rgb = np.zeros((2, 4, 3), dtype=np.uint8)
    rgb[0, 0] = [255, 0, 0]
    rgb[1, 3] = [0, 255, 0]
    rgb[0, 2] = [0, 254, 0]  # not an exact match: background
    inst, d = restate_color(rgb, cm)
    assert d == {1: 0, 2: 1}
    assert inst[1, 3] == 1 and inst[0, 0] == 2 and inst[0, 2] == 255


# ------------------------------------------------------------------------------------------- host tensors refused
def test_cpu_tensors_are_refused():
    m = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(Wm2fError):
        A.connected_components(m)
    with pytest.raises(Wm2fError):
        A.resize_nearest(m, (2, 2))
    with pytest.raises(Wm2fError):
        A.semantic_to_instance_map(m.to(torch.int32))
    with pytest.raises(Wm2fError):
        A.color_mask_to_instance_map(torch.zeros(4, 4, 3, dtype=torch.uint8), {"a": {"color": [1, 2, 3], "id": 0}})
    from weed_instance_segmentation_amd import ops, _lib
    with pytest.raises(Wm2fError):
        ops.label_components(m, _lib.WM2F_CCL_BINARY)
    with pytest.raises(Wm2fError):
        ops.resize_nearest_tables(m, [0, 1], [0, 1])


def test_four_connectivity_is_not_offered():
    with pytest.raises(ValueError):
        A.connected_components(torch.zeros(2, 2, dtype=torch.uint8), connectivity=4)


# ------------------------------------------------------------------------------------------- dataset file handling
def _png(path, arr, mode=None):
    from PIL import Image
    (Image.fromarray(arr, mode) if mode else Image.fromarray(arr)).save(path)


def test_semantic_png_reader_keeps_16_bit_values(tmp_path):
    a = np.array([[0, 1, 1000], [65535, 2, 0]], dtype=np.uint16)
    p = str(tmp_path / "m.png")
    _png(p, a)
    got = A._read_semantic_png(p)
    assert got.dtype == np.uint16
    np.testing.assert_array_equal(got, a)
    b = np.array([[0, 3], [4, 0]], dtype=np.uint8)
    _png(p, b)
    got = A._read_semantic_png(p)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, b)


def test_palette_semantic_png_raises(tmp_path):
    from PIL import Image
    im = Image.fromarray(np.array([[0, 1], [2, 1]], dtype=np.uint8)).convert("P")
    p = str(tmp_path / "m.png")
    im.save(p)
    with pytest.raises(ValueError, match="mode"):
        A._read_semantic_png(p)


def test_dataset_file_pairing(tmp_path):
    img, ann = tmp_path / "images", tmp_path / "ann"
    img.mkdir()
    ann.mkdir()
    rgb = np.zeros((4, 4, 3), dtype=np.uint8)
    for name in ["b.png", "a.png", "c.png"]:
        _png(str(img / name), rgb)
    for name in ["a.png", "c.png"]:
        _png(str(ann / name), np.zeros((4, 4), dtype=np.uint16))
    ds = A.PhenoBenchDataset(str(img), str(ann), processor=None, label2id={})
    assert [os.path.basename(i) for i, _ in ds.valid_files] == ["a.png", "c.png"] and len(ds) == 2
    ds = A.PhenoBenchDataset(str(img), str(ann), processor=None, label2id={}, max_images=1)
    assert len(ds) == 1

    img2, ann2 = tmp_path / "cw_images", tmp_path / "cw_ann"
    img2.mkdir()
    ann2.mkdir()
    for name in ["001_image.png", "002_image.png"]:
        _png(str(img2 / name), rgb)
    _png(str(ann2 / "002_annotation.png"), rgb)
    ds = A.CropWeedDataset(str(img2), str(ann2), processor=None, label2id={"crop": 5, "weed": 6})
    assert [os.path.basename(m) for _, m in ds.valid_files] == ["002_annotation.png"]
    assert [v["id"] for v in ds.color_map().values()] == [5, 6]
