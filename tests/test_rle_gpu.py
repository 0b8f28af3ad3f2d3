"""Run-length encoding and decoding of id maps on the GPU: every comparison is exact equality against
the plain-loop restatement of tests/rle_reference.py."""
import functools
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
import rle_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
# a pixel; a line shorter than a wave; a wave boundary at a line end (and one past it); several wave steps and a tail;
# tall and narrow; several groups of rows and more than one wave of columns
SHAPES = [(1, 1), (3, 5), (7, 64), (7, 65), (5, 130), (130, 5), (97, 131)]
DTYPES = [torch.float32, torch.int32, torch.uint8]
ORDERS = [0, 1]
N_SMALL = 3


def _from_flat(flat, shape, order):
    H, W = shape
    return flat.reshape(H, W) if order == 0 else flat.reshape(W, H).T.copy()


@functools.lru_cache(maxsize=None)
def _hand_maps(shape, order):
    """(5, H, W) int64, ids in [-1, 3): all background; one segment that fills the map; a run that wraps from the last
    pixel of a line to the first of the next; a segment that owns the last pixel; two ids alternating along the scan."""
    H, W = shape
    HW, L = H * W, (W if order == 0 else H)
    background = np.full(HW, -1)
    full = np.full(HW, 1)
    wrap = np.full(HW, -1)
    wrap[max(0, L - 1):min(HW, L + 1)] = 0
    last = np.full(HW, -1)
    last[-1] = 2
    board = np.arange(HW) % 2
    m = np.stack([_from_flat(f, shape, order) for f in (background, full, wrap, last, board)]).astype(np.int64)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _blob_maps(shape):
    """(3, H, W) int64 random blobs over -1, a different number of segments per image (2, 5 and 9 of N = 9)."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    out = np.full((3, H, W), -1, np.int64)
    for b, n in enumerate((2, 5, 9)):
        for k in range(n):
            for _ in range(2):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                out[b, y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, W + 1))] = k
        noise = rng.random((H, W)) < 0.03
        out[b][noise] = rng.integers(-1, n, int(noise.sum()))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, order, shift):
    """The restatement's CSR of the hand maps or the blobs; shift = 1 is the uint8 form (every id one higher, N too)."""
    maps, N = (_hand_maps(shape, order), N_SMALL) if kind == "hand" else (_blob_maps(shape), 9)
    return R.csr(maps + shift, N + shift, order)


def _device_maps(maps, dtype):
    """ids in [-1, N) as fp32 / int32; uint8 holds no -1, so there every id is one higher (and N with it)."""
    shift = 1 if dtype == torch.uint8 else 0
    return torch.from_numpy(maps + shift).to(dtype).to(DEV), shift


def _check(t, N, order, ref):
    from weed_instance_segmentation_amd import ops
    counts, positions, offsets = ops.labelmap_toggles(t, N, order)
    rc, rp, ro = ref
    assert positions.dtype == torch.int32 and positions.is_cuda and positions.shape == (int(ro[-1]),)
    assert np.array_equal(counts, rc) and np.array_equal(offsets, ro)
    assert np.array_equal(positions.cpu().numpy(), rp)
    c2, bad = ops.labelmap_toggle_counts(t, N, order)
    assert c2.dtype == torch.int32 and np.array_equal(c2.cpu().numpy(), rc) and bad.cpu().tolist() == [0] * t.shape[0]
    return counts


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES)
def test_hand_maps_equal_the_restatement(shape, order, dtype):
    t, shift = _device_maps(_hand_maps(shape, order), dtype)
    counts = _check(t, N_SMALL + shift, order, _reference("hand", shape, order, shift))
    HW = shape[0] * shape[1]
    s = shift  # slot of id -1 (of id 0 for uint8, which has no slot-0 pixel)
    assert counts[0].tolist() == [0] * s + [2, 0, 0, 0]  # all background: toggles [0, HW] of one slot
    assert counts[1, s + 2] == 2 and counts[1].sum() == 2  # one segment that fills the map
    # every position toggles both ids, the two ends one: 2 HW in all, and HW + 1 -- the most a segment can have -- for the
    # id that owns both ends of an odd-sized map
    assert counts[4, s + 1] == HW + HW % 2 and counts[4, s + 1] + counts[4, s + 2] == 2 * HW


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES)
def test_blobs_equal_the_restatement(shape, order, dtype):
    t, shift = _device_maps(_blob_maps(shape), dtype)
    _check(t, 9 + shift, order, _reference("blob", shape, order, shift))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES)
def test_ids_at_the_cap_and_a_value_beyond(shape, order, dtype):
    from weed_instance_segmentation_amd import _lib, ops
    N = 256 if dtype == torch.uint8 else _lib.WM2F_RLE_MAX_IDS
    lo = 0 if dtype == torch.uint8 else -1
    rng = np.random.default_rng(shape[0])
    m = rng.choice([lo, N - 1], size=(1,) + shape)  # the lowest and the highest id of [-1, N)
    m[0, -1, -1] = N - 1
    t = torch.from_numpy(m).to(dtype).to(DEV)
    _check(t, N, order, R.csr(m, N, order))
    # N - 1 is outside [-1, N - 1): the count launch reports it, the host layer raises
    _, bad = ops.labelmap_toggle_counts(t, N - 1, order)
    assert bad.cpu().tolist() == [int((m == N - 1).sum())] == [R.toggle_lists(m[0], N - 1, order)[1]]
    with pytest.raises(ValueError, match="outside"):
        ops.labelmap_toggles(t, N - 1, order)
    with pytest.raises(ValueError):
        ops.labelmap_toggles(t, _lib.WM2F_RLE_MAX_IDS + 1, order)


def test_float_values_that_are_no_id_are_out_of_range():
    from weed_instance_segmentation_amd import ops
    m = torch.tensor([[[-1.0, 0.0, 1.5], [2.0, float("nan"), -2.0]]], device=DEV)
    _, bad = ops.labelmap_toggle_counts(m, 3, 0)
    assert bad.cpu().tolist() == [3]


@pytest.mark.parametrize("order", ORDERS)
def test_two_encodes_are_bit_identical(order):
    from weed_instance_segmentation_amd import ops
    t, _ = _device_maps(_blob_maps((97, 131)), torch.float32)
    a, b = ops.labelmap_toggles(t, 9, order), ops.labelmap_toggles(t, 9, order)
    assert torch.equal(a[1], b[1]) and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("shape", [(3, 5), (97, 131)])
def test_coco_and_hf_encodings(shape):
    from weed_instance_segmentation_amd import encode_label_maps, rle_from_string
    from weed_instance_segmentation_amd.postprocess import convert_segmentation_to_rle
    maps = _blob_maps(shape).copy()
    maps[0, -1, -1] = 1  # id 1 owns the last pixel of image 0
    t = torch.from_numpy(maps).float().to(DEV)
    plain = encode_label_maps(t, n=9, format="coco", compressed=False)
    packed = encode_label_maps(t, n=9, format="coco")
    hf = encode_label_maps(t, n=9, format="hf")
    for b in range(3):
        ids = np.unique(maps[b]).tolist()
        assert list(plain[b]) == list(packed[b]) == list(hf[b]) == ids  # only ids with a pixel, ascending
        for k in ids:
            c = R.coco_counts(maps[b] == k)
            assert plain[b][k] == {"size": list(shape), "counts": c}
            assert packed[b][k]["counts"] == R.to_string(c) and rle_from_string(packed[b][k]["counts"]) == c
        assert list(hf[b].values()) == convert_segmentation_to_rle(t[b])
    assert len(plain[0][1]["counts"]) % 2 == 0 and plain[0][1]["counts"][-1] > 0  # no trailing 0-run
    one = encode_label_maps(t[1], format="hf")  # one map, n from the map
    assert one == hf[1]


@pytest.mark.parametrize("fmt", ["coco", "hf"])
def test_round_trip_on_the_device(fmt):
    from weed_instance_segmentation_amd import decode_rle, encode_label_maps
    t, _ = _device_maps(_blob_maps((97, 131)), torch.float32)
    back = decode_rle(encode_label_maps(t, n=9, format=fmt), size=(97, 131), format=fmt)
    assert back.dtype == torch.int32 and back.is_cuda and torch.equal(back, t.to(torch.int32))
    one = decode_rle(encode_label_maps(t[2], n=9, format=fmt), size=(97, 131), format=fmt, background=-1)
    assert torch.equal(one, t[2].to(torch.int32))
    if fmt == "coco":  # the size comes with the RLEs; chosen values; masks (H * W % 4 == 0)
        q = t[:, :96, :].contiguous()
        rles = encode_label_maps(q[0], n=9)
        vals = {k: 10 * (k + 1) for k in rles}
        assert torch.equal(decode_rle(rles, values=vals), (10 * (q[0] + 1)).to(torch.int32))
        masks = decode_rle(rles, as_masks=True)
        assert masks.dtype == torch.uint8 and torch.equal(masks.bool(), torch.stack([q[0] == k for k in rles]))


@pytest.mark.parametrize("order", ORDERS)
def test_paint_follows_painters_order(order):
    from weed_instance_segmentation_amd import ops
    B, H, W = 2, 9, 70
    HW = H * W
    rng = np.random.default_rng(order)
    runs = [(0, 0, HW, 5), (0, 3, 200, 6), (0, 100, 150, 7), (1, HW - 1, 1, 8), (1, 10, 0, 9), (0, 120, 3, 6)]
    for _ in range(24):  # overlapping runs, many of them across line ends
        s = int(rng.integers(0, HW))
        runs.append((int(rng.integers(0, B)), s, int(rng.integers(0, min(HW - s, 90) + 1)), int(rng.integers(0, 50))))
    base = rng.integers(-3, 0, (B, H, W)).astype(np.int32)
    out = torch.from_numpy(base).to(DEV)
    same = ops.rle_paint_(out, torch.tensor(runs, dtype=torch.int32, device=DEV), order)
    assert same is out and np.array_equal(out.cpu().numpy(), R.paint(base, runs, order))
    assert (out[1] < 0).any()  # uncovered pixels keep their value


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("bad", [(0, 62, 2, 4), (0, -1, 2, 4), (0, 0, -1, 4), (1, 0, 1, 4), (0, 2 ** 31 - 1, 2 ** 31 - 1, 4)])
def test_paint_refuses_a_run_outside_its_image(order, bad):
    """rle_check_kernel compares every run with H * W before anything is stored, and the two kernels that store return
    at once when it found one: (0, 62, 2) ends one past the 7 x 9 map and must leave the map as it was, together with
    the good runs of the same call."""
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    out = torch.full((1, 7, 9), -1, dtype=torch.int32, device=DEV)
    runs = torch.tensor([(0, 0, 10, 1), bad, (0, 20, 5, 2)], dtype=torch.int32, device=DEV)
    with pytest.raises(Wm2fError, match="run 1"):
        ops.rle_paint_(out, runs, order)
    assert (out == -1).all()
    ops.rle_paint_(out, runs[[0, 2]].contiguous(), order)  # the good runs alone paint
    assert int((out == 1).sum()) == 10 and int((out == 2).sum()) == 5


def test_rle_to_instance_map():
    from weed_instance_segmentation_amd.annotations import rle_to_instance_map
    m = np.zeros((6, 8), bool)
    m[1:4, 2:5] = True
    m2 = np.zeros((6, 8), bool)
    m2[3:6, 4:8] = True
    rles = [{"size": [6, 8], "counts": R.to_string(R.coco_counts(m))}, {"size": [6, 8], "counts": R.coco_counts(m2)}]
    got = rle_to_instance_map(rles, [1, 256], (6, 8))
    want = np.full((6, 8), 255, np.int32)
    want[m] = 1
    want[m2] = 256  # the later one wins the overlap
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError):
        rle_to_instance_map(rles, [1, 2], (6, 9))


# ------------------------------------------------------------------------------------------------ the post-processor
def _outputs():
    g = load_golden("postprocess_instances.npz")
    T = torch.from_numpy
    return SimpleNamespace(class_queries_logits=T(g["class_logits"]).to(DEV), masks_queries_logits=T(g["mask_logits"]).to(DEV))


SIZES = [[50, 70], [33, 47], [50, 70]]  # two target sizes in one batch


def test_return_coco_annotation_equals_the_per_image_route():
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor, convert_segmentation_to_rle
    p = Mask2FormerInstancePostProcessor()
    rle = p.post_process_instance_segmentation(_outputs(), threshold=0.5, target_sizes=SIZES, return_coco_annotation=True)
    maps = p.post_process_instance_segmentation(_outputs(), threshold=0.5, target_sizes=SIZES)
    assert len(rle) == 3
    for a, b in zip(rle, maps):
        assert a["segments_info"] == b["segments_info"]
        assert a["segmentation"] == convert_segmentation_to_rle(b["segmentation"])
        assert all(type(v) is int for l in a["segmentation"] for v in l)


def test_coco_results_of_the_post_processor(tmp_path):
    from weed_instance_segmentation_amd import coco_results, instance_statistics, rle_from_string, save_coco_results
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    res = Mask2FormerInstancePostProcessor().post_process_instance_segmentation(
        _outputs(), threshold=0.5, target_sizes=SIZES, return_instance_stats=True)
    names = ["a.png", "b.png", "c.png"]
    entries = coco_results(res, names, category_of={k: k + 1 for k in range(4)})
    assert entries and json.loads(json.dumps(entries)) == entries
    seen = 0
    for i, r in enumerate(res):
        n = len(r["segments_info"])
        if n == 0:
            continue
        area, bbox, _ = instance_statistics(r["segmentation"], n=n)
        mine = [e for e in entries if e["image_id"] == names[i]]
        live = [s for s in r["segments_info"] if s["area"] > 0]
        assert len(mine) == len(live)
        for e, s in zip(mine, live):
            counts = rle_from_string(e["segmentation"]["counts"])
            assert e["segmentation"]["size"] == SIZES[i] and sum(counts) == SIZES[i][0] * SIZES[i][1]
            assert e["area"] == sum(counts[1::2]) == int(area[s["id"]])
            assert e["bbox"] == bbox[s["id"]].tolist()
            assert e["category_id"] == s["label_id"] + 1 and e["score"] == s["score"]
            mask = R.decode_coco(counts, *SIZES[i])
            assert np.array_equal(mask, (r["segmentation"] == s["id"]).cpu().numpy())
            seen += 1
    assert seen
    path = tmp_path / "results.json"
    assert save_coco_results(str(path), res, names, category_of={k: k + 1 for k in range(4)}) == entries
    assert json.loads(path.read_text()) == entries
