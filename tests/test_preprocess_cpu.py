"""Host half of the device preprocessing (weed_instance_segmentation_amd/preprocess.py): Pillow's tap
and index tables, the output-size rule, the normalisation table, configuration files, and the refusals.  `restate` is
a vectorised numpy restatement of the whole contract; it is checked here against the dependency's fixture and used by
tests/test_preprocess_gpu.py as the reference at full size."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from weed_instance_segmentation_amd import preprocess as P
from weed_instance_segmentation_amd.preprocess import Mask2FormerImageProcessor


def _apply_bilinear(a: np.ndarray, bounds: np.ndarray, coef: np.ndarray, axis: int) -> np.ndarray:
    """One Pillow 8-bit pass along `axis` of a uint8 array: clip8((2^21 + sum coef * u8) >> 22)."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    k = coef.shape[1]
    taps = np.arange(k)[None, :]
    valid = taps < bounds[:, 1:2]
    idx = np.where(valid, bounds[:, 0:1] + taps, 0)
    c = np.where(valid, coef, 0).astype(np.int64)
    s = (1 << (P.PRECISION_BITS - 1)) + np.einsum("nk,nk...->n...", c, a[idx])
    return np.moveaxis(np.clip(s >> P.PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def restate(images, maps=None, id2sem=None, **kw):
    """The contract of DESIGN section 12 in numpy: (pixel_values, pixel_mask, [mask_labels], [class_labels])."""
    proc = Mask2FormerImageProcessor(**{k: v for k, v in kw.items() if k != "pad_size"})
    s = {k: getattr(proc, k) for k in P._SETTINGS}
    s["pad_size"] = kw.get("pad_size")
    sizes = [P.output_size(im.shape[0], im.shape[1], s["size"], s["size_divisor"]) for im in images]
    Hp, Wp = (s["pad_size"]["height"], s["pad_size"]["width"]) if s["pad_size"] else (max(h for h, _ in sizes),
                                                                                       max(w for _, w in sizes))
    lut = P.normalize_table(s["do_rescale"], s["rescale_factor"], s["do_normalize"], s["image_mean"], s["image_std"])
    B = len(images)
    pv = np.zeros((B, 3, Hp, Wp), np.float32)
    pm = np.zeros((B, Hp, Wp), np.int64)
    ml, cl = [], []
    for b, (im, (h, w)) in enumerate(zip(images, sizes)):
        H, W = im.shape[:2]
        r = _apply_bilinear(_apply_bilinear(im, *P.bilinear_tables(W, w), 1), *P.bilinear_tables(H, h), 0)
        pv[b, :, :h, :w] = lut[np.arange(3)[:, None, None], r.transpose(2, 0, 1)]
        pm[b, :h, :w] = 1
        if maps is None:
            continue
        m = maps[b]
        if s["do_reduce_labels"]:
            m = np.where(m == 0, s["ignore_index"], m.astype(np.int64) - 1).astype(np.uint8)
        m = m[P.nearest_table(H, h)][:, P.nearest_table(W, w)]
        ids = np.unique(m)
        if s["ignore_index"] is not None:
            ids = ids[ids != s["ignore_index"]]
        masks = np.full((len(ids), Hp, Wp), s["ignore_index"] if s["ignore_index"] is not None else 0, np.float32)
        masks[:, :h, :w] = m[None] == ids[:, None, None]
        ml.append(masks)
        d = id2sem[b] if isinstance(id2sem, list) else id2sem
        if d is None:
            cl.append(ids.astype(np.int64))
        elif s["do_reduce_labels"]:
            cl.append(np.array([d[int(i) + 1] - 1 for i in ids], np.int64))
        else:
            cl.append(np.array([d[int(i)] for i in ids], np.int64))
    return pv, pm, ml, cl


def fixture_cases():
    g = load_golden("preprocess_pil.npz")
    out = []
    for name in json.loads(str(g["cases"])):
        ims = [g[k] for k in sorted(k for k in g if k.startswith(name + ".img"))]
        maps = [g[f"{name}.map{b}"] for b in range(len(ims))] if f"{name}.map0" in g else None
        id2sem = json.loads(str(g[f"{name}.id2sem"]))
        if id2sem is not None:
            id2sem = [{int(k): v for k, v in d.items()} for d in id2sem]
        exp = {"pixel_values": g[f"{name}.pixel_values"], "pixel_mask": g[f"{name}.pixel_mask"]}
        if maps is not None:
            exp["mask_labels"] = [g[f"{name}.mask_labels{b}"] for b in range(len(ims))]
            exp["class_labels"] = [g[f"{name}.class_labels{b}"] for b in range(len(ims))]
        out.append((name, ims, maps, id2sem, json.loads(str(g[f"{name}.kwargs"])), exp))
    return out


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_restatement_equals_the_dependency_fixture(case):
    name, ims, maps, id2sem, kw, exp = case
    pv, pm, ml, cl = restate(ims, maps, id2sem, **kw)
    assert np.array_equal(pv, exp["pixel_values"]) and pv.dtype == exp["pixel_values"].dtype
    assert np.array_equal(pm, exp["pixel_mask"])
    if maps is not None:
        for b in range(len(ims)):
            assert ml[b].shape == exp["mask_labels"][b].shape
            assert np.array_equal(ml[b], exp["mask_labels"][b])
            assert np.array_equal(cl[b], exp["class_labels"][b])


def test_fixture_covers_a_lost_id_and_an_empty_map():
    g = load_golden("preprocess_pil.npz")
    assert 7 in g["downscale_3x_lost_id.map0"] and 7 not in g["downscale_3x_lost_id.class_labels0"]
    assert g["empty_instances.mask_labels0"].shape[0] == 0


@pytest.mark.parametrize("resample", ["BILINEAR", "NEAREST"])
def test_tables_equal_pillow_resize(resample):
    """Every table against Pillow's own resize, one axis at a time, sizes 1 to 1500 (up, down and unchanged)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    for _ in range(60):
        n_in, n_out = (int(v) for v in rng.integers(1, 1501, 2))
        if rng.random() < 0.1:
            n_out = n_in
        if resample == "BILINEAR":
            a = rng.integers(0, 256, (3, n_in, 3), dtype=np.uint8)
            ref = np.asarray(Image.fromarray(a).resize((n_out, 3), Image.Resampling.BILINEAR))
            assert np.array_equal(_apply_bilinear(a, *P.bilinear_tables(n_in, n_out), 1), ref), (n_in, n_out)
            a = rng.integers(0, 256, (n_in, 2, 3), dtype=np.uint8)
            ref = np.asarray(Image.fromarray(a).resize((2, n_out), Image.Resampling.BILINEAR))
            assert np.array_equal(_apply_bilinear(a, *P.bilinear_tables(n_in, n_out), 0), ref), (n_in, n_out)
        else:
            m = rng.integers(0, 256, (n_in, 5), dtype=np.uint8)
            ref = np.asarray(Image.fromarray(m).resize((5, n_out), Image.Resampling.NEAREST))
            assert np.array_equal(m[P.nearest_table(n_in, n_out)], ref), (n_in, n_out)
            ref = np.asarray(Image.fromarray(m.T.copy()).resize((n_out, 5), Image.Resampling.NEAREST))
            assert np.array_equal(m.T[:, P.nearest_table(n_in, n_out)], ref), (n_in, n_out)


def test_two_pass_bilinear_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(12)
    for H, W, h, w in [(768, 1024, 800, 1088), (1024, 1024, 1024, 1024), (4000, 3000, 1088, 800), (37, 53, 96, 128)]:
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(a).resize((w, h), Image.Resampling.BILINEAR))
        r = _apply_bilinear(_apply_bilinear(a, *P.bilinear_tables(W, w), 1), *P.bilinear_tables(H, h), 0)
        assert np.array_equal(r, ref), (H, W, h, w)


def test_output_size_equals_the_dependency():
    tt = pytest.importorskip("transformers.image_transforms")
    iu = pytest.importorskip("transformers.image_utils")
    rng = np.random.default_rng(13)
    for _ in range(300):
        H, W = (int(v) for v in rng.integers(1, 5000, 2))
        se, le = int(rng.integers(16, 1200)), int(rng.integers(16, 2000))
        d = int(rng.choice([0, 1, 32]))
        exp = tt.get_size_with_aspect_ratio((H, W), se, le)
        if d:
            exp = tuple(int(np.ceil(v / d) * d) for v in exp)
        assert P.output_size(H, W, {"shortest_edge": se, "longest_edge": le}, d) == exp
        mh, mw = int(rng.integers(8, 2000)), int(rng.integers(8, 2000))
        assert P.output_size(H, W, {"max_height": mh, "max_width": mw}, 0) == \
            iu.get_image_size_for_max_height_width((H, W), mh, mw)
    with pytest.raises(ValueError):
        P.output_size(10, 10, {"shortest_edge": 8}, 32)


def test_normalize_table_equals_the_dependency():
    tt = pytest.importorskip("transformers.image_transforms")
    from transformers.image_utils import ChannelDimension
    x = np.tile(np.arange(256, dtype=np.uint8), (3, 1))[:, :, None]  # (3, 256, 1) channel-first
    r = tt.rescale(x, 1 / 255, data_format=ChannelDimension.FIRST, input_data_format=ChannelDimension.FIRST)
    r = tt.normalize(r, P.IMAGENET_DEFAULT_MEAN, P.IMAGENET_DEFAULT_STD, data_format=ChannelDimension.FIRST,
                     input_data_format=ChannelDimension.FIRST)
    assert np.array_equal(P.normalize_table(True, 1 / 255, True, P.IMAGENET_DEFAULT_MEAN, P.IMAGENET_DEFAULT_STD),
                          r[:, :, 0])


def _settings(p):
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in
            [("size", p.size), ("size_divisor", p.size_divisor), ("image_mean", list(p.image_mean)),
             ("image_std", list(p.image_std)), ("ignore_index", p.ignore_index), ("do_reduce_labels", p.do_reduce_labels),
             ("rescale_factor", p.rescale_factor), ("do_resize", p.do_resize), ("do_normalize", p.do_normalize),
             ("do_rescale", p.do_rescale), ("resample", int(p.resample))]}


def test_config_round_trips_with_the_dependency(tmp_path):
    pil = pytest.importorskip("transformers.models.mask2former.image_processing_pil_mask2former")
    ours = Mask2FormerImageProcessor(size={"shortest_edge": 640, "longest_edge": 1024}, ignore_index=255,
                                     do_reduce_labels=True, image_mean=[0.5, 0.4, 0.3], size_divisor=16)
    ours.save_pretrained(str(tmp_path / "a"))
    theirs = pil.Mask2FormerImageProcessorPil.from_pretrained(str(tmp_path / "a"))
    assert _settings(theirs) == _settings(ours)
    theirs2 = pil.Mask2FormerImageProcessorPil(size={"height": 512, "width": 768}, ignore_index=0)
    theirs2.save_pretrained(str(tmp_path / "b"))
    assert _settings(Mask2FormerImageProcessor.from_pretrained(str(tmp_path / "b"))) == _settings(theirs2)
    assert _settings(Mask2FormerImageProcessor()) == _settings(pil.Mask2FormerImageProcessorPil())


def test_legacy_keys(tmp_path):
    d = tmp_path / "legacy"
    d.mkdir()
    (d / "preprocessor_config.json").write_text(json.dumps(
        {"size": 512, "max_size": 900, "size_divisibility": 64, "reduce_labels": True, "ignore_index": 255,
         "image_processor_type": "MaskFormerImageProcessor"}))
    p = Mask2FormerImageProcessor.from_pretrained(str(d))
    assert p.size == {"shortest_edge": 512, "longest_edge": 900}
    assert p.size_divisor == 64 and p.do_reduce_labels is True


def test_hub_name_raises_file_not_found():
    with pytest.raises(FileNotFoundError):
        Mask2FormerImageProcessor.from_pretrained("facebook/mask2former-swin-large-coco-instance")


def test_cpu_device_raises():
    from weed_instance_segmentation_amd._lib import Wm2fError
    with pytest.raises(Wm2fError):
        Mask2FormerImageProcessor()(images=np.zeros((8, 8, 3), np.uint8), device="cpu")


@pytest.mark.parametrize("bad", [np.zeros((8, 8, 3), np.float32), np.zeros((3, 8, 8), np.uint8), np.zeros((8, 8), np.uint8),
                                 torch.zeros(8, 8, 3), "image.png", [[1, 2, 3]]])
def test_unsupported_images_raise_value_error(bad):
    with pytest.raises(ValueError, match="uint8"):
        Mask2FormerImageProcessor()(images=bad)


def test_ids_above_255_raise_value_error():
    with pytest.raises(ValueError, match="outside the range"):
        Mask2FormerImageProcessor()(images=np.zeros((8, 8, 3), np.uint8), segmentation_maps=np.full((8, 8), 300))


def test_only_bilinear_images():
    with pytest.raises(NotImplementedError):
        Mask2FormerImageProcessor(resample=0)


def test_plain_rows_are_the_identity_window_rows_in_the_plain_layout():
    """The processor builds one set of rows (16 and 12 columns, the identity window for a call without `augment`) and
    hands the plain kernels their (B, 12) / (B, 7) layout through `_plain_rows`.  The expected rows are written out
    here column by column, table offsets in the order the tables are laid out and workspace offsets as a running sum."""
    sizes_in = [(37, 150), (700, 520), (64, 48)]   # an upscale, a heavy downscale, an unchanged size
    frames = [(61, 391), (40, 150), (64, 48)]
    plain, lplain, n_tab, ws_off, in_off = [], [], 0, 0, 0
    for (H, W), (h, w) in zip(sizes_in, frames):
        (bx, cx), (by, cy) = P.bilinear_tables(W, w), P.bilinear_tables(H, h)
        sizes = [bx.size, cx.size, by.size, cy.size, w, h]
        tx, ox, ty, oy, xi, yi = (n_tab + int(v) for v in np.cumsum([0] + sizes[:-1]))
        n_tab += sum(sizes)
        plain.append([in_off * 3, ws_off, H, W, h, w, tx, ox, cx.shape[1], ty, oy, cy.shape[1]])
        lplain.append([in_off, H, W, h, w, xi, yi])
        ws_off += H * w * 3
        in_off += H * W
    desc, ldesc, tables = P._descriptors(sizes_in, frames, [[0, 0, 0, h, w] for h, w in frames], True)
    assert tables.dtype == np.int32 and tables.size == n_tab
    assert desc.shape == (3, 16) and ldesc.shape == (3, 12)
    for d in (desc, ldesc):
        assert np.array_equal(d[:, -5:], [[0, 0, 0, h, w] for h, w in frames])
    desc[:, 0] = [r[0] for r in plain]
    ldesc[:, 0] = [r[0] for r in lplain]
    got, lgot = P._plain_rows(desc, ldesc)
    assert got.dtype == np.int64 and np.array_equal(got, plain)
    assert lgot.dtype == np.int64 and np.array_equal(lgot, lplain)


def test_package_exports_the_processor():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor
    assert pkg.Mask2FormerImageProcessor is Mask2FormerImageProcessor
    assert issubclass(Mask2FormerImageProcessor, Mask2FormerInstancePostProcessor)
    assert not os.path.exists(os.path.join(os.path.dirname(pkg.__file__), "transformers"))
