"""Colour jitter on the GPU: csrc/photometric.hip through `adjust_colors`, `ops.photometric_u8`, the
processor and a dataset, byte for byte against the Pillow fixture, the numpy restatement (tests/photometric_reference.py)
and Pillow run here.  Every comparison is torch.equal.  Needs an MI355X (-m gpu)."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import photometric_reference as R
from test_photometric_cpu import all_colours, contrast_positions, golden_cases
from weed_instance_segmentation_amd import _lib
from weed_instance_segmentation_amd.augment import AugmentParams, PhotometricParams, TrainAugmentation, adjust_colors

pytestmark = pytest.mark.gpu
B, C, S, H = R.KINDS
IG = 255
FOUR = ((S, 1.2), (C, 0.6), (H, -0.2), (B, 1.1))


@pytest.fixture(scope="module")
def proc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from weed_instance_segmentation_amd import Mask2FormerImageProcessor
    return Mask2FormerImageProcessor()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(im, ops):
    return adjust_colors(T(im), PhotometricParams(ops))


# ------------------------------------------------------------------------------------------------ fixture, sizes, batches
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_pillow_fixture(proc, case):
    """1 x 1, 1 x 5, 5 x 7, 64 x 64 and odd widths are among the cases; `batch_mixed` is three images of different odd
    sizes, one chain empty and one without contrast, so the sum launch covers one image of three."""
    outs = adjust_colors([T(im) for im in case["images"]], [PhotometricParams(ops) for ops in case["chains"]])
    assert len(outs) == len(case["outs"])
    for got, want, im, ops in zip(outs, case["outs"], case["images"], case["chains"]):
        assert got.dtype == torch.uint8 and got.shape == want.shape and got.is_cuda
        assert torch.equal(got, T(want))
        if not ops:
            assert torch.equal(got, T(im)), "an empty chain leaves the image untouched"


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (5, 7), (33, 130), (64, 64)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_sizes_against_the_restatement(proc, hw):
    im = np.random.default_rng(hw[0] * 1000 + hw[1]).integers(0, 256, (*hw, 3), dtype=np.uint8)
    for ops in [FOUR, ((C, 1.7),), ((H, 0.3), (S, 0.85)), ((B, 0.8), (C, 1.2), (S, 1.6))]:
        assert torch.equal(_run(im, ops), T(R.apply(im, ops))), ops


def test_batch_with_every_misalignment(proc):
    """Packed one behind the other, the images start at byte offsets 0, 3, 0, 1, 2 (mod 4); heads of 0 to 3 pixels and
    tails of 0 to 3; chains differ, one is empty, two have no contrast.  Host inputs (numpy) take the copy route."""
    sizes = [(1, 1), (1, 3), (5, 7), (3, 5), (9, 11), (33, 37)]
    assert [o % 4 for o in np.cumsum([0] + [h * w * 3 for h, w in sizes])[:-1]] == [0, 3, 0, 1, 2, 3]
    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    chains = [FOUR, ((C, 0.6),), (), ((H, 0.1), (C, 1.1), (B, 1.2)), ((S, 1.7), (B, 0.85)), ((H, -0.4),)]
    outs = adjust_colors(ims, [PhotometricParams(c) for c in chains])
    for got, im, ops in zip(outs, ims, chains):
        assert torch.equal(got, T(R.apply(im, ops))), ops
    again = adjust_colors(ims, [PhotometricParams(c) for c in chains])
    assert all(torch.equal(a, b) for a, b in zip(outs, again))


def test_inputs_are_never_written_and_one_params_serves_all(proc):
    rng = np.random.default_rng(6)
    ims = [T(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in [(7, 5), (4, 9)]]
    keep = [t.clone() for t in ims]
    outs = adjust_colors(ims, PhotometricParams(FOUR))
    for got, t, k in zip(outs, ims, keep):
        assert torch.equal(t, k) and got.data_ptr() != t.data_ptr()
        assert torch.equal(got, T(R.apply(k.cpu().numpy(), FOUR)))
    one = adjust_colors(Image.fromarray(keep[0].cpu().numpy()), PhotometricParams(FOUR))  # a PIL image, one result
    assert isinstance(one, torch.Tensor) and torch.equal(one, outs[0])


# ------------------------------------------------------------------------------------------------ the unfused blend
def saturation_grid() -> np.ndarray:
    """(256, 512, 3): at row d, column v a colour with one channel = v and the other two chosen so that L is d or as near
    as the colour cube allows: blue = v in the left half (weight 7471), red = v in the right half (weight 19595)."""
    d, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    left = np.clip(np.rint((d * 65536 - 7471 * v) / (19595 + 38470)), 0, 255)
    right = np.clip(np.rint((d * 65536 - 19595 * v) / (38470 + 7471)), 0, 255)
    return np.concatenate([np.stack([left, left, v], -1), np.stack([v, right, right], -1)], 1).astype(np.uint8)


CONTRAST_MEANS = tuple(range(32, 224, 6))  # 32 means: one batch


def contrast_ramps():
    """32 grey images of 1024 pixels, one per mean d: every grey value once, and 768 filler pixels (255s, one remainder,
    0s) that bring the sum of L to exactly 1024 d.  Contrast then blends every v with d."""
    out = []
    for d in CONTRAST_MEANS:
        fill = 1024 * d - 255 * 256 // 2
        g = np.concatenate([np.arange(256), np.full(fill // 255, 255), [fill % 255], np.zeros(767 - fill // 255)])
        assert g.size == 1024 and g.sum() == 1024 * d
        out.append(np.repeat(g.astype(np.uint8)[:, None], 3, 1).reshape(32, 32, 3))
    return out


@pytest.mark.parametrize("f", R.DISCRIMINATING, ids=lambda f: f"{f:.4g}")
def test_blend_is_not_fused(proc, f):
    """The (d, v) grid as images, per enhancer, at the factors where a fused multiply-add gives other bytes.  A build that
    lets the compiler contract a * (v - d) + d fails here.  Each input is first shown to tell the two apart."""
    grid_v = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (2, 256, 3))  # brightness: d = 0 regardless
    sat = saturation_grid()
    ramps = contrast_ramps()
    assert [R.contrast_mean(r) for r in ramps] == list(CONTRAST_MEANS)
    want_b, want_s = R.brightness(grid_v, f), R.saturation(sat, f)
    want_c = [R.contrast(r, f) for r in ramps]
    fused_s = R.saturation(sat, f, fused=True)
    fused_c = [R.contrast(r, f, fused=True) for r in ramps]
    assert not np.array_equal(want_s, fused_s), "the saturation grid must tell a fused blend apart"
    assert any(not np.array_equal(a, b) for a, b in zip(want_c, fused_c)), "the ramps must tell a fused blend apart"
    got_b, got_s = _run(grid_v, ((B, f),)), _run(sat, ((S, f),))
    got_c = adjust_colors(ramps, PhotometricParams(((C, f),)))
    assert torch.equal(got_s, T(want_s)) and not torch.equal(got_s, T(fused_s))
    assert all(torch.equal(g, T(w)) for g, w in zip(got_c, want_c))
    assert torch.equal(got_b, T(want_b))  # with d = 0 the sum is exact, so brightness cannot tell the two apart


def test_blend_at_plain_factors(proc):
    sat = saturation_grid()
    for f in (0.0, 1.0, 0.5, 2.0):
        assert torch.equal(_run(sat, ((S, f),)), T(R.saturation(sat, f))), f
        assert torch.equal(_run(sat, ((B, f), (C, f))), T(R.apply(sat, ((B, f), (C, f))))), f
    assert torch.equal(_run(sat, ((B, 1.0), (S, 1.0), (C, 1.0))), T(sat)), "factor 1 is the identity"


# ------------------------------------------------------------------------------------------------ all 2^24 colours
@pytest.fixture(scope="module")
def colours():
    return all_colours()


def test_all_colours_through_a_hue_step_against_pillow(proc, colours):
    got = _run(colours, ((H, -0.03),))
    h, s, v = Image.fromarray(colours).convert("HSV").split()
    dh = R.hue_dh(-0.03)
    want = np.asarray(Image.merge("HSV", (h.point(lambda x: (x + dh) % 256), s, v)).convert("RGB"))
    assert torch.equal(got, T(want))
    zero = _run(colours, ((H, 0.0),))
    assert torch.equal(zero, T(np.asarray(Image.fromarray(colours).convert("HSV").convert("RGB"))))
    assert not torch.equal(zero, T(colours)), "dh = 0 is not special-cased"


def test_all_colours_through_a_four_step_chain(proc, colours):
    """48 MB, 4096 blocks' worth of grid-stride work, contrast third: the sum launch runs brightness and hue first."""
    ops = ((B, 1.1), (H, 0.25), (C, 0.8), (S, 1.2))
    assert torch.equal(_run(colours, ops), T(R.apply(colours, ops)))


# ------------------------------------------------------------------------------------------------ contrast
@pytest.mark.parametrize("ops", contrast_positions(), ids=lambda o: "-".join(k[0] for k, _ in o))
def test_contrast_at_each_position_of_a_chain(proc, ops):
    im = np.random.default_rng(17).integers(0, 200, (23, 41, 3), dtype=np.uint8)
    assert torch.equal(_run(im, ops), T(R.apply(im, ops)))
    big = np.random.default_rng(18).integers(0, 256, (301, 517, 3), dtype=np.uint8)  # many workgroups add to one sum
    assert torch.equal(_run(big, ops), T(R.apply(big, ops)))


def test_contrast_mean_rounds_a_half_up(proc):
    im = np.array([[[10, 10, 10], [11, 11, 11]]], dtype=np.uint8)
    assert R.contrast_mean(im) == 11
    assert _run(im, ((C, 0.0),)).cpu().tolist() == [[[11] * 3, [11] * 3]]
    for f in (0.6, 1.7):
        assert torch.equal(_run(im, ((C, f),)), T(R.pil_apply(im, ((C, f),))))


# ------------------------------------------------------------------------------------------------ the C ABI
def _desc(rows):
    return np.array([r + [0] * (_lib.WM2F_PHOTO_DESC_LEN - len(r)) for r in rows], dtype=np.int64)


def _bits(f):
    return int(np.float32(f).view(np.uint32))


def test_raw_descriptor_hue_bytes(proc):
    """dh = 128 cannot come from a shift in [-0.5, 0.5]; the kernel takes every byte."""
    from weed_instance_segmentation_amd import ops
    im = np.random.default_rng(23).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for dh in (0, 1, 127, 128, 255):
        buf = T(im).reshape(-1).clone()
        assert ops.photometric_u8(buf, _desc([[0, 37, 53, 1, 3, dh]])) is buf
        assert torch.equal(buf.view(37, 53, 3), T(R.hue(im, dh))), dh


def test_image_behind_two_gib(proc):
    """Byte offsets are 64-bit: a 5 x 7 image at offset 2^31 + 5 of a buffer that is only allocated, never filled."""
    from weed_instance_segmentation_amd import ops
    im = np.random.default_rng(29).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    off = (1 << 31) + 5
    buf = torch.empty(off + 4096, dtype=torch.uint8, device="cuda")
    buf[off - 8:off + 128] = 7
    buf[off:off + 105] = T(im).reshape(-1)
    ops.photometric_u8(buf, _desc([[off, 5, 7, 2, 1, _bits(1.2), 2, _bits(0.6)]]))
    assert torch.equal(buf[off:off + 105].view(5, 7, 3), T(R.apply(im, ((C, 1.2), (S, 0.6)))))
    assert bool((buf[off - 8:off] == 7).all()) and bool((buf[off + 105:off + 128] == 7).all()), "neighbours untouched"


def test_kernel_rejects_what_it_does_not_build(proc):
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    buf = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device="cuda")
    one = _bits(1.0)
    bad = [("repeated", [[0, 8, 8, 2, 0, one, 0, one]]), ("unknown kind", [[0, 8, 8, 1, 4, one]]),
           ("n_ops", [[0, 8, 8, 5, 0, one]]), ("n_ops", [[0, 8, 8, -1]]),
           ("finite and >= 0", [[0, 8, 8, 1, 0, _bits(-0.5)]]), ("finite and >= 0", [[0, 8, 8, 1, 1, _bits(np.inf)]]),
           ("finite and >= 0", [[0, 8, 8, 1, 2, _bits(np.nan)]]), ("dh", [[0, 8, 8, 1, 3, 256]]),
           ("outside", [[3, 8, 8, 1, 0, one]]), ("outside", [[0, 8, 9, 0]]), ("outside", [[-3, 8, 8, 1, 0, one]]),
           ("bad size", [[0, 0, 8, 1, 0, one]]), ("exceeds", [[0, 1, 16385, 1, 0, one]]),
           ("exceeds", [[0, 1, 1, 0]] * 33)]
    for match, rows in bad:
        with pytest.raises(Wm2fError, match=match):
            ops.photometric_u8(buf, _desc(rows))
    assert not buf.any(), "a refused call writes nothing"
    with pytest.raises(ValueError, match="desc"):
        ops.photometric_u8(buf, np.zeros((1, 11), np.int64))
    with pytest.raises(TypeError):
        ops.photometric_u8(buf.to(torch.int32), _desc([[0, 8, 8, 0]]))
    lib = _lib.load()
    assert lib.wm2f_photometric_workspace(3) == 24 and lib.wm2f_photometric_workspace(0) == -1
    assert lib.wm2f_photometric_workspace(33) == -1


# ------------------------------------------------------------------------------------------------ the processor
GEOMETRY = "composed_with_geometry"  # the fixture's case that also stores the processor's outputs


def _geometry_case():
    c = next(c for c in golden_cases() if c["name"] == GEOMETRY)
    g, n = c["raw"], GEOMETRY
    r = json.loads(str(g[f"{n}.params"]))[0]
    id2sem = [{int(k): v for k, v in d.items()} for d in json.loads(str(g[f"{n}.id2sem"]))]
    return dict(image=c["images"][0], map=g[f"{n}.map0"], id2sem=id2sem, pad=json.loads(str(g[f"{n}.pad_size"])),
                geometry=AugmentParams(r[0], (r[1], r[2]), (r[3], r[4]), (r[5], r[6])),
                params=AugmentParams(r[0], (r[1], r[2]), (r[3], r[4]), (r[5], r[6]), PhotometricParams(c["chains"][0])),
                pixel_values=g[f"{n}.pixel_values"], pixel_mask=g[f"{n}.pixel_mask"],
                mask_labels=g[f"{n}.mask_labels0"], class_labels=g[f"{n}.class_labels0"])


def test_processor_composes_colour_with_geometry(proc):
    c = _geometry_case()
    call = lambda im, p: proc.preprocess([im], [c["map"]], c["id2sem"], augment=[p], pad_size=c["pad"],  # noqa: E731
                                         ignore_index=IG)
    out = call(c["image"], c["params"])
    assert torch.equal(out["pixel_values"], T(c["pixel_values"])) and torch.equal(out["pixel_mask"], T(c["pixel_mask"]))
    assert torch.equal(out["mask_labels"][0], T(c["mask_labels"]))
    assert torch.equal(out["class_labels"][0], T(c["class_labels"]))
    plain = call(c["image"], c["geometry"])
    assert not torch.equal(plain["pixel_values"], out["pixel_values"])
    assert torch.equal(plain["pixel_mask"], out["pixel_mask"])
    assert torch.equal(plain["mask_labels"][0], out["mask_labels"][0])
    assert torch.equal(plain["class_labels"][0], out["class_labels"][0])
    # a device-resident input is bit-identical after the call; two calls give identical bytes
    dev_im = T(c["image"])
    keep = dev_im.clone()
    again = call(dev_im, c["params"])
    assert torch.equal(dev_im, keep)
    assert torch.equal(again["pixel_values"], out["pixel_values"])
    # the colour step alone, then the geometry alone, is the same thing
    two = call(adjust_colors(dev_im, c["params"].photometric), c["geometry"])
    assert torch.equal(two["pixel_values"], out["pixel_values"])
    # an empty chain and photometric=None are the call of section 20
    empty = call(c["image"], AugmentParams(*[getattr(c["geometry"], k) for k in ("flip", "size", "origin", "window")],
                                           PhotometricParams()))
    assert torch.equal(empty["pixel_values"], plain["pixel_values"])


def test_processor_batch_with_and_without_chains(proc):
    """Three images in one call: a chain with contrast, none, a chain without contrast; images only."""
    rng = np.random.default_rng(41)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(33, 37), (17, 91), (45, 23)]]
    chains = [((C, 1.2), (H, 0.1)), None, ((S, 1.6), (B, 0.8))]
    geo = [AugmentParams(1, (40, 44), (3, 2), (32, 32)), AugmentParams(0, (24, 100), (0, 10), (24, 32)),
           AugmentParams(1, (45, 23))]
    with_p = [AugmentParams(g.flip, g.size, g.origin, g.window, None if c is None else PhotometricParams(c))
              for g, c in zip(geo, chains)]
    pad = {"height": 48, "width": 32}
    out = proc.preprocess(ims, augment=with_p, pad_size=pad)
    jittered = [im if c is None else R.apply(im, c) for im, c in zip(ims, chains)]
    want = proc.preprocess(jittered, augment=geo, pad_size=pad)
    assert torch.equal(out["pixel_values"], want["pixel_values"]) and torch.equal(out["pixel_mask"], want["pixel_mask"])


# ------------------------------------------------------------------------------------------------ datasets
def test_pheno_bench_dataset_with_colour_jitter(proc, tmp_path):
    from test_augment_gpu import _pheno_folder
    from weed_instance_segmentation_amd.annotations import PhenoBenchDataset
    img_dir, ann_dir = _pheno_folder(tmp_path)
    kw = dict(scale=(0.5, 2.0), crop_size=(128, 160))
    plain_aug = TrainAugmentation(**kw)
    aug = TrainAugmentation(**kw, brightness=0.3, contrast=0.3, saturation=0.3, hue=0.05)
    gen = lambda s: torch.Generator().manual_seed(s)  # noqa: E731
    plain = PhenoBenchDataset(img_dir, ann_dir, proc, {}, augment=plain_aug)
    ds = PhenoBenchDataset(img_dir, ann_dir, proc, {}, augment=aug)
    for i in range(2):
        plain.generator, ds.generator = gen(3 + i), gen(3 + i)  # the colour draws come after the geometry's
        base, item = plain[i], ds[i]
        p = item["augment"]
        assert p == aug.sample(*item["original_map"].shape, gen(3 + i))
        assert p.photometric is not None and len(p.photometric.ops) == 4
        g = base["augment"]
        assert (p.flip, p.size, p.origin, p.window) == (g.flip, g.size, g.origin, g.window) and g.photometric is None
        assert torch.equal(item["mask_labels"], base["mask_labels"]) and torch.equal(item["class_labels"], base["class_labels"])
        assert not torch.equal(item["pixel_values"], base["pixel_values"])
        image = np.asarray(Image.open(ds.valid_files[i][0]).convert("RGB"))
        again = proc.preprocess([image], augment=[p], pad_size=aug.pad_size)
        assert torch.equal(again["pixel_values"][0], item["pixel_values"])
        pil = proc.preprocess([R.pil_apply(image, p.photometric.ops)], augment=[g], pad_size=aug.pad_size)
        assert torch.equal(pil["pixel_values"][0], item["pixel_values"]), "replayed in Pillow, then the geometry alone"
