"""Orientation augmentation on the GPU: csrc/orient.hip through `rotate_images`, `rotate_maps`,
`ops.orient_u8`, `ops.orient_labels`, the processor and a dataset, byte for byte against the Pillow fixture, the numpy
restatement (tests/rotate_reference.py) and Pillow run here.  Every comparison is torch.equal.  Needs an MI355X (-m gpu).

The CPU search of tests/test_rotate_cpu.py found no input that a fused build would change, so no such case is pinned
here; contraction is switched off by the build."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import rotate_reference as R
from test_rotate_cpu import golden_cases, inputs
from weed_instance_segmentation_amd import _lib
from weed_instance_segmentation_amd.augment import (AugmentParams, PhotometricParams, RotateParams, TrainAugmentation,
                                                    rotate_images, rotate_maps)

pytestmark = pytest.mark.gpu
IG = 255
FILL, MAP_FILL, BIG_FILL = (7, 130, 255), 9, 70001
ANGLES = (1, -7.5, 13.37, 45, 90, 270, 359.9, 30.000001, 89.99, -180.5)


@pytest.fixture(scope="module")
def proc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from weed_instance_segmentation_amd import Mask2FormerImageProcessor
    return Mask2FormerImageProcessor()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def want_image(im, p):
    return T(R.orient_image(im, p.vflip, p.turns, p.angle, p.fill))


def want_map(m, p):
    return T(R.orient_map(m, p.vflip, p.turns, p.angle, p.map_fill))


# ------------------------------------------------------------------------------------------------ fixture and sizes
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_pillow_fixture(proc, case):
    """The eight flip / turn combinations, the angles 1, 13.37, 45, 90 on a non-square and -7.5, odd widths, a batch of
    three sizes, an int32 map with ids above 255: images and maps in one call each."""
    outs = rotate_images(case["images"], case["params"])
    mouts = rotate_maps(case["maps"], case["params"])
    for got, mgot, want, mwant, m in zip(outs, mouts, case["outs"], case["mouts"], case["maps"]):
        assert got.dtype == torch.uint8 and got.is_cuda and got.shape == want.shape
        assert torch.equal(got, T(want))
        assert mgot.dtype == T(m).dtype and mgot.shape == mwant.shape
        assert torch.equal(mgot, T(mwant))


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (5, 7), (33, 130), (64, 64), (257, 31)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_sizes_against_the_restatement(proc, hw):
    """Every named angle, alone and behind a flip and a turn, as one batch per kind of input."""
    im, m8, m32 = inputs(*hw)
    ps = [RotateParams(angle=a, fill=FILL, map_fill=MAP_FILL) for a in ANGLES]
    ps += [RotateParams(bool(k & 1), k % 4, a, FILL, MAP_FILL) for k, a in enumerate(ANGLES)]
    ps += [RotateParams(bool(v), k) for v in (0, 1) for k in range(4)]
    for got, p in zip(rotate_images([im] * len(ps), ps), ps):
        assert torch.equal(got, want_image(im, p)), p
    for got, p in zip(rotate_maps([m8] * len(ps), ps), ps):
        assert torch.equal(got, want_map(m8, p)), p
    big = [RotateParams(p.vflip, p.turns, p.angle, map_fill=BIG_FILL) for p in ps]
    for got, p in zip(rotate_maps([m32] * len(big), big), big):
        assert torch.equal(got, want_map(m32, p)), p


def test_one_input_against_pillow_run_here(proc):
    im, m8, m32 = inputs(47, 61)
    p = RotateParams(True, 3, 13.37, FILL, MAP_FILL)
    assert torch.equal(rotate_images(Image.fromarray(im), p), T(R.pil_orient_image(im, True, 3, 13.37, FILL)))
    assert torch.equal(rotate_maps(m8, p), T(R.pil_orient_map(m8, True, 3, 13.37, MAP_FILL)))
    q = RotateParams(True, 3, 13.37, FILL, BIG_FILL)
    assert torch.equal(rotate_maps(T(m32), q), T(R.pil_orient_map(m32, True, 3, 13.37, BIG_FILL)))


# ------------------------------------------------------------------------------------------------ batches and workgroups
def test_batch_with_every_misalignment(proc):
    """Six images packed one behind the other: their byte offsets cover every residue mod 4 (and so do their rows').  One
    identity entry, one pure flip, one pure turn on a non-square image and three rotations."""
    sizes = [(1, 1), (1, 3), (5, 7), (3, 5), (9, 11), (33, 37)]
    assert sorted({int(o) % 4 for o in np.cumsum([0] + [h * w * 3 for h, w in sizes])[:-1]}) == [0, 1, 2, 3]
    ps = [RotateParams(angle=30.0, fill=FILL), RotateParams(), RotateParams(True), RotateParams(turns=1),
          RotateParams(False, 3, -7.5, FILL, MAP_FILL), RotateParams(True, 0, 45.0, FILL, MAP_FILL)]
    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    ms = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w in sizes]
    outs, mouts = rotate_images(ims, ps), rotate_maps(ms, ps)
    for got, mgot, im, m, p in zip(outs, mouts, ims, ms, ps):
        assert torch.equal(got, want_image(im, p)) and torch.equal(mgot, want_map(m, p)), p
    assert torch.equal(outs[1], T(ims[1])), "nothing enabled: a copy"
    again = rotate_images(ims, ps)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))


def test_many_workgroups_and_partial_tiles(proc):
    """130 x 300: 3 x 5 tiles of 64 x 64, partial in both directions, turned and not."""
    im, m8, m32 = inputs(130, 300)
    ps = [RotateParams(v, k, a, FILL, MAP_FILL) for v, k, a in
          [(False, 0, 13.37), (True, 0, 0.0), (False, 1, 0.0), (False, 2, 0.0), (True, 3, 0.0), (True, 1, -33.0)]]
    for got, p in zip(rotate_images([im] * len(ps), ps), ps):
        assert torch.equal(got, want_image(im, p)), p
    for got, p in zip(rotate_maps([m8] * len(ps), ps), ps):
        assert torch.equal(got, want_map(m8, p)), p
    for got, p in zip(rotate_maps([m32] * len(ps), ps), ps):
        assert torch.equal(got, want_map(m32, p)), p


def test_inputs_are_never_written(proc):
    im, m8, _ = inputs(20, 33)
    t, tm = T(im), T(m8)
    keep, keep_m = t.clone(), tm.clone()
    p = RotateParams(True, 1, 20.0)
    got, mgot = rotate_images(t, p), rotate_maps(tm, p)
    assert torch.equal(t, keep) and torch.equal(tm, keep_m) and got.data_ptr() != t.data_ptr()
    assert torch.equal(got, want_image(im, p)) and torch.equal(mgot, want_map(m8, p))
    with pytest.raises(ValueError, match="params"):
        rotate_images([t, t], [p])
    with pytest.raises(ValueError, match="map_fill"):
        rotate_maps(tm, RotateParams(angle=3.0, map_fill=256))
    with pytest.raises(ValueError, match="uint8 or int32"):
        rotate_maps(tm.to(torch.int64), p)


# ------------------------------------------------------------------------------------------------ rotation edge cases
def test_45_degrees_fills_the_corners_exactly(proc):
    im, m8, _ = inputs(64, 64)
    im[im == 255] = 254  # so that a (255, 255, 255) pixel is fill and nothing else
    m8[m8 == 255] = 254
    p = RotateParams(angle=45.0, fill=(255, 255, 255), map_fill=255)
    got, mgot = rotate_images(im, p), rotate_maps(m8, p)
    want, mwant = R.orient_image(im, angle=45.0, fill=(255, 255, 255)), R.orient_map(m8, angle=45.0, fill=255)
    filled, mfilled = (got == 255).all(-1), mgot == 255
    for y, x in [(0, 0), (0, 63), (63, 0), (63, 63)]:
        assert bool(filled[y, x]) and bool(mfilled[y, x])
    assert torch.equal(filled, T((want == 255).all(-1))) and torch.equal(mfilled, T(mwant == 255))
    assert 0 < int(filled.sum()) < 64 * 64 // 2
    assert torch.equal(got, T(want)) and torch.equal(mgot, T(mwant))


def test_90_degrees_on_a_non_square_lands_on_the_edge(proc):
    """Source coordinates are exact multiples of 0.5 here: x_in = 0 and x_in = W are both hit."""
    im, m8, m32 = inputs(5, 9)
    for a in (90, 270, -90, 450):
        p = RotateParams(angle=a, fill=FILL, map_fill=MAP_FILL)
        assert torch.equal(rotate_images(im, p), T(R.pil_orient_image(im, angle=a, fill=FILL))), a
        assert torch.equal(rotate_maps(m8, p), T(R.pil_orient_map(m8, angle=a, fill=MAP_FILL))), a


# ------------------------------------------------------------------------------------------------ the C ABI
def _row(in_off, H, W, out_off, vflip=0, turns=0, affine=0, m=None, fx=None, fill=(0, 0, 0)):
    m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] if m is None else m
    bits = [int(np.array(v, np.float64).view(np.int64)) for v in m]
    return [in_off, H, W, out_off, vflip, turns, affine, *bits, *([65536, 0, 0, 0, 65536, 0] if fx is None else fx), *fill]


def test_kernel_rejects_what_it_does_not_build(proc):
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    src = torch.zeros(8 * 8 * 3 * 2, dtype=torch.uint8, device="cuda")
    dst = torch.zeros_like(src)
    D = lambda rows: np.array(rows, dtype=np.int64)  # noqa: E731
    bad = [("outside the input", [_row(195, 8, 8, 0)]), ("outside the input", [_row(-3, 8, 8, 0)]),
           ("outside the input", [_row(0, 8, 17, 0)]), ("outside the output", [_row(0, 8, 8, 195)]),
           ("outside the output", [_row(0, 8, 8, -1)]), ("overlap", [_row(0, 8, 8, 0), _row(192, 8, 8, 191)]),
           ("turns", [_row(0, 8, 8, 0, turns=4)]), ("turns", [_row(0, 8, 8, 0, turns=-1)]),
           ("vflip", [_row(0, 8, 8, 0, vflip=2)]), ("affine", [_row(0, 8, 8, 0, affine=2)]),
           ("not finite", [_row(0, 8, 8, 0, affine=1, m=[1.0, 0.0, np.inf, 0.0, 1.0, 0.0])]),
           ("not finite", [_row(0, 8, 8, 0, affine=1, m=[np.nan, 0.0, 0.0, 0.0, 1.0, 0.0])]),
           ("fill byte", [_row(0, 8, 8, 0, fill=(0, 256, 0))]), ("fill byte", [_row(0, 8, 8, 0, fill=(-1, 0, 0))]),
           ("bad size", [_row(0, 0, 8, 0)]), ("exceeds", [_row(0, 1, 16385, 0)]), ("exceeds", [_row(0, 1, 1, 0)] * 33)]
    for match, rows in bad:
        with pytest.raises(Wm2fError, match=match):
            ops.orient_u8(src, dst, D(rows))
    with pytest.raises(Wm2fError, match="overlap"):
        ops.orient_u8(src[:200], src[100:300], D([_row(0, 8, 8, 0)]))
    assert not dst.any(), "a refused call writes nothing"
    msrc = torch.zeros(128, dtype=torch.uint8, device="cuda")
    mdst = torch.zeros_like(msrc)
    for match, rows in [("outside the input", [_row(65, 8, 8, 0)]), ("overlap", [_row(0, 8, 8, 0), _row(64, 8, 8, 63)]),
                        ("fill id", [_row(0, 8, 8, 0, fill=(256, 0, 0))]), ("turns", [_row(0, 8, 8, 0, turns=5)]),
                        ("int32", [_row(0, 8, 8, 0, affine=1, fx=[65536, 0, 2 ** 31, 0, 65536, 0])])]:
        with pytest.raises(Wm2fError, match=match):
            ops.orient_labels(msrc, mdst, D(rows))
    with pytest.raises(Wm2fError, match="fill id"):
        ops.orient_labels(msrc.view(torch.int32), mdst.view(torch.int32), D([_row(0, 4, 8, 0, fill=(2 ** 31, 0, 0))]))
    with pytest.raises(ValueError, match="desc"):
        ops.orient_u8(src, dst, np.zeros((1, 21), np.int64))
    with pytest.raises(TypeError):
        ops.orient_u8(src.to(torch.int32), dst, D([_row(0, 8, 8, 0)]))
    with pytest.raises(TypeError):
        ops.orient_labels(msrc, mdst.view(torch.int32), D([_row(0, 8, 8, 0)]))
    assert len(_row(0, 1, 1, 0)) == _lib.WM2F_ORIENT_DESC_LEN


def test_raw_descriptor_runs_and_respects_its_neighbours(proc):
    """in_off and out_off of the caller's own choice, bytes around the output untouched."""
    from weed_instance_segmentation_amd import ops
    im = inputs(5, 7)[0]
    p = RotateParams(True, 1, 13.37, FILL)
    src = torch.full((400,), 3, dtype=torch.uint8, device="cuda")
    dst = torch.full((400,), 7, dtype=torch.uint8, device="cuda")
    src[13:13 + 105] = T(im).reshape(-1)
    assert ops.orient_u8(src, dst, np.array([p.desc_row(13, 5, 7, 101)], dtype=np.int64)) is dst
    assert torch.equal(dst[101:206].view(7, 5, 3), want_image(im, p))
    assert bool((dst[:101] == 7).all()) and bool((dst[206:] == 7).all()), "neighbours untouched"


def test_image_behind_two_gib(proc):
    """Byte offsets are 64-bit: a 5 x 7 image read from and written to offset 2^31 + 5 of buffers that are only allocated,
    never filled.  (tests/test_photometric_gpu.py allocates the same 2 GiB.)"""
    from weed_instance_segmentation_amd import ops
    im = inputs(5, 7)[0]
    off = (1 << 31) + 5
    src = torch.empty(off + 4096, dtype=torch.uint8, device="cuda")
    dst = torch.empty(off + 4096, dtype=torch.uint8, device="cuda")
    src[off:off + 105] = T(im).reshape(-1)
    dst[off - 8:off + 128] = 7
    p = RotateParams(False, 3, -7.5, FILL)
    ops.orient_u8(src, dst, np.array([p.desc_row(off, 5, 7, off)], dtype=np.int64))
    assert torch.equal(dst[off:off + 105].view(7, 5, 3), want_image(im, p))
    assert bool((dst[off - 8:off] == 7).all()) and bool((dst[off + 105:off + 128] == 7).all()), "neighbours untouched"


# ------------------------------------------------------------------------------------------------ the processor
COMPOSED = "composed_with_everything"


def _composed_case():
    c = next(c for c in golden_cases() if c["name"] == COMPOSED)
    g, n = c["raw"], COMPOSED
    r = json.loads(str(g[f"{n}.rows"]))[0]
    chain = tuple((k, v) for k, v in json.loads(str(g[f"{n}.chain"])))
    id2sem = [{int(k): v for k, v in d.items()} for d in json.loads(str(g[f"{n}.id2sem"]))]
    geo = (r[0], (r[1], r[2]), (r[3], r[4]), (r[5], r[6]))
    return dict(image=c["images"][0], map=c["maps"][0], id2sem=id2sem, pad=json.loads(str(g[f"{n}.pad_size"])),
                rotate=c["params"][0], chain=chain, geo=geo, oriented=c["outs"][0], oriented_map=c["mouts"][0],
                params=AugmentParams(*geo, PhotometricParams(chain), c["params"][0]),
                pixel_values=g[f"{n}.pixel_values"], pixel_mask=g[f"{n}.pixel_mask"],
                mask_labels=g[f"{n}.mask_labels0"], class_labels=g[f"{n}.class_labels0"])


def _same(a, b):
    return (torch.equal(a["pixel_values"], b["pixel_values"]) and torch.equal(a["pixel_mask"], b["pixel_mask"])
            and all(torch.equal(x, y) for x, y in zip(a["mask_labels"], b["mask_labels"]))
            and all(torch.equal(x, y) for x, y in zip(a["class_labels"], b["class_labels"])))


def test_processor_composes_orientation_with_colour_and_geometry(proc):
    """Colour jitter, vertical flip, one turn (75 x 96 -> 96 x 75), 13.37 degrees, then horizontal flip, resize and crop
    of the turned frame: the fixture's Pillow outputs."""
    c = _composed_case()
    call = lambda im, m, p: proc.preprocess([im], [m], c["id2sem"], augment=[p], pad_size=c["pad"],  # noqa: E731
                                            ignore_index=IG)
    out = call(c["image"], c["map"], c["params"])
    assert torch.equal(out["pixel_values"], T(c["pixel_values"])) and torch.equal(out["pixel_mask"], T(c["pixel_mask"]))
    assert torch.equal(out["mask_labels"][0], T(c["mask_labels"]))
    assert torch.equal(out["class_labels"][0], T(c["class_labels"]))
    # device-resident inputs are bit-identical after the call; two calls give identical results
    dev_im, dev_m = T(c["image"]), T(c["map"])
    keep, keep_m = dev_im.clone(), dev_m.clone()
    again = call(dev_im, dev_m, c["params"])
    assert torch.equal(dev_im, keep) and torch.equal(dev_m, keep_m)
    assert _same(again, out)
    # the stage alone, then the call without it, is the same thing
    from weed_instance_segmentation_amd.augment import adjust_colors
    two = call(rotate_images(adjust_colors(dev_im, PhotometricParams(c["chain"])), c["rotate"]),
               rotate_maps(dev_m, c["rotate"]), AugmentParams(*c["geo"]))
    assert _same(two, out)
    # rotate=None and a RotateParams with nothing enabled are the call without the field
    H, W = c["image"].shape[:2]
    geo = (1, (60, 64), (20, 0), (33, 31))
    plain = call(c["image"], c["map"], AugmentParams(*geo))
    assert _same(call(c["image"], c["map"], AugmentParams(*geo, None, None)), plain)
    assert _same(call(c["image"], c["map"], AugmentParams(*geo, None, RotateParams())), plain)
    assert not torch.equal(plain["pixel_values"], out["pixel_values"])


def test_processor_batch_with_and_without_orientation(proc):
    """Three images in one call: rotated and turned, untouched (rotate=None), flipped; with do_reduce_labels, where
    map_fill is a raw id and is reduced with the map."""
    rng = np.random.default_rng(41)
    sizes = [(33, 37), (17, 91), (45, 23)]
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    ms = [rng.integers(0, 5, (h, w)).astype(np.uint8) for h, w in sizes]
    rots = [RotateParams(False, 1, 20.0, FILL, 0), None, RotateParams(True, map_fill=3)]
    geo = [(1, (40, 44), (3, 2), (32, 32)), (0, (24, 100), (0, 10), (24, 32)), (1, (45, 23), (0, 0), (45, 23))]
    id2sem = {i: i for i in range(6)}
    pad = {"height": 48, "width": 32}
    for reduce in (False, True):
        kw = dict(pad_size=pad, ignore_index=IG, do_reduce_labels=reduce)
        out = proc.preprocess(ims, ms, id2sem, augment=[AugmentParams(*g, None, r) for g, r in zip(geo, rots)], **kw)
        o_ims = [im if r is None else R.orient_image(im, r.vflip, r.turns, r.angle, r.fill) for im, r in zip(ims, rots)]
        o_ms = [m if r is None else R.orient_map(m, r.vflip, r.turns, r.angle, r.map_fill) for m, r in zip(ms, rots)]
        want = proc.preprocess(o_ims, o_ms, id2sem, augment=[AugmentParams(*g) for g in geo], **kw)
        assert _same(out, want), reduce


def test_instance_rotated_out_of_the_frame_is_absent(proc):
    """Ids 1 .. 4 in a 64 x 64 map; id 3 lives in the top-left 6 x 6 corner only, which 45 degrees turns out of the
    frame."""
    m = np.zeros((64, 64), np.uint8)
    m[20:30, 20:44], m[34:44, 20:30], m[0:6, 0:6], m[34:44, 34:44] = 1, 2, 3, 4
    im = inputs(64, 64)[0]
    assert 3 not in R.orient_map(m, angle=45.0) and 3 in R.orient_map(m, angle=5.0)
    id2sem = {i: i for i in range(5)}
    call = lambda a: proc.preprocess([im], [m], id2sem, ignore_index=IG,  # noqa: E731
                                     augment=[AugmentParams(0, (64, 64), rotate=RotateParams(angle=a))])
    out, near = call(45.0), call(5.0)
    assert out["class_labels"][0].tolist() == [0, 1, 2, 4] and near["class_labels"][0].tolist() == [0, 1, 2, 3, 4]
    assert out["mask_labels"][0].shape == (4, 64, 64)
    want = R.orient_map(m, angle=45.0)
    for k, i in enumerate([0, 1, 2, 4]):
        assert torch.equal(out["mask_labels"][0][k], T((want == i).astype(np.float32)))


# ------------------------------------------------------------------------------------------------ datasets
def test_pheno_bench_dataset_with_orientation(proc, tmp_path):
    from test_augment_gpu import _pheno_folder
    from weed_instance_segmentation_amd.annotations import PhenoBenchDataset
    img_dir, ann_dir = _pheno_folder(tmp_path)
    aug = TrainAugmentation(scale=(0.5, 2.0), crop_size=(128, 160), vflip_prob=0.5, quarter_turns=True, rotate=25,
                            fill=(124, 116, 104), map_fill=255)
    gen = lambda s: torch.Generator().manual_seed(s)  # noqa: E731
    ds = PhenoBenchDataset(img_dir, ann_dir, proc, {}, augment=aug)
    seen = set()
    for i in range(2):
        ds.generator = gen(3 + i)
        item = ds[i]
        p = item["augment"]
        assert p == aug.sample(*item["original_map"].shape, gen(3 + i)) and p.rotate is not None and p.rotate.enabled
        seen.add(p.rotate.turns)
        r = p.rotate
        image = np.asarray(Image.open(ds.valid_files[i][0]).convert("RGB"))
        m, id2sem = item["original_map"], item["id_to_semantic"]
        # on the device again
        again = proc.preprocess([image], [m], id2sem, augment=[p], pad_size=aug.pad_size, ignore_index=IG)
        assert torch.equal(again["pixel_values"][0], item["pixel_values"])
        assert torch.equal(again["mask_labels"][0], item["mask_labels"])
        assert torch.equal(again["class_labels"][0], item["class_labels"])
        # in Pillow, then the call without the stage
        o_im = R.pil_orient_image(image, r.vflip, r.turns, r.angle, r.fill)
        o_m = R.pil_orient_map(m.astype(np.uint8), r.vflip, r.turns, r.angle, r.map_fill)
        pil = proc.preprocess([o_im], [o_m], id2sem, augment=[AugmentParams(p.flip, p.size, p.origin, p.window)],
                              pad_size=aug.pad_size, ignore_index=IG)
        assert torch.equal(pil["pixel_values"][0], item["pixel_values"]), "replayed in Pillow, then the geometry alone"
        assert torch.equal(pil["mask_labels"][0], item["mask_labels"])
        assert torch.equal(pil["class_labels"][0], item["class_labels"])
    assert seen, "the recipe drew turns"
