"""Orientation augmentation without a GPU: the numpy restatement (tests/rotate_reference.py) against
Pillow run here and against the fixture, `RotateParams`, the draws of `TrainAugmentation.sample`, and the search for an
input that a fused build would change."""
import json
import math

import numpy as np
import pytest
import torch
from PIL import Image

import rotate_reference as R
from conftest import load_golden
from weed_instance_segmentation_amd import _lib
from weed_instance_segmentation_amd.augment import AugmentParams, RotateParams, TrainAugmentation

FILL, MAP_FILL, BIG_FILL = (7, 130, 255), 9, 70001


def golden_cases():
    g = load_golden("rotate_pil.npz")
    out = []
    for name in json.loads(str(g["cases"])):
        params = [RotateParams(bool(v), k, a, tuple(f), mf) for v, k, a, f, mf in json.loads(str(g[f"{name}.params"]))]
        n = len(params)
        out.append(dict(name=name, params=params, raw=g, images=[g[f"{name}.img{b}"] for b in range(n)],
                        maps=[g[f"{name}.map{b}"] for b in range(n)], outs=[g[f"{name}.out{b}"] for b in range(n)],
                        mouts=[g[f"{name}.mout{b}"] for b in range(n)]))
    return out


def inputs(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    return (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8),
            rng.integers(0, 70000, (H, W)).astype(np.int32))


def test_package_exports():
    import weed_instance_segmentation_amd as pkg
    from weed_instance_segmentation_amd import augment, ops
    assert pkg.RotateParams is RotateParams and pkg.rotate_images is augment.rotate_images
    assert pkg.rotate_maps is augment.rotate_maps
    assert callable(ops.orient_u8) and callable(ops.orient_labels)
    for name in ("wm2f_orient_u8", "wm2f_orient_labels_u8", "wm2f_orient_labels_i32"):
        assert name in _lib.SIGNATURES


# ------------------------------------------------------------------------------------------------ restatement = Pillow
@pytest.mark.parametrize("hw", R.SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_rotation_equals_pillow(hw):
    """33 angles and more per size: RGB bilinear, L nearest and I (int32) nearest, with fills other than 0."""
    im, m8, m32 = inputs(*hw)
    for a in R.angles(hw[0]):
        assert np.array_equal(R.orient_image(im, angle=a, fill=FILL), R.pil_orient_image(im, angle=a, fill=FILL)), a
        assert np.array_equal(R.orient_map(m8, angle=a, fill=MAP_FILL), R.pil_orient_map(m8, angle=a, fill=MAP_FILL)), a
        assert np.array_equal(R.orient_map(m32, angle=a, fill=BIG_FILL), R.pil_orient_map(m32, angle=a, fill=BIG_FILL)), a


@pytest.mark.parametrize("hw", [(5, 9), (6, 6)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_flips_and_turns_equal_pillow(hw):
    """All eight combinations, alone and in front of a rotation; 90, 270, -90 and 450 on both shapes."""
    im, m8, m32 = inputs(*hw)
    for vf in (False, True):
        for k in range(4):
            for a in (0.0, 33.3, 90, 270, -90, 450, 180, 360, -180):
                assert np.array_equal(R.orient_image(im, vf, k, a, FILL), R.pil_orient_image(im, vf, k, a, FILL)), (vf, k, a)
                assert np.array_equal(R.orient_map(m8, vf, k, a, MAP_FILL), R.pil_orient_map(m8, vf, k, a, MAP_FILL)), (vf, k, a)
                assert np.array_equal(R.orient_map(m32, vf, k, a, BIG_FILL), R.pil_orient_map(m32, vf, k, a, BIG_FILL)), (vf, k, a)
    assert R.orient_image(im, turns=1).shape == (hw[1], hw[0], 3)


def test_shortcut_angles():
    """Pillow routes 0, 180, 360, -180 to transpose on any image, 90 and 270 on a square one only."""
    assert [R.shortcut(a, 5, 9) for a in (0, 180, 360, -180, 90, 270, -90, 450)] == [0, 2, 0, 2, None, None, None, None]
    assert [R.shortcut(a, 6, 6) for a in (0, 180, 360, -180, 90, 270, -90, 450)] == [0, 2, 0, 2, 1, 3, 3, 1]
    im = inputs(5, 9)[0]
    got = R.orient_image(im, angle=90, fill=FILL)  # the transform, not a turn: the frame stays 5 x 9 and has fill in it
    assert got.shape == im.shape and (got == np.asarray(FILL, np.uint8)).all(-1).any()
    for H, W in [(5, 9), (6, 6)]:
        for a in (0, 180, 360, -180, 90, 270):
            p = RotateParams(False, 1, float(a))
            k = R.shortcut(a, *p.out_size(H, W))
            assert p.folded(H, W) == (((1 + k) % 4, False) if k is not None else (1, True)), (H, W, a)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_equals_the_fixture(case):
    assert str(case["raw"]["pillow_version"]).startswith("12.")
    for im, m, p, out, mout in zip(case["images"], case["maps"], case["params"], case["outs"], case["mouts"]):
        assert np.array_equal(R.orient_image(im, p.vflip, p.turns, p.angle, p.fill), out)
        assert np.array_equal(R.orient_map(m, p.vflip, p.turns, p.angle, p.map_fill), mout)
        assert out.shape[:2] == p.out_size(*im.shape[:2]) == mout.shape


# ------------------------------------------------------------------------------------------------ RotateParams
def test_rotate_params_validation():
    p = RotateParams()
    assert (p.vflip, p.turns, p.angle, p.fill, p.map_fill) == (False, 0, 0.0, (0, 0, 0), 0) and not p.enabled
    assert RotateParams(angle=360).enabled is False and RotateParams(angle=-720.0).enabled is False
    assert RotateParams(True).enabled and RotateParams(turns=3).enabled and RotateParams(angle=1e-9).enabled
    assert RotateParams(1, 2, 5, [1, 2, 3], 7) == RotateParams(True, 2, 5.0, (1, 2, 3), 7)
    with pytest.raises(Exception):
        p.turns = 1  # frozen
    for bad in (dict(vflip=2), dict(vflip="yes"), dict(turns=4), dict(turns=-1), dict(turns=1.0), dict(turns=True),
                dict(angle=math.inf), dict(angle=math.nan), dict(angle="3"), dict(angle=True), dict(fill=(0, 0)),
                dict(fill=(0, 0, 256)), dict(fill=(0, -1, 0)), dict(fill=(0.5, 0, 0)), dict(fill=5), dict(map_fill=1.5),
                dict(map_fill=2 ** 31), dict(map_fill=True)):
        with pytest.raises(ValueError):
            RotateParams(**bad)
    with pytest.raises(ValueError, match="rotate"):
        AugmentParams(0, (4, 4), rotate="no")
    assert AugmentParams(0, (4, 4)) == AugmentParams(0, (4, 4), (0, 0), (4, 4), None, None)
    assert AugmentParams.identity(3, 5).rotate is None


def test_matrix_and_fixed_are_pillows():
    """`.matrix` and `.fixed` put through the restatement's sampling give Image.rotate's bytes: no second copy of the
    formula is compared, Pillow's own result is."""
    for H, W in [(33, 130), (64, 64), (5, 7)]:
        im, m8, _ = inputs(H, W)
        for a in (1, -7.5, 13.37, 45, 89.99, 270.5, 30.000001):
            p = RotateParams(angle=a)
            want = np.asarray(Image.fromarray(im).rotate(a, resample=Image.BILINEAR))
            assert np.array_equal(R.rotate_bilinear(im, a, m=p.matrix(H, W)), want)
            want = np.asarray(Image.fromarray(m8).rotate(a, resample=Image.NEAREST))
            assert np.array_equal(R.rotate_nearest(m8, a, a=p.fixed(H, W)), want)


def test_desc_row():
    p = RotateParams(True, 1, 13.37, (1, 2, 3), 300)
    row = p.desc_row(12, 5, 9, 24)
    assert len(row) == _lib.WM2F_ORIENT_DESC_LEN == 22
    assert row[:7] == [12, 5, 9, 24, 1, 1, 1] and row[19:] == [1, 2, 3]
    m = [float(np.array(v, np.int64).view(np.float64)) for v in row[7:13]]
    assert m == p.matrix(9, 5) == R.matrix(13.37, 9, 5), "the matrix of the TURNED (9, 5) frame, as bit patterns"
    assert row[13:19] == p.fixed(9, 5) and all(isinstance(v, int) for v in row)
    assert p.desc_row(0, 5, 9, 0, labels=True)[19:] == [300, 0, 0]
    assert RotateParams(False, 1, 180.0).desc_row(0, 5, 9, 0)[4:7] == [0, 3, 0], "180 folds into the turn"
    assert RotateParams(False, 0, 90.0).desc_row(0, 6, 6, 0)[4:7] == [0, 1, 0], "90 on a square is a turn"
    assert RotateParams(False, 0, 90.0).desc_row(0, 5, 9, 0)[4:7] == [0, 0, 1], "90 on a non-square is the transform"
    for H, W in [(16384, 16384), (16384, 1)]:
        for a in (45.0, 13.37, 135.0, 300.0):
            assert all(-2 ** 31 <= v < 2 ** 31 for v in RotateParams(angle=a).fixed(H, W)), "int32, as Pillow's accumulators"


# ------------------------------------------------------------------------------------------------ the draws
def _todays_sample(aug, H, W, g):
    """The four draws of DESIGN section 20, written out: what `sample` did before orientation existed."""
    flip = int(torch.rand(1, generator=g).item() < aug.flip_prob)
    lo, hi = aug.scale
    f = lo + (hi - lo) * float(torch.rand(1, dtype=torch.float64, generator=g).item())
    Ch, Cw = aug.crop_size
    r = min(Ch * f / H, Cw * f / W)
    h, w = max(1, int(round(H * r))), max(1, int(round(W * r)))
    ch, cw = min(Ch, h), min(Cw, w)
    y0 = int(torch.randint(h - ch + 1, (1,), generator=g).item())
    x0 = int(torch.randint(w - cw + 1, (1,), generator=g).item())
    return AugmentParams(flip, (h, w), (y0, x0), (ch, cw))


JITTER = dict(scale=(0.5, 2.0), crop_size=(64, 80))


def test_sample_without_orientation_takes_no_new_draw():
    for aug in (TrainAugmentation(**JITTER), TrainAugmentation(**JITTER, vflip_prob=0.0, quarter_turns=False, rotate=None,
                                                               fill=(9, 9, 9), map_fill=3)):
        assert not aug.orients
        for seed in range(10):
            g, ref = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
            p = aug.sample(96, 64, g)
            assert p == _todays_sample(aug, 96, 64, ref) and p.rotate is None
            assert torch.equal(g.get_state(), ref.get_state())


PINNED_SEED = 11
# flip, size, origin, window, (vflip, turns, angle) of that seed on a 96 x 64 source: three turns make the frame 64 x 96
PINNED = (0, (71, 106), (4, 7), (64, 80), (True, 3, 23.11754221116022))


def test_sample_with_orientation_takes_three_draws_first():
    aug = TrainAugmentation(**JITTER, vflip_prob=0.5, quarter_turns=True, rotate=30, fill=(1, 2, 3), map_fill=4)
    assert aug.orients and aug.rotate_range == (-30.0, 30.0)
    turns, sizes = set(), set()
    for seed in range(40):
        g, ref = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        p = aug.sample(96, 64, g)
        u = float(torch.rand(1, generator=ref).item())
        k = int(torch.randint(4, (1,), generator=ref).item())
        ua = float(torch.rand(1, dtype=torch.float64, generator=ref).item())
        r = p.rotate
        assert (r.vflip, r.turns, r.angle) == (u < 0.5, k, min(-30.0 + 60.0 * ua, 30.0))
        assert -30.0 <= r.angle <= 30.0 and r.fill == (1, 2, 3) and r.map_fill == 4
        Ht, Wt = (64, 96) if k & 1 else (96, 64)
        rest = _todays_sample(aug, Ht, Wt, ref)  # the four draws that follow see the turned frame
        assert (p.flip, p.size, p.origin, p.window) == (rest.flip, rest.size, rest.origin, rest.window)
        assert torch.equal(g.get_state(), ref.get_state()), "exactly three more draws"
        turns.add(k), sizes.add(p.size[0] > p.size[1])
    assert turns == {0, 1, 2, 3} and sizes == {False, True}, "(h, w) follows the turned frame"


def test_sample_draws_are_discarded_for_options_that_are_off():
    full = TrainAugmentation(**JITTER, vflip_prob=1.0, quarter_turns=True, rotate=(10, 20))
    for kw in (dict(vflip_prob=1.0), dict(quarter_turns=True), dict(rotate=(10, 20))):
        aug = TrainAugmentation(**JITTER, **kw)
        for seed in range(6):
            g, ref = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
            p, q = aug.sample(96, 64, g), full.sample(96, 64, ref)
            assert torch.equal(g.get_state(), ref.get_state()), "always all three draws"
            assert p.rotate.vflip == ("vflip_prob" in kw) and q.rotate.vflip
            assert p.rotate.turns == (q.rotate.turns if "quarter_turns" in kw else 0)
            assert p.rotate.angle == (q.rotate.angle if "rotate" in kw else 0.0)
            if "rotate" in kw:
                assert 10.0 <= p.rotate.angle <= 20.0


def test_sample_pinned_values():
    aug = TrainAugmentation(**JITTER, vflip_prob=0.5, quarter_turns=True, rotate=30)
    p = aug.sample(96, 64, torch.Generator().manual_seed(PINNED_SEED))
    assert p == AugmentParams(*PINNED[:4], None, RotateParams(*PINNED[4]))
    colour = TrainAugmentation(**JITTER, vflip_prob=0.5, quarter_turns=True, rotate=30, brightness=0.2)
    q = colour.sample(96, 64, torch.Generator().manual_seed(PINNED_SEED))
    assert (q.flip, q.size, q.origin, q.window, q.rotate) == (p.flip, p.size, p.origin, p.window, p.rotate)
    assert q.photometric is not None, "the colour draws still come last"


def test_train_augmentation_validation():
    for bad in (dict(vflip_prob=1.5), dict(vflip_prob=-0.1), dict(quarter_turns=1), dict(rotate=-5), dict(rotate=(3, 1)),
                dict(rotate="x"), dict(rotate=(0, math.inf)), dict(fill=(0, 0, 300)), dict(map_fill=0.5)):
        with pytest.raises(ValueError):
            TrainAugmentation(**JITTER, **bad)
    assert TrainAugmentation(**JITTER, rotate=0).rotate_range == (0.0, 0.0)
    edge = TrainAugmentation(short_edge=(32, 48), size_divisor=0, quarter_turns=True)
    for seed in range(8):
        p = edge.sample(96, 64, torch.Generator().manual_seed(seed))
        assert (p.size[0] > p.size[1]) == (p.rotate.turns % 2 == 0), "the short-edge recipe sees the turned frame too"


# ------------------------------------------------------------------------------------------------ fused or not
def test_fma_emulation_is_exact():
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-300, 300, 3000), rng.uniform(0, 1, 3000)
    c = rng.integers(0, 256, 3000).astype(np.float64)
    got = R._fma(a, b, c)
    assert np.array_equal(got, R.fma_exact(a, b, c))
    assert (got != a * b + c).any(), "the operands tell one rounding from two"
    m = R.matrix(13.37, 96, 64)
    y = np.arange(96.0) + 0.5
    assert np.array_equal(R._fma(m[1], y, m[0] * 3.5), R.fma_exact(m[1], y, m[0] * 3.5))


def test_search_for_an_input_that_fusion_would_change():
    """96 x 64 and 33 x 130 at every angle of the list, the blend and the coordinates fused (both ways the coordinate sum
    can contract), exact products rounded once.  Fused coordinates differ in the last bit at many pixels, yet no byte
    changes: the search finds no discriminating case, so none is pinned, and the rule is enforced by
    the build (contraction off for csrc/orient.hip).  Should this test ever find one, pin it here and in
    tests/test_rotate_gpu.py."""
    found, coords_differ = [], 0
    for H, W in [(96, 64), (33, 130)]:
        im = inputs(H, W)[0]
        for a in R.angles(H):
            if R.shortcut(a, H, W) is not None:
                continue
            want = R.rotate_bilinear(im, a)
            for f in (1, 2):
                got = R.rotate_bilinear(im, a, fused=f)
                if not np.array_equal(want, got):
                    y, x, c = (int(v[0]) for v in np.nonzero(want != got))
                    found.append(((H, W), a, f, (y, x, c)))
            m = R.matrix(a, H, W)
            yy, xx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
            coords_differ += int((R._fma(m[1], yy, m[0] * xx) + m[2] != m[0] * xx + m[1] * yy + m[2]).sum())
    assert coords_differ > 0, "the search does exercise fused coordinates that differ"
    assert found == [], f"a fused build changes bytes here: pin these cases: {found[:5]}"
