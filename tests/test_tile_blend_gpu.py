"""Blending tile scores on the GPU: wm2f_tile_blend, blend_tile_scores and segment_tiled_semantic.
Every comparison with the numpy restatement of tests/tile_blend_reference.py is exact: the map equal, the scores equal
bit for bit.  The inputs carry exact ties between classes (the last class repeats class 0)."""
import functools
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
import tile_blend_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (H, W, tile, overlap), score grid ("tile": the tile size itself, the identity resize), classes, flip codes.
# 150 x 150: origins 0, 28, 57, 86 (odd ones among them: a lane's two pixels straddle a tile border), triple overlaps;
# W = 53 and W = 1: odd, pixel-by-pixel stores; every other width is even (8-byte stores); 700 x 900 at 384: several
# workgroups along both axes; 37 x 53 at tile 64: one tile whose scale 24 / 37 is no dyadic number.  Classes on both sides
# of the chunk of 4 held in registers (3, 4, 5, 8, 9) and of the 8 the post-processor holds.
CASES = [
    ((150, 150, 64, 31), (24, 24), 3, (0,)),
    ((150, 150, 64, 31), (24, 24), 5, (1,)),
    ((96, 160, 64, 16), (16, 40), 4, (0,)),
    ((150, 150, 64, 31), (16, 40), 9, (0, 1, 2, 3)),
    ((150, 150, 64, 31), "tile", 19, (2, 1)),
    ((37, 53, 32, 8), (24, 24), 1, (0,)),
    ((37, 53, 32, 8), (16, 40), 8, (0, 3)),
    ((37, 53, 64, 16), (24, 24), 3, (0, 3)),
    ((1, 70, 32, 8), (24, 24), 3, (0, 1)),
    ((70, 1, 32, 8), (16, 40), 9, (0,)),
    ((96, 160, 64, 16), "tile", 8, (0, 1, 2, 3)),
    ((96, 160, 64, 16), (24, 24), 19, (0,)),
    ((700, 900, 384, 96), (384, 384), 3, (0,)),
    ((700, 900, 384, 96), (24, 24), 9, (0, 1)),
]


def _ids(case):
    (H, W, tile, overlap), grid, C, flips = case
    g = "tile" if grid == "tile" else f"{grid[0]}x{grid[1]}"
    return f"{H}x{W}-t{tile}-o{overlap}-g{g}-C{C}-F{''.join(map(str, flips))}"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _i32(seq):
    return torch.tensor(list(seq), dtype=torch.int32, device=DEV)


def _bits_equal(t, a):
    got = t.cpu().numpy()
    return got.shape == a.shape and np.array_equal(got.view(np.int32), np.ascontiguousarray(a).view(np.int32))


@functools.lru_cache(maxsize=None)
def _case(case):
    from weed_instance_segmentation_amd import tile_windows
    (H, W, tile, overlap), grid, C, flips = case
    g = tile_windows(H, W, tile, overlap)
    gh, gw = (g.th, g.tw) if grid == "tile" else grid
    seed = abs(hash((H, W, tile, overlap, gh, gw, C, flips))) % (2 ** 31)
    scores = R.random_scores(len(flips), g.n_tiles, C, gh, gw, seed)
    ramp = max(1, overlap)
    seg, out = R.blend(scores, g.ys, g.xs, flips, H, W, g.th, g.tw, ramp, ramp)
    return SimpleNamespace(grid=g, scores=scores, flips=flips, ramp=(ramp, ramp), seg=seg, out=out, H=H, W=W, C=C)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kernel_equals_the_restatement(case):
    from weed_instance_segmentation_amd import ops
    c = _case(case)
    g = c.grid
    scores, ys, xs, flips = _dev(c.scores), _i32(g.ys), _i32(g.xs), _i32(c.flips)
    seg, out = ops.tile_blend(scores, ys, xs, flips, (c.H, c.W), (g.th, g.tw), c.ramp, want_scores=True)
    assert seg.dtype == torch.int32 and out.dtype == torch.float32 and tuple(out.shape) == (c.C, c.H, c.W)
    got = seg.cpu().numpy()
    print("mismatching pixels", int((got != c.seg).sum()), "of", got.size, "classes present", np.unique(c.seg).tolist())
    assert np.array_equal(got, c.seg)
    assert _bits_equal(out, c.out)
    if c.C >= 2:  # the tie is live: class 0 wins somewhere, and nowhere does its copy
        assert (c.seg == 0).any() and not (c.seg == c.C - 1).any()
    # repeatability, and the map alone
    seg2, out2 = ops.tile_blend(scores, ys, xs, flips, (c.H, c.W), (g.th, g.tw), c.ramp, want_scores=True)
    assert torch.equal(seg2, seg) and torch.equal(out2.view(torch.int32), out.view(torch.int32))
    seg3, none = ops.tile_blend(scores, ys, xs, flips, (c.H, c.W), (g.th, g.tw), c.ramp)
    assert none is None and torch.equal(seg3, seg)


def test_blend_tile_scores_takes_a_grid():
    from weed_instance_segmentation_amd import blend_tile_scores
    c = _case(((150, 150, 64, 31), (16, 40), 9, (0, 1, 2, 3)))
    got = blend_tile_scores(_dev(c.scores), c.grid, flips=("none", "h", "v", "hv"), ramp=31, return_scores=True)
    assert np.array_equal(got["segmentation"].cpu().numpy(), c.seg) and _bits_equal(got["scores"], c.out)
    one = _case(((150, 150, 64, 31), (24, 24), 3, (0,)))
    got = blend_tile_scores(_dev(one.scores[0]), one.grid, ramp=(31, 31))  # (T, C, gh, gw): one view
    assert set(got) == {"segmentation"} and np.array_equal(got["segmentation"].cpu().numpy(), one.seg)
    # the default ramp is the smallest actual overlap per axis: origins 0, 28, 57, 86 with side 64 overlap by 36, 35, 35
    seg, out = R.blend(one.scores, one.grid.ys, one.grid.xs, (0,), 150, 150, 64, 64, 35, 35)
    got = blend_tile_scores(_dev(one.scores), one.grid, return_scores=True)
    assert np.array_equal(got["segmentation"].cpu().numpy(), seg) and _bits_equal(got["scores"], out)


def test_a_gap_in_the_grid_gives_minus_one_and_zero_scores():
    from weed_instance_segmentation_amd import ops
    ys, xs, th, tw, H, W = [0, 40], [0, 20], 32, 32, 72, 60  # rows 32 .. 39 and columns 52 .. 59 are covered by no tile
    scores = R.random_scores(2, 4, 3, 8, 8, seed=5)
    seg, out = ops.tile_blend(_dev(scores), _i32(ys), _i32(xs), _i32((0, 3)), (H, W), (th, tw), (8, 8), want_scores=True)
    want_seg, want_out = R.blend(scores, ys, xs, (0, 3), H, W, th, tw, 8, 8)
    assert (want_seg[32:40] == -1).all() and (want_seg[:, 52:] == -1).all() and (want_seg[:32, :52] >= 0).all()
    assert not want_out[:, 32:40].any() and not want_out[:, :, 52:].any()
    assert np.array_equal(seg.cpu().numpy(), want_seg) and _bits_equal(out, want_out)


def test_exact_flip_property():
    """Identity grid, two views, the second the mirrored picture computed 'on the flipped tile': wherever a single tile
    covers, 2 w v / 2 w is v itself (w an integer <= 2^8, v on a 2^-12 raster: every step exact), so the scores equal the
    one-view scores bit for bit.  A kernel that forgets to mirror averages a picture with its mirror image."""
    from weed_instance_segmentation_amd import ops, tile_windows
    H, W = 96, 160
    g = tile_windows(H, W, 64, 16)
    one = R.random_scores(1, g.n_tiles, 3, 64, 64, seed=9)
    assert not np.array_equal(one, np.flip(one, -1))  # asymmetric
    two = np.concatenate([one, np.flip(one, -1)])
    args = (_i32(g.ys), _i32(g.xs))
    seg1, out1 = ops.tile_blend(_dev(one), *args, _i32((0,)), (H, W), (64, 64), (16, 16), want_scores=True)
    seg2, out2 = ops.tile_blend(_dev(two), *args, _i32((0, 1)), (H, W), (64, 64), (16, 16), want_scores=True)
    sole = torch.from_numpy(R.counts(g.ys, g.xs, 1, 64, 64, H, W) == 1).to(DEV)
    assert int(sole.sum()) > 1000
    assert torch.equal(out2[:, sole].view(torch.int32), out1[:, sole].view(torch.int32))
    assert torch.equal(seg2[sole], seg1[sole])
    _, unmirrored = ops.tile_blend(_dev(two), *args, _i32((0, 0)), (H, W), (64, 64), (16, 16), want_scores=True)
    assert not torch.equal(unmirrored[:, sole], out1[:, sole])
    want_seg, want_out = R.blend(two, g.ys, g.xs, (0, 1), H, W, 64, 64, 16, 16)
    assert np.array_equal(seg2.cpu().numpy(), want_seg) and _bits_equal(out2, want_out)


def test_scores_past_two_to_the_31_elements():
    """1024 tiles of one row each, 15 classes on the 384 x 384 grid: 2.26e9 score elements, the last tiles' lie past 2^31.
    Only the last four tiles are filled and compared."""
    from weed_instance_segmentation_amd import ops
    T, C, G, keep = 1024, 15, 384, 4
    assert (T - keep) * C * G * G > 2 ** 31
    scores = torch.empty(1, T, C, G, G, device=DEV)
    tail = R.random_scores(1, keep, C, G, G, seed=31)
    scores[0, T - keep:] = _dev(tail[0])
    seg, out = ops.tile_blend(scores, _i32(range(T)), _i32([0]), _i32([0]), (T, 8), (1, 8), (1, 1), want_scores=True)
    want_seg, want_out = R.blend(tail, list(range(keep)), [0], (0,), keep, 8, 1, 8, 1, 1)
    assert np.array_equal(seg[T - keep:].cpu().numpy(), want_seg) and _bits_equal(out[:, T - keep:].contiguous(), want_out)


# ------------------------------------------------------------------------------- continuity with the post-processor
def _outputs(B, Q, C, h, w, seed):
    """Random model outputs as the post-processor takes them."""
    gen = torch.Generator().manual_seed(seed)
    return SimpleNamespace(masks_queries_logits=(torch.randn(B, Q, h, w, generator=gen) * 3).to(DEV),
                           class_queries_logits=(torch.randn(B, Q, C + 1, generator=gen) * 2).to(DEV))


def test_one_tile_equals_the_post_processor():
    """An image no larger than a tile, one view: the post-processor's own resize of the 384 x 384 scores to (H, W).

    Exact at (48, 96): 384 / 48 and 384 / 96 are even integers, every bilinear weight is 1/2, every product is exact, and
    the two kernels agree whether or not the compiler contracts a product and a sum into a fused multiply-add.
    csrc/postprocess_sp.hip is built with contraction allowed while csrc/tile_blend.hip is not, so at a size whose
    weights are no powers of two -- (50, 70) here -- the last bit may differ: there the bound is 1e-6 of the largest
    score (each of the three products-and-sums of a sample moves by at most one rounding, 3 * 2^-24 relative, when it is
    fused), and the figure is printed."""
    from weed_instance_segmentation_amd import Mask2FormerInstancePostProcessor, blend_tile_scores, tile_windows
    post = Mask2FormerInstancePostProcessor()
    outputs = _outputs(1, 12, 5, 16, 24, seed=1)
    S = post.post_process_semantic_segmentation(outputs, target_sizes=None, return_segmentation_scores=True)[0]["segmentation_scores"]
    assert tuple(S.shape) == (5, 384, 384)
    for (H, W), exact in (((48, 96), True), ((50, 70), False)):
        want = post.post_process_semantic_segmentation(outputs, target_sizes=[(H, W)], return_segmentation_scores=True)[0]
        got = blend_tile_scores(S.unsqueeze(0), tile_windows(H, W, 128, 32), return_scores=True)
        diff = float((got["scores"] - want["segmentation_scores"]).abs().max())
        print(f"{H} x {W}: largest score difference {diff:.3e}, largest score {float(S.max()):.3f}")
        if exact:
            assert torch.equal(got["scores"].view(torch.int32), want["segmentation_scores"].view(torch.int32))
            assert torch.equal(got["segmentation"].long(), want["segmentation"])
            assert len(torch.unique(want["segmentation"])) >= 2
        else:
            assert diff <= 1e-6 * float(S.max())


def test_a_sole_tile_region_equals_that_tiles_own_result():
    """96 x 160 at tile 64, overlap 16: where one tile alone covers, the blend is that tile's own
    `target_sizes=[(64, 64)]` result, exactly (384 / 64 = 6: every bilinear weight is 1/2, see above)."""
    from weed_instance_segmentation_amd import Mask2FormerInstancePostProcessor, blend_tile_scores, tile_windows
    post = Mask2FormerInstancePostProcessor()
    g = tile_windows(96, 160, 64, 16)
    T = g.n_tiles
    outputs = _outputs(T, 10, 4, 16, 16, seed=2)
    res = post.post_process_semantic_segmentation(outputs, target_sizes=None, return_segmentation_scores=True)
    S = torch.stack([r["segmentation_scores"] for r in res])
    own = post.post_process_semantic_segmentation(outputs, target_sizes=[(64, 64)] * T, return_segmentation_scores=True)
    got = blend_tile_scores(S, g, return_scores=True)
    sole = R.counts(g.ys, g.xs, 1, 64, 64, 96, 160) == 1
    checked = 0
    for t, (y0, x0, y1, x1) in enumerate(g.windows):
        m = torch.from_numpy(sole[y0:y1, x0:x1]).to(DEV)
        checked += int(m.sum())
        assert torch.equal(got["scores"][:, y0:y1, x0:x1][:, m].view(torch.int32), own[t]["segmentation_scores"][:, m].view(torch.int32))
        assert torch.equal(got["segmentation"][y0:y1, x0:x1][m].long(), own[t]["segmentation"][m])
    assert checked == int(sole.sum()) > 1000


# ------------------------------------------------------------------------------------------------ the model route
@functools.lru_cache(maxsize=None)
def _tiny_model():
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    g = load_golden("full_tiny.npz")
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig.from_dict(json.loads(str(g["config_json"]))))
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    return model.cuda().eval()


def test_segment_tiled_semantic_equals_the_hand_composition():
    from weed_instance_segmentation_amd import Mask2FormerImageProcessor, segment_tiled_semantic, tile_windows
    from weed_instance_segmentation_amd.panoptic_metrics import MeanIoU
    model = _tiny_model()
    proc = Mask2FormerImageProcessor(do_resize=False)  # a 64 x 64 tile is fed as 64 x 64
    image = np.random.default_rng(11).integers(0, 256, (96, 160, 3), dtype=np.uint8)
    got = segment_tiled_semantic(image, model, proc, tile=64, overlap=16, batch_size=2, flips=("none", "h"), return_scores=True)
    # by hand: the same public calls with the same batching, then the numpy restatement
    g = tile_windows(96, 160, 64, 16)
    assert g.ys == [0, 32] and g.xs == [0, 48, 96]  # neighbours overlap by 32 rows and 16 columns: the default ramps
    dev_image = torch.from_numpy(image).cuda()
    crops = [dev_image[y0:y1, x0:x1] for y0, x0, y1, x1 in g.windows]
    views = []
    with torch.no_grad():
        for flipped in (False, True):
            grids = []
            for s in range(0, len(crops), 2):
                batch = [torch.flip(c, [1]) for c in crops[s:s + 2]] if flipped else crops[s:s + 2]
                inputs = proc(images=batch)
                assert tuple(inputs["pixel_values"].shape[-2:]) == (64, 64)
                outputs = model(pixel_values=inputs["pixel_values"])
                res = proc.post_process_semantic_segmentation(outputs, target_sizes=None, return_segmentation_scores=True)
                grids += [r["segmentation_scores"].cpu().numpy() for r in res]
            views.append(np.stack(grids))
    scores = np.stack(views)
    assert scores.shape[:2] == (2, 6) and scores.shape[3:] == (384, 384)
    want_seg, want_out = R.blend(scores, g.ys, g.xs, (0, 1), 96, 160, 64, 64, 32, 16)
    seg = got["segmentation"]
    print("classes", np.unique(want_seg, return_counts=True))
    assert seg.is_cuda and seg.dtype == torch.int32 and tuple(seg.shape) == (96, 160)
    assert np.array_equal(seg.cpu().numpy(), want_seg) and _bits_equal(got["scores"], want_out)
    assert len(np.unique(want_seg)) >= 2, "a constant map: the test would pass on next to nothing"
    # a second call returns identical tensors; the map alone is the same map
    again = segment_tiled_semantic(image, model, proc, tile=64, overlap=16, batch_size=2, flips=("none", "h"))
    assert set(again) == {"segmentation"} and torch.equal(again["segmentation"], seg)
    # downstream: the mIoU metric takes the int32 map
    metric = MeanIoU(num_classes=scores.shape[2])
    metric.update([seg], [seg])
    assert float(metric.compute()["miou"]) == 1.0


def test_errors():
    from weed_instance_segmentation_amd import _lib, ops
    s = torch.zeros(1, 4, 2, 8, 8, device=DEV)
    ys, xs, fl = _i32([0, 8]), _i32([0, 8]), _i32([0])
    with pytest.raises(_lib.Wm2fError):
        ops.tile_blend(s.cpu(), ys, xs, fl, (16, 16), (8, 8), (2, 2))
    with pytest.raises(TypeError):
        ops.tile_blend(s.double(), ys, xs, fl, (16, 16), (8, 8), (2, 2))
    with pytest.raises(TypeError):
        ops.tile_blend(s, ys.long(), xs, fl, (16, 16), (8, 8), (2, 2))
    with pytest.raises(ValueError, match="tiles"):
        ops.tile_blend(s, ys, _i32([0]), fl, (16, 16), (8, 8), (2, 2))
    with pytest.raises(ValueError, match="flips"):
        ops.tile_blend(s, ys, xs, _i32([0, 1]), (16, 16), (8, 8), (2, 2))
    with pytest.raises(ValueError, match="ramps"):
        ops.tile_blend(s, ys, xs, fl, (16, 16), (8, 8), (0, 2))
    with pytest.raises(_lib.Wm2fError, match="at most"):  # sides beyond the cap: the library's own answer
        ops.tile_blend(s, ys, xs, fl, (16, 16385), (8, 8), (2, 2))
    with pytest.raises(_lib.Wm2fError, match="at most"):  # more than WM2F_TILE_MAX_TILES tiles
        ops.tile_blend(torch.zeros(1, 1025, 1, 1, 1, device=DEV), _i32(range(1025)), _i32([0]), fl, (1025, 1), (1, 1), (1, 1))
