"""Simple Copy-Paste, host side: the sampler's draws and their order, id allocation, parameter
validation, the compact-batch requirement, the C ABI's three entry points, and the numpy restatement
(tests/copy_paste_reference.py) held to its second, mask-stack formulation over seeded random cases.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import copy_paste_reference as R
from weed_instance_segmentation_amd import CopyPaste, CopyPasteParams, _lib, allocate_paste_ids
from weed_instance_segmentation_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IG = 255


# ------------------------------------------------------------------------------------------------------ shared cases
def random_maps(rng, B, H, W, n_ids=6, fill=0.45, id_pool=None):
    """(B, H, W) int32 maps of rectangles with ids from `id_pool` on an ignore_index ground, and their id -> class dicts."""
    maps = np.full((B, H, W), IG, dtype=np.int32)
    dicts = []
    for b in range(B):
        pool = list(range(40)) if id_pool is None else list(id_pool)
        ids = sorted(rng.choice(pool, size=min(n_ids, len(pool)), replace=False).tolist())
        for i in ids:
            if rng.random() > fill and i != ids[0]:
                continue
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            y1, x1 = int(rng.integers(y0, H)) + 1, int(rng.integers(x0, W)) + 1
            maps[b, y0:y1, x0:x1] = i
        dicts.append({int(i): int(i) % 3 for i in ids})
    return maps, dicts


def random_pixels(rng, B, C, H, W):
    return rng.standard_normal((B, C, H, W)).astype(np.float32)


def cyclic_params(dicts, maps, shift, min_visible=0.0, rng=None):
    """0 <- 2, 1 <- 0, 2 <- 1 (every image is source and destination), all (or a random half of) the source's ids."""
    B = len(dicts)
    source = [(b - 1) % B for b in range(B)]
    selected, new_ids = [], []
    for b in range(B):
        ids = sorted(dicts[source[b]])
        if rng is not None:
            ids = [i for i in ids if rng.random() < 0.6]
        selected.append(tuple(ids))
        new_ids.append(allocate_paste_ids(ids, dicts[b]))
    return CopyPasteParams(tuple(source), tuple(selected), tuple(new_ids), tuple(shift), min_visible)


def run_reference(pixels, maps, p, window=None):
    num, den = p.fraction()
    return R.copy_paste_reference(pixels, maps, p.source, p.lut(), p.shift, window, num, den, IG)


# --------------------------------------------------------------------------------------------------------- sampler
IDMAPS = [{1: 0, 2: 1, 5: 1, 255: 0}, {0: 1, 3: 0}, {4: 1, 7: 1, 9: 0, 300: 1}, {}]


def test_same_seed_same_parameters():
    recipe = CopyPaste(prob=0.7, select=0.6, shift=(3, 5), min_visible=0.25, max_instances=2)
    a = recipe.sample(IDMAPS, torch.Generator().manual_seed(11))
    b = recipe.sample(IDMAPS, torch.Generator().manual_seed(11))
    c = recipe.sample(IDMAPS, torch.Generator().manual_seed(12))
    assert a == b and isinstance(a, CopyPasteParams) and len(a) == 4
    assert a != c or a.source == (-1,) * 4
    assert a.min_visible == 0.25 and a.fraction() == (1, 4)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("classes", [None, (1,)])
def test_draw_order(seed, classes):
    """Replays the documented draws by hand: paste, source, one keep per allowed source id ascending, dy, dx."""
    recipe = CopyPaste(prob=0.6, select=0.5, shift=(2, 4), classes=classes)
    got = recipe.sample(IDMAPS, torch.Generator().manual_seed(seed))
    g = torch.Generator().manual_seed(seed)
    B = len(IDMAPS)
    for b in range(B):
        paste = float(torch.rand(1, generator=g).item()) < 0.6
        k = int(torch.randint(B - 1, (1,), generator=g).item())
        s = k if k < b else k + 1
        cand = [i for i in sorted(IDMAPS[s]) if 0 <= i <= 254 and (classes is None or IDMAPS[s][i] in classes)]
        kept = [i for i in cand if float(torch.rand(1, generator=g).item()) < 0.5]
        dy = int(torch.randint(5, (1,), generator=g).item()) - 2
        dx = int(torch.randint(9, (1,), generator=g).item()) - 4
        if paste and kept:
            assert got.source[b] == s and got.selected[b] == tuple(kept) and got.shift[b] == (dy, dx)
            assert got.new_ids[b] == allocate_paste_ids(kept, IDMAPS[b])
        else:
            assert got.source[b] == -1 and got.selected[b] == () and got.new_ids[b] == () and got.shift[b] == (0, 0)
    # the stream is where the documented draws leave it
    assert torch.equal(g.get_state(), _state_after(recipe, seed))


def _state_after(recipe, seed):
    g = torch.Generator().manual_seed(seed)
    recipe.sample(IDMAPS, g)
    return g.get_state()


def test_one_image_pastes_nothing_and_draws_nothing():
    g = torch.Generator().manual_seed(3)
    before = g.get_state()
    p = CopyPaste(prob=1.0, select=1.0).sample([{1: 0}], g)
    assert p.source == (-1,) and p.selected == ((),) and torch.equal(g.get_state(), before)


def test_prob_and_select_extremes_and_limits():
    never = CopyPaste(prob=0.0).sample(IDMAPS, torch.Generator().manual_seed(0))
    assert never.source == (-1,) * 4
    always = CopyPaste(prob=1.0, select=1.0).sample(IDMAPS[:3], torch.Generator().manual_seed(0))
    for b in range(3):
        s = always.source[b]
        assert s not in (-1, b)
        assert always.selected[b] == tuple(i for i in sorted(IDMAPS[s]) if i <= 254)  # 255 and 300 are no instances
    weeds = CopyPaste(prob=1.0, select=1.0, classes=(1,)).sample(IDMAPS[:3], torch.Generator().manual_seed(0))
    for b in range(3):
        if weeds.source[b] >= 0:
            assert all(IDMAPS[weeds.source[b]][i] == 1 for i in weeds.selected[b])
    capped = CopyPaste(prob=1.0, select=1.0, max_instances=1).sample(IDMAPS[:3], torch.Generator().manual_seed(0))
    assert all(len(s) <= 1 for s in capped.selected)
    assert CopyPaste(prob=1.0, select=1.0, shift=None).sample(IDMAPS[:3], torch.Generator().manual_seed(5)).shift == ((0, 0),) * 3


@pytest.mark.parametrize("kw", [dict(prob=1.5), dict(select=-0.1), dict(min_visible=2), dict(max_instances=-1),
                                dict(shift=-1), dict(shift=(1, 2, 3)), dict(prob=True)])
def test_recipe_validation(kw):
    with pytest.raises(ValueError):
        CopyPaste(**kw)


# --------------------------------------------------------------------------------------------------- id allocation
def test_free_ids_skip_the_destinations_keys():
    assert allocate_paste_ids((3, 4, 9), {0: 1, 1: 0, 3: 1}) == (2, 4, 5)
    assert allocate_paste_ids((), {0: 1}) == ()
    assert allocate_paste_ids((7,), {"0": 1, "2": 0}) == (1,)


def test_255_is_never_allocated_and_surplus_is_dropped():
    dest = {i: 0 for i in range(251)}
    new = allocate_paste_ids((1, 2, 3, 4, 5, 6), dest)
    assert new == (251, 252, 253, 254)  # four of six: the two highest source ids are not pasted
    assert allocate_paste_ids((1, 2), {i: 0 for i in range(255)}) == ()
    p = CopyPasteParams((1, -1), ((1, 2, 3, 4, 5, 6), ()), (new, ()), ((0, 0), (0, 0)))
    lut = p.lut()
    assert lut.shape == (2, 256) and lut.dtype == np.int32
    assert lut[0, 1:7].tolist() == [251, 252, 253, 254, -1, -1] and (lut[1] == -1).all() and lut[0, 255] == -1


# ---------------------------------------------------------------------------------------------- parameter validation
GOOD = dict(source=(1, -1), selected=((2, 5), ()), new_ids=((0, 2), ()), shift=((0, 0), (3, -2)))


def test_params_normalise():
    p = CopyPasteParams([1, -1], [[2, 5], []], [[0, 2], []], [[0, 0], [3, -2]], 1)
    assert p == CopyPasteParams(**GOOD, min_visible=1.0) and p.fraction() == (1, 1)
    assert CopyPasteParams(**GOOD, min_visible=1 / 3).fraction() == (1, 3)
    assert CopyPasteParams(**GOOD, min_visible=0.3).fraction() == (3, 10)
    assert CopyPasteParams(**GOOD).fraction() == (0, 1)


@pytest.mark.parametrize("change", [
    dict(source=(0, -1)),                       # its own source
    dict(source=(2, -1)),                       # outside the batch
    dict(source=(1,)),                          # lengths
    dict(selected=((5, 2), ())),                # not ascending
    dict(selected=((2, 2), ())),                # repeated
    dict(selected=((2, 255), ())),              # 255 is no instance
    dict(selected=((2, 5), (1,))),              # selected without source
    dict(new_ids=((0, 0), ())),                 # repeated
    dict(new_ids=((0, 255), ())),               # 255 is never an id
    dict(new_ids=((0, 1, 2), ())),              # more than selected
    dict(shift=((0, 0), (1.5, 0))),             # whole pixels only
    dict(shift=((0, 0),)),
    dict(min_visible=1.01), dict(min_visible=-0.1), dict(min_visible="half"),
])
def test_params_validation(change):
    with pytest.raises(ValueError):
        CopyPasteParams(**{**GOOD, **change})


# ---------------------------------------------------------------------------------------------------- compact only
def _batch(compact: bool):
    pv = torch.zeros(2, 3, 4, 4)
    b = {"pixel_values": pv, "mask_labels": [None, None], "class_labels": [None, None], "target_sizes": [(4, 4)] * 2,
         "original_maps": [None, None], "id_mappings": [{1: 0}, {2: 1, 5: 0}], "file_names": ["a", "b"]}
    if compact:
        b["instance_maps"] = [torch.full((4, 4), 255, dtype=torch.uint8)] * 2
    else:
        b["mask_labels"] = [torch.zeros(1, 4, 4), torch.zeros(2, 4, 4)]
        b["class_labels"] = [torch.tensor([0]), torch.tensor([1, 0])]
    return b


def test_mask_stack_batches_are_refused():
    p = CopyPasteParams(**GOOD)
    with pytest.raises(ValueError, match="compact"):
        D.copy_paste(_batch(False), p)
    half = _batch(True)
    half["instance_maps"] = [half["instance_maps"][0], None]
    with pytest.raises(ValueError, match="compact"):
        D.copy_paste(half, p)


def test_host_checks_come_before_the_device():
    with pytest.raises(ValueError, match="CopyPasteParams"):
        D.copy_paste(_batch(True), {"source": (1, -1)})
    with pytest.raises(ValueError, match="already names"):
        D.copy_paste(_batch(True), CopyPasteParams((1, -1), ((2,), ()), ((1,), ()), ((0, 0), (0, 0))))
    with pytest.raises(ValueError, match="not an instance of its source"):
        D.copy_paste(_batch(True), CopyPasteParams((1, -1), ((3,), ()), ((0,), ()), ((0, 0), (0, 0))))
    with pytest.raises(ValueError, match="images"):
        D.copy_paste(_batch(True), CopyPasteParams((-1,), ((),), ((),), ((0, 0),)))


def test_no_cpu_fallback():
    with pytest.raises(_lib.Wm2fError):
        D.copy_paste(_batch(True), CopyPasteParams(**GOOD), device="cpu")


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wm2f.h")).read(), flags=re.S)
    for name, n_args in (("wm2f_copy_paste_select", 12), ("wm2f_copy_paste", 12), ("wm2f_copy_paste_prune", 9)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
    assert "#define WM2F_COPY_PASTE_DESC_LEN %d" % _lib.WM2F_COPY_PASTE_DESC_LEN in src
    from weed_instance_segmentation_amd import _build, ops
    assert "copy_paste.hip" in _build.SOURCES and callable(ops.copy_paste)


# ------------------------------------------------------------------------------- the restatement, two formulations
def test_reference_by_hand():
    """One 4 x 6 case worked out on paper: id 7 of image 1 (a 2 x 2 block) goes to image 0 shifted by (1, 2) as id 1 and
    covers all of instance 3 and half of instance 0."""
    maps = np.full((2, 4, 6), IG, dtype=np.int32)
    maps[0, 1, 2:4] = 3          # two pixels, both covered
    maps[0, 2:4, 3:5] = 0        # four pixels, (2, 3) covered
    maps[0, 0, 0] = -1
    maps[1, 0:2, 0:2] = 7
    maps[1, 3, 5] = 300
    pix = np.arange(2 * 1 * 4 * 6, dtype=np.float32).reshape(2, 1, 4, 6)
    lut = np.full((2, 256), -1)
    lut[0, 7] = 1
    out, new, lut_final, areas = R.copy_paste_reference(pix, maps, [1, -1], lut, [(1, 2), (0, 0)], None, 1, 2, IG)
    want = maps[0].copy()
    want[1:3, 2:4] = 1
    assert np.array_equal(new[0], want) and np.array_equal(new[1], maps[1])
    assert lut_final[0, 7] == 1 and (np.delete(lut_final[0], 7) == -1).all() and (lut_final[1] == -1).all()
    assert areas[0, 0, 3] == 2 and areas[0, 1, 3] == 0 and areas[0, 0, 0] == 4 and areas[0, 1, 0] == 3
    assert areas[0, 0, 1] == 0 and areas[0, 1, 1] == 4 and areas[0, 2, 7] == 4 and areas[0].sum() == 2 + 4 + 3 + 4 + 4
    assert areas[1, 0, 7] == 4 and areas[1, 1, 7] == 4 and areas[1, 2].sum() == 0
    wp = pix[0].copy()
    wp[0, 1:3, 2:4] = pix[1, 0, 0:2, 0:2]
    assert np.array_equal(out[0], wp) and np.array_equal(out[1], pix[1])
    # at 4/5 instance 0 (3 of 4 left) is repainted; at 3/4 it stays
    _, new45, _, _ = R.copy_paste_reference(pix, maps, [1, -1], lut, [(1, 2), (0, 0)], None, 4, 5, IG)
    assert (new45[0][maps[0] == 0] == [1, IG, IG, IG]).all()
    _, new34, _, _ = R.copy_paste_reference(pix, maps, [1, -1], lut, [(1, 2), (0, 0)], None, 3, 4, IG)
    assert np.array_equal(new34[0], want)
    # shifted so that half of the block leaves the window: struck at 3/4, pasted at 1/2
    _, clip, lf, _ = R.copy_paste_reference(pix, maps, [1, -1], lut, [(0, 5), (0, 0)], None, 3, 4, IG)
    assert np.array_equal(clip[0], maps[0]) and lf[0, 7] == -1
    _, clip, lf, ar = R.copy_paste_reference(pix, maps, [1, -1], lut, [(0, 5), (0, 0)], None, 1, 2, IG)
    assert lf[0, 7] == 1 and (clip[0, 0:2, 5] == 1).all() and ar[0, 1, 1] == 2


def test_shift_out_of_the_frame_strikes_everything():
    rng = np.random.default_rng(0)
    maps, dicts = random_maps(rng, 3, 5, 7)
    pix = random_pixels(rng, 3, 3, 5, 7)
    p = cyclic_params(dicts, maps, [(5, 0), (0, -7), (-5, 7)])
    out, new, lut_final, areas = run_reference(pix, maps, p)
    assert np.array_equal(out.view(np.uint32), pix.view(np.uint32)) and np.array_equal(new, maps)
    assert (lut_final == -1).all() and np.array_equal(areas[:, 0], areas[:, 1])


@pytest.mark.parametrize("seed", range(40))
def test_map_formulation_equals_stack_formulation(seed):
    """Seeded random batches: what `expand_labels` would make of the restatement's maps equals the mask-stack
    formulation -- destination masks & ~union, pasted masks appended, empty masks removed -- with the same visibility
    rule, and the pixels are the source's under the union and the destination's elsewhere."""
    rng = np.random.default_rng(1000 + seed)
    H, W = int(rng.integers(1, 14)), int(rng.integers(1, 14))
    maps, dicts = random_maps(rng, 3, H, W, n_ids=int(rng.integers(1, 7)))
    pix = random_pixels(rng, 3, 2, H, W)
    shift = [(int(rng.integers(-H, H + 1)), int(rng.integers(-W, W + 1))) for _ in range(3)]
    window = [(int(rng.integers(0, H + 1)), int(rng.integers(0, W + 1))) for _ in range(3)] if seed % 2 else None
    mv = [0.0, 0.5, 1 / 3, 0.25, 1.0][seed % 5]
    p = cyclic_params(dicts, maps, shift, mv, rng)
    num, den = p.fraction()
    out, new, lut_final, areas = run_reference(pix, maps, p, window)
    for b in range(3):
        s = p.source[b]
        merged = {**dicts[b], **{v: dicts[s][i] for i, v in zip(p.selected[b], p.new_ids[b])}}
        got_masks, got_classes = R.map_to_stacks(new[b], merged, IG)
        dm, _ = R.map_to_stacks(maps[b], dicts[b], IG)
        d_ids = [int(i) for i in np.unique(maps[b]) if i != IG]
        sm, _ = R.map_to_stacks(maps[s], dicts[s], IG)
        s_ids = [int(i) for i in np.unique(maps[s]) if i != IG]
        want = R.copy_paste_stacks(dm, d_ids, sm, s_ids, dict(zip(p.selected[b], p.new_ids[b])), p.shift[b],
                                   (H, W) if window is None else window[b], num, den)
        assert [i for i, _ in want] == [int(i) for i in np.unique(new[b]) if i != IG]
        assert len(want) == len(got_masks)
        for (i, m), g, c in zip(want, got_masks, got_classes):
            assert np.array_equal(m, g) and c == merged[i]
        union = np.zeros((H, W), dtype=bool)
        for i, m in want:
            if i in p.new_ids[b]:
                union |= m
        moved = R.shifted(pix[s], *p.shift[b], 0)
        assert np.array_equal(out[b], np.where(union[None], moved, pix[b]))
        assert areas[b, 1].sum() <= H * W and (areas[b, 0, 255], areas[b, 1, 255], areas[b, 2, 255]) == (0, 0, 0)
