"""Preconditions of the K2 path tests (tests/k2_cases.py, test_k2_paths_gpu.py), checked on the host: every instantiation
the dispatch of csrc/masked_xattn.hip can launch has a table case, by the route function the launchers themselves use; the
route function agrees with what the code states elsewhere; every value family and every mask family has the property it is
named for, under the route of the case that uses it; the stock fp32 route is a meaningful comparator on every value family."""
import math

import pytest
import torch

import k2_cases as K
from k2_cases import (BF16, BF16_BWD, BF16_FWD, BWD_FULL, BWD_GENERAL, F32, FWD_FULL, FWD_GENERAL, UNSUPPORTED)

# (kernel, D, NQT, accumulate): the instantiations the dispatch macros of masked_xattn.hip enumerate -- WM2F_XL in
# wm2f_masked_xattn_fwd (general and full-tile), WM2F_XB in wm2f_masked_xattn_bf16_fwd, WM2F_BD in wm2f_masked_xattn_bwd
# (general with its run-time `accumulate`, full-tile at D = 32) and WM2F_BB in wm2f_masked_xattn_bf16_bwd.
ENUMERATED = [
    (FWD_GENERAL, 16, 1, 0), (FWD_GENERAL, 16, 2, 0), (FWD_GENERAL, 16, 4, 0), (FWD_GENERAL, 16, 7, 0),
    (FWD_GENERAL, 32, 1, 0), (FWD_GENERAL, 32, 2, 0), (FWD_GENERAL, 32, 4, 0), (FWD_GENERAL, 32, 7, 0),
    (FWD_GENERAL, 64, 1, 0), (FWD_GENERAL, 64, 2, 0),
    (FWD_FULL, 16, 1, 0), (FWD_FULL, 16, 2, 0), (FWD_FULL, 16, 4, 0), (FWD_FULL, 16, 7, 0),
    (FWD_FULL, 32, 1, 0), (FWD_FULL, 32, 2, 0), (FWD_FULL, 32, 4, 0), (FWD_FULL, 32, 7, 0),
    (FWD_FULL, 64, 1, 0), (FWD_FULL, 64, 2, 0),
    (BF16_FWD, 32, 1, 0), (BF16_FWD, 32, 2, 0), (BF16_FWD, 32, 4, 0), (BF16_FWD, 32, 7, 0),
    (BWD_GENERAL, 16, 4, 0), (BWD_GENERAL, 16, 7, 0), (BWD_GENERAL, 16, 7, 1),
    (BWD_GENERAL, 32, 4, 0), (BWD_GENERAL, 32, 7, 0), (BWD_GENERAL, 32, 7, 1),
    (BWD_GENERAL, 64, 3, 0), (BWD_GENERAL, 64, 3, 1),
    (BWD_FULL, 32, 4, 0), (BWD_FULL, 32, 7, 0),
    (BF16_BWD, 32, 4, 0), (BF16_BWD, 32, 7, 0),
]

LATTICE = [(B, H, Q, N, D) for B in (1, 2, 6, 32) for H in (1, 2, 8, 26) for Q in (1, 16, 17, 40, 64, 65, 100, 112, 113, 130, 200, 240)
           for N in (1, 16, 37, 80, 256, 464, 528, 656, 1024, 4096) for D in (16, 32, 64)]


def _reached(cases):
    """Instantiations the cases reach with a non-trivial mask, by the route function (not by what the table claims)."""
    got = set()
    for c in cases:
        if c.mask == "none":
            continue
        for backward in ((False, True) if c.bwd is not None else (False,)):
            r = K.case_route(c, backward)
            got.add((r.kernel, c.D, r.nqt, r.accumulate))
    return got


def test_every_instantiation_has_a_case():
    assert sorted(ENUMERATED) == sorted(K.INSTANTIATIONS) and len(set(ENUMERATED)) == len(ENUMERATED)
    got = _reached(K.CASES)
    missing = [i for i in ENUMERATED if i not in got]
    assert not missing, f"no table case reaches {missing}"
    assert got <= set(ENUMERATED), f"the dispatch reaches {got - set(ENUMERATED)}, which the list does not name"
    # the check has teeth: without its full-tile backward cases the table does not pass it
    fewer = [c for c in K.CASES if c.bwd is None or c.bwd.kernel != BWD_FULL]
    assert {(BWD_FULL, 32, 4, 0), (BWD_FULL, 32, 7, 0)} == set(ENUMERATED) - _reached(fewer)


def test_no_shape_reaches_an_instantiation_outside_the_list():
    """The whole lattice, both directions and dtypes: nothing outside ENUMERATED (e.g. 3 query tiles at D = 64 in the
    forward, or an accumulating NQT = 4 backward) is ever launched."""
    names = set(ENUMERATED)
    for B, H, Q, N, D in LATTICE:
        for dtype in (F32, BF16):
            for backward in (False, True):
                for aligned in (True, False):
                    r = K.route(B, H, Q, N, D, dtype, backward, aligned)
                    assert r.kernel == UNSUPPORTED or (r.kernel, D, r.nqt, r.accumulate) in names, (B, H, Q, N, D, dtype, backward, r)


@pytest.mark.parametrize("c", K.CASES, ids=lambda c: c.name)
def test_table_claims_the_route_the_library_takes(c):
    assert K.case_route(c, False) == c.fwd
    if c.bwd is not None:
        assert K.case_route(c, True) == c.bwd
    assert c.values in K.VALUE_FAMILIES and c.mask in K.MASK_FAMILIES
    # every tensor of a case stays small: the largest operand and the fp64 score chunk of the reference
    assert c.B * c.N * c.heads * c.D * 4 <= 32 << 20 and min(c.B, 8) * c.heads * c.Q * c.N * 8 <= 32 << 20


def test_route_function_agrees_with_the_code():
    for B, H, Q, N, D in LATTICE:
        n_tiles, q_tiles = -(-N // 16), -(-Q // 16)
        fwd, odd = K.route(B, H, Q, N, D), K.route(B, H, Q, N, D, aligned=False)
        bwd = K.route(B, H, Q, N, D, backward=True)
        # a mask at an address that is no multiple of 4 takes the general forward; an aligned one the full-tile kernel
        # exactly at whole key tiles
        assert odd.kernel == FWD_GENERAL and odd[1:] == fwd[1:]
        assert fwd.kernel == (FWD_FULL if N % 16 == 0 else FWD_GENERAL)
        assert fwd.nqt in ((1, 2) if D == 64 else (1, 2, 4, 7)) and fwd.accumulate == 0
        assert bwd.nqt == (3 if D == 64 else 4 if q_tiles <= 4 else 7)
        # full-tile backward: exactly D = 32, whole key tiles, one query chunk, at least 8 tiles per split
        assert (bwd.kernel == BWD_FULL) == (D == 32 and N % 16 == 0 and bwd.q_chunks == 1 and bwd.tiles_per_split >= 8)
        assert bwd.kernel in (BWD_FULL, BWD_GENERAL) and bwd.accumulate == int(bwd.q_chunks > 1 and bwd.kernel == BWD_GENERAL)
        for r in (fwd, bwd):
            assert r.n_splits >= 1 and r.n_splits * r.tiles_per_split >= n_tiles > (r.n_splits - 1) * 0
            assert r.q_chunks * r.nqt * 16 >= Q > (r.q_chunks - 1) * r.nqt * 16
            assert r.n_splits <= max(1, -(-n_tiles // K.WAVES))
        # bf16: head_dim 32 and whole key tiles only, aligned operands, the backward up to 112 queries
        for backward in (False, True):
            b16 = K.route(B, H, Q, N, D, BF16, backward)
            ok = D == 32 and N % 16 == 0 and not (backward and Q > 112)
            assert (b16.kernel == (BF16_BWD if backward else BF16_FWD)) if ok else (b16 == K.Route(UNSUPPORTED, 0, 0, 0, 0, 0))
            assert K.route(B, H, Q, N, D, BF16, backward, aligned=False).kernel == UNSUPPORTED
            if ok:  # the same splits as the fp32 kernels, the same chunks as the fp32 forward
                assert b16[2:5] == (bwd if backward else fwd)[2:5]
    # byte offsets beyond 32 bits: the general kernels
    assert K.route(1, 8, 10, 1 << 21, 32).kernel == FWD_GENERAL and K.route(1, 8, 10, (1 << 21) - 16, 32).kernel == FWD_FULL
    assert K.route(32, 8, 10, 1 << 21, 32, backward=True).kernel == BWD_GENERAL
    assert K.route(1, 16, 10, 1 << 21, 32, BF16).kernel == UNSUPPORTED and K.route(1, 8, 10, 1 << 21, 32, BF16).kernel == BF16_FWD
    # refused arguments
    for bad in ((0, 1, 1, 16, 32), (1, 1, 1, 16, 48), (1, 1, 0, 16, 32), (1, 1, 1, 0, 32)):
        assert K.route(*bad).kernel == UNSUPPORTED
    assert K.route(1, 1, 1, 16, 32, dtype=2).kernel == UNSUPPORTED


def _tiles_per_wave(N, rt, split):
    t0, t1 = K.split_tiles(N, rt, split)
    return [len(range(t0 + w, t1, K.WAVES)) for w in range(K.WAVES)]


def test_table_holds_the_edge_cases():
    """A trailing split without tiles in a forward and in a backward case, a wave without a tile, a wave with an odd number
    of tiles (its last half-iteration runs on a tile marked dead), Q % 16 != 0, Q = exactly one full chunk, two chunks."""
    def has(pred, backward):
        return [c.name for c in K.CASES if (c.bwd is not None or not backward) and pred(c, c.bwd if backward else c.fwd)]
    empty = lambda c, r: K.split_tiles(c.N, r, r.n_splits - 1)[0] == K.split_tiles(c.N, r, r.n_splits - 1)[1]
    assert has(empty, False) and has(empty, True)
    idle = lambda c, r: any(0 in _tiles_per_wave(c.N, r, s) for s in range(r.n_splits) if sum(_tiles_per_wave(c.N, r, s)))
    odd = lambda c, r: any(n % 2 == 1 for s in range(r.n_splits) for n in _tiles_per_wave(c.N, r, s))
    for kernel_f, kernel_b in ((FWD_FULL, BWD_FULL), (BF16_FWD, BF16_BWD)):  # the kernels with the two-tile loop body
        assert has(lambda c, r: r.kernel == kernel_f and idle(c, r), False) and has(lambda c, r: r.kernel == kernel_f and odd(c, r), False)
        assert has(lambda c, r: r.kernel == kernel_b and odd(c, r), True)
    # (a full-tile fp32 backward split has at least 8 tiles unless it is the last of more than 8: no idle wave at these sizes)
    assert has(lambda c, r: r.kernel == BF16_BWD and idle(c, r), True)
    assert has(idle, False) and has(lambda c, r: r.kernel == BWD_GENERAL and idle(c, r), True)
    assert has(lambda c, r: c.Q % 16 != 0, False) and has(lambda c, r: c.Q == r.nqt * 16 and r.q_chunks == 1, False)
    assert has(lambda c, r: c.Q == r.nqt * 16 and r.q_chunks == 1, True)
    assert has(lambda c, r: r.q_chunks > 1, False) and has(lambda c, r: r.accumulate == 1, True)
    # every value family and every mask family is used, each on a forward and on a backward kernel
    # (with scores that compete: under single_open p is one-hot, nothing rescales and out is a copy of one v row)
    many = lambda c: c.mask != "single_open"
    for fam in K.VALUE_FAMILIES:
        assert [c for c in K.CASES if c.values == fam and many(c) and c.fwd.kernel == FWD_FULL], fam  # the log2-domain, lazily rescaling one
        if fam != "asc4":
            assert [c for c in K.BACKWARD_CASES if c.values == fam and many(c)], fam
    for fam in ("randn", "wide150", "asc8.5", "offset_v", "outlier"):
        assert [c for c in K.BACKWARD_CASES if c.values == fam and many(c) and c.bwd.kernel == BWD_FULL], fam
    for fam in ("randn", "wide30", "wide150", "asc8.5", "offset_v", "outlier"):
        assert [c for c in K.BACKWARD_CASES if c.values == fam and many(c) and c.bwd.kernel == BWD_GENERAL], fam
    for fam in K.MASK_FAMILIES:
        assert [c for c in K.CASES if c.mask == fam and c.dtype == F32] and [c for c in K.BACKWARD_CASES if c.mask == fam], fam
        if fam != "bernoulli":
            assert [c for c in K.BACKWARD_CASES if c.mask == fam and c.bwd.kernel in (BWD_FULL, BF16_BWD)], fam


# ------------------------------------------------------------------------------------------------------- value families
HOST_SHAPE = (1, 2, 24, 464, 32)  # 29 key tiles


@pytest.mark.parametrize("family", K.VALUE_FAMILIES)
def test_value_family_on_the_host(family):
    """Stock fp32 arithmetic is finite on the family and within 1e-4 (relative Frobenius) of fp64 -- so the comparator of the
    accuracy rule means something there -- and the family has the property it is named for."""
    B, H, Q, N, D = HOST_SHAPE
    q, k, v, go = K.values(family, B, H, Q, N, D, 5)
    m, _ = K.mask("bernoulli", B, Q, N, 6)
    for mm in (None, m):
        ref = K.attention(q, k, v, mm, H, go)
        f32 = K.attention(q, k, v, mm, H, go, dtype=torch.float32)
        for name in ("out", "grad_q", "grad_k", "grad_v"):
            assert torch.isfinite(f32[name]).all() and torch.isfinite(ref[name]).all(), name
        e_out, e_lse = K.fro_err(f32["out"], ref["out"]), K.abs_err(f32["lse"], ref["lse"])
        print(f"k2 host {family} mask {mm is not None}: stock fp32 out {e_out:.2e} lse {e_lse:.2e} "
              + " ".join(f"{n} {K.fro_err(f32[n], ref[n]):.2e}" for n in ("grad_q", "grad_k", "grad_v")))
        assert e_out < 1e-4 and e_lse < 1e-4 * max(1.0, ref["lse"].abs().max().item())
    s = torch.matmul(K._heads(q.double(), H), K._heads(k.double(), H).transpose(-1, -2)) / K.LN2  # log2 units, as the kernel counts
    tile_max = s.view(B, H, Q, N // 16, 16).amax(-1)
    if family.startswith("wide"):
        assert abs(s.std().item() * K.LN2 / float(family[4:]) - 1) < 0.1
    elif family.startswith("asc"):
        step = float(family[3:])
        d1, d4 = tile_max[..., 1:] - tile_max[..., :-1], tile_max[..., 4:] - tile_max[..., :-4]
        assert (d1 - step).abs().max() < 0.4 and (d4 - 4 * step).abs().max() < 0.4
        if step in K.ASCENDING_STEPS:  # neighbouring tiles: both sides of kTau
            assert bool((d1 < K.K_TAU).all()) == (step < K.K_TAU) and bool((d1 > K.K_TAU).all()) == (step > K.K_TAU)
        else:  # a wave's own stride of four tiles: both sides of kTau
            assert bool((d4 < K.K_TAU).all()) == (4 * step < K.K_TAU) and bool((d4 > K.K_TAU).all()) == (4 * step > K.K_TAU)
    elif family.startswith("desc"):
        assert bool((tile_max[..., 1:] < tile_max[..., :-1] - K.K_TAU).all())
    elif family == "outlier":
        top = s.topk(2, -1).values * K.LN2
        assert bool((top[..., 0] - top[..., 1] >= 60).all())
        assert set(s.argmax(-1).flatten().tolist()) == set(K.outlier_keys(N))
    elif family == "uniform":
        ref = K.attention(q, k, v, m, H)
        n_open = (~K.effective_mask(m, B, Q, N)).sum(-1).double()
        assert torch.allclose(ref["lse"], n_open.log()[:, None].expand(B, H, Q), rtol=0, atol=1e-12)
    elif family == "offset_v":
        assert abs(v.mean().item() - 1000) < 1


def test_ascending_steps_straddle_the_lazy_rescale():
    assert sorted(K.ASCENDING_STEPS) == [4.0, 7.5, 8.5, 12.0] and K.K_TAU == 8.0
    assert max(s for s in K.ASCENDING_STEPS if s < K.K_TAU) >= K.K_TAU - 0.5 and min(s for s in K.ASCENDING_STEPS if s > K.K_TAU) <= K.K_TAU + 0.5
    assert [4 * s < K.K_TAU for s in K.ASCENDING_WAVE_STEPS] == [True, False]


# -------------------------------------------------------------------------------------------------------- mask families
def _routes(c):
    return [r for r in (c.fwd, c.bwd) if r is not None]


@pytest.mark.parametrize("c", K.CASES, ids=lambda c: c.name)
def test_mask_family_has_its_property(c):
    q, k, v, go, m, ro = K.case_inputs(c)
    B, Q, N = c.B, c.Q, c.N
    assert q.shape == go.shape == (B, Q, c.heads * c.D) and k.shape == v.shape == (B, N, c.heads * c.D)
    if c.dtype == BF16:
        assert all(torch.equal(t, t.bfloat16().float()) for t in (q, k, v, go))
    if c.mask == "none":
        assert m is None and ro is None
        return
    assert m.shape == (B, Q, N) and m.dtype == torch.bool
    blocked_rows = m.all(-1)
    if c.mask == "no_row_open":
        assert ro is None and not blocked_rows.any()
        return
    assert torch.equal(ro, (~blocked_rows).to(torch.int32))
    n_tiles = -(-N // 16)
    if c.mask == "bernoulli":
        assert blocked_rows[0, 0] and blocked_rows.sum() == 1
    elif c.mask == "blob":
        multi = [r for r in _routes(c) if r.n_splits > 1]
        assert multi and not blocked_rows.any() and (~m).sum(-1).min() >= 2
        for r in multi:  # for some query, every key of a whole non-empty split is blocked; also a whole wave's tiles elsewhere
            dead = [m[:, :, 16 * t0:16 * t1].all(-1) for t0, t1 in (K.split_tiles(N, r, s) for s in range(r.n_splits)) if t1 > t0]
            assert any(bool(d.any()) for d in dead), r
        h, w = K.key_grid(N)
        assert h * w == N
    elif c.mask in ("leading_dead", "trailing_dead"):
        assert K.DEAD_TILES > 2 * K.WAVES and n_tiles > K.DEAD_TILES and not blocked_rows.any()
        dead = slice(0, 16 * K.DEAD_TILES) if c.mask == "leading_dead" else slice(N - 16 * K.DEAD_TILES, N)
        assert m[:, :, dead].all()
        for r in _routes(c):  # some wave meets at least two dead tiles before (after) a live one, or a whole split is dead
            assert r.tiles_per_split > 2 * K.WAVES or r.tiles_per_split <= K.DEAD_TILES, r
    elif c.mask == "single_open":
        assert bool(((~m).sum(-1) == 1).all())
        keys = set((~m).float().argmax(-1).flatten().tolist())
        tps = (c.bwd or c.fwd).tiles_per_split
        want = {0, N - 1, 15, 16} | ({16 * tps - 1, 16 * tps} if 16 * tps < N - 1 else set())
        assert keys == {kk for kk in want if kk < N}, (keys, want)
    elif c.mask == "all_blocked_rows":
        assert blocked_rows[:, 0].all() and blocked_rows[:, Q - 1].all() and not blocked_rows.all()
        assert Q < 32 or blocked_rows[:, 16:32].all()
    else:
        raise AssertionError(c.mask)


def test_a_whole_query_tile_of_blocked_rows_exists():
    assert [c for c in K.BACKWARD_CASES if c.mask == "all_blocked_rows" and c.Q >= 32 and c.bwd.kernel == BWD_FULL]
    assert [c for c in K.BACKWARD_CASES if c.mask == "all_blocked_rows" and c.Q >= 32 and c.bwd.kernel == BWD_GENERAL]


@pytest.mark.parametrize("c", [c for c in K.BACKWARD_CASES if c.mask in K.ZERO_CHECK], ids=lambda c: c.name)
def test_exactly_zero_check_has_keys(c):
    """Every backward case of a family with unattended keys really has some: the reference's grad_k / grad_v rows there are
    exactly zero, which is what the GPU test holds the kernels to."""
    q, k, v, go, m, ro = K.case_inputs(c)
    dead = K.unattended_keys(c, m)
    assert dead is not None and dead.any() and not dead.all(-1).any()
    if c.B * c.heads * c.Q * c.N <= 1 << 22:  # the small ones: the fp64 reference agrees that these rows are zero
        ref = K.attention(q, k, v, m, c.heads, go)
        mags = K.error_scales(q, k, v, m, c.heads, go)
        assert mags["mag_k"].permute(0, 2, 1)[dead].abs().max() == 0 and mags["mag_v"].permute(0, 2, 1)[dead].abs().max() == 0
        for name in ("grad_k", "grad_v"):
            assert ref[name][dead].abs().max() == 0
            # (one open key per row: p is one-hot, dS = p (dP - delta) = 0 and grad_k is zero everywhere)
            assert ref[name][~dead].abs().max() > 0 or (name == "grad_k" and c.mask == "single_open")


def test_measures():
    ref = torch.tensor([[[1.0, 2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]], dtype=torch.float64)  # heads = 2, D = 2
    x = ref.float().clone()
    assert K.fro_err(x, ref) == 0 and K.row_err(x, ref, 2) == 0 and K.abs_err(x, ref) == 0
    x[0, 0, 0] = 1.5
    assert math.isclose(K.row_err(x, ref, 2), 0.25) and math.isclose(K.fro_err(x, ref), 0.5 / math.sqrt(5))
    x[0, 1, 3] = 1e-20  # a nonzero where the reference row is exactly zero
    assert K.row_err(x, ref, 2) == float("inf")
    x[0, 1, 3] = float("nan")
    assert K.fro_err(x, ref) == float("inf") and K.row_err(x, ref, 2) == float("inf") and K.abs_err(x, ref) == float("inf")
    mag = torch.tensor([[[4.0, 4.0], [0.0, 0.0]]], dtype=torch.float64)  # (B, heads, rows): head 0 has terms, head 1 none
    y = ref.float().clone()
    assert K.grad_fro_err(y, ref, mag) == 0 and K.grad_row_err(y, ref, mag) == 0
    y[0, 0, 1] = 3.0
    assert math.isclose(K.grad_row_err(y, ref, mag), 0.25) and math.isclose(K.grad_fro_err(y, ref, mag), 1 / math.sqrt(32))
    y[0, 0, 2] = 1e-20  # a row without terms must be exactly zero
    assert K.grad_row_err(y, ref, mag) == float("inf")
    assert K.rule(1.9e-6, 1e-6) and not K.rule(2.1e-6, 1e-6) and K.rule(9e-7, 0.0) and not K.rule(1.1e-6, 0.0)
    assert K.rule_bf16(1e-3, 1e-3) and not K.rule_bf16(1.01e-3, 1e-3) and not K.rule_bf16(1e-3, 3e-2)
