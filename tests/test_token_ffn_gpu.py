"""The encoder's feed-forward pair as one kernel (csrc/token_gemm_split.hip, wm2f_token_ffn_split_fwd):
    out, out + pos = LayerNorm(relu(x W1^T + b1) W2^T + b2 + residual)
with the (M, F) intermediate kept in registers.  The reference of every bit-for-bit check is the two-launch route it
replaces (wm2f_token_linear_split_fwd twice): by construction both feed identical operands to identical MFMA sequences.

Token counts, by the CU count C (one persistent workgroup per CU while there are tiles, 8 waves, one 16-token tile per wave
and turn): one tile, fewer tiles than waves, a ragged last tile, one more tile than CUs, several turns with uneven shares.
F = 256, 512, 1024: one, two and four slices of hidden features.  pos absent, with one row per token, and with 17 rows."""
import functools
import math

import pytest
import torch

import split_gemm_cases as S

pytestmark = pytest.mark.gpu

M_FORMS = {
    "1": lambda C: 1,
    "16": lambda C: 16,
    "17": lambda C: 17,
    "16*8+3": lambda C: 16 * 8 + 3,
    "16C-11": lambda C: 16 * C - 11,
    "16(C+1)": lambda C: 16 * (C + 1),
    "16(8C+1)": lambda C: 16 * (8 * C + 1),
    "16(16C+3)-5": lambda C: 16 * (16 * C + 3) - 5,
}
FS = (256, 512, 1024)
CASES = [(m, F) for m in M_FORMS for F in FS]
D = 256
EXTRA_ROWS = 16 * 3
POS_SHORT = 17
CHUNK = 16 * 7 + 3
EPS = 1e-5
VARIANTS = ("none", "m", "s")  # pos absent, one row per token, POS_SHORT rows


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def n_cu(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=2)
def _case(family, M, F):
    """Inputs of M + EXTRA_ROWS tokens on the device (the run at M takes the first M rows), computed once per case:
    x, w1, b1, w2, b2, gamma, beta, residual, pos with one row per token, pos with POS_SHORT rows.
    family "onehot" is "ints" with W2[n, (37 n + 5) mod F] = 1 and zero elsewhere."""
    Mx = M + EXTRA_ROWS
    seed = 11 * M + F
    ints = family in ("ints", "onehot")
    x, w1, b1 = S.operands("ints" if ints else family, Mx, D, F, seed)
    _, w2, b2 = S.operands("ints" if ints else "randn", 1, F, D, seed + 10)
    w1, w2 = S.as_w1x1(w1), S.as_w1x1(w2)
    if family == "onehot":
        w2 = torch.zeros(D, F)
        w2[torch.arange(D), (37 * torch.arange(D) + 5) % F] = 1.0
    gamma, beta = S.extra((D,), seed + 1), S.extra((D,), seed + 2)
    r, pos_m, pos_s = S.extra((Mx, D), seed + 3, ints), S.extra((Mx, D), seed + 4, ints), S.extra((POS_SHORT, D), seed + 5, ints)
    return tuple(t.cuda() for t in (x, w1, b1, w2, b2, gamma, beta, r, pos_m, pos_s))


def _ffn(x, w1s, b1, w2s, b2, r, gamma, beta, pos=None, K=D, F=None, N=D, out=None, out_pos=None):
    """The fused kernel through the C ABI (any pos_rows): out, or (out, out + pos[token % pos_rows])."""
    from weed_instance_segmentation_amd.ops._core import _launch, _p
    M = x.shape[0]
    x = x.contiguous()
    r = None if r is None else r.contiguous()
    out = torch.empty(M, D, device=x.device) if out is None else out
    if pos is not None:
        pos = pos.contiguous()
        out_pos = torch.empty_like(out) if out_pos is None else out_pos
    _launch("wm2f_token_ffn_split_fwd", x, _p(x), _p(w1s), _p(b1), _p(w2s), _p(b2), _p(r), _p(gamma), _p(beta), _p(pos), _p(out),
            _p(out_pos), M, K, b1.numel() if F is None else F, N, 0 if pos is None else pos.shape[0], EPS)
    return out if pos is None else (out, out_pos)


def _two(x, w1p, b1, w2s, b2, r, gamma, beta, pos=None):
    """The two launches the kernel replaces, through the C ABI: fc1 + ReLU, then fc2 + residual + LayerNorm (+ pos)."""
    from weed_instance_segmentation_amd.ops._core import _launch, _p
    M, F = x.shape[0], b1.numel()
    x, r = x.contiguous(), r.contiguous()
    h = torch.empty(M, F, device=x.device)
    _launch("wm2f_token_linear_split_fwd", x, _p(x), _p(w1p), _p(b1), _p(None), _p(None), _p(None), _p(None), _p(h), _p(None),
            M, D, F, 1, 0, 0.0, 0)
    out = torch.empty(M, D, device=x.device)
    out_pos = torch.empty_like(out) if pos is not None else None
    if pos is not None:
        pos = pos.contiguous()
    _launch("wm2f_token_linear_split_fwd", h, _p(h), _p(w2s), _p(b2), _p(r), _p(gamma), _p(beta), _p(pos), _p(out), _p(out_pos),
            M, F, D, 0, 0 if pos is None else pos.shape[0], EPS, 0)
    return out if pos is None else (out, out_pos)


def _splits(ops, case):
    """(W1 in the fused kernel's row order, W1 plain, W2 plain) as split weights."""
    w1, w2 = case[1], case[3]
    return ops.split_weight_rows(w1, ops.ROWS_FFN), ops.split_weight(w1), ops.split_weight(w2)


def _runs(fn, case, w1s, w2s, lo, hi):
    """fn (_ffn or _two) on rows lo .. hi of the case with every pos variant: {"none": out, "m": out, "m+": out + pos, ...}."""
    xx, _, b1, _, b2, gamma, beta, rr, pos_m, pos_s = case
    x, r = xx[lo:hi], rr[lo:hi]
    outs = {"none": fn(x, w1s, b1, w2s, b2, r, gamma, beta)}
    outs["m"], outs["m+"] = fn(x, w1s, b1, w2s, b2, r, gamma, beta, pos=pos_m[lo:hi])
    # row t of the whole run takes pos_s[t % POS_SHORT]: a chunk that starts at lo sees the table rotated by lo
    rot = pos_s[(torch.arange(POS_SHORT, device=pos_s.device) + lo) % POS_SHORT]
    outs["s"], outs["s+"] = fn(x, w1s, b1, w2s, b2, r, gamma, beta, pos=rot)
    return outs


def _max_diff(a, b):
    return (a.double() - b.double()).abs().max().item()


# ------------------------------------------------------------------------------------------------------ 1. permutation
@pytest.mark.parametrize("m_form,F", CASES)
def test_row_map_on_exact_integers(ops, n_cu, m_form, F):
    """Small-integer x and W1 with all rows distinct, one-hot W2, integer b2 and residual: every partial sum is exact, so
    an error in the row map, the bias map or the slice order moves an output of fc2 by whole units.  Both outputs equal
    the two-launch route bit for bit, and W1 with its rows reversed gives something else."""
    M = M_FORMS[m_form](n_cu)
    case = _case("onehot", M, F)
    w1 = case[1]
    assert torch.unique(w1, dim=0).shape[0] == F  # all rows distinct
    w1f, w1p, w2s = _splits(ops, case)
    fused, two = _runs(_ffn, case, w1f, w2s, 0, M), _runs(_two, case, w1p, w2s, 0, M)
    for name in fused:
        assert fused[name].shape == (M, D) and torch.isfinite(fused[name]).all()
        assert torch.equal(fused[name], two[name]), (name, M, F, _max_diff(fused[name], two[name]))
    # the fp64 value of what the LayerNorm normalises is an exact integer: the fused result sits on its LayerNorm
    x, b1, w2, b2, gamma, beta, r = case[0][:M], case[2], case[3], case[4], case[5], case[6], case[7][:M]
    h, _, _ = S.token_ref(x, w1, b1, relu=True)
    ref, _, _ = S.token_ref(h, w2, b2, residual=r, ln=(gamma, beta, EPS))
    assert _max_diff(fused["none"], ref) <= 3e-6 * ref.abs().max().item() * math.sqrt(F)
    rev = _ffn(x, ops.split_weight_rows(w1.flip(0).contiguous(), ops.ROWS_FFN), b1, w2s, b2, r, gamma, beta)
    assert not torch.equal(rev, fused["none"]), (M, F)


# --------------------------------------------------------------------------------------------------------- 2. accuracy
@pytest.mark.parametrize("m_form,F", CASES)
def test_values_against_fp64(ops, n_cu, m_form, F):
    """randn and small integers against the fp64 chain (token_ref twice, ReLU in between) under the LayerNorm rule of
    test_token_gemm_overlap_gpu.py, e <= 2 e32 + 1e-6 with e32 from the same chain through token_fp32, and
    e <= 3e-6 max|ref| sqrt(F)."""
    M = M_FORMS[m_form](n_cu)
    for family in ("randn", "ints"):
        case = _case(family, M, F)
        xx, w1, b1, w2, b2, gamma, beta, rr, _, _ = case
        x, r = xx[:M], rr[:M]
        lnp = (gamma, beta, EPS)
        w1f, _, w2s = _splits(ops, case)
        outs = _runs(_ffn, case, w1f, w2s, 0, M)
        h, _, _ = S.token_ref(x, w1, b1, relu=True)
        ref, _, _ = S.token_ref(h, w2, b2, residual=r, ln=lnp)
        h32 = S.token_fp32(ops, x, w1, b1, relu=True)
        out32 = S.token_fp32(ops, h32, w2, b2, residual=r, ln=lnp)
        e32 = _max_diff(out32, ref)
        for name in VARIANTS:
            out = outs[name]
            e = _max_diff(out, ref)
            print(f"token ffn {name} M={M} F={F} {family}: e {e:.3e} e32 {e32:.3e}")
            assert torch.isfinite(out).all()
            assert e <= 2 * e32 + 1e-6, (name, M, F, family, e, e32)
            assert e <= 3e-6 * ref.abs().max().item() * math.sqrt(F), (name, M, F, family, e)


# --------------------------------------------------------------------------------------- 3. against the two-launch route
@pytest.mark.parametrize("m_form,F", CASES)
def test_bits_of_the_two_launch_route(ops, n_cu, m_form, F):
    """Identical operands through identical MFMA sequences: every shape was bit-equal on the first GPU run, so this asserts
    torch.equal."""
    M = M_FORMS[m_form](n_cu)
    case = _case("randn", M, F)
    w1f, w1p, w2s = _splits(ops, case)
    fused, two = _runs(_ffn, case, w1f, w2s, 0, M), _runs(_two, case, w1p, w2s, 0, M)
    diffs = {name: _max_diff(fused[name], two[name]) for name in fused}
    print(f"token ffn vs two launches M={M} F={F}: largest difference {max(diffs.values()):.3e} {diffs}")
    for name in fused:
        assert torch.equal(fused[name], two[name]), (name, M, F, diffs[name])


# ------------------------------------------------------------------------------------------------- 4. cuts and repeats
@pytest.mark.parametrize("m_form,F", CASES)
def test_same_bits_however_the_rows_are_cut(ops, n_cu, m_form, F):
    M = M_FORMS[m_form](n_cu)
    case = _case("randn", M, F)
    pos_m, pos_s = case[8], case[9]
    w1f, _, w2s = _splits(ops, case)
    base = _runs(_ffn, case, w1f, w2s, 0, M)
    for i in range(5):
        again = _runs(_ffn, case, w1f, w2s, 0, M)
        for name, out in base.items():
            assert torch.equal(again[name], out), ("repeat", i, name, M, F)
    long = _runs(_ffn, case, w1f, w2s, 0, M + EXTRA_ROWS)  # another tile distribution over workgroups, waves and turns
    for name, out in base.items():
        assert torch.equal(long[name][:M], out), ("prefix", name, M, F)
    parts = [_runs(_ffn, case, w1f, w2s, lo, min(lo + CHUNK, M)) for lo in range(0, M, CHUNK)]
    for name, out in base.items():
        assert torch.equal(torch.cat([p[name] for p in parts]), out), ("chunks", name, M, F)
    # pos changes nothing in `out`, and the second output is one fp32 addition on the first
    rows = torch.arange(M, device=pos_s.device)
    assert torch.equal(base["m"], base["none"]) and torch.equal(base["s"], base["none"])
    assert torch.equal(base["m+"], base["none"] + pos_m[:M]), (M, F)
    assert torch.equal(base["s+"], base["none"] + pos_s[rows % POS_SHORT]), (M, F)


# ------------------------------------------------------------------------------------------------------- 5. non-finite
@pytest.mark.parametrize("F", FS)
def test_non_finite_inputs(ops, F):
    M, bad = 16 * 8 + 3, 77
    case = _case("randn", M, F)
    w1f, _, w2s = _splits(ops, case)
    clean = _runs(_ffn, case, w1f, w2s, 0, M)
    xx = case[0].clone()
    xx[bad, 5] = float("nan")
    dirty = _runs(_ffn, (xx,) + case[1:], w1f, w2s, 0, M)
    keep = torch.arange(M, device=xx.device) != bad
    for name in clean:
        assert not torch.isfinite(dirty[name][bad]).any(), name  # the LayerNorm spreads it over the token's row
        assert torch.equal(dirty[name][keep], clean[name][keep]), name  # and no other token sees it
    big = _case("fltmax", M, F)  # FLT_MAX, -FLT_MAX and 3.3961e38 in x against W1 columns at 2^-30
    w1f, _, w2s = _splits(ops, big)
    for name, out in _runs(_ffn, big, w1f, w2s, 0, M).items():
        assert torch.isfinite(out).all(), name


# --------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_untouched(ops):
    from weed_instance_segmentation_amd._lib import Wm2fError
    M = 40
    dev = "cuda"
    x = torch.randn(M, 320, device=dev)
    big = torch.zeros(1024 * 320 * 6, device=dev, dtype=torch.uint8)
    b1, b2, gamma, beta, r = (torch.zeros(n, device=dev) for n in (1024, D, D, D, M * 320))
    pos = torch.zeros(POS_SHORT, D, device=dev)
    calls = {
        "F = 320": dict(F=320),
        "K = 288": dict(K=288),
        "N = 288": dict(N=288),
        "no LayerNorm": dict(gamma=None, beta=None),
        "no residual": dict(r=None),
    }
    for what, kw in calls.items():
        out, out_pos = torch.full((M, 320), 7.0, device=dev), torch.full((M, 320), 7.0, device=dev)
        args = dict(r=r, gamma=gamma, beta=beta, K=D, F=1024, N=D)
        args.update(kw)
        with pytest.raises(Wm2fError):
            _ffn(x, big, b1, big, b2, args["r"], args["gamma"], args["beta"], pos=pos, K=args["K"], F=args["F"], N=args["N"],
                 out=out, out_pos=out_pos)
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (out_pos == 7.0).all(), what
    with pytest.raises(Wm2fError):  # the row-ordered split wants whole blocks of 32 rows
        ops.split_weight_rows(torch.zeros(48, 64, device=dev), ops.ROWS_FFN)
    with pytest.raises(Wm2fError):
        ops.split_weight_rows(torch.zeros(64, 64, device=dev), 2)


def test_row_ordered_split_is_the_split_of_the_permuted_weight(ops):
    w = torch.randn(1024, 256, device="cuda")
    order = ops.ffn_row_order(1024).cuda()
    assert torch.equal(ops.split_weight_rows(w, ops.ROWS_FFN), ops.split_weight(w[order].contiguous()))
    assert torch.equal(ops.split_weight_rows(w, ops.ROWS_NATURAL), ops.split_weight(w))


# ------------------------------------------------------------------------------------------------------------ 7. cache
def test_cached_splits_follow_in_place_weight_updates(ops):
    from weed_instance_segmentation_amd.derived import derived_peek
    torch.manual_seed(3)
    owner = torch.nn.Module()
    fc1, fc2 = torch.nn.Linear(D, 1024).cuda(), torch.nn.Linear(1024, D).cuda()
    ln = torch.nn.LayerNorm(D).cuda()
    x, r = torch.randn(200, D, device="cuda"), torch.randn(200, D, device="cuda")

    def cached():
        with torch.no_grad():
            return ops.token_ffn(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias, r, (ln.weight, ln.bias, ln.eps),
                                 w1_split=ops.split_weight_rows_cached(owner, "fc1_ffn", fc1.weight),
                                 w2_split=ops.split_weight_cached(owner, "fc2", fc2.weight))

    def fresh():
        with torch.no_grad():
            return ops.token_ffn(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias, r, (ln.weight, ln.bias, ln.eps))

    first = cached()
    assert torch.equal(first, fresh())
    kept = derived_peek(owner, "fc1_ffn")
    assert ops.split_weight_rows_cached(owner, "fc1_ffn", fc1.weight) is kept  # no re-split without a change
    for lin in (fc1, fc2):
        before = cached()
        with torch.no_grad():
            lin.weight.mul_(1.5)
        after = cached()
        assert not torch.equal(after, before)
        assert torch.equal(after, fresh())


# ---------------------------------------------------------------------------------------------------------- 8. routing
def test_encoder_layer_routing(ops, monkeypatch):
    from weed_instance_segmentation_amd import Mask2FormerConfig
    from weed_instance_segmentation_amd.modeling import PixelDecoderEncoderLayer, PixelDecoderEncoderOnly
    torch.manual_seed(5)
    cfg = Mask2FormerConfig(num_labels=3)
    assert cfg.feature_size == D and cfg.encoder_feedforward_dim == 1024
    layer = PixelDecoderEncoderLayer(cfg).cuda().eval()
    level_hw = [(8, 8), (4, 4), (2, 2)]
    S_ = sum(h * w for h, w in level_hw)
    hidden, pos = torch.randn(2, S_, D, device="cuda"), torch.randn(S_, D, device="cuda")
    ref = PixelDecoderEncoderOnly.reference_points(level_hw, hidden.device)

    def run(flag):
        monkeypatch.setattr(ops, "TOKEN_FFN_FUSED", flag)
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        try:
            with torch.no_grad():
                out = layer(hidden, pos, ref, level_hw)
            torch.cuda.synchronize()
        finally:
            ops.set_kernel_timer(None)
        return out, {t: len(v) for t, v in timer.records.items()}

    (on, on_pos), tags_on = run(True)
    (off, off_pos), tags_off = run(False)
    two = ("token_linear_K256_N1024", "token_linear_K1024_N256")
    assert tags_on.get("token_ffn_K256_F1024_split") == 1, tags_on
    assert not any(t.startswith(two) for t in tags_on), tags_on
    assert not any(t.startswith("token_ffn") for t in tags_off), tags_off
    assert tags_off.get("token_linear_K256_N1024_split") == 1 and tags_off.get("token_linear_K1024_N256_ln_split") == 1, tags_off
    print(f"encoder layer, fused vs two launches: {_max_diff(on, off):.3e} {_max_diff(on_pos, off_pos):.3e}")
    assert torch.equal(on, off) and torch.equal(on_pos, off_pos)


@pytest.mark.parametrize("level", ["high", "medium"])
def test_lower_precision_levels_give_the_two_launch_bits(ops, n_cu, monkeypatch, level):
    """The kernel is built for one, two and three pieces, so the layer keeps one route at every ops.SPLIT_PRECISION."""
    monkeypatch.setattr(ops, "SPLIT_PRECISION", level)
    for M, F in ((16 * 8 + 3, 512), (16 * (n_cu + 1), 1024)):
        xx, w1, b1, w2, b2, gamma, beta, rr, pos_m, _ = _case("randn", M, F)
        x, r, lnp = xx[:M], rr[:M], (gamma, beta, EPS)
        fused = ops.token_ffn(x, w1, b1, w2, b2, r, lnp, pos=pos_m[:M])
        two = ops.token_linear(ops.token_linear(x, w1, b1, relu=True), w2, b2, residual=r, ln=lnp, pos=pos_m[:M])
        assert torch.equal(fused[0], two[0]) and torch.equal(fused[1], two[1]), (level, M, F)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "SPLIT_PRECISION", "highest")
        full = ops.token_ffn(x, w1, b1, w2, b2, r, lnp, pos=pos_m[:M])
    assert not torch.equal(full[0], fused[0])
