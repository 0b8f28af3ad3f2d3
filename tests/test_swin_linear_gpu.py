"""ops.swin_linear (csrc/swin_linear_split.hip) on the GPU: the Swin backbone's Linears on the split-bf16
kernel, against fp64 references at the three precision levels, bit for bit across tile configurations, row positions and
row cuts, with non-finite tokens, through the 2 GiB row cut, inside SwinBackbone and inside a captured HIP graph.

The accuracy rule is the project's (tests/split_gemm_cases.py, tests/split_precision_reference.py):
    e <= 2 e32 + floor(level),   e = max |out - ref64| / (sum_k |x_k w_k| + |b| + |r|),
e32 the same measure of the stock fp32 chain on the GPU (torch.addmm, then F.gelu or the add).  For the GELU epilogue the
denominator is that of the value the GELU is applied to: |gelu'| <= 1.13, and the comparator goes through the same function.

Shapes.  The token tiles of the table are 256 and 64 tokens, the feature tiles 128 and 96 features: M in {1, 15, 16, 17, 33,
65, 257, 256 CUs + 17}, K in {32, 96, 160} (one k-step, an odd count, a count that leaves the two-panel ring on either half),
N in {16, 48, 96, 272} (below a feature tile, the n_out = 3 minimum, one whole 96-wide tile, a partial last tile under both
widths), and three Swin-L shapes with M = 64.

An unaligned view of x (a data pointer that is not a multiple of 16 bytes) is handled, not refused: the op copies it, as
_req copies a strided tensor; test_unaligned_and_strided_views_are_copied holds the result to the aligned call's bits.

The kernel's sum starts from +0 and adds the bias to it, so an `epilogue = 0` output is never -0: the GELU test's values
hold +0, both signs of the smallest normal number, and whatever the subnormal inputs give."""
import json

import pytest
import torch
import torch.nn.functional as F

import split_gemm_cases as S
import split_precision_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPILOGUES = ("bias", "nobias", "gelu", "res", "qkv")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg(ops):
    import weed_instance_segmentation_amd as _pkg
    return _pkg


@pytest.fixture(scope="module")
def n_configs(ops):
    from weed_instance_segmentation_amd._lib import load
    return int(load().wm2f_swin_linear_split_configs())


def _run(ops, x, w, b, epi, r=None, config=-1, w_split=None):
    if epi == "qkv":
        return torch.cat(ops.swin_linear(x, w, b, n_out=3, config=config, w_split=w_split), -1)
    return ops.swin_linear(x, w, None if epi == "nobias" else b, gelu=epi == "gelu", residual=r if epi == "res" else None,
                           config=config, w_split=w_split)


def _ref64(x, w, b, epi, r=None):
    xd, wd = x.double(), w.double()
    y, mag = xd @ wd.t(), xd.abs() @ wd.abs().t()
    if epi != "nobias":
        y, mag = y + b.double(), mag + b.double().abs()
    if epi == "gelu":
        y = F.gelu(y)
    if epi == "res":
        y, mag = y + r.double(), mag + r.double().abs()
    return y, mag


def _fp32(x, w, b, epi, r=None):
    y = x @ w.t() if epi == "nobias" else torch.addmm(b, x, w.t())
    if epi == "gelu":
        y = F.gelu(y)
    if epi == "res":
        y = y + r
    return y


def _case(family, M, K, N, seed):
    x, w, b = S.operands(family, M, K, N, seed)
    r = S.extra((M, N), seed + 1, ints=family == "ints")
    return x.cuda(), S.as_w1x1(w).cuda(), b.cuda(), r.cuda()


# ------------------------------------------------------------------------------------------------------------ accuracy
# fltmax is left out for the GELU, which is not monotone: the existing tests leave it out of such epilogues as well
ACCURACY = [(e, f) for e in EPILOGUES for f in S.FAMILIES if not (e == "gelu" and f == "fltmax")]


@pytest.mark.parametrize("level", R.LEVELS)
@pytest.mark.parametrize("epi,family", ACCURACY)
def test_accuracy_rule_per_family_epilogue_and_level(ops, pkg, epi, family, level):
    x, w, b, r = _case(family, 83, 160, 96, 11)
    ref, mag = _ref64(x, w, b, epi, r)
    with pkg.inference_precision(level):
        out = _run(ops, x, w, b, epi, r)
        again = _run(ops, x, w, b, epi, r)
    assert torch.equal(out, again)
    e, e32 = S.rel_err(out, ref, mag), S.rel_err(_fp32(x, w, b, epi, r), ref, mag)
    print(f"{epi} {family} {level}: e = {e:.3e}, e32 = {e32:.3e}")
    assert R.rule(e, e32, level), (e, e32)


def _ms(ops):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return (1, 15, 16, 17, 33, 65, 257, 256 * n_cu + 17)


@pytest.mark.parametrize("N", [16, 48, 96, 272])
@pytest.mark.parametrize("K", [32, 96, 160])
def test_shapes_accuracy_and_bits_under_every_config(ops, n_configs, K, N):
    """Every M of the list at this (K, N), the epilogues in rotation: the rule at "highest", the same bits twice and under
    every entry of the tile table, and rows of the M-row call equal to 1-row calls on them."""
    epis = [e for e in EPILOGUES if e != "qkv" or N % 48 == 0]
    for i, M in enumerate(_ms(ops)):
        epi = epis[(i + K // 32 + N // 16) % len(epis)]
        x, w, b, r = _case("randn", M, K, N, 100 + i)
        ws = ops.split_weight(w)
        out = _run(ops, x, w, b, epi, r, w_split=ws)
        ref, mag = _ref64(x, w, b, epi, r)
        e, e32 = S.rel_err(out, ref, mag), S.rel_err(_fp32(x, w, b, epi, r), ref, mag)
        print(f"M {M} K {K} N {N} {epi}: e = {e:.3e}, e32 = {e32:.3e}")
        assert S.rule(e, e32), (M, epi, e, e32)
        assert torch.equal(out, _run(ops, x, w, b, epi, r, w_split=ws))
        for c in range(n_configs):
            assert torch.equal(out, _run(ops, x, w, b, epi, r, config=c, w_split=ws)), (M, epi, c)
        for row in sorted({0, M // 2, M - 1}):
            one = _run(ops, x[row:row + 1], w, b, epi, r[row:row + 1], w_split=ws)
            assert torch.equal(one, out[row:row + 1]), (M, epi, row)


@pytest.mark.parametrize("K,N,epi", [(6144, 1536, "res"), (1536, 6144, "gelu"), (3072, 1536, "nobias")],
                         ids=["swin_l_stage4_fc2", "swin_l_stage4_fc1", "swin_l_merge3"])
def test_swin_l_shapes_with_few_tokens(ops, n_configs, K, N, epi):
    x, w, b, r = _case("randn", 64, K, N, 5)
    ws = ops.split_weight(w)
    out = _run(ops, x, w, b, epi, r, w_split=ws)
    ref, mag = _ref64(x, w, b, epi, r)
    e, e32 = S.rel_err(out, ref, mag), S.rel_err(_fp32(x, w, b, epi, r), ref, mag)
    print(f"K {K} N {N} {epi}: e = {e:.3e}, e32 = {e32:.3e}")
    assert S.rule(e, e32), (e, e32)
    for c in range(n_configs):
        assert torch.equal(out, _run(ops, x, w, b, epi, r, config=c, w_split=ws)), c


# ---------------------------------------------------------------------------------------------------------- GELU alone
def test_gelu_instance_applies_to_the_bias_epilogues_value(ops):
    """Where v >= 6, erf(v / sqrt 2) rounds to 1 in fp32 and 0.5 v (1 + 1) is v itself: there the GELU output IS the value
    it was applied to, and it carries the bits of the bias epilogue's output -- the two share the accumulation."""
    x, w, b, _ = _case("randn", 70, 96, 96, 3)
    x, b = x * 16.0, b + 30.0
    v = ops.swin_linear(x, w, b)
    out = ops.swin_linear(x, w, b, gelu=True)
    big = v >= 6.0
    assert big.float().mean().item() > 0.5
    assert torch.equal(out[big], v[big])


def test_gelu_error_on_the_kernels_own_value(ops):
    """eps = max |out_gelu - gelu64(v)| / max(|v|, 2^-126) <= 2 eps_torch + 2^-23, v the kernel's epilogue-0 output on the
    same inputs and eps_torch the same measure of F.gelu(v) in fp32 on the GPU.  x carries the value in column 0 against a
    weight column of ones: the six products of a value with 1 are its three pieces, which sum back to it exactly."""
    tiny = 2.0 ** -126
    special = torch.tensor([0.0, -0.0, tiny, -tiny, tiny / 2, -tiny / 4, 2.0 ** -149, 1e-30, -1e-30, 1e-6, -1e-6, 3.0, -3.0,
                            5.5, -5.5, 5.9, -5.9, 8.0, -8.0, 10.0, -10.0, 12.0, -12.0])
    vals = torch.cat([torch.linspace(-12.0, 12.0, 4001), special])
    M = vals.numel()
    x = torch.zeros(M, 32)
    x[:, 0] = vals
    w = torch.zeros(16, 32)
    w[:, 0] = 1.0
    x, w = x.cuda(), w.cuda()
    v = ops.swin_linear(x, w, None)
    out = ops.swin_linear(x, w, None, gelu=True)
    normal = (vals.abs() >= tiny).cuda()
    assert torch.equal(v[normal][:, 0], vals.cuda()[normal])  # the kernel reproduces every normal value
    assert v.min().item() == -12.0 and v.max().item() == 12.0
    assert (v == 0).any() and (v == tiny).any() and (v == -tiny).any()  # zero and the subnormal edge
    assert (v > 6).any() and (v < -6).any()                              # erf saturated on either side
    den = v.double().abs().clamp_min(tiny)
    ref = F.gelu(v.double())
    eps = ((out.double() - ref).abs() / den).max().item()
    eps_torch = ((F.gelu(v).double() - ref).abs() / den).max().item()
    print(f"gelu: eps = {eps:.3e}, eps_torch = {eps_torch:.3e}")
    assert eps <= 2.0 * eps_torch + 2.0 ** -23, (eps, eps_torch)


# ---------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("epi", EPILOGUES)
def test_rows_cut_into_two_calls_give_the_whole(ops, epi):
    x, w, b, r = _case("randn", 301, 96, 96, 21)
    whole = _run(ops, x, w, b, epi, r)
    for cut in (37, 256, 300):
        parts = [_run(ops, x[:cut], w, b, epi, r[:cut]), _run(ops, x[cut:], w, b, epi, r[cut:])]
        assert torch.equal(torch.cat(parts), whole), cut


def test_unaligned_and_strided_views_are_copied(ops):
    x, w, b, r = _case("randn", 45, 96, 96, 22)
    want = _run(ops, x, w, b, "res", r)
    flat = torch.zeros(x.numel() + 4, device="cuda")
    for off in (1, 2, 3):  # a data pointer 4, 8 and 12 bytes past a 16-byte boundary
        xv = flat[off:off + x.numel()].view_as(x).copy_(x)
        assert xv.data_ptr() % 16 == 4 * off
        assert torch.equal(_run(ops, xv, w, b, "res", r), want)
    bv = torch.zeros(b.numel() + 1, device="cuda")[1:].copy_(b)
    rv = torch.zeros(r.numel() + 1, device="cuda")[1:].view_as(r).copy_(r)
    assert torch.equal(_run(ops, x, w, bv, "res", rv), want)
    wide = torch.zeros(45, 200, device="cuda")
    wide[:, :96] = x
    assert torch.equal(_run(ops, wide[:, :96], w, b, "res", r), want)  # a strided view: _req's copy


@pytest.mark.parametrize("epi", EPILOGUES)
def test_one_piece_is_three_pieces_on_h_rounded_operands(ops, pkg, epi):
    x, w, b, r = _case("randn", 50, 160, 96, 23)
    with pkg.inference_precision("medium"):
        one = _run(ops, x, w, b, epi, r)
    three = _run(ops, R.h_piece(x), R.h_piece(w), b, epi, r)
    assert torch.equal(one, three)


@pytest.mark.parametrize("level", R.LEVELS)
@pytest.mark.parametrize("epi", ["bias", "nobias", "res", "qkv"])
def test_power_of_two_scalings_commute_bit_for_bit(ops, pkg, epi, level):
    x, w, b = S.equivariance_operands(40, 96, 96, 24)
    r = S.floor_at_2_pow_minus_10(S.extra((40, 96), 25))
    x, w, b, r = x.cuda(), S.as_w1x1(w).cuda(), b.cuda(), r.cuda()
    with pkg.inference_precision(level):
        base = _run(ops, x, w, b, epi, r)
        for a_, b_ in S.SCALINGS:
            s = 2.0 ** (a_ + b_)
            got = _run(ops, x * 2.0 ** a_, w * 2.0 ** b_, b * s, epi, r * s)
            assert torch.equal(got, base * s), (a_, b_)


# ---------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("level", R.LEVELS)
@pytest.mark.parametrize("epi", EPILOGUES)
def test_a_non_finite_token_poisons_its_own_outputs_only(ops, pkg, epi, level):
    x, w, b, r = _case("randn", 41, 96, 96, 26)
    with pkg.inference_precision(level):
        clean = _run(ops, x, w, b, epi, r)
        bad = x.clone()
        bad[3, 5], bad[17, 95], bad[40, 0] = float("inf"), float("nan"), float("-inf")
        out = _run(ops, bad, w, b, epi, r)
    rows = torch.zeros(41, dtype=torch.bool, device="cuda")
    rows[[3, 17, 40]] = True
    assert not torch.isfinite(out[rows]).any()
    assert torch.equal(out[~rows], clean[~rows])


@pytest.mark.parametrize("level", R.LEVELS)
def test_flt_max_inputs_stay_finite(ops, pkg, level):
    x, w, b, r = _case("fltmax", 20, 96, 96, 27)
    ref, _ = _ref64(x, w, b, "res", r)
    assert ref.abs().max().item() < S.FLT_MAX  # representable
    with pkg.inference_precision(level):
        for epi in ("bias", "res", "qkv"):
            assert torch.isfinite(_run(ops, x, w, b, epi, r)).all(), epi


# ----------------------------------------------------------------------------------------------------------- 2 GiB cut
@pytest.mark.parametrize("epi", EPILOGUES)
def test_the_row_cut_of_large_operands(ops, monkeypatch, epi):
    from weed_instance_segmentation_amd.ops import gemm
    x, w, b, r = _case("randn", 77, 96, 96, 28)
    whole = _run(ops, x, w, b, epi, r)
    launches = []
    real = gemm._launch
    monkeypatch.setattr(gemm, "_launch", lambda *a, **kw: (launches.append(a[0]), real(*a, **kw))[1])
    monkeypatch.setattr(gemm, "_SWIN_LINEAR_LIMIT", 4 * 96 * 10 + 1)  # ten rows per call
    cut = _run(ops, x, w, b, epi, r, w_split=ops.split_weight(w))
    assert launches.count("wm2f_swin_linear_split_fwd_p") == 8
    assert torch.equal(cut, whole)


def test_argument_errors(ops):
    from weed_instance_segmentation_amd._lib import Wm2fError
    x, w, b, r = _case("randn", 8, 96, 96, 29)
    with pytest.raises(Wm2fError):
        ops.swin_linear(x.clone().requires_grad_(), w, b)
    with torch.no_grad():
        ops.swin_linear(x.clone().requires_grad_(), w, b)
    with pytest.raises(ValueError):
        ops.swin_linear(x, w, b, gelu=True, residual=r)
    with pytest.raises(ValueError):
        ops.swin_linear(x, w, b, gelu=True, n_out=3)
    with pytest.raises(ValueError):
        ops.swin_linear(x, w, b, w_split=torch.zeros(10, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.swin_linear(x[:, :48], w[:, :48], b)  # K = 48
    with pytest.raises(Wm2fError):
        ops.swin_linear(x, w, b, config=99)
    assert ops.swin_linear_applies(x, w) and ops.swin_linear_applies(x, w, 3) and not ops.swin_linear_applies(x, w[:72], 3)


# ------------------------------------------------------------------------------------------------------------ backbone
def _fixture_backbone():
    from weed_instance_segmentation_amd.backbone_swin import SwinBackbone
    g = load_golden("swin_tiny_backbone.npz")
    cfg = json.loads(str(g["config_json"]))
    m = SwinBackbone(cfg)
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    return g, cfg, m.cuda()


def _count(monkeypatch, ops):
    calls = []
    real = ops.swin_linear

    def counted(*a, **kw):
        calls.append(tuple(a[1].shape))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "swin_linear", counted)
    return calls


def test_backbone_routes_23_linears_and_meets_the_fixture(ops, monkeypatch):
    g, cfg, m = _fixture_backbone()
    m.eval()
    monkeypatch.setattr(ops, "SWIN_LINEAR_SPLIT", True)
    calls = _count(monkeypatch, ops)
    keys = list(m.state_dict())
    for tag in ("a", "b"):
        del calls[:]
        with torch.no_grad():
            fm = m(torch.from_numpy(g[f"x_{tag}"]).cuda())
        assert len(calls) == 23  # the five 32 / 64 / 128-wide layers x 4, three reductions; the 16-wide stage is not routed
        assert all(K % 32 == 0 for _, K in calls)
        for i, f in enumerate(fm):
            torch.testing.assert_close(f.cpu(), torch.from_numpy(g[f"fm_{tag}_{i}"]), rtol=1e-4, atol=1e-4)
    assert list(m.state_dict()) == keys and all("swin_" not in k for k in keys)
    monkeypatch.setattr(ops, "SWIN_LINEAR_SPLIT", False)
    del calls[:]
    with torch.no_grad():
        m(torch.from_numpy(g["x_a"]).cuda())
    assert not calls


def test_backbone_flag_as_levels(ops, pkg, monkeypatch):
    g, cfg, m = _fixture_backbone()
    m.eval()
    x = torch.from_numpy(g["x_a"]).cuda()
    calls = _count(monkeypatch, ops)
    monkeypatch.setattr(ops, "SWIN_LINEAR_SPLIT", ("high",))
    with torch.no_grad():
        m(x)
        assert not calls
        with pkg.inference_precision("high"):
            m(x)
    assert len(calls) == 23


def test_backbone_autocast_training_and_frozen_routes(ops, monkeypatch):
    g, cfg, m = _fixture_backbone()
    monkeypatch.setattr(ops, "SWIN_LINEAR_SPLIT", True)
    calls = _count(monkeypatch, ops)
    x = torch.from_numpy(g["x_a"]).cuda()
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        m(x)
    assert not calls
    m.train()
    sum(f.square().mean() for f in m(x)).backward()
    assert not calls
    grads = [p.grad for n, p in m.named_parameters() if not n.startswith("swin.layernorm.")]
    assert all(gr is not None and torch.isfinite(gr).all() for gr in grads)
    m.eval()
    for p in m.parameters():
        p.requires_grad_(False)
    m(x)  # frozen backbone, grad mode on: nothing to record
    assert len(calls) == 23


def test_backbone_sees_weight_updates(ops, monkeypatch):
    from weed_instance_segmentation_amd.derived import drop_derived
    monkeypatch.setattr(ops, "SWIN_LINEAR_SPLIT", True)
    g, cfg, m = _fixture_backbone()
    m.eval()
    x = torch.from_numpy(g["x_a"]).cuda()
    blk = m.swin.encoder.layers[1].blocks[0]

    def fresh(edit):
        _, _, f = _fixture_backbone()
        f.eval()
        with torch.no_grad():
            edit(f.swin.encoder.layers[1].blocks[0])
            return f(x)

    with torch.no_grad():
        before = m(x)
        blk.attention.o_proj.weight.mul_(2)  # a _version bump
        blk.attention.k_proj.bias.add_(0.5)  # the merged bias follows its sources
        after = m(x)
    want = fresh(lambda b: (b.attention.o_proj.weight.mul_(2), b.attention.k_proj.bias.add_(0.5)))
    assert all(torch.equal(a, b) for a, b in zip(after, want)) and not torch.equal(after[-1], before[-1])
    blk.mlp.fc1.weight.data.mul_(2)  # no key sees a write through .data
    drop_derived(m)
    with torch.no_grad():
        after = m(x)
    want = fresh(lambda b: (b.attention.o_proj.weight.mul_(2), b.attention.k_proj.bias.add_(0.5), b.mlp.fc1.weight.mul_(2)))
    assert all(torch.equal(a, b) for a, b in zip(after, want))


def test_inference_precision_reaches_the_backbone(ops, pkg, monkeypatch):
    monkeypatch.setattr(ops, "SWIN_LINEAR_SPLIT", True)
    g, cfg, m = _fixture_backbone()
    m.eval()
    x = torch.from_numpy(g["x_a"]).cuda()
    level = pkg.get_inference_precision()
    with torch.no_grad():
        hi = m(x)
        with pkg.inference_precision("medium"):
            med = m(x)
        assert pkg.get_inference_precision() == level
        assert not torch.equal(med[-1], hi[-1])
        assert all(torch.equal(a, b) for a, b in zip(m(x), hi))
        monkeypatch.setattr(ops, "SWIN_LINEAR_SPLIT", False)
        with pkg.inference_precision("medium"):
            stock_med = m(x)
        stock = m(x)
    assert all(torch.equal(a, b) for a, b in zip(stock_med, stock))  # the stock route has no levels


def test_graph_capture_replays_to_eager(ops, monkeypatch):
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    from weed_instance_segmentation_amd.graph import GraphedForward
    monkeypatch.setattr(ops, "SWIN_LINEAR_SPLIT", True)
    cd = json.loads(str(load_golden("full_tiny.npz")["config_json"]))
    cd["backbone_config"] = {"model_type": "swin", "embed_dim": 32, "depths": [1, 1, 2, 1], "num_heads": [1, 2, 4, 8],
                             "window_size": 4, "mlp_ratio": 2.0, "patch_size": 4, "num_channels": 3,
                             "out_features": ["stage1", "stage2", "stage3", "stage4"], "drop_path_rate": 0.0}
    torch.manual_seed(3)
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig.from_dict(cd)).cuda().eval()
    x1 = torch.randn(2, 3, 72, 104, device="cuda")  # 18 x 26 tokens: padding on both axes
    x2 = torch.randn_like(x1)
    calls = _count(monkeypatch, ops)
    fwd = GraphedForward(model, x1)
    assert calls
    for x in (x1, x2, x1):
        out = fwd(x)
        with torch.no_grad():
            ref = model(pixel_values=x)
        scale = ref.masks_queries_logits.abs().max().item()
        assert (out.masks_queries_logits - ref.masks_queries_logits).abs().max().item() / scale < 1e-5
