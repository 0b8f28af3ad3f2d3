"""GroupNorm folded into the split convolutions around it: the group statistics from the convolution
epilogues (ops.conv1x1_gn(stats_groups=...), ops.conv3x3_stats), the normalising operand load of the 1x1 kernel
(ops.conv1x1_gn(norm=...)) and the pixel decoder's forward with the route on and off.

The error bound of the statistics.  A workgroup adds in fp32 (u = 2^-24 per rounding), everything after it in fp64:
    in a lane      the 8 stored values of a row tile, one after the other from 0: 7 rounded additions for the sum (0 + v is
                   exact), 8 rounded fused multiply-adds for the squares (the first rounds v^2);
    across lanes   4 additions over the 16 lanes of a DPP row, then log2(cpg / 4) <= 2 over the rows that share a group.
The longest fp32 chain under a value is therefore 7 + 6 = 13 roundings for the sum and 8 + 6 = 14 for the squares, and
|S - S_ref| <= ((1 + u)^d - 1) sum|v| <= (d + 1) u sum|v| (d u < 2^-19; the extra u also covers the fp64 additions of the
wave partials, the atomics and the reference's own fp64 sum, each below 2^-52 sum|v| per addition).  D_SUM and D_SQ are
those d + 1: derived, not fitted."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
D_SUM, D_SQ = 13 + 1, 14 + 1
NT = [256, 256, 256, 128, 64]  # channels of a workgroup tile, per entry of the kernels' configuration table
CPGS = (4, 8, 16)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ternary(shape, g):
    return torch.randint(-1, 2, shape, generator=g, device="cuda").float()


def _ref_stats(out, G):
    """fp64 (sum, sum of squares) and (sum |v|, sum v^2) of the stored output per (image, group)."""
    B = out.shape[0]
    v = out.double().reshape(B, G, -1)
    return torch.stack((v.sum(-1), (v * v).sum(-1)), -1), torch.stack((v.abs().sum(-1), (v * v).sum(-1)), -1)


def _check_stats(stats, out, G, exact, what):
    ref, mag = _ref_stats(out, G)
    assert stats.shape == ref.shape and stats.dtype == torch.float64
    if exact:
        assert torch.equal(stats, ref), what
        return
    err = (stats - ref).abs()
    bound = torch.stack((D_SUM * U * mag[..., 0], D_SQ * U * mag[..., 1]), -1)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst |S - S_ref| / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


def _configs(N):
    return [ci for ci, nt in enumerate(NT) if N % nt == 0]


# ------------------------------------------------------------------------------------------------- statistics, 1x1
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("with_bias", [False, True], ids=["raw", "bias"])
@pytest.mark.parametrize("K,N", [(32, 64), (96, 256)])
def test_conv1x1_statistics(ops, K, N, with_bias, stride, B):
    for hw_i, (H, W) in enumerate([(1, 1), (3, 5), (9, 11), (37, 41)]):
        for family in ("ternary", "randn"):
            if family == "ternary" and K != 32:
                continue  # |v| <= 33, v^2 <= 1089: every fp32 partial of a workgroup (512 values) is an exact integer
            g = _gen(1000 * K + 10 * hw_i + stride + B)
            if family == "ternary":
                x, w = _ternary((B, K, H, W), g), _ternary((N, K, 1, 1), g)
                b = _ternary((N,), g) if with_bias else None
            else:
                x = torch.randn(B, K, H, W, generator=g, device="cuda")
                w = torch.randn(N, K, 1, 1, generator=g, device="cuda") / math.sqrt(K)
                b = torch.randn(N, generator=g, device="cuda") if with_bias else None
            ws = ops.split_weight(w.view(N, K))
            for ci in _configs(N):
                want = ops.conv1x1(x, w, b, stride=stride, w_split=ws, config=ci)
                for cpg in CPGS:
                    G = N // cpg
                    what = f"1x1 K{K} N{N} {H}x{W} s{stride} B{B} {family} cfg{ci} cpg{cpg}"
                    out, stats = ops.conv1x1_gn(x, w, b, stride=stride, w_split=ws, config=ci, stats_groups=G)
                    assert torch.equal(out, want), what
                    _check_stats(stats, out, G, family == "ternary", what)
            if stride == 2 and family == "randn":  # the pixels the stride skips are never read
                xn = torch.full_like(x, float("nan"))
                xn[:, :, ::2, ::2] = x[:, :, ::2, ::2]
                out, stats = ops.conv1x1_gn(xn, w, b, stride=2, w_split=ws, stats_groups=N // 8)
                assert torch.equal(out, ops.conv1x1(x, w, b, stride=2, w_split=ws))
                _check_stats(stats, out, N // 8, False, f"1x1 NaN between the samples {H}x{W}")


# ------------------------------------------------------------------------------------------------- statistics, 3x3
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cin,N", [(32, 64), (96, 192)])
def test_conv3x3_statistics(ops, Cin, N, stride, B):
    for hw_i, (H, W) in enumerate([(1, 1), (2, 3), (17, 1), (33, 31)]):
        for family in ("ternary", "randn"):
            if family == "ternary" and Cin != 32:
                continue
            g = _gen(2000 * Cin + 10 * hw_i + stride + B)
            if family == "ternary":
                # five of the nine taps: |v| <= 5 * 32 = 160, so the 512 squares of a workgroup partial stay below
                # 512 * 25600 < 2^24 and every fp32 partial is an exact integer
                x, w = _ternary((B, Cin, H, W), g), _ternary((N, Cin, 3, 3), g)
                w[:, :, 0::2, 0::2] = 0.0
            else:
                x = torch.randn(B, Cin, H, W, generator=g, device="cuda")
                w = torch.randn(N, Cin, 3, 3, generator=g, device="cuda") / math.sqrt(9 * Cin)
            ws = ops.split_weight_3x3(w)
            for ci in _configs(N):
                want = ops.conv3x3(x, w, stride=stride, w_split=ws, config=ci)
                for cpg in CPGS:
                    G = N // cpg
                    what = f"3x3 C{Cin} N{N} {H}x{W} s{stride} B{B} {family} cfg{ci} cpg{cpg}"
                    out, stats = ops.conv3x3_stats(x, w, G, stride=stride, w_split=ws, config=ci)
                    assert torch.equal(out, want), what
                    _check_stats(stats, out, G, family == "ternary", what)


def test_other_group_sizes_are_refused_before_any_launch(ops):
    """cpg outside {4, 8, 16}: an error through the C ABI; neither the output nor the workspace is touched."""
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    s = ops._stream(torch.zeros(1, device="cuda"))
    N, K = 64, 32
    x = torch.randn(1, K, 8, 8, device="cuda")
    w1, w3 = torch.randn(N, K, device="cuda"), torch.randn(N, K, 3, 3, device="cuda")
    ws1, ws3 = ops.split_weight(w1), ops.split_weight_3x3(w3)
    for G in (32, 2, 1, 64, 5, 0):  # cpg 2, 32, 64, 1; G does not divide N; no groups
        out = torch.full((1, N, 8, 8), 7.0, device="cuda")
        stats = torch.full((max(G, 1), 2), 7.0, device="cuda", dtype=torch.float64)
        rc = lib.wm2f_conv1x1_split_gn_fwd(ops._p(x), ops._p(ws1), ops._p(None), ops._p(out), ops._p(stats), G, ops._p(None),
                                           ops._p(None), ops._p(None), 0, 0.0, 0, 1, K, N, 8, 8, 1, -1, s)
        assert rc != 0
        rc = lib.wm2f_conv3x3_split_stats_fwd(ops._p(x), ops._p(ws3), ops._p(out), ops._p(stats), G, 1, K, N, 8, 8, 1, -1, s)
        assert rc != 0
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (stats == 7.0).all()
    assert not ops.conv_group_stats_applies(N, 32) and ops.conv_group_stats_applies(N, 8)


# ------------------------------------------------------------------------------------------------- normalised operand
@pytest.mark.parametrize("relu", [False, True], ids=["affine", "relu"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K,G", [(32, 4), (96, 12), (96, 32)])
def test_conv1x1_normalised_operand(ops, K, G, B, relu):
    """One shared workspace: the fused call against the apply pass on a copy followed by ops.conv1x1, bit for bit; then
    a NaN in x."""
    N, eps = 64, 1e-5
    for hw_i, (H, W) in enumerate([(1, 1), (9, 11), (37, 41)]):
        g = _gen(3000 * K + 100 * G + 10 * hw_i + B)
        x = torch.randn(B, K, H, W, generator=g, device="cuda") * 3.0 + 0.5
        w = torch.randn(N, K, 1, 1, generator=g, device="cuda") / math.sqrt(K)
        b = torch.randn(N, generator=g, device="cuda")
        gamma = torch.randn(K, generator=g, device="cuda")
        beta = torch.randn(K, generator=g, device="cuda")
        stats, _ = _ref_stats(x, G)  # the workspace both routes read
        ws = ops.split_weight(w.view(N, K))
        for ci in _configs(N):
            two = ops.group_norm_act_from_stats_(x.clone(), stats, G, gamma, beta, eps, relu=relu)
            want = ops.conv1x1(two, w, b, w_split=ws, config=ci)
            got = ops.conv1x1_gn(x, w, b, w_split=ws, config=ci, norm=(stats, G, gamma, beta, eps, relu))
            assert torch.equal(got, want), (K, G, H, W, B, relu, ci)
        # a NaN in x, the workspace unchanged: fmaxf maps it to 0 under the ReLU; without it exactly that pixel's outputs
        bi, hi, wi = B - 1, H // 2, W // 3
        xn = x.clone()
        xn[bi, K // 2, hi, wi] = float("nan")
        got = ops.conv1x1_gn(xn, w, b, w_split=ws, norm=(stats, G, gamma, beta, eps, relu))
        two = ops.group_norm_act_from_stats_(xn.clone(), stats, G, gamma, beta, eps, relu=relu)
        assert torch.equal(got.isnan(), ops.conv1x1(two, w, b, w_split=ws).isnan())
        expect = torch.zeros_like(got, dtype=torch.bool)
        if not relu:
            expect[bi, :, hi, wi] = True
        assert torch.equal(got.isnan(), expect), (K, G, H, W, B, relu)


def test_apply_only_passes_match_the_passes_with_statistics(ops):
    """The apply-only entry points from the workspace a convolution epilogue filled, against the two-launch entry points
    on the same map (the statistics differ by fp32 partial sums and fp64 order only)."""
    g = _gen(7)
    B, K, N, H, W, G = 2, 64, 64, 12, 20, 8
    x = torch.randn(B, K, H, W, generator=g, device="cuda")
    w = torch.randn(N, K, 1, 1, generator=g, device="cuda") / 8.0
    b = torch.randn(N, generator=g, device="cuda")
    gamma, beta = torch.randn(N, generator=g, device="cuda"), torch.randn(N, generator=g, device="cuda")
    up = torch.randn(B, N, H // 2, W // 2, generator=g, device="cuda")
    out, stats = ops.conv1x1_gn(x, w, b, stats_groups=G)
    for relu, u in ((True, None), (False, up)):
        got = ops.group_norm_act_from_stats_(out.clone(), stats, G, gamma, beta, 1e-5, up=u, relu=relu)
        want = ops.group_norm_act_(out.clone(), G, gamma, beta, 1e-5, up=u, relu=relu)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    tok = torch.zeros(B, H * W + 8, N, device="cuda")
    tok2 = torch.zeros_like(tok)
    ops.group_norm_tokens_from_stats_(out, stats, None, G, gamma, beta, 1e-5, tok, 4)
    ops.group_norm_tokens_(ops.conv1x1(x, w), b, G, gamma, beta, 1e-5, tok2, 4)
    torch.testing.assert_close(tok, tok2, rtol=1e-5, atol=1e-5)
    assert (tok[:, :4] == 0).all() and (tok[:, 4 + H * W:] == 0).all()


# ------------------------------------------------------------------------------------------------- end to end
# Routes on and off differ by roundings at the last bit of fp32: the fp32 partial sums of the statistics are cut differently
# (relative D u on a sum), the input projections add their bias before the affine map instead of inside its shift, and the
# fp64 atomics land in another order.  Each moves a normalised tensor by about one ulp of its largest value, so the
# yardstick is max(|old - old'|, 2^-23 max|old|): two runs of the old route, floored at one ulp because those two runs
# are often bit-identical (fp64 sums of a few hundred fp32 partials are mostly exact in any order).  MARGIN = 64 lets that
# ulp grow by 4 through each post-norm encoder layer (two in the decoder below, one LayerNorm-bounded residual block
# each; the tiny model's route does not change at all, see the test) times 4 for the four sources above.
MARGIN = 64.0


def _compare(new, old, old2, what):
    for k, (a, r, r2) in enumerate(zip(new, old, old2)):
        yard = max((r - r2).abs().max().item(), 2.0 ** -23 * r.abs().max().item())
        d = (a - r).abs().max().item()
        print(f"{what}[{k}]: |new - old| = {d:.3e}, yardstick {yard:.3e}, ratio {d / yard:.2f}")
        assert torch.isfinite(a).all() and d <= MARGIN * yard, (what, k, d, yard)


def test_tiny_model_forward_route_on_and_off(ops):
    """The tiny model of tests/test_model_gpu.py.  Its GroupNorms have 2 channels per group, so every predicate fails and
    the forward must take the old route whichever way the switch stands."""
    import json
    import numpy as np
    from conftest import load_golden
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    gold = load_golden("full_tiny.npz")
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig.from_dict(json.loads(str(gold["config_json"]))))
    model.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in gold.items() if k.startswith("sd.")}, strict=True)
    model = model.cuda().eval()
    x = torch.from_numpy(gold["pixel_values"]).cuda()

    def run():
        with torch.no_grad():
            o = model(pixel_values=x)
        return [o.masks_queries_logits, o.class_queries_logits, o.pixel_decoder_last_hidden_state]

    assert ops.CONV_GN_FUSED is True
    new = run()
    ops.CONV_GN_FUSED = False
    try:
        old, old2 = run(), run()
    finally:
        ops.CONV_GN_FUSED = True
    _compare(new, old, old2, "tiny model")


def test_pixel_decoder_forward_route_on_and_off(ops, monkeypatch):
    """A pixel decoder at the benchmark's widths (256 features in 32 groups: 8 channels per group) on small maps, where
    every one of the six sites takes the new route; the calls are counted to prove it."""
    from weed_instance_segmentation_amd import Mask2FormerConfig
    from weed_instance_segmentation_amd.modeling import Mask2FormerPixelDecoder
    torch.manual_seed(0)
    cfg = Mask2FormerConfig(num_labels=3, encoder_layers=2)
    dec = Mask2FormerPixelDecoder(cfg, [256, 512, 1024, 2048]).cuda().eval()
    with torch.no_grad():
        for m in dec.modules():  # non-trivial affine maps
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)
    g = _gen(11)
    feats = [torch.randn(2, c, s, s, generator=g, device="cuda") for c, s in ((256, 32), (512, 16), (1024, 8), (2048, 4))]
    calls = {"conv1x1_gn": 0, "conv3x3_stats": 0, "group_norm_act_": 0, "group_norm_tokens_": 0}
    for name in calls:
        def counted(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, counted)

    def run():
        with torch.no_grad():
            mask, outs = dec(feats)
        return [mask, *outs]

    new = run()
    assert calls == {"conv1x1_gn": 5, "conv3x3_stats": 1, "group_norm_act_": 0, "group_norm_tokens_": 0}, calls
    monkeypatch.setattr(ops, "CONV_GN_FUSED", False)
    old, old2 = run(), run()
    assert calls == {"conv1x1_gn": 5, "conv3x3_stats": 1, "group_norm_act_": 4, "group_norm_tokens_": 6}, calls
    _compare(new, old, old2, "pixel decoder")
