"""The staged route of the split 3x3 convolution (csrc/conv3x3_split.hip): conv3x3_staged_kernel splits an
8 x 32 pixel tile plus its one-pixel halo once per channel block into LDS and reads the nine taps from there, where the
direct kernel loads and splits every element once per tap.  The MFMAs and their order are the direct kernel's, so the output
must be the direct route's bit for bit -- at every piece count and where non-finite values appear -- and the exact integer
result where the operands are small integers.

The statistics instance is held to the bound of tests/test_conv_groupnorm_fused_gpu.py (derived there: 13 + 1
and 14 + 1 roundings of u = 2^-24 on the sum and on the squares), and is exact for ternary operands at Cin = 32: with five
of the nine taps |v| <= 5 * 32 = 160, so the 512 squares of a workgroup partial stay below 512 * 25600 < 2^24 and every fp32
partial is an exact integer.  At Cin = 64, 96 and 160 five taps would pass 2^24 (512 * (5 * 96)^2), so the ternary weights
keep the centre tap alone there: |v| <= Cin <= 160, the same bound."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TH, TW = 8, 32  # the pixel tile that was built
MAPS = [(1, 1), (2, 3), (17, 1), (1, 17), (TH, TW), (TH + 1, TW + 1), (2 * TH - 1, TW - 1), (3, 2 * TW + 3)]
SHAPES = [(32, 64), (96, 192), (160, 64), (64, 256)]  # one, three, five and two channel blocks
NT = [256, 256, 256, 128, 64]
WN1 = (0, 3, 4)  # the WN = 1 entries of the tile table: (16, 1), (8, 1), (4, 1)
U = 2.0 ** -24
D_SUM, D_SQ = 13 + 1, 14 + 1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _entries(N):
    return [ci for ci in WN1 if N % NT[ci] == 0]


def _ref64(x, w, b, relu):
    """fp64 im2col reference: F.unfold, one matmul, the epilogue."""
    B, C, H, W = x.shape
    N = w.shape[0]
    cols = F.unfold(x.double(), 3, padding=1)  # (B, 9 C, P), row c * 9 + tap
    y = (w.double().reshape(N, C * 9) @ cols).reshape(B, N, H, W)
    if b is not None:
        y = y + b.double()[None, :, None, None]
    return torch.relu(y) if relu else y


def _check_stats(stats, out, G, exact, what):
    B = out.shape[0]
    v = out.double().reshape(B, G, -1)
    ref = torch.stack((v.sum(-1), (v * v).sum(-1)), -1)
    mag = torch.stack((v.abs().sum(-1), (v * v).sum(-1)), -1)
    assert stats.shape == ref.shape and stats.dtype == torch.float64
    if exact:
        assert torch.equal(stats, ref), what
        return
    err = (stats - ref).abs()
    bound = torch.stack((D_SUM * U * mag[..., 0], D_SQ * U * mag[..., 1]), -1)
    assert (err <= bound).all(), (what, (err / bound.clamp_min(1e-300)).max().item())


EPILOGUES = [("raw", False, False), ("bias", True, False), ("bias_relu", True, True)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cin,N", SHAPES)
def test_staged_equals_direct_and_exact_integers(ops, Cin, N, B):
    for mi, (H, W) in enumerate(MAPS):
        g = _gen(100 * Cin + 10 * mi + B)
        xr = torch.randn(B, Cin, H, W, generator=g, device="cuda")
        wr = torch.randn(N, Cin, 3, 3, generator=g, device="cuda") / math.sqrt(9 * Cin)
        br = torch.randn(N, generator=g, device="cuda")
        xi = torch.randint(-3, 4, (B, Cin, H, W), generator=g, device="cuda").float()
        wi = torch.randint(-2, 3, (N, Cin, 3, 3), generator=g, device="cuda").float()
        bi = torch.randint(-4, 5, (N,), generator=g, device="cuda").float()
        wsr, wsi = ops.split_weight_3x3(wr), ops.split_weight_3x3(wi)
        for name, with_bias, relu in EPILOGUES:
            want_r = ops.conv3x3_route(xr, wr, 0, br if with_bias else None, relu, w_split=wsr)
            want_i = _ref64(xi, wi, bi if with_bias else None, relu)  # |sums| <= 9 * 160 * 6 + 4: exact in fp32
            for ci in _entries(N):
                what = f"C{Cin} N{N} {H}x{W} B{B} {name} cfg{ci}"
                got = ops.conv3x3_route(xr, wr, 1, br if with_bias else None, relu, w_split=wsr, config=ci)
                assert torch.equal(got, want_r), what
                assert torch.equal(ops.conv3x3_route(xr, wr, 1, br if with_bias else None, relu, w_split=wsr, config=ci), got), what
                if B > 1:  # a sub-batch gives the same bits
                    sub = ops.conv3x3_route(xr[1:2].contiguous(), wr, 1, br if with_bias else None, relu, w_split=wsr, config=ci)
                    assert torch.equal(sub, got[1:2]), what
                gi = ops.conv3x3_route(xi, wi, 1, bi if with_bias else None, relu, w_split=wsi, config=ci)
                assert torch.equal(gi.double(), want_i), what


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cin,N", SHAPES)
def test_staged_statistics(ops, Cin, N, B):
    for mi, (H, W) in enumerate(MAPS):
        for family in ("ternary", "randn"):
            g = _gen(7000 + 100 * Cin + 10 * mi + B)
            if family == "ternary":
                x = torch.randint(-1, 2, (B, Cin, H, W), generator=g, device="cuda").float()
                w = torch.randint(-1, 2, (N, Cin, 3, 3), generator=g, device="cuda").float()
                if Cin == 32:  # five taps, |v| <= 160: the module docstring
                    w[:, :, 0::2, 0::2] = 0.0
                else:  # more channel blocks: the centre tap alone, |v| <= Cin <= 160, the same bound on a partial
                    centre = w[:, :, 1, 1].clone()
                    w.zero_()
                    w[:, :, 1, 1] = centre
            else:
                x = torch.randn(B, Cin, H, W, generator=g, device="cuda")
                w = torch.randn(N, Cin, 3, 3, generator=g, device="cuda") / math.sqrt(9 * Cin)
            ws = ops.split_weight_3x3(w)
            want = ops.conv3x3_route(x, w, 0, w_split=ws)
            for ci in _entries(N):
                for cpg in (4, 8, 16):
                    what = f"stats C{Cin} N{N} {H}x{W} B{B} {family} cfg{ci} cpg{cpg}"
                    out, stats = ops.conv3x3_stats_route(x, w, N // cpg, 1, w_split=ws, config=ci)
                    assert torch.equal(out, want), what
                    _check_stats(stats, out, N // cpg, family == "ternary", what)


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_inputs_match_the_direct_route(ops, value):
    Cin, N, H, W = 64, 256, 2 * TH + 1, 2 * TW + 1
    g = _gen(5)
    x0 = torch.randn(2, Cin, H, W, generator=g, device="cuda")
    w = torch.randn(N, Cin, 3, 3, generator=g, device="cuda") / math.sqrt(9 * Cin)
    b = torch.randn(N, generator=g, device="cuda")
    ws = ops.split_weight_3x3(w)
    # a map corner, the last pixel of a tile, the first pixel of the tile to its right and of the tile below
    for (h, w_) in [(0, 0), (H - 1, W - 1), (TH - 1, TW - 1), (TH - 1, TW), (TH, TW - 1), (TH, 0)]:
        x = x0.clone()
        x[1, 37, h, w_] = value
        for relu in (False, True):
            want = ops.conv3x3_route(x, w, 0, b, relu, w_split=ws)
            assert not torch.isfinite(want).all()
            for ci in _entries(N):
                got = ops.conv3x3_route(x, w, 1, b, relu, w_split=ws, config=ci)
                assert torch.equal(torch.isnan(got), torch.isnan(want)), (h, w_, relu, ci)
                assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)), (h, w_, relu, ci)


@pytest.mark.parametrize("level", ["high", "medium"])
def test_lower_piece_counts_match_the_direct_route(ops, level, monkeypatch):
    monkeypatch.setattr(ops, "SPLIT_PRECISION", level)
    for Cin, N in SHAPES:
        for mi, (H, W) in enumerate(MAPS):
            g = _gen(9000 + 100 * Cin + mi)
            x = torch.randn(2, Cin, H, W, generator=g, device="cuda")
            w = torch.randn(N, Cin, 3, 3, generator=g, device="cuda") / math.sqrt(9 * Cin)
            b = torch.randn(N, generator=g, device="cuda")
            ws = ops.split_weight_3x3(w)
            want = ops.conv3x3_route(x, w, 0, b, True, w_split=ws)
            want_s, _ = ops.conv3x3_stats_route(x, w, N // 8, 0, w_split=ws)
            for ci in _entries(N):
                assert torch.equal(ops.conv3x3_route(x, w, 1, b, True, w_split=ws, config=ci), want), (level, Cin, N, H, W, ci)
                out, stats = ops.conv3x3_stats_route(x, w, N // 8, 1, w_split=ws, config=ci)
                assert torch.equal(out, want_s), (level, Cin, N, H, W, ci)
                _check_stats(stats, out, N // 8, False, f"{level} C{Cin} N{N} {H}x{W} cfg{ci}")


def test_refusals_launch_nothing_and_leave_the_output_untouched(ops):
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    B, C, H, W = 1, 256, 9, 11
    g = _gen(3)
    x = torch.randn(B, C, H, W, generator=g, device="cuda")
    w = torch.randn(C, C, 3, 3, generator=g, device="cuda")
    ws = ops.split_weight_3x3(w)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for stride, config in ((2, -1), (2, 0), (1, 1), (1, 2)):  # stride 2; the WN > 1 entries (8, 2) and (4, 4)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        out = torch.full((B, C, Ho, Wo), 7.25, device="cuda")
        rc = lib.wm2f_conv3x3_split_fwd_r(p(x), p(ws), None, p(out), B, C, C, H, W, stride, 0, config, 3, 1, stream)
        torch.cuda.synchronize()
        assert rc != 0 and (out == 7.25).all(), (stride, config, rc)
        stats = torch.full((B, 32, 2), -3.5, device="cuda", dtype=torch.float64)
        rc = lib.wm2f_conv3x3_split_stats_fwd_r(p(x), p(ws), p(out), p(stats), 32, B, C, C, H, W, stride, config, 3, 1, stream)
        torch.cuda.synchronize()
        assert rc != 0 and (out == 7.25).all() and (stats == -3.5).all(), (stride, config, rc)
        # the same launch under route 0 and under the rule goes through
        for route in (0, -1):
            rc = lib.wm2f_conv3x3_split_fwd_r(p(x), p(ws), None, p(out), B, C, C, H, W, stride, 0, config, 3, route, stream)
            assert rc == 0, (stride, config, route)
    with pytest.raises(ValueError):
        ops.conv3x3_route(x, w, 2, w_split=ws)
    with pytest.raises(_lib.Wm2fError):
        ops.conv3x3_route(x, w, 1, w_split=ws, stride=2)


# ------------------------------------------------------------------------------------------------- routing, end to end
def _staged_is_picked(N, H, W, B):
    from weed_instance_segmentation_amd import _lib
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    entry = ctypes.c_int(-1)
    return _lib.load().wm2f_conv3x3_split_route(N, H, W, 1, B, n_cu, 3, ctypes.byref(entry)) == 1


def test_bottleneck_switch_on_and_off(ops, monkeypatch):
    from weed_instance_segmentation_amd.backbone_resnet import BottleNeckLayer
    torch.manual_seed(0)
    blk = BottleNeckLayer(256, 256, 1).cuda().eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 2.0)
    x = torch.randn(2, 256, 64, 64, generator=_gen(1), device="cuda")
    assert ops.CONV3X3_STAGED is True
    assert _staged_is_picked(64, 64, 64, 2), "the conv2 of this block is a site of the staged route"
    with torch.no_grad():
        on = blk(x)
        monkeypatch.setattr(ops, "CONV3X3_STAGED", False)
        off = blk(x)
    assert torch.equal(on, off)


def test_pixel_decoder_switch_on_and_off(ops, monkeypatch):
    """The pixel decoder at the benchmark's widths on 32^2 ... 4^2 maps (the pattern of
    tests/test_conv_groupnorm_fused_gpu.py).  On a 32-wide map a staged tile is a direct workgroup's 256 pixels wave for wave,
    so layer_1's statistics are the same fp32 partials under both routes."""
    from weed_instance_segmentation_amd import Mask2FormerConfig
    from weed_instance_segmentation_amd.modeling import Mask2FormerPixelDecoder
    torch.manual_seed(0)
    cfg = Mask2FormerConfig(num_labels=3, encoder_layers=2)
    dec = Mask2FormerPixelDecoder(cfg, [256, 512, 1024, 2048]).cuda().eval()
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)
    g = _gen(11)
    feats = [torch.randn(2, c, s, s, generator=g, device="cuda") for c, s in ((256, 32), (512, 16), (1024, 8), (2048, 4))]
    calls = {"conv3x3_stats": 0}

    def counted(*a, _f=ops.conv3x3_stats, **kw):
        calls["conv3x3_stats"] += 1
        return _f(*a, **kw)
    monkeypatch.setattr(ops, "conv3x3_stats", counted)

    def run():
        with torch.no_grad():
            mask, outs = dec(feats)
        return [mask, *outs]

    assert ops.CONV3X3_STAGED is True
    assert _staged_is_picked(256, 32, 32, 2), "layer_1 (256 -> 256 on the 32^2 map) is a site of the staged route"
    on = run()
    monkeypatch.setattr(ops, "CONV3X3_STAGED", False)
    off = run()
    assert calls["conv3x3_stats"] == 2
    for a, r in zip(on, off):
        assert torch.equal(a, r)
