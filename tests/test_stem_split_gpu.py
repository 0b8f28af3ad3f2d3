"""wm2f_stem7x7_pool_fwd (the ResNet stem as one split-bf16 kernel: conv 7x7 / 2, bias, ReLU, max pool 3x3 / 2;
csrc/stem_split.hip): exact on small integers, under the split kernels' accuracy rule on random and
mixed-exponent data, finite at FLT_MAX, bit-identical across repeats, sub-batches and grids, non-finite exactly in a
NaN's receptive field, no store outside the output, refusals, the split=False route, and the backbone.

Figures of the first run on an MI355X (the rule: e <= 2 e32 + 2^-23): see DESIGN.md §26."""
import pytest
import torch
import torch.nn.functional as F

import split_gemm_cases as G
import stem_reference as S

pytestmark = pytest.mark.gpu

CASES = [(H, W, cin, B) for (H, W) in S.MAPS for cin in S.CINS for B in S.BATCHES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def _dev(*ts):
    return [t.cuda() for t in ts]


@pytest.mark.parametrize("H,W,cin,B", CASES)
def test_stem_small_integers_are_exact(ops, H, W, cin, B):
    x, w, b, ref, _ = S.case("ints", B, cin, H, W)
    out = ops.stem_conv_pool(*_dev(x, w, b))
    assert out.shape == ref.shape
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("family", ["randn", "wide"])
@pytest.mark.parametrize("H,W,cin,B", CASES)
def test_stem_accuracy_rule(ops, H, W, cin, B, family):
    x, w, b, ref, mag = S.case(family, B, cin, H, W)
    xd, wd, bd = _dev(x, w, b)
    e = G.rel_err(ops.stem_conv_pool(xd, wd, bd).cpu(), ref, mag)
    e32 = G.rel_err(S.stem_fp32(xd, wd, bd).cpu(), ref, mag)
    print(f"stem {family} {H}x{W} Cin={cin} B={B}: e = {e:.3e}, e32 = {e32:.3e}")
    assert G.rule(e, e32), (e, e32)


@pytest.mark.parametrize("H,W,cin,B", CASES)
def test_stem_flt_max_inputs_stay_finite(ops, H, W, cin, B):
    x, w, b, ref, mag = S.case("fltmax", B, cin, H, W)
    xd, wd, bd = _dev(x, w, b)
    out = ops.stem_conv_pool(xd, wd, bd).cpu()
    assert torch.isfinite(out).all()
    # and they are the right numbers, not merely finite: the rule of the other families
    assert G.rule(G.rel_err(out, ref, mag), G.rel_err(S.stem_fp32(xd, wd, bd).cpu(), ref, mag))


@pytest.mark.parametrize("H,W,cin,B", CASES)
def test_stem_same_bits_for_repeats_sub_batches_and_grids(ops, H, W, cin, B):
    x, w, b, _, _ = S.case("randn", B, cin, H, W)
    xd, wd, bd = _dev(x, w, b)
    ws = ops.split_weight_stem(wd)
    out = ops.stem_conv_pool(xd, wd, bd, w_split=ws)
    assert torch.equal(ops.stem_conv_pool(xd, wd, bd, w_split=ws), out)
    assert torch.equal(ops.stem_conv_pool(xd, wd, bd), out)  # an uncached split is the same split
    for i in range(B):
        assert torch.equal(ops.stem_conv_pool(xd[i:i + 1].contiguous(), wd, bd, w_split=ws), out[i:i + 1]), i
    for grid in (1, 2):  # at 66 x 130 with B = 3 every wave of these grids walks several units
        assert torch.equal(ops.stem_conv_pool(xd, wd, bd, w_split=ws, grid=grid), out), grid


@pytest.mark.parametrize("H,W,cin,B", CASES)
def test_stem_nonfinite_exactly_in_the_receptive_field(ops, H, W, cin, B):
    x, w, b, _, _ = S.case("randn", B, cin, H, W)
    xd, wd, bd = _dev(x, w, b)
    ws = ops.split_weight_stem(wd)
    spots = [("corner", 0, 0), ("corner", H - 1, W - 1), ("edge", 0, W // 2), ("edge", H // 2, W - 1),
             ("interior", H // 2, W // 2)]
    for k, (what, y, xx) in enumerate(spots):
        bi, c = k % B, k % cin
        bad = xd.clone()
        bad[bi, c, y, xx] = (float("nan"), float("inf"), -float("inf"))[k % 3]
        want = S.nonfinite_mask(B, H, W, [(bi, y, xx)])
        fin = torch.isfinite(ops.stem_conv_pool(bad, wd, bd, w_split=ws)).cpu()
        assert torch.equal(fin, ~want[:, None].expand_as(fin)), (what, y, xx)


@pytest.mark.parametrize("H,W,cin,B", CASES)
def test_stem_stores_stay_inside_the_output(ops, H, W, cin, B):
    from weed_instance_segmentation_amd import _lib
    x, w, b, _, _ = S.case("randn", B, cin, H, W)
    xd, wd, bd = _dev(x, w, b)
    ws = ops.split_weight_stem(wd)
    want = ops.stem_conv_pool(xd, wd, bd, w_split=ws)
    n, pad = want.numel(), 4096
    lib = _lib.load()
    for grid in (0, 1):
        buf = torch.full((n + 2 * pad,), -7.0, device="cuda")
        out = buf[pad:pad + n]
        ops.check(lib.wm2f_stem7x7_pool_fwd(ops._p(xd), ops._p(ws), ops._p(bd), ops._p(out), B, cin, S.N, H, W, grid,
                                            ops._stream(xd)), "wm2f_stem7x7_pool_fwd")
        assert torch.equal(out.view_as(want), want)
        assert bool((buf[:pad] == -7.0).all()) and bool((buf[pad + n:] == -7.0).all())


def test_stem_refusals(ops):
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    x = torch.randn(1, 4, 16, 16, device="cuda")
    w = torch.randn(64, 3, 7, 7, device="cuda")
    b = torch.randn(64, device="cuda")
    ws = ops.split_weight_stem(w)
    out = torch.full((1, 64, 4, 4), -7.0, device="cuda")
    s = ops._stream(x)
    p = ops._p

    def refused(*args):
        rc = lib.wm2f_stem7x7_pool_fwd(*args, 0, s)
        torch.cuda.synchronize()
        return rc != 0 and bool((out == -7.0).all())

    assert refused(p(x), p(ws), p(b), p(out), 1, 4, 64, 16, 16)  # Cin = 4: 196 taps do not fit K = 160
    assert refused(p(x), p(ws), p(b), p(out), 1, 3, 32, 16, 16)  # N = 32
    assert refused(p(x), p(ws), p(b), p(out), 1, 0, 64, 16, 16)
    assert refused(p(x), p(ws), p(b), p(out), 0, 3, 64, 16, 16)
    assert refused(p(x), p(ws), p(b), p(out), 1, 3, 64, 0, 16)
    for hole in range(4):
        args = [p(x), p(ws), p(b), p(out)]
        args[hole] = p(None)
        assert refused(*args, 1, 3, 64, 16, 16), hole
    with pytest.raises(_lib.Wm2fError):
        ops.check(lib.wm2f_stem7x7_pool_fwd(p(x), p(ws), p(b), p(out), 1, 4, 64, 16, 16, 0, s), "wm2f_stem7x7_pool_fwd")
    with pytest.raises(ValueError):
        ops.stem_conv_pool(x[:, :3].contiguous(), w, b, w_split=ops.split_weight(torch.randn(64, 64, device="cuda")))
    # shapes the kernel does not build take the library route
    assert not ops.stem_conv_pool_applies(x, torch.randn(64, 4, 7, 7, device="cuda"))
    assert not ops.stem_conv_pool_applies(x[:, :3], torch.randn(32, 3, 7, 7, device="cuda"))


@pytest.mark.parametrize("H,W", [(64, 96), (33, 31), (16, 16)])
def test_stem_split_false_is_the_library_route(ops, H, W):
    x, w, b, _, _ = S.case("randn", 3, 3, H, W)
    xd, wd, bd = _dev(x, w, b)
    y = F.conv2d(xd, wd, None, 2, 3)
    if y.shape[-2] % 2 == 0 and y.shape[-1] % 8 == 0:
        want = ops.bias_relu_maxpool(y, bd)
    else:
        want = F.max_pool2d(torch.relu_(y.add_(bd[None, :, None, None])), 3, 2, 1)
    assert torch.equal(ops.stem_conv_pool(xd, wd, bd, split=False), want)
    # and a weight the kernel is not built for takes it too
    w4 = torch.randn(64, 4, 7, 7, device="cuda")
    x4 = torch.randn(2, 4, H, W, device="cuda")
    assert torch.equal(ops.stem_conv_pool(x4, w4, bd), ops.stem_conv_pool(x4, w4, bd, split=False))


def test_backbone_stem_route_and_determinism(ops, monkeypatch):
    """ResNet-50, B = 2, 3 x 96 x 160, no_grad + eval: every returned feature map against the eager stem route
    (F.conv2d + bias_relu_maxpool) to 1e-5 max |ref|, two forwards bit-identical, and the split cache follows the fold."""
    from weed_instance_segmentation_amd import Mask2FormerConfig
    from weed_instance_segmentation_amd.backbone_resnet import build_backbone
    from weed_instance_segmentation_amd.derived import derived_peek
    torch.manual_seed(0)
    cfg = dict(Mask2FormerConfig(num_labels=3).backbone_config)
    cfg["out_features"] = ["stem", "stage1", "stage2", "stage3", "stage4"]
    net = build_backbone(cfg).cuda().eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 3, 96, 160, device="cuda")
    emb = net.embedder.embedder
    with torch.no_grad():
        got = net(x)
        split0 = derived_peek(emb, "stem")
        again = net(x)
        assert derived_peek(emb, "stem") is split0
        with monkeypatch.context() as mp:
            mp.setattr(ops, "stem_conv_pool_applies", lambda *a: False)
            ref = net(x)
    assert len(got) == 5 and got[0].shape == (2, 64, 24, 40)
    for a, r, g in zip(again, ref, got):
        assert torch.equal(a, g)  # every backbone kernel is deterministic
        d, m = (g - r).abs().max().item(), r.abs().max().item()
        print(f"backbone map {tuple(g.shape)}: max |d| = {d:.3e}, max |ref| = {m:.3e}, ratio {d / m:.3e}")
        assert d <= 1e-5 * m
    with torch.no_grad():
        emb.normalization.running_var.mul_(3.0)  # a new BatchNorm fold
        got2 = net(x)
    assert derived_peek(emb, "stem") is not split0
    assert not torch.equal(got2[0], got[0])
