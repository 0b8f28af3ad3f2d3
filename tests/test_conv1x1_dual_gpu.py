"""wm2f_conv1x1_split_dual_fwd_p (csrc/conv1x1_split.hip): a bottleneck's conv3 and its projection shortcut
as one split-bf16 GEMM over the concatenated K,  out = relu(W1 . x1 + W2 . x2[::s, ::s] + b),  and its routing in
BottleNeckLayer.forward (ops.SHORTCUT_FOLD).

Values: small integers are held to the fp64 reference bit for bit; random data to the rule of tests/split_gemm_cases.py,
e <= 2 e32 + 2^-23, with e32 from the two-call split=False route (library convolution, then bias + residual + ReLU) on the
same data and mag = sum |x w| over both sources + |b|.  Everything else is bit equality: repeated calls, sub-batches, every
tile configuration that fits N, an uncached split, a source whose weight is zero against the one-source kernel."""
import copy
import functools
import re

import pytest
import torch

import split_gemm_cases as S
import split_precision_reference as R

pytestmark = pytest.mark.gpu

KN = [(32, 32, 64), (64, 64, 256), (96, 160, 192), (128, 256, 512)]  # (K1, K2, N)
MAPS = [(1, 1), (1, 17), (3, 3), (4, 6), (17, 13), (33, 31)]        # (Ho, Wo)
NAN, INF = float("nan"), float("inf")


def _geometries(Ho, Wo):
    """(stride2, H2, W2): stride 1, and at stride 2 an even and an odd source size along each axis."""
    return [(1, Ho, Wo), (2, 2 * Ho, 2 * Wo), (2, 2 * Ho - 1, 2 * Wo - 1), (2, 2 * Ho, 2 * Wo - 1)]


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


@functools.lru_cache(maxsize=None)
def _case(family, B, K1, K2, N, Ho, Wo, s, H2, W2):
    """x1 (B, K1, Ho, Wo), w1 (N, K1), x2 (B, K2, H2, W2), w2 (N, K2), bias (N) on the GPU."""
    seed = K1 + 3 * K2 + 7 * N + 31 * Ho + Wo + 5 * H2 + 11 * W2 + s + B
    x1, w1, b = S.operands(family, B * Ho * Wo, K1, N, seed)
    x2, w2, _ = S.operands(family, B * H2 * W2, K2, N, seed + 1)
    return tuple(t.cuda() for t in (S.as_image(x1, B, Ho, Wo), S.as_w1x1(w1), S.as_image(x2, B, H2, W2), S.as_w1x1(w2), b))


def _ref(x1, w1, x2, w2, b, s):
    """fp64 reference and the error measure's denominator."""
    y1, m1 = S.conv1x1_ref(x1, w1, b)
    y2, m2 = S.conv1x1_ref(x2, w2, None, stride=s)
    return (y1 + y2).relu(), m1 + m2


def _fits(N):
    return [ci for ci, nt in enumerate(S.NT) if N % nt == 0]


# ------------------------------------------------------------------------------------------------ values and determinism
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K1,K2,N", KN)
def test_values_and_determinism(ops, K1, K2, N, B):
    for Ho, Wo in MAPS:
        for s, H2, W2 in _geometries(Ho, Wo):
            for family in ("ints", "randn"):
                x1, w1, x2, w2, b = _case(family, B, K1, K2, N, Ho, Wo, s, H2, W2)
                what = f"dual K={K1}+{K2} N={N} {Ho}x{Wo} from {H2}x{W2}/{s} B={B} {family}"
                ws1, ws2 = ops.split_weight(w1), ops.split_weight(w2)
                out = ops.conv1x1_dual(x1, w1, x2, w2, b, s, w1_split=ws1, w2_split=ws2)
                assert out.shape == (B, N, Ho, Wo), what
                ref, mag = _ref(x1, w1, x2, w2, b, s)
                if family == "ints":
                    assert torch.equal(out, ref.float()), what
                else:
                    e = S.rel_err(out, ref, mag)
                    e32 = S.rel_err(ops.conv1x1_dual(x1, w1, x2, w2, b, s, split=False), ref, mag)
                    print(f"{what}: e {e:.3e} e32 {e32:.3e}")
                    assert S.rule(e, e32), (what, e, e32)
                assert torch.equal(ops.conv1x1_dual(x1, w1, x2, w2, b, s, w1_split=ws1, w2_split=ws2), out), what  # again
                assert torch.equal(ops.conv1x1_dual(x1, w1, x2, w2, b, s), out), what  # an uncached split is the same split
                for ci in _fits(N):  # every tile configuration that fits N
                    assert torch.equal(ops.conv1x1_dual(x1, w1, x2, w2, b, s, w1_split=ws1, w2_split=ws2, config=ci), out), (what, ci)
                for b0, b1 in ((B - 1, B), (0, max(1, B - 1))):  # sub-batches
                    got = ops.conv1x1_dual(x1[b0:b1].contiguous(), w1, x2[b0:b1].contiguous(), w2, b, s, w1_split=ws1, w2_split=ws2)
                    assert torch.equal(got, out[b0:b1]), (what, b0, b1)


@pytest.mark.parametrize("family", S.VALUE_FAMILIES)
def test_value_families(ops, family):
    K1, K2, N, B, Ho, Wo = 96, 160, 64, 2, 9, 11
    for s, H2, W2 in _geometries(Ho, Wo)[:3]:
        x1, w1, x2, w2, b = _case(family, B, K1, K2, N, Ho, Wo, s, H2, W2)
        out = ops.conv1x1_dual(x1, w1, x2, w2, b, s)
        ref, mag = _ref(x1, w1, x2, w2, b, s)
        e = S.rel_err(out, ref, mag)
        e32 = S.rel_err(ops.conv1x1_dual(x1, w1, x2, w2, b, s, split=False), ref, mag)
        print(f"dual {family} /{s}: e {e:.3e} e32 {e32:.3e}")
        assert S.rule(e, e32), (family, s, e, e32)
        assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------- the source switch and the second pointer
@pytest.mark.parametrize("K1,K2,N", KN)
def test_a_zero_weight_leaves_the_one_source_kernel(ops, K1, K2, N):
    for Ho, Wo in ((4, 6), (33, 31)):
        for s, H2, W2 in _geometries(Ho, Wo)[:3]:
            x1, w1, x2, w2, b = _case("randn", 3, K1, K2, N, Ho, Wo, s, H2, W2)
            got = ops.conv1x1_dual(x1, w1, x2, torch.zeros_like(w2), b, s)
            assert torch.equal(got, ops.conv1x1(x1, w1, b, relu=True)), (Ho, Wo, s, "W2 = 0")
            got = ops.conv1x1_dual(x1, torch.zeros_like(w1), x2, w2, b, s)
            assert torch.equal(got, ops.conv1x1(x2, w2, b, relu=True, stride=s)), (Ho, Wo, s, "W1 = 0")


@pytest.mark.parametrize("K1,K2,N", KN)
def test_the_split_of_a_concatenation_is_the_concatenation_of_the_splits(ops, K1, K2, N):
    g = torch.Generator(device="cuda").manual_seed(K1 + K2 + N)
    w1 = torch.randn(N, K1, generator=g, device="cuda")
    w2 = torch.randn(N, K2, generator=g, device="cuda")
    assert torch.equal(ops.split_weight(torch.cat([w1, w2], 1)), torch.cat([ops.split_weight(w1), ops.split_weight(w2)]))


# ------------------------------------------------------------------------------------------------------- pixel handling
@pytest.mark.parametrize("K1,K2,N", [(32, 32, 64), (96, 160, 192)])
def test_unsampled_pixels_are_never_read(ops, K1, K2, N):
    for Ho, Wo in ((3, 3), (17, 13)):
        for s, H2, W2 in _geometries(Ho, Wo)[1:]:
            x1, w1, x2, w2, b = _case("randn", 2, K1, K2, N, Ho, Wo, s, H2, W2)
            out = ops.conv1x1_dual(x1, w1, x2, w2, b, s)
            poisoned = torch.full_like(x2, NAN)
            poisoned[:, :, ::2, ::2] = x2[:, :, ::2, ::2]
            assert torch.equal(ops.conv1x1_dual(x1, w1, poisoned, w2, b, s), out), (Ho, Wo, H2, W2)
            assert torch.isfinite(out).all()


@pytest.mark.parametrize("source", [1, 2])
@pytest.mark.parametrize("K1,K2,N", [(32, 32, 64), (128, 256, 512)])
def test_a_nonfinite_pixel_reaches_exactly_its_outputs(ops, K1, K2, N, source):
    B = 2
    for Ho, Wo in ((1, 17), (17, 13), (33, 31)):  # 17, 221 and 1023 pixels: ragged tails of every tile width
        for s, H2, W2 in _geometries(Ho, Wo)[:3]:
            x1, w1, x2, w2, b = (t.clone() for t in _case("randn", B, K1, K2, N, Ho, Wo, s, H2, W2))
            K = K1 if source == 1 else K2
            bad = [(0, 3, 0, 0, NAN), (0, K - 1, Ho - 1, Wo - 1, INF), (1, 17 % K, Ho // 2, Wo // 2, -INF),
                   (1, 0, Ho - 1, Wo - 1, NAN)]  # the last pixel of the ragged tail in both images
            want = torch.ones(B, Ho, Wo, dtype=torch.bool, device="cuda")
            for bi, k, ho, wo, v in bad:
                if source == 1:
                    x1[bi, k, ho, wo] = v
                else:
                    x2[bi, k, s * ho, s * wo] = v
                want[bi, ho, wo] = False
            fin = torch.isfinite(ops.conv1x1_dual(x1, w1, x2, w2, b, s))
            assert torch.equal(fin, want[:, None].expand_as(fin)), (Ho, Wo, s, H2, W2)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_untouched(ops):
    from weed_instance_segmentation_amd import _lib
    lib = _lib.load()
    B, K1, K2, N, Ho, Wo = 1, 64, 64, 64, 4, 6
    x1 = torch.randn(B, K1, Ho, Wo, device="cuda")
    x2 = torch.randn(B, K2, 2 * Ho, 2 * Wo, device="cuda")
    ws1, ws2 = ops.split_weight(torch.randn(N, K1, device="cuda")), ops.split_weight(torch.randn(N, K2, device="cuda"))
    bias = torch.randn(N, device="cuda")
    out = torch.full((B, N, Ho, Wo), -7.0, device="cuda")
    s = ops._stream(x1)
    ptrs = [x1, ws1, x2, ws2, bias, out]
    good = dict(B=B, K1=K1, K2=K2, N=N, Ho=Ho, Wo=Wo, H2=2 * Ho, W2=2 * Wo, stride2=2, config=-1, pieces=3)

    def call(null=None, **change):
        a = {**good, **change}
        p = [ops._p(None if i == null else t) for i, t in enumerate(ptrs)]
        return lib.wm2f_conv1x1_split_dual_fwd_p(*p, a["B"], a["K1"], a["K2"], a["N"], a["Ho"], a["Wo"], a["H2"], a["W2"],
                                                 a["stride2"], a["config"], a["pieces"], s)

    refused = [dict(null=i) for i in range(6)]
    refused += [dict(K1=48), dict(K2=80), dict(N=96), dict(stride2=3), dict(stride2=0), dict(stride2=1),  # 8 x 12 at stride 1
                dict(H2=2 * Ho + 1), dict(W2=2 * Wo - 2), dict(H2=Ho, W2=Wo),
                # an image of x1, of x2, of out at 2 GiB; either split above it (nothing is read before the refusal)
                dict(K1=128, K2=32, Ho=2048, Wo=2048, H2=2048, W2=2048, stride2=1),
                dict(K1=32, K2=128, Ho=2048, Wo=2048, H2=2048, W2=2048, stride2=1),
                dict(K1=32, K2=32, N=128, Ho=2048, Wo=2048, H2=2048, W2=2048, stride2=1),
                dict(K1=10944, N=32768, Ho=1, Wo=1, H2=1, W2=1), dict(K2=10944, N=32768, Ho=1, Wo=1, H2=1, W2=1),
                dict(config=0), dict(config=3), dict(config=5), dict(config=-2),  # N = 64: only the 64-channel entry divides it
                dict(pieces=0), dict(pieces=4)]
    for change in refused:
        assert call(**change) == _lib.WM2F_EINVAL, change
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call() == 0 and call(config=4) == 0  # and the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())
    with pytest.raises(ValueError):
        ops.conv1x1_dual(x1, torch.randn(N, K1, device="cuda"), x2, torch.randn(N, K2, device="cuda"), None, 2)


# ----------------------------------------------------------------------------------------------------- precision levels
@pytest.mark.parametrize("level", ["high", "medium"])
def test_precision_levels(ops, pkg, level):
    suffix = {"high": "_p2", "medium": "_p1"}[level]
    for K1, K2, N in ((96, 160, 192), (128, 256, 512)):
        Ho, Wo = 17, 13
        for s, H2, W2 in _geometries(Ho, Wo)[:3]:
            for family in ("ints", "randn"):
                x1, w1, x2, w2, b = _case(family, 3, K1, K2, N, Ho, Wo, s, H2, W2)
                timer = ops.KernelTimer()
                ops.set_kernel_timer(timer)
                try:
                    with pkg.inference_precision(level):
                        out = ops.conv1x1_dual(x1, w1, x2, w2, b, s)
                    torch.cuda.synchronize()
                finally:
                    ops.set_kernel_timer(None)
                assert list(timer.records) == [f"conv1x1_K{K1}+{K2}_N{N}_P{Ho * Wo}{suffix}"]
                ref, mag = _ref(x1, w1, x2, w2, b, s)
                if family == "ints":  # bf16-exact operands: the bits of every level
                    assert torch.equal(out, ref.float())
                    continue
                e = S.rel_err(out, ref, mag)
                e32 = S.rel_err(ops.conv1x1_dual(x1, w1, x2, w2, b, s, split=False), ref, mag)
                print(f"dual {level} K={K1}+{K2} /{s}: e {e:.3e} e32 {e32:.3e}")
                assert R.rule(e, e32, level), (level, K1, K2, s, e, e32)
                with pkg.inference_precision(level):  # the two-call route at this level: the same rule, nothing tighter
                    two = ops.conv1x1(x1, w1, b, ops.conv1x1(x2, w2, None, stride=s), True)
                assert R.rule(S.rel_err(two, ref, mag), e32, level)
                assert not torch.equal(out, ops.conv1x1_dual(x1, w1, x2, w2, b, s))  # and not the bits of "highest"


# -------------------------------------------------------------------------------------------------------------- routing
def _block(cin, cout, stride, seed):
    from weed_instance_segmentation_amd.backbone_resnet import BottleNeckLayer
    torch.manual_seed(seed)
    blk = BottleNeckLayer(cin, cout, stride).cuda().eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    return blk


BLOCKS = [(64, 256, 1, 8, 12), (256, 512, 2, 20, 14)]


def _tags(ops, fn):
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    return out, {t: len(v) for t, v in timer.records.items()}


@pytest.mark.parametrize("cin,cout,stride,H,W", BLOCKS)
def test_block_routes_through_one_launch(ops, monkeypatch, cin, cout, stride, H, W):
    blk = _block(cin, cout, stride, seed=cin)
    x = torch.randn(2, cin, H, W, device="cuda")
    on, tags_on = _tags(ops, lambda: blk(x))
    with monkeypatch.context() as mp:
        mp.setattr(ops, "SHORTCUT_FOLD", False)
        off, tags_off = _tags(ops, lambda: blk(x))
    assert (on - off).abs().max().item() <= 1e-5 * off.abs().max().item()
    dual = [t for t in tags_on if re.match(r"conv1x1_K\d+\+\d+_", t)]
    Ho, Wo = S.out_hw(H, W, stride)
    assert dual == [f"conv1x1_K{cout // 4}+{cin}_N{cout}_P{Ho * Wo}"] and tags_on[dual[0]] == 1
    assert not any("+" in t for t in tags_off)
    assert sum(tags_on.values()) == sum(tags_off.values()) - 1


@pytest.mark.parametrize("cin,cout,stride,H,W", BLOCKS)
def test_block_follows_in_place_changes(ops, cin, cout, stride, H, W):
    from weed_instance_segmentation_amd.derived import derived_peek
    blk = _block(cin, cout, stride, seed=cin + 1)
    x = torch.randn(2, cin, H, W, device="cuda")
    with torch.no_grad():
        last = blk(x)
    assert derived_peek(blk, "shortcut_bias") is not None
    assert derived_peek(blk.layer[2], "conv") is not None and derived_peek(blk.shortcut, "conv") is not None
    changes = (lambda: blk.layer[2].convolution.weight.mul_(-1.5), lambda: blk.shortcut.normalization.running_var.mul_(3.0),
               lambda: blk.shortcut.normalization.bias.add_(0.75))
    for change in changes:
        with torch.no_grad():
            change()
            got = blk(x)
            fresh = copy.deepcopy(blk)  # the derived values are not part of a module: a copy has never run
            assert derived_peek(fresh, "shortcut_bias") is None
            want = fresh(x)
        assert not torch.equal(got, last)
        assert torch.equal(got, want)
        last = got


def test_stage_is_deterministic(ops):
    from weed_instance_segmentation_amd.backbone_resnet import Stage
    torch.manual_seed(5)
    stage = Stage(64, 256, 1, 2, False).cuda().eval()
    x = torch.randn(2, 64, 9, 7, device="cuda")
    (first, tags) = _tags(ops, lambda: stage(x))
    assert sum(1 for t in tags if "+" in t) == 1
    with torch.no_grad():
        assert torch.equal(stage(x), first)
