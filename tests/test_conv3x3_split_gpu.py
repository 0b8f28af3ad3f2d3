"""wm2f_conv3x3_split_fwd (split-bf16 3x3 implicit GEMM in NCHW, csrc/conv3x3_split.hip) at the model's
shapes: accuracy against fp64 next to an fp32 im2col GEMM on the same data, bit-identity on repeated runs, sub-batches and
tile configurations, the padded borders on tiny and odd maps, non-finite propagation, refusals, the split-weight cache,
and the model's no-grad forward against the split=False route."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


RAW, BIAS, RELU = "raw", "bias", "relu"
NT = [256, 256, 256, 128, 64]  # channels of a workgroup tile, per entry of the kernel's configuration table

# (Cin = N, H, W, stride, epilogue): every distinct 3x3 site of the benchmark (ResNet-50 conv2 with bias + ReLU, the FPN
# layer_1 raw; B = 8 at 1024^2), the 800 x 1088 maps, then tiny and odd maps that exercise every border case
SITES = [
    (64, 256, 256, 1, RELU), (128, 256, 256, 2, RELU), (128, 128, 128, 1, RELU), (256, 128, 128, 2, RELU),
    (256, 64, 64, 1, RELU), (512, 64, 64, 2, RELU), (512, 32, 32, 1, RELU), (256, 256, 256, 1, RAW),
    (64, 200, 272, 1, RELU), (128, 200, 272, 2, RELU), (128, 100, 136, 1, RELU), (256, 100, 136, 2, RELU),
    (256, 50, 68, 1, RELU), (512, 50, 68, 2, RELU), (512, 25, 34, 1, RELU), (256, 200, 272, 1, RAW),
    (64, 1, 1, 1, RELU), (64, 1, 1, 2, BIAS), (128, 2, 3, 1, RAW), (128, 2, 3, 2, RELU), (64, 5, 7, 1, BIAS),
    (256, 5, 7, 2, RELU), (96, 37, 41, 1, RELU), (96, 37, 41, 2, RAW),
]


def _case(B, C, N, H, W, epi, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g, device="cuda")
    w = torch.randn(N, C, 3, 3, generator=g, device="cuda") * (1.0 / math.sqrt(9 * C))
    b = torch.randn(N, generator=g, device="cuda") * 0.1 if epi != RAW else None
    return x, w, b


def _err(out, x, w, b, relu, stride):
    """max |out - ref| / (sum_k |x_k w_k| + |b|) over the outputs, ref = F.unfold + matmul in fp64 on the GPU."""
    cols = F.unfold(x.double(), 3, padding=1, stride=stride)  # (B, Cin 9, P), column order c-major like w.flatten(1)
    wd = w.double().flatten(1)
    ref = torch.matmul(wd, cols)
    mag = torch.matmul(wd.abs(), cols.abs())
    del cols
    if b is not None:
        ref += b.double()[None, :, None]
        mag += b.double().abs()[None, :, None]
    if relu:
        ref = ref.relu()
    return ((out.double().flatten(2) - ref).abs() / mag.clamp_min(1e-300)).max().item()


def _im2col_fp32(x, w, b, relu, stride):
    """The fp32 reference of the bound: the same convolution as an fp32 im2col GEMM (not MIOpen's Winograd)."""
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.matmul(w.flatten(1), F.unfold(x, 3, padding=1, stride=stride))
    if b is not None:
        y = y + b[None, :, None]
    if relu:
        y = y.relu()
    return y.view(B, -1, Ho, Wo)


@pytest.mark.parametrize("C,H,W,stride,epi", SITES)
def test_conv3x3_split_accuracy_determinism_and_sub_batches(ops, C, H, W, stride, epi):
    B, N = 8, C if C % 64 == 0 else 64
    x, w, b = _case(B, C, N, H, W, epi, seed=C + 7 * H + W + stride)
    relu = epi == RELU
    ws = ops.split_weight_3x3(w)
    out = ops.conv3x3(x, w, b, relu, stride, w_split=ws)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert out.shape == (B, N, Ho, Wo)
    for i in (0, B - 1):  # the fp64 comparison on two images of the batch
        sl = slice(i, i + 1)
        e = _err(out[sl], x[sl], w, b, relu, stride)
        e32 = _err(_im2col_fp32(x[sl], w, b, relu, stride), x[sl], w, b, relu, stride)
        assert e <= 2 * e32, (i, e, e32)
    # the library route agrees to fp32 rounding
    ref = ops.conv3x3(x[:1], w, b, relu, stride, split=False)
    assert (out[:1] - ref).abs().max().item() <= 1e-4 * max(ref.abs().max().item(), 1.0)
    assert torch.equal(ops.conv3x3(x, w, b, relu, stride, w_split=ws), out)
    assert torch.equal(ops.conv3x3(x, w, b, relu, stride), out)  # an uncached split is the same split
    for b0, b1 in ((B - 1, B), (2, 5)):  # sub-batches choose other tile configurations: the same bits
        assert torch.equal(ops.conv3x3(x[b0:b1].contiguous(), w, b, relu, stride, w_split=ws), out[b0:b1])
    for ci, nt in enumerate(NT):  # every tile configuration that fits N: the same bits
        if N % nt == 0:
            assert torch.equal(ops.conv3x3(x[:2], w, b, relu, stride, w_split=ws, config=ci), out[:2])


@pytest.mark.parametrize("C,H,W,stride,epi", [(256, 25, 34, 1, RAW), (512, 25, 34, 1, RELU), (128, 50, 68, 2, RELU),
                                              (64, 37, 41, 1, BIAS), (64, 5, 7, 2, RAW)])
def test_conv3x3_split_nonfinite_inputs(ops, C, H, W, stride, epi):
    B, N = 2, 64 if C == 64 else 128
    x, w, b = _case(B, C, N, H, W, epi, seed=3 * C + H)
    relu = epi == RELU
    bad = [(0, 3, 0, 0, float("nan")), (0, C - 1, H - 1, W - 1, float("inf")), (1, 40 % C, H // 2, 1, -float("inf")),
           (1, 0, H - 1, 0, float("nan"))]
    hit = torch.zeros(B, 1, H, W, device="cuda")
    for bi, k, h, ww, v in bad:
        x[bi, k, h, ww] = v
        hit[bi, 0, h, ww] = 1.0
    # an output is non-finite exactly where its 3x3 window (padding 1, stride s) holds a non-finite input
    want = F.conv2d(hit, torch.ones(1, 1, 3, 3, device="cuda"), None, stride, 1)[:, 0] == 0
    out = ops.conv3x3(x, w, b, relu, stride)
    fin = torch.isfinite(out)
    assert torch.equal(fin, want[:, None].expand_as(fin))


def test_conv3x3_split_refusals(ops):
    from weed_instance_segmentation_amd import _lib
    x = torch.randn(1, 64, 8, 8, device="cuda")
    w = torch.randn(64, 64, 3, 3, device="cuda")
    ws = ops.split_weight_3x3(w)
    out = torch.empty(1, 64, 8, 8, device="cuda")
    lib = _lib.load()
    s = ops._stream(x)
    for args in ((1, 48, 64, 8, 8, 1, 0), (1, 64, 48, 8, 8, 1, 0), (1, 64, 64, 8, 8, 3, 0), (0, 64, 64, 8, 8, 1, 0)):
        assert lib.wm2f_conv3x3_split_fwd(ops._p(x), ops._p(ws), ops._p(None), ops._p(out), *args, -1, s) != 0
    # a ReLU without bias; a configuration out of range; one whose tile does not divide N
    assert lib.wm2f_conv3x3_split_fwd(ops._p(x), ops._p(ws), ops._p(None), ops._p(out), 1, 64, 64, 8, 8, 1, 1, -1, s) != 0
    assert lib.wm2f_conv3x3_split_fwd(ops._p(x), ops._p(ws), ops._p(None), ops._p(out), 1, 64, 64, 8, 8, 1, 0, 5, s) != 0
    assert lib.wm2f_conv3x3_split_fwd(ops._p(x), ops._p(ws), ops._p(None), ops._p(out), 1, 64, 64, 8, 8, 1, 0, 0, s) != 0
    with pytest.raises(_lib.Wm2fError):
        ops.check(lib.wm2f_conv3x3_split_fwd(ops._p(x), ops._p(ws), ops._p(None), ops._p(out), 1, 48, 64, 8, 8, 1, 0, -1, s),
                  "wm2f_conv3x3_split_fwd")
    with pytest.raises(ValueError):
        ops.conv3x3(x, w, None, relu=True)
    with pytest.raises(ValueError):
        ops.conv3x3(x, w, w_split=ops.split_weight(torch.randn(64, 64, device="cuda")))
    # shapes the kernel does not build take the library route
    x48 = torch.randn(1, 48, 9, 9, device="cuda")
    w48 = torch.randn(64, 48, 3, 3, device="cuda")
    assert torch.equal(ops.conv3x3(x48, w48), F.conv2d(x48, w48, None, 1, 1))


def test_conv_layer_split_cache_follows_the_folded_weight(ops):
    from weed_instance_segmentation_amd.backbone_resnet import BottleNeckLayer
    from weed_instance_segmentation_amd.derived import derived_peek
    torch.manual_seed(0)
    blk = BottleNeckLayer(256, 512, 2).cuda().eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 1.5)
    conv2 = blk.layer[1]
    x = torch.randn(2, 256, 64, 48, device="cuda")

    def both():
        with torch.no_grad():
            got = blk(x)
            ops.CONV3X3_SPLIT = False
            try:
                ref = blk(x)
            finally:
                ops.CONV3X3_SPLIT = True
        return got, ref

    got, ref = both()
    split0 = derived_peek(conv2, "conv3x3")
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    with torch.no_grad():
        conv2.convolution.weight.mul_(-1.5)  # a new weight version of conv2
    got2, ref2 = both()
    split1 = derived_peek(conv2, "conv3x3")
    assert split1 is not split0 and not torch.equal(split1, split0)
    assert not torch.equal(got2, got)
    assert (got2 - ref2).abs().max().item() <= 1e-5 * ref2.abs().max().item()
    with torch.no_grad():
        conv2.normalization.running_var.mul_(3.0)  # a new BatchNorm fold
    got3, ref3 = both()
    assert derived_peek(conv2, "conv3x3") is not split1
    assert not torch.equal(got3, got2)
    assert (got3 - ref3).abs().max().item() <= 1e-5 * ref3.abs().max().item()
    with torch.no_grad():
        split2 = derived_peek(conv2, "conv3x3")
        assert torch.equal(blk(x), got3)  # unchanged parameters: the cached split, the same bits
    assert derived_peek(conv2, "conv3x3") is split2


def test_pixel_decoder_split_cache_follows_the_weight(ops):
    from weed_instance_segmentation_amd.modeling import Mask2FormerPixelDecoder
    dec = type("D", (), {})()  # any plain object owns a cache
    conv = torch.nn.Conv2d(256, 256, 3, padding=1, bias=False).cuda()
    x = torch.randn(1, 256, 20, 24, device="cuda")
    with torch.no_grad():
        a = Mask2FormerPixelDecoder._conv3x3(dec, conv, x, "layer_1")
        assert torch.equal(Mask2FormerPixelDecoder._conv3x3(dec, conv, x, "layer_1"), a)
        conv.weight.mul_(2.0)
        b = Mask2FormerPixelDecoder._conv3x3(dec, conv, x, "layer_1")
        ref = F.conv2d(x, conv.weight, None, 1, 1)
    assert (b - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert not torch.equal(b, a)


def test_model_forward_split_vs_library_route(ops):
    """The no-grad forward of the benchmark's model (ResNet-50) at 800 x 1088 (stage 4 at 25 x 34): the 3x3 split route
    against the split=False route, and run to run."""
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    torch.manual_seed(0)
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig(num_labels=3, num_queries=100)).cuda().eval()
    x = torch.randn(2, 3, 800, 1088, device="cuda")
    with torch.no_grad():
        got = model(pixel_values=x)
        ops.CONV3X3_SPLIT = False
        try:
            ref = model(pixel_values=x)
        finally:
            ops.CONV3X3_SPLIT = True
        again = model(pixel_values=x)
    for k in ("masks_queries_logits", "class_queries_logits"):
        a, r = getattr(got, k), getattr(ref, k)
        assert torch.isfinite(a).all()
        assert (a - r).abs().max().item() <= 1e-3 * r.abs().max().item(), k
        # run to run, only the stock library's 7x7 stem convolution may vary
        assert (getattr(again, k) - a).abs().max().item() <= 1e-4 * a.abs().max().item(), k
