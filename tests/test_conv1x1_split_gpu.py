"""wm2f_conv1x1_split_fwd (split-bf16 1x1 convolution in NCHW, csrc/conv1x1_split.hip) at the model's
shapes: accuracy against fp64 next to the fp32 library convolution (ops.conv1x1(..., split=False)) on the same data,
bit-identity on repeated runs and sub-batches, non-finite propagation, the split-weight cache, and the model's no-grad
forward against the split=False route."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


RAW, BIAS, RELU, RES = "raw", "bias", "relu", "res"
NT = [256, 256, 256, 128, 64]  # channels of a workgroup tile, per entry of the kernel's configuration table

# (K, N, H, W, stride, epilogue): every distinct 1x1 site of the benchmark (ResNet-50, B = 8 at 1024^2), then the
# 800 x 1088 product shapes whose maps are not multiples of 16 pixels (stage 4: 25 x 34 = 850)
SITES = [
    (64, 64, 256, 256, 1, RELU), (64, 256, 256, 256, 1, RAW), (64, 256, 256, 256, 1, RES), (256, 64, 256, 256, 1, RELU),
    (256, 128, 256, 256, 1, RELU), (256, 512, 256, 256, 2, RAW), (128, 512, 128, 128, 1, RES), (512, 128, 128, 128, 1, RELU),
    (512, 256, 128, 128, 1, RELU), (512, 1024, 128, 128, 2, RAW), (256, 1024, 64, 64, 1, RES), (1024, 256, 64, 64, 1, RELU),
    (1024, 512, 64, 64, 1, RELU), (1024, 2048, 64, 64, 2, RAW), (512, 2048, 32, 32, 1, RES), (2048, 512, 32, 32, 1, RELU),
    (2048, 256, 32, 32, 1, RAW), (1024, 256, 64, 64, 1, RAW), (512, 256, 128, 128, 1, RAW), (256, 256, 256, 256, 1, RAW),
    (256, 256, 256, 256, 1, BIAS),
    (2048, 512, 25, 34, 1, RELU), (512, 2048, 25, 34, 1, RES), (1024, 2048, 50, 68, 2, RAW), (2048, 256, 25, 34, 1, RAW),
    (256, 512, 200, 272, 2, RAW), (64, 256, 200, 272, 1, RES),
]


def _case(B, K, N, H, W, stride, epi, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, K, H, W, generator=g, device="cuda")
    w = torch.randn(N, K, 1, 1, generator=g, device="cuda") * (1.0 / math.sqrt(K))
    b = torch.randn(N, generator=g, device="cuda") * 0.1 if epi != RAW else None
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = torch.randn(B, N, Ho, Wo, generator=g, device="cuda") if epi == RES else None
    return x, w, b, r


def _err(out, x, w, b, r, relu, stride):
    """max |out - ref| / (sum_k |x_k w_k| + |b| + |r|) over the outputs, ref in fp64 on the GPU."""
    xs = x[:, :, ::stride, ::stride].double().flatten(2)
    wd = w.double().flatten(1)
    ref = torch.matmul(wd, xs)
    mag = torch.matmul(wd.abs(), xs.abs())
    if b is not None:
        ref += b.double()[None, :, None]
        mag += b.double().abs()[None, :, None]
    if r is not None:
        ref += r.double().flatten(2)
        mag += r.double().abs().flatten(2)
    if relu:
        ref = ref.relu()
    return ((out.double().flatten(2) - ref).abs() / mag.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("K,N,H,W,stride,epi", SITES)
def test_conv1x1_split_accuracy_determinism_and_sub_batches(ops, K, N, H, W, stride, epi):
    B = 8
    x, w, b, r = _case(B, K, N, H, W, stride, epi, seed=K + 7 * N + H + stride)
    relu = epi in (RELU, RES)
    ws = ops.split_weight(w.view(N, K))
    out = ops.conv1x1(x, w, b, r, relu, stride, w_split=ws)
    assert out.shape == (B, N, (H - 1) // stride + 1, (W - 1) // stride + 1)
    ref32 = ops.conv1x1(x, w, b, None if r is None else r.clone(), relu, stride, split=False)
    for i in (0, B - 1):  # the fp64 comparison on two images of the batch
        sl = slice(i, i + 1)
        e = _err(out[sl], x[sl], w, b, None if r is None else r[sl], relu, stride)
        e32 = _err(ref32[sl], x[sl], w, b, None if r is None else r[sl], relu, stride)
        assert e <= 2 * e32, (i, e, e32)
    del ref32
    assert torch.equal(ops.conv1x1(x, w, b, r, relu, stride, w_split=ws), out)
    assert torch.equal(ops.conv1x1(x, w, b, r, relu, stride), out)  # an uncached split is the same split
    for b0, b1 in ((B - 1, B), (2, 5)):  # sub-batches choose other tile configurations: the same bits
        got = ops.conv1x1(x[b0:b1].contiguous(), w, b, None if r is None else r[b0:b1].contiguous(), relu, stride, w_split=ws)
        assert torch.equal(got, out[b0:b1])
    for ci, nt in enumerate(NT):  # every tile configuration that fits N: the same bits
        if N % nt == 0:
            assert torch.equal(ops.conv1x1(x[:2], w, b, None if r is None else r[:2], relu, stride, w_split=ws, config=ci), out[:2])


@pytest.mark.parametrize("K,N,H,W,stride,epi", [(256, 256, 25, 34, 1, BIAS), (512, 2048, 25, 34, 1, RES),
                                               (1024, 512, 50, 68, 2, RAW), (64, 64, 37, 41, 1, RELU)])
def test_conv1x1_split_nonfinite_inputs(ops, K, N, H, W, stride, epi):
    B = 2
    x, w, b, r = _case(B, K, N, H, W, stride, epi, seed=3 * K + N)
    relu = epi in (RELU, RES)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    bad = [(0, 3, 0, 0, float("nan")), (0, K - 1, Ho - 1, Wo - 1, float("inf")), (1, 40 % K, Ho // 2, 1, -float("inf")),
           (1, 0, Ho - 1, 0, float("nan"))]
    want = torch.ones(B, Ho, Wo, dtype=torch.bool, device="cuda")
    for bi, k, ho, wo, v in bad:
        x[bi, k, stride * ho, stride * wo] = v
        want[bi, ho, wo] = False
    if stride == 2:  # an unsampled pixel does not reach the output
        x[0, 5, 1, 1] = float("nan")
    out = ops.conv1x1(x, w, b, r, relu, stride)
    fin = torch.isfinite(out)
    assert torch.equal(fin, want[:, None].expand_as(fin))


def test_conv1x1_split_refusals(ops):
    from weed_instance_segmentation_amd import _lib
    x = torch.randn(1, 64, 8, 8, device="cuda")
    w = torch.randn(64, 64, device="cuda")
    ws = ops.split_weight(w)
    out = torch.empty(1, 64, 8, 8, device="cuda")
    lib = _lib.load()
    s = ops._stream(x)
    for args in ((1, 48, 64, 8, 8, 1, 0), (1, 64, 48, 8, 8, 1, 0), (1, 64, 64, 8, 8, 3, 0)):  # K % 32, N % 64, stride
        assert lib.wm2f_conv1x1_split_fwd(ops._p(x), ops._p(ws), ops._p(None), ops._p(None), ops._p(out), *args, -1, s) != 0
    # a ReLU without bias, a residual without ReLU
    assert lib.wm2f_conv1x1_split_fwd(ops._p(x), ops._p(ws), ops._p(None), ops._p(None), ops._p(out), 1, 64, 64, 8, 8, 1, 1, -1, s) != 0
    assert lib.wm2f_conv1x1_split_fwd(ops._p(x), ops._p(ws), ops._p(w), ops._p(out), ops._p(out), 1, 64, 64, 8, 8, 1, 0, -1, s) != 0
    with pytest.raises(_lib.Wm2fError):
        ops.check(lib.wm2f_conv1x1_split_fwd(ops._p(x), ops._p(ws), ops._p(None), ops._p(None), ops._p(out), 1, 48, 64, 8, 8, 1, 0, -1, s),
                  "wm2f_conv1x1_split_fwd")


def test_conv_layer_split_cache_follows_the_folded_weight(ops):
    from weed_instance_segmentation_amd.backbone_resnet import BottleNeckLayer
    torch.manual_seed(0)
    blk = BottleNeckLayer(256, 512, 2).cuda().eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 256, 64, 48, device="cuda")

    def both():
        with torch.no_grad():
            got = blk(x)
            ops.CONV1X1_SPLIT = False
            try:
                ref = blk(x)
            finally:
                ops.CONV1X1_SPLIT = True
        return got, ref

    got, ref = both()
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    with torch.no_grad():
        blk.layer[2].convolution.weight.mul_(-1.5)   # a new weight version of conv3
        blk.shortcut.normalization.running_var.mul_(3.0)  # a new fold of the shortcut
    got2, ref2 = both()
    assert not torch.equal(got2, got)
    assert (got2 - ref2).abs().max().item() <= 1e-5 * ref2.abs().max().item()


def test_model_forward_split_vs_library_route(ops):
    """The no-grad forward of the benchmark's model (ResNet-50) at 800 x 1088 (stage 4 at 25 x 34): the split route
    against the split=False route."""
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    torch.manual_seed(0)
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig(num_labels=3, num_queries=100)).cuda().eval()
    x = torch.randn(2, 3, 800, 1088, device="cuda")
    with torch.no_grad():
        got = model(pixel_values=x)
        ops.CONV1X1_SPLIT = False
        try:
            ref = model(pixel_values=x)
        finally:
            ops.CONV1X1_SPLIT = True
        again = model(pixel_values=x)
    for k in ("masks_queries_logits", "class_queries_logits"):
        a, r = getattr(got, k), getattr(ref, k)
        assert torch.isfinite(a).all()
        assert (a - r).abs().max().item() <= 1e-3 * r.abs().max().item(), k
        # run to run, only the stock library's 3x3 convolutions (atomic split-K) vary
        assert (getattr(again, k) - a).abs().max().item() <= 1e-4 * a.abs().max().item(), k
