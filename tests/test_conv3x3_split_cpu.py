"""Host side of the split-bf16 3x3 convolution (csrc/conv3x3_split.hip): the tile configuration table
covers every site of the model, the routing predicate refuses what the kernel does not build, and the tap-major weight
reorder the kernel reads is the convolution's im2col order."""
import numpy as np
import pytest
import torch

from weed_instance_segmentation_amd import _lib, ops

# (N, P, B) of the 3x3 sites: ResNet-50 conv2 (stride 1 and the stride-2 first blocks) and the FPN layer_1 at B = 8,
# 1024^2, then the 800 x 1088 maps
SITES = [(64, 65536, 8), (128, 16384, 8), (256, 4096, 8), (512, 1024, 8), (256, 65536, 8),
         (64, 200 * 272, 8), (128, 100 * 136, 8), (256, 50 * 68, 8), (512, 25 * 34, 8), (256, 200 * 272, 8),
         (64, 1, 1), (512, 6, 1)]
NT = [256, 256, 256, 128, 64]  # the table's workgroup tile widths (channels)


@pytest.mark.parametrize("N,P,B", SITES)
def test_every_site_has_a_configuration(N, P, B):
    ci = _lib.load().wm2f_conv3x3_split_config(N, P, B, 256)
    assert 0 <= ci < len(NT) and N % NT[ci] == 0


def test_configuration_refusals():
    lib = _lib.load()
    assert lib.wm2f_conv3x3_split_config(48, 1024, 1, 256) == -1  # no tile divides N
    assert lib.wm2f_conv3x3_split_config(64, 0, 1, 256) == -1
    assert lib.wm2f_conv3x3_split_config(64, 1024, 0, 256) == -1
    assert lib.wm2f_conv3x3_split_config(64, 1024, 1, 0) == -1


def test_conv3x3_applies_only_to_built_shapes():
    x = torch.zeros(1, 64, 8, 8)
    w = torch.zeros(64, 64, 3, 3)
    assert not ops.conv3x3_applies(x, w)  # on the host
    meta = torch.empty(1, 64, 8, 8, device="meta")
    assert not ops.conv3x3_applies(meta, w)
    assert not ops.conv3x3_applies(meta, torch.zeros(64, 64, 1, 1))  # 1x1
    assert not ops.conv3x3_applies(meta, torch.zeros(64, 64, 5, 5))  # 5x5
    assert not ops.conv3x3_applies(meta, torch.zeros(64, 32, 3, 3))  # grouped: Cin of the weight is not that of x
    assert not ops.conv3x3_applies(torch.empty(1, 48, 8, 8, device="meta"), torch.zeros(64, 48, 3, 3))  # Cin % 32
    assert not ops.conv3x3_applies(meta, torch.zeros(48, 64, 3, 3))  # N % 64
    assert not ops.conv3x3_applies(meta, w, stride=3)


def test_dilated_and_grouped_layers_are_not_routed():
    from weed_instance_segmentation_amd.backbone_resnet import _split_3x3
    x = torch.zeros(1, 64, 8, 8)
    for conv in (torch.nn.Conv2d(64, 64, 3, padding=2, dilation=2, bias=False),
                 torch.nn.Conv2d(64, 64, 3, padding=1, groups=2, bias=False),
                 torch.nn.Conv2d(64, 64, 3, padding=0, bias=False)):
        with torch.no_grad():
            assert not _split_3x3(conv, x, conv.weight)


@pytest.mark.parametrize("H,W,stride", [(5, 7, 1), (5, 7, 2), (1, 1, 1), (2, 3, 2), (6, 4, 1)])
def test_tap_major_reorder_times_im2col_is_the_convolution(H, W, stride):
    """Column k = (3 dy + dx) Cin + c of the kernel's B operand reads x[c, s ho + dy - 1, s wo + dx - 1] (zero outside);
    the weight reordered (N, 3, 3, Cin) and flattened is its A operand: their product is the convolution."""
    rng = np.random.default_rng(H * 31 + W * 7 + stride)
    Cin, N = 4, 3
    x = rng.standard_normal((Cin, H, W))
    w = rng.standard_normal((N, Cin, 3, 3))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    cols = np.zeros((9 * Cin, Ho * Wo))
    for ho in range(Ho):
        for wo in range(Wo):
            for dy in range(3):
                for dx in range(3):
                    hi, wi = stride * ho + dy - 1, stride * wo + dx - 1
                    if 0 <= hi < H and 0 <= wi < W:
                        cols[(3 * dy + dx) * Cin:(3 * dy + dx + 1) * Cin, ho * Wo + wo] = x[:, hi, wi]
    a = w.transpose(0, 2, 3, 1).reshape(N, 9 * Cin)
    got = (a @ cols).reshape(N, Ho, Wo)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x)[None], torch.from_numpy(w), None, stride, 1)[0].numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
