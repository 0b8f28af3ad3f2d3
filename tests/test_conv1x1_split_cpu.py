"""Host side of the split-bf16 1x1 convolution (csrc/conv1x1_split.hip): the tile configuration table
covers every site of the model, and the routing predicate refuses what the kernel does not build."""
import pytest
import torch

from weed_instance_segmentation_amd import _lib, ops

# (N, P, B) of the 1x1 sites: ResNet-50 + pixel decoder at B = 8, 1024^2, and the 800 x 1088 stage-4 map (P = 850)
SITES = [(64, 65536, 8), (256, 65536, 8), (128, 65536, 8), (512, 16384, 8), (128, 16384, 8), (256, 16384, 8),
         (1024, 4096, 8), (256, 4096, 8), (512, 4096, 8), (2048, 1024, 8), (512, 1024, 8), (256, 1024, 8),
         (512, 850, 8), (2048, 850, 1), (256, 850, 1)]
NT = [256, 256, 256, 128, 64]  # the table's workgroup tile widths (channels)


@pytest.mark.parametrize("N,P,B", SITES)
def test_every_site_has_a_configuration(N, P, B):
    ci = _lib.load().wm2f_conv1x1_split_config(N, P, B, 256)
    assert 0 <= ci < len(NT) and N % NT[ci] == 0


def test_configuration_refusals():
    lib = _lib.load()
    assert lib.wm2f_conv1x1_split_config(48, 1024, 1, 256) == -1  # no tile divides N
    assert lib.wm2f_conv1x1_split_config(64, 0, 1, 256) == -1


def test_conv1x1_applies_only_to_built_shapes():
    x = torch.zeros(1, 64, 8, 8)
    w = torch.zeros(64, 64, 1, 1)
    assert not ops.conv1x1_applies(x, w)  # on the host
    meta = torch.empty(1, 64, 8, 8, device="meta")
    assert not ops.conv1x1_applies(meta, w)
    assert not ops.conv1x1_applies(x, torch.zeros(64, 64, 3, 3))
