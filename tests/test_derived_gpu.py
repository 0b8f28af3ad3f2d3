"""derived.py on the GPU (DESIGN.md "Derived weights"): the fold and the splits of a backbone block follow a weight that
is replaced through `.data`, drop_derived answers a write through `.data`, the token Linears' splits follow their weights,
and a model that has run on the GPU can be saved."""
import io
import json

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def test_backbone_block_follows_data_writes(ops):
    from weed_instance_segmentation_amd import drop_derived
    from weed_instance_segmentation_amd.backbone_resnet import BottleNeckLayer
    from weed_instance_segmentation_amd.derived import derived_peek
    torch.manual_seed(0)
    blk = BottleNeckLayer(64, 256, 1).cuda().eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 1.5)
    conv2 = blk.layer[1]
    x = torch.randn(1, 64, 8, 12, device="cuda")

    def never_run():
        fresh = BottleNeckLayer(64, 256, 1).cuda().eval()
        fresh.load_state_dict(blk.state_dict())
        with torch.no_grad():
            return fresh(x)

    with torch.no_grad():
        out0 = blk(x)
    assert torch.equal(out0, never_run())
    # the fold, the 1x1 and the 3x3 split routes all ran
    assert [derived_peek(layer, "conv") is not None for layer in blk.layer] == [True, False, True]
    assert derived_peek(blk.shortcut, "conv") is not None and all(derived_peek(m, "fold") is not None for m in blk.layer)
    fold0, split0 = derived_peek(conv2, "fold"), derived_peek(conv2, "conv3x3")
    assert split0.dtype == torch.uint8 and split0.numel() == 64 * 9 * 64 * 6

    p = conv2.convolution.weight
    p.data = p.data * -1.5  # another storage: the same object, the same _version
    with torch.no_grad():
        out1 = blk(x)
    fold1, split1 = derived_peek(conv2, "fold"), derived_peek(conv2, "conv3x3")
    assert fold1[0] is not fold0[0] and not torch.equal(fold1[0], fold0[0])
    assert split1 is not split0 and not torch.equal(split1, split0)
    assert not torch.equal(out1, out0)
    assert torch.equal(out1, never_run())

    p.data.mul_(2)  # nothing a key can see: drop_derived is the answer
    drop_derived(blk)
    assert derived_peek(conv2, "fold") is None and derived_peek(conv2, "conv3x3") is None
    with torch.no_grad():
        out2 = blk(x)
    assert not torch.equal(out2, out1)
    assert torch.equal(out2, never_run())


def test_token_linear_splits_follow_their_weights(ops):
    """The cached splits of an encoder layer (output_proj, fc1 plain and in the fused kernel's row order, fc2) on a bare owner,
    K = N = 256, M = 64."""
    from weed_instance_segmentation_amd.derived import derived_peek
    torch.manual_seed(1)
    owner = type("D", (), {})()
    lins = {n: torch.nn.Linear(256, 256).cuda() for n in ("output_proj", "fc1", "fc2")}
    x = torch.randn(64, 256, device="cuda")

    def split(name):
        if name == "fc1_ffn":
            return ops.split_weight_rows_cached(owner, name, lins["fc1"].weight)
        return ops.split_weight_cached(owner, name, lins[name].weight)

    for name in ("output_proj", "fc1", "fc1_ffn", "fc2"):
        lin = lins[name[:3] if name == "fc1_ffn" else name]
        with torch.no_grad():
            s0 = split(name)
            assert split(name) is s0 and derived_peek(owner, name) is s0  # no re-split without a change
            fresh0 = ops.split_weight_rows(lin.weight) if name == "fc1_ffn" else ops.split_weight(lin.weight)
            assert torch.equal(s0, fresh0)
            if name != "fc1_ffn":
                y0 = ops.token_linear(x, lin.weight, lin.bias, w_split=s0)
                assert torch.equal(y0, ops.token_linear(x, lin.weight, lin.bias))
            lin.weight.mul_(1.5)
            s1 = split(name)
            assert s1 is not s0 and not torch.equal(s1, s0)
            assert split(name) is s1
            if name != "fc1_ffn":
                y1 = ops.token_linear(x, lin.weight, lin.bias, w_split=s1)
                assert not torch.equal(y1, y0) and torch.equal(y1, ops.token_linear(x, lin.weight, lin.bias))


def test_a_model_that_ran_on_the_gpu_can_be_saved(ops):
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    g = load_golden("full_tiny.npz")
    torch.manual_seed(0)
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig.from_dict(json.loads(str(g["config_json"])))).cuda().eval()
    x = torch.from_numpy(g["pixel_values"]).cuda()
    with torch.no_grad():
        out = model(pixel_values=x).masks_queries_logits
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    with torch.no_grad():
        assert torch.equal(loaded(pixel_values=x).masks_queries_logits, out)
