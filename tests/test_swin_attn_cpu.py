"""Fused shifted-window attention, the part that needs no GPU: the op refuses CPU tensors, the predicate answers as
documented, the CPU route of the Swin backbone is what it was, and the float64 restatement of the kernel's contract
(swin_attn_reference.py) IS the stock route's arithmetic -- padding-token rule, shift and mask included."""
import json

import pytest
import torch

from conftest import load_golden
from swin_attn_reference import swin_window_attention_reference


def test_op_refuses_cpu_tensors():
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd._lib import Wm2fError
    q = torch.randn(1, 16, 32)
    with pytest.raises(Wm2fError):
        ops.swin_window_attention(q, q, q, torch.zeros(49, 1), (4, 4), 1, 4, 0)
    with pytest.raises(Wm2fError):
        ops.swin_window_attention(q.bfloat16(), q.bfloat16(), q.bfloat16(), torch.zeros(49, 1), (4, 4), 1, 4, 2)


def test_predicate():
    from weed_instance_segmentation_amd.ops import swin_window_attention_applies as applies
    for ws in (4, 7, 12):
        for D in (16, 32):
            for dt in (torch.float32, torch.bfloat16):
                assert applies(ws, D, dt, "cuda")
                assert applies(ws, D, dt, torch.device("cuda", 0))
                assert not applies(ws, D, dt, "cpu")
    assert not applies(7, 24, torch.float32, "cuda")  # the reduced-width model of test_config4
    assert not applies(7, 24, torch.bfloat16, "cuda")
    assert not applies(7, 64, torch.float32, "cuda")
    assert not applies(8, 32, torch.float32, "cuda")
    assert not applies(7, 32, torch.float16, "cuda")
    assert not applies(7, 32, torch.float64, "cuda")


def test_cpu_backbone_route_unchanged():
    from weed_instance_segmentation_amd.backbone_swin import SwinBackbone
    g = load_golden("swin_tiny_backbone.npz")
    m = SwinBackbone(json.loads(str(g["config_json"]))).eval()
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    for tag in ("a", "b"):
        with torch.no_grad():
            fm = m(torch.from_numpy(g[f"x_{tag}"]))
        for i, f in enumerate(fm):
            torch.testing.assert_close(f, torch.from_numpy(g[f"fm_{tag}_{i}"]), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("qkv_bias", [True, False])
@pytest.mark.parametrize("dims", [(24, 24), (17, 25), (5, 40), (3, 3)])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("ws", [4, 7, 12])
def test_contract_is_the_stock_route(ws, shifted, dims, qkv_bias):
    """Stock Layer in float64 on CPU, o_proj the identity and the MLP's output zeroed: forward(x) - x is the layer's
    attention in image order.  The contract, fed with the same Linears' image-order q / k / v and their biases as the
    padding rows, must give the same numbers to float32 rounding of a probability (the stock softmax is float32)."""
    from weed_instance_segmentation_amd.backbone_swin import Layer
    heads, D = 2, 16
    dim, shift = heads * D, (ws // 2 if shifted else 0)
    torch.manual_seed(ws * 100 + shift * 10 + dims[0])
    layer = Layer({"window_size": ws, "qkv_bias": qkv_bias, "mlp_ratio": 1.0}, dim, heads, 0.0, shift).double().eval()
    at = layer.attention
    with torch.no_grad():
        at.relative_position_bias.relative_position_bias_table.normal_()
        for lin in (at.q_proj, at.k_proj, at.v_proj):
            if lin.bias is not None:
                lin.bias.normal_()
        at.o_proj.weight.copy_(torch.eye(dim, dtype=torch.float64))
        at.o_proj.bias.zero_()
        layer.mlp.fc2.weight.zero_()
        layer.mlp.fc2.bias.zero_()
        H, W = dims
        x = torch.randn(2, H * W, dim, dtype=torch.float64)
        stock = layer(x, dims) - x
        h = layer.layernorm_before(x)
        ref = swin_window_attention_reference(at.q_proj(h), at.k_proj(h), at.v_proj(h),
                                              at.relative_position_bias.relative_position_bias_table, dims, heads, ws, shift,
                                              at.k_proj.bias, at.v_proj.bias)
    torch.testing.assert_close(ref, stock, rtol=0, atol=1e-6)
