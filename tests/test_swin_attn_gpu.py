"""wm2f_swin_window_attn_fwd (csrc/swin_attn.hip) on the GPU: the op against the float64 contract
(swin_attn_reference.py, pinned to the stock route by test_swin_attn_cpu.py), the Swin-L stage shapes at 1024 x 1024,
the bf16 form against the stock bf16-autocast arithmetic on the same inputs, the Swin backbone's inference route against
the transformers fixture with the fused calls counted, the routing rules, and HIP-graph capture."""
import json

import pytest
import torch

from conftest import load_golden
from swin_attn_reference import gather_windows, scatter_windows, swin_window_attention_reference, window_slots

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from weed_instance_segmentation_amd import ops as _ops
    return _ops


def _inputs(B, dims, heads, D, ws, qkv_bias, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    N, E = dims[0] * dims[1], heads * D
    r = lambda *s: torch.randn(*s, generator=g)
    q, k, v = (r(B, N, E).to(dtype).cuda() for _ in range(3))
    table = r((2 * ws - 1) ** 2, heads).cuda()
    k_pad, v_pad = (r(E).to(dtype).cuda(), r(E).to(dtype).cuda()) if qkv_bias else (None, None)
    return q, k, v, table, k_pad, v_pad


CASES = [(ws, 32) for ws in (4, 7, 12)] + [(4, 16)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("qkv_bias", [True, False])
@pytest.mark.parametrize("dims", [(24, 24), (17, 25), (5, 40)])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("ws,D", CASES)
def test_op_fp32_matches_contract(ops, ws, D, shifted, dims, qkv_bias, B):
    """Tolerance: that of test_kernels_gpu.py::test_k2_golden -- the same arithmetic on the same instruction."""
    heads, shift = 3, (ws // 2 if shifted else 0)
    q, k, v, table, k_pad, v_pad = _inputs(B, dims, heads, D, ws, qkv_bias, 1000 * ws + 10 * dims[0] + shift + B)
    out = ops.swin_window_attention(q, k, v, table, dims, heads, ws, shift, k_pad, v_pad)
    ref = swin_window_attention_reference(q, k, v, table, dims, heads, ws, shift, k_pad, v_pad)
    assert out.dtype == torch.float32 and out.shape == q.shape
    torch.testing.assert_close(out.double(), ref, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("side,heads,shift", [(256, 6, 6), (64, 24, 0), (64, 24, 6)])
def test_op_fp32_swin_large_stage_shapes(ops, side, heads, shift):
    """Swin-L at 1024 x 1024: stage 1 (256 x 256 tokens, 6 heads) and stage 3 (64 x 64, 24 heads), window 12 -- both pad."""
    dims = (side, side)
    q, k, v, table, k_pad, v_pad = _inputs(1, dims, heads, 32, 12, True, side + shift)
    out = ops.swin_window_attention(q, k, v, table, dims, heads, 12, shift, k_pad, v_pad)
    ref = swin_window_attention_reference(q, k, v, table, dims, heads, 12, shift, k_pad, v_pad)
    torch.testing.assert_close(out.double(), ref, rtol=1e-4, atol=2e-5)


def _stock_bf16(q, k, v, table, dims, heads, ws, shift, k_pad, v_pad):
    """The parent route's arithmetic on the same bf16 q / k / v: Attention.forward's lines after the projections, under
    bf16 autocast, with the layer's own bias module and shift mask; window order built by index (swin_attn_reference)."""
    from weed_instance_segmentation_amd.backbone_swin import Layer
    H, W = dims
    B, N, E = q.shape
    D, L = E // heads, ws * ws
    layer = Layer({"window_size": ws}, E, heads, 0.0, shift).cuda()
    with torch.no_grad():
        layer.attention.relative_position_bias.relative_position_bias_table.copy_(table)
    tok, real, _ = (t.cuda() for t in window_slots(H, W, ws, shift))
    sh = lambda t, pad: gather_windows(t, pad, tok, real).view(-1, L, heads, D).transpose(1, 2)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        qw, kw, vw = sh(q, None), sh(k, k_pad), sh(v, v_pad)
        bias = layer.attention.relative_position_bias()
        mask = layer._mask(-(-H // ws) * ws, -(-W // ws) * ws, torch.float32, q.device)
        if mask is not None:
            nW = mask.shape[0]
            bias = bias + mask[None, :, None].expand(qw.shape[0] // nW, -1, -1, -1, -1).reshape(-1, 1, L, L)
        a = torch.matmul(qw, kw.transpose(2, 3)) * D ** -0.5 + bias
        a = torch.nn.functional.softmax(a, dim=-1, dtype=torch.float32).to(qw.dtype)
        o = torch.matmul(a, vw).transpose(1, 2).reshape(B, -1, L, E)
    assert o.dtype == torch.bfloat16
    return scatter_windows(o, tok, real, B, N)


@pytest.mark.parametrize("dims", [(24, 24), (17, 25)])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("ws,D", CASES)
def test_op_bf16_no_worse_than_stock_bf16(ops, ws, D, shifted, dims):
    """bf16 form against the float64 contract on the same bf16-rounded inputs.  The bound is the error of the stock
    bf16-autocast arithmetic on those inputs (margin 1.0): the kernel keeps scores in fp32 where stock rounds them to bf16."""
    heads, shift, B = 3, (ws // 2 if shifted else 0), 2
    q, k, v, table, k_pad, v_pad = _inputs(B, dims, heads, D, ws, True, 77 * ws + dims[1] + shift, torch.bfloat16)
    out = ops.swin_window_attention(q, k, v, table, dims, heads, ws, shift, k_pad, v_pad)
    assert out.dtype == torch.bfloat16
    ref = swin_window_attention_reference(q, k, v, table, dims, heads, ws, shift, k_pad, v_pad)
    stock = _stock_bf16(q, k, v, table, dims, heads, ws, shift, k_pad, v_pad)
    err = lambda t: ((t.double() - ref).norm() / ref.norm()).item()
    e_fused, e_stock = err(out), err(stock)
    print(f"swin bf16 ws{ws} D{D} shift{shift} {dims}: fused {e_fused:.3e} stock {e_stock:.3e}")
    assert e_stock < 2e-2, "the stock comparison itself is broken"
    assert e_fused <= e_stock


def test_op_argument_checks(ops):
    from weed_instance_segmentation_amd._lib import Wm2fError
    q, k, v, table, k_pad, v_pad = _inputs(1, (8, 8), 2, 32, 4, True, 5)
    with pytest.raises(ValueError):
        ops.swin_window_attention(q, k, v, table, (8, 9), 2, 4, 0)
    with pytest.raises(ValueError):
        ops.swin_window_attention(q, k, v, table, (8, 8), 2, 4, 4)
    with pytest.raises(ValueError):
        ops.swin_window_attention(q, k, v, table[:, :1], (8, 8), 2, 4, 0)
    with pytest.raises(ValueError):  # head_dim 64: not built, never reached from the backbone
        ops.swin_window_attention(q, k, v, table[:, :1].contiguous(), (8, 8), 1, 4, 0)
    with pytest.raises(TypeError):
        ops.swin_window_attention(q, k.bfloat16(), v, table, (8, 8), 2, 4, 0)
    with pytest.raises(Wm2fError):  # no backward: nobody trains through it silently
        ops.swin_window_attention(q.clone().requires_grad_(), k, v, table, (8, 8), 2, 4, 0)
    with torch.no_grad():
        ops.swin_window_attention(q.clone().requires_grad_(), k, v, table, (8, 8), 2, 4, 0)


def _count_fused(monkeypatch, ops):
    calls = []
    real = ops.swin_window_attention

    def counted(*a, **kw):
        calls.append(a[0].dtype)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "swin_window_attention", counted)
    return calls


def _fixture_backbone():
    from weed_instance_segmentation_amd.backbone_swin import SwinBackbone
    g = load_golden("swin_tiny_backbone.npz")
    cfg = json.loads(str(g["config_json"]))
    m = SwinBackbone(cfg)
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    return g, cfg, m.cuda()


def test_backbone_inference_runs_fused_and_matches_fixture(ops, monkeypatch):
    """transformers' SwinBackbone fixture (70 x 98 and 64 x 64 inputs: every padding path, both shifts) at the CPU
    test's tolerance, through the fused op: one call per layer."""
    g, cfg, m = _fixture_backbone()
    m.eval()
    calls = _count_fused(monkeypatch, ops)
    for tag in ("a", "b"):
        del calls[:]
        with torch.no_grad():
            fm = m(torch.from_numpy(g[f"x_{tag}"]).cuda())
        assert len(calls) == sum(cfg["depths"]) and all(d == torch.float32 for d in calls)
        for i, f in enumerate(fm):
            torch.testing.assert_close(f.cpu(), torch.from_numpy(g[f"fm_{tag}_{i}"]), rtol=1e-4, atol=1e-4)


def test_backbone_fused_and_stock_routes_agree_under_autocast(ops, monkeypatch):
    from weed_instance_segmentation_amd import backbone_swin
    g, cfg, m = _fixture_backbone()
    m.eval()
    x = torch.from_numpy(g["x_a"]).cuda()
    calls = _count_fused(monkeypatch, ops)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        fused = m(x)
    assert len(calls) == sum(cfg["depths"]) and all(d == torch.bfloat16 for d in calls)
    monkeypatch.setattr(backbone_swin, "FUSED_WINDOW_ATTENTION", False)
    del calls[:]
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        stock = m(x)
    assert not calls
    for a, b in zip(fused, stock):  # two bf16 evaluations of one network: agreement at bf16 resolution of the features
        assert ((a.float() - b.float()).norm() / b.float().norm()).item() < 3e-2


def test_routing_training_and_unsupported_head_dim_stay_stock(ops, monkeypatch):
    from weed_instance_segmentation_amd.backbone_swin import SwinBackbone
    g, cfg, m = _fixture_backbone()
    calls = _count_fused(monkeypatch, ops)
    m.train()
    x = torch.from_numpy(g["x_a"]).cuda()
    sum(f.square().mean() for f in m(x)).backward()
    assert not calls
    grads = [p.grad for n, p in m.named_parameters() if not n.startswith("swin.layernorm.")]
    assert all(gr is not None and torch.isfinite(gr).all() for gr in grads)
    m.eval()  # eval alone does not switch: parameters still require grad and grad mode is on
    m(x)
    assert not calls
    for p in m.parameters():
        p.requires_grad_(False)
    m(x)  # frozen backbone, grad mode on: nothing to record
    assert len(calls) == sum(cfg["depths"])
    del calls[:]
    m24 = SwinBackbone({"embed_dim": 24, "depths": [1, 1], "num_heads": [1, 2], "window_size": 7,
                        "out_features": ["stage1", "stage2"]}).cuda().eval()
    with torch.no_grad():
        out = m24(torch.randn(1, 3, 64, 64, device="cuda"))
    assert not calls and all(torch.isfinite(f).all() for f in out)


def test_graph_capture_replays_to_eager(ops, monkeypatch):
    """The op allocates nothing and launches on the current stream: a captured forward of a tiny Swin model replays to the
    eager numbers, also after the input changes."""
    from weed_instance_segmentation_amd import Mask2FormerConfig, Mask2FormerForUniversalSegmentation
    from weed_instance_segmentation_amd.graph import GraphedForward
    cd = json.loads(str(load_golden("full_tiny.npz")["config_json"]))
    cd["backbone_config"] = {"model_type": "swin", "embed_dim": 16, "depths": [1, 1, 2, 1], "num_heads": [1, 2, 4, 4],
                             "window_size": 4, "mlp_ratio": 2.0, "patch_size": 4, "num_channels": 3,
                             "out_features": ["stage1", "stage2", "stage3", "stage4"], "drop_path_rate": 0.0}
    torch.manual_seed(3)
    model = Mask2FormerForUniversalSegmentation(Mask2FormerConfig.from_dict(cd)).cuda().eval()
    x1 = torch.randn(2, 3, 72, 104, device="cuda")  # 18 x 26 tokens: padding on both axes
    x2 = torch.randn_like(x1)
    calls = _count_fused(monkeypatch, ops)
    fwd = GraphedForward(model, x1)
    assert calls
    for x in (x1, x2, x1):
        out = fwd(x)
        with torch.no_grad():
            ref = model(pixel_values=x)
        scale = ref.masks_queries_logits.abs().max().item()
        assert (out.masks_queries_logits - ref.masks_queries_logits).abs().max().item() / scale < 1e-5
