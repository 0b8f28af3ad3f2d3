"""Fused shifted-window attention (ops.swin_window_attention) against the stock route of
backbone_swin.py at the stage shapes of Swin-T (window 7), Swin-B and Swin-L (window 12).

    python tools/swin_attn_bench.py --model swin_t [--rounds 5] [--iters 10] [--out profiles/swin_window_attn_bench.jsonl]
    python tools/swin_attn_bench.py --model backbones          # whole-backbone forwards, one line per model and dtype

One process per --model, each under its own time limit and chained, with at most 16 CPU threads:

    timeout -k 10 300 python tools/swin_attn_bench.py --model swin_t && \\
    timeout -k 10 300 python tools/swin_attn_bench.py --model swin_b && \\
    timeout -k 10 300 python tools/swin_attn_bench.py --model swin_l && \\
    timeout -k 10 300 python tools/swin_attn_bench.py --model backbones

Per (model, stage, input 1024 x 1024 | 800 x 1344, B = 1 | 8, fp32 | bf16, shifted layer) one JSON line:
- `fused_ms`: the op alone on image-order q / k / v (the Linears are outside both routes);
- `stock_ms`: the same file's stock route between the Linears: pad, roll, window partition (of q, k and v here, of the
  one input there), Attention.forward's arithmetic with the layer's bias module and shift mask, window reverse, roll,
  crop; under bf16 autocast for the bf16 lines, as the parent route runs;
- both are HIP-event times per call, median over --rounds rounds of --iters calls, the two routes alternating round by
  round in one process after 3 warm-up calls each; `max_abs_diff` compares their outputs.
The `backbones` lines time SwinBackbone.forward (B = 1, 1024 x 1024) with backbone_swin.FUSED_WINDOW_ATTENTION on and off.

--train times forward + backward instead (default --out profiles/swin_window_attn_bwd_bench.jsonl), 1024 x 1024 only:
ops.swin_window_attention_train against the same stock lines with autograd on, q / k / v and the bias table requiring
grad, one fixed cotangent (`"train": true` lines; `max_rel_diff_grad_q` compares the two routes' grad_q); the `backbones`
lines are SwinBackbone in train() with every parameter requiring grad, forward + backward of sum(f.square().mean()).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from weed_instance_segmentation_amd import backbone_swin, ops  # noqa: E402
from weed_instance_segmentation_amd.backbone_swin import Layer, SwinBackbone, _window_partition, _window_reverse  # noqa: E402

MODELS = {
    "swin_t": {"embed_dim": 96, "depths": [2, 2, 6, 2], "num_heads": [3, 6, 12, 24], "window_size": 7},
    "swin_b": {"embed_dim": 128, "depths": [2, 2, 18, 2], "num_heads": [4, 8, 16, 32], "window_size": 12},
    "swin_l": {"embed_dim": 192, "depths": [2, 2, 18, 2], "num_heads": [6, 12, 24, 48], "window_size": 12},
}
INPUTS = [(1024, 1024), (800, 1344)]


def stock_attention(layer: Layer, q, k, v, dims):
    """backbone_swin.Layer.forward between the Linears, on projected tokens (the padding rows are zeros: bias-free)."""
    H, W = dims
    B, _, C = q.shape
    ws, at = layer.ws, layer.attention
    pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws
    Hp, Wp = H + pb, W + pr

    def windows(t):
        t = F.pad(t.view(B, H, W, C), (0, 0, 0, pr, 0, pb))
        if layer.shift > 0:
            t = torch.roll(t, shifts=(-layer.shift, -layer.shift), dims=(1, 2))
        t = _window_partition(t, ws).view(-1, ws * ws, C)
        return t.view(t.shape[0], ws * ws, at.heads, at.head_dim).transpose(1, 2)

    qw, kw, vw = windows(q), windows(k), windows(v)
    nB, L = qw.shape[0], ws * ws
    bias = at.relative_position_bias()
    mask = layer._mask(Hp, Wp, torch.float32, q.device)  # the layer-norm output's dtype, also under autocast
    if mask is not None:
        nW = mask.shape[0]
        bias = bias + mask[None, :, None].expand(nB // nW, -1, -1, -1, -1).reshape(-1, 1, L, L)
    a = torch.matmul(qw, kw.transpose(2, 3)) * at.head_dim ** -0.5 + bias
    a = F.softmax(a, dim=-1, dtype=torch.float32).to(qw.dtype)
    a = torch.matmul(a, vw).transpose(1, 2).reshape(nB, L, C)
    a = _window_reverse(a.view(-1, ws, ws, C), ws, Hp, Wp)
    if layer.shift > 0:
        a = torch.roll(a, shifts=(layer.shift, layer.shift), dims=(1, 2))
    if pr > 0 or pb > 0:
        a = a[:, :H, :W, :].contiguous()
    return a.view(B, H * W, C)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, rounds, iters):
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(times, fns):
            t.append(event_ms(fn, iters))
    return [statistics.median(t) for t in times]


def bench_stages(name, args, f):
    cfg = MODELS[name]
    ws = cfg["window_size"]
    for size in (INPUTS[:1] if args.train else INPUTS):
        for stage, heads in enumerate(cfg["num_heads"]):
            dims = (size[0] // (4 << stage), size[1] // (4 << stage))
            dim = cfg["embed_dim"] << stage
            layer = Layer({"window_size": ws, "qkv_bias": False}, dim, heads, 0.0, ws // 2).cuda().eval()
            with torch.no_grad():
                layer.attention.relative_position_bias.relative_position_bias_table.normal_(std=0.5)
            table = layer.attention.relative_position_bias.relative_position_bias_table.detach()
            for B in (1, 8):
                for dtype in (torch.float32, torch.bfloat16):
                    g = torch.Generator(device="cuda").manual_seed(stage + B)
                    q, k, v = (torch.randn(B, dims[0] * dims[1], dim, device="cuda", generator=g).to(dtype) for _ in range(3))

                    def fused():
                        return ops.swin_window_attention(q, k, v, table, dims, heads, ws, layer.shift)

                    def stock():
                        with torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
                            return stock_attention(layer, q, k, v, dims)

                    if args.train:
                        param = layer.attention.relative_position_bias.relative_position_bias_table
                        leaves = [q.requires_grad_(), k.requires_grad_(), v.requires_grad_(), param]
                        cot = torch.randn(q.shape, device="cuda", generator=g).to(dtype)
                        fwd_fused = lambda: ops.swin_window_attention_train(q, k, v, param, dims, heads, ws, layer.shift)
                        fused_t = lambda: torch.autograd.grad(fwd_fused(), leaves, cot)
                        stock_t = lambda: torch.autograd.grad(stock(), leaves, cot)
                        gf, gs = fused_t()[0].float(), stock_t()[0].float()
                        diff = ((gf - gs).norm() / gs.norm()).item()
                        fused_ms, stock_ms = alternate([fused_t, stock_t], args.rounds, args.iters)
                        rec = {"model": name, "train": True, "stage": stage + 1, "input": list(size), "tokens": list(dims),
                               "B": B, "heads": heads, "head_dim": dim // heads, "window": ws, "shift": layer.shift,
                               "dtype": str(dtype).split(".")[1], "fused_ms": round(fused_ms, 4),
                               "stock_ms": round(stock_ms, 4), "speedup": round(stock_ms / fused_ms, 2),
                               "max_rel_diff_grad_q": diff}
                        print(json.dumps(rec), flush=True)
                        f.write(json.dumps(rec) + "\n")
                        del q, k, v, cot, gf, gs
                        torch.cuda.empty_cache()
                        continue
                    with torch.no_grad():
                        diff = (fused().float() - stock().float()).abs().max().item()
                        fused_ms, stock_ms = alternate([fused, stock], args.rounds, args.iters)
                    rec = {"model": name, "stage": stage + 1, "input": list(size), "tokens": list(dims), "B": B,
                           "heads": heads, "head_dim": dim // heads, "window": ws, "shift": layer.shift,
                           "dtype": str(dtype).split(".")[1], "fused_ms": round(fused_ms, 4), "stock_ms": round(stock_ms, 4),
                           "speedup": round(stock_ms / fused_ms, 2), "max_abs_diff": diff}
                    print(json.dumps(rec), flush=True)
                    f.write(json.dumps(rec) + "\n")
                    del q, k, v
                    torch.cuda.empty_cache()


def bench_backbones(args, f):
    for name, cfg in MODELS.items():
        model = SwinBackbone({**cfg, "out_features": ["stage1", "stage2", "stage3", "stage4"]}).cuda().eval()
        if args.train:
            model.train()
        x = torch.randn(1, 3, 1024, 1024, device="cuda")
        for dtype in (torch.float32, torch.bfloat16):
            def run(on):
                def fn():
                    backbone_swin.FUSED_WINDOW_ATTENTION = on
                    if args.train:
                        with torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
                            loss = sum(fm.square().mean() for fm in model(x))
                        model.zero_grad(set_to_none=True)
                        return loss.backward()
                    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
                        return model(x)
                return fn

            fused_ms, stock_ms = alternate([run(True), run(False)], args.rounds, max(args.iters // 2, 1))
            backbone_swin.FUSED_WINDOW_ATTENTION = True
            rec = {"model": name, "whole_backbone_forward_backward" if args.train else "whole_backbone_forward": True, "input": [1024, 1024], "B": 1,
                   "dtype": str(dtype).split(".")[1], "fused_ms": round(fused_ms, 3), "stock_ms": round(stock_ms, 3),
                   "speedup": round(stock_ms / fused_ms, 2)}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, choices=list(MODELS) + ["backbones"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--train", action="store_true", help="forward + backward instead of the inference forward")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "swin_window_attn_bwd_bench.jsonl" if args.train else "swin_window_attn_bench.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("swin_attn_bench needs an MI355X")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        if args.model == "backbones":
            bench_backbones(args, f)
        else:
            bench_stages(args.model, args, f)


if __name__ == "__main__":
    main()
