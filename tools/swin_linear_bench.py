"""The Swin backbone's Linears on the split-bf16 kernel (ops.swin_linear) against the stock route
(F.linear, then F.gelu or the add; three F.linear calls for q, k and v), fp32, 1024 x 1024 inputs.

    python tools/swin_linear_bench.py --mode sites --model swin_l [--batches 1 8] [--rounds 5] [--iters 10] [--out ...]
    python tools/swin_linear_bench.py --mode backbones [--model swin_l]

One process per call, each under its own time limit and chained, with at most 16 CPU threads:

    timeout -k 10 300 python tools/swin_linear_bench.py --mode sites --model swin_t && \\
    timeout -k 10 300 python tools/swin_linear_bench.py --mode sites --model swin_b && \\
    timeout -k 10 400 python tools/swin_linear_bench.py --mode sites --model swin_l && \\
    timeout -k 10 400 python tools/swin_linear_bench.py --mode backbones

`sites`: per (model, stage, call site qkv | o_proj | fc1 | fc2 | reduction, B) one JSON line with `stock_ms` and, per level,
`ms[level][config]` for every entry of the kernel's tile table, `host_config` (wm2f_swin_linear_split_config), and the bf16
MFMA throughput of the fastest entry, 2 M N K x products(level) / time.  HIP-event times per call, medians over --rounds
rounds of --iters calls, all routes alternating round by round in one process after 3 warm-up calls each.
`backbones`: SwinBackbone.forward, B = 1 and B = 8, ops.SWIN_LINEAR_SPLIT False against True at the three levels: `off_ms`,
`on_ms[level]`, and `off_spread_ms`, the spread (max - min) of the flag-off rounds: the route is a level's default when it
beats flag-off by more than that spread on the Swin-L B = 8 line.
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

from weed_instance_segmentation_amd import ops  # noqa: E402
from weed_instance_segmentation_amd._lib import load  # noqa: E402
from weed_instance_segmentation_amd.backbone_swin import SwinBackbone  # noqa: E402

MODELS = {
    "swin_t": {"embed_dim": 96, "depths": [2, 2, 6, 2], "num_heads": [3, 6, 12, 24], "window_size": 7},
    "swin_b": {"embed_dim": 128, "depths": [2, 2, 18, 2], "num_heads": [4, 8, 16, 32], "window_size": 12},
    "swin_l": {"embed_dim": 192, "depths": [2, 2, 18, 2], "num_heads": [6, 12, 24, 48], "window_size": 12},
}
LEVELS = ("highest", "high", "medium")
PRODUCTS = {"highest": 6, "high": 3, "medium": 1}


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, rounds, iters):
    """Per function the list of its rounds' times, the functions alternating round by round."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(times, fns):
            t.append(event_ms(fn, iters))
    return times


def sites_of(cfg):
    """(stage, site, K, N, tokens per image at 1024 x 1024)"""
    out = []
    for s in range(4):
        C, tok = cfg["embed_dim"] << s, (256 >> s) ** 2
        out += [(s + 1, "qkv", C, 3 * C, tok), (s + 1, "o_proj", C, C, tok), (s + 1, "fc1", C, 4 * C, tok), (s + 1, "fc2", 4 * C, C, tok)]
        if s < 3:
            out.append((s + 1, "reduction", 4 * C, 2 * C, tok // 4))
    return out


def bench_sites(name, args, f):
    n_cfg = int(load().wm2f_swin_linear_split_configs())
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for stage, site, K, N, tok in sites_of(MODELS[name]):
        for B in args.batches:
            M = B * tok
            g = torch.Generator(device="cuda").manual_seed(stage)
            x = torch.randn(M, K, device="cuda", generator=g)
            w = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
            b = None if site == "reduction" else torch.randn(N, device="cuda", generator=g)
            r = torch.randn(M, N, device="cuda", generator=g) if site in ("o_proj", "fc2") else None
            ws = ops.split_weight(w)
            kw = {"gelu": site == "fc1", "residual": r, "n_out": 3 if site == "qkv" else 1, "w_split": ws}

            def stock():
                if site == "qkv":
                    C = N // 3
                    return [F.linear(x, w[i * C:(i + 1) * C], b[i * C:(i + 1) * C]) for i in range(3)]
                y = F.linear(x, w, b)
                return F.gelu(y) if site == "fc1" else (y + r if r is not None else y)

            def split(level, c):
                def fn():
                    ops.SPLIT_PRECISION = level
                    return ops.swin_linear(x, w, b, config=c, **kw)
                return fn

            fns = [stock] + [split(level, c) for level in LEVELS for c in range(n_cfg)]
            with torch.no_grad():
                times = alternate(fns, args.rounds, args.iters)
            ops.SPLIT_PRECISION = "highest"
            med = [statistics.median(t) for t in times]
            rec = {"model": name, "stage": stage, "site": site, "B": B, "M": M, "K": K, "N": N, "stock_ms": round(med[0], 4),
                   "ms": {}, "host_config": {}, "best_tflops_bf16": {}, "speedup_host": {}}
            for li, level in enumerate(LEVELS):
                ms = med[1 + li * n_cfg:1 + (li + 1) * n_cfg]
                host = int(load().wm2f_swin_linear_split_config(M, N, 3 - li, n_cu))
                rec["ms"][level] = [round(t, 4) for t in ms]
                rec["host_config"][level] = host
                rec["best_tflops_bf16"][level] = round(2.0 * M * N * K * PRODUCTS[level] / (min(ms) * 1e-3) / 1e12, 1)
                rec["speedup_host"][level] = round(med[0] / ms[host], 2)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            del x, w, r, ws
            torch.cuda.empty_cache()


def bench_backbones(args, f):
    for name in ([args.model] if args.model else list(MODELS)):
        model = SwinBackbone({**MODELS[name], "out_features": ["stage1", "stage2", "stage3", "stage4"]}).cuda().eval()
        for B in args.batches:
            x = torch.randn(B, 3, 1024, 1024, device="cuda")

            def run(flag, level):
                def fn():
                    ops.SWIN_LINEAR_SPLIT, ops.SPLIT_PRECISION = flag, level
                    with torch.no_grad():
                        return model(x)
                return fn

            times = alternate([run(False, "highest")] + [run(True, level) for level in LEVELS], args.rounds, max(args.iters // 2, 1))
            ops.SPLIT_PRECISION = "highest"
            off = times[0]
            rec = {"model": name, "whole_backbone_forward": True, "input": [1024, 1024], "B": B, "dtype": "float32",
                   "off_ms": round(statistics.median(off), 3), "off_spread_ms": round(max(off) - min(off), 3), "on_ms": {},
                   "on_spread_ms": {}, "speedup": {}}
            for level, t in zip(LEVELS, times[1:]):
                rec["on_ms"][level] = round(statistics.median(t), 3)
                rec["on_spread_ms"][level] = round(max(t) - min(t), 3)
                rec["speedup"][level] = round(statistics.median(off) / statistics.median(t), 2)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            del x
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["sites", "backbones"])
    ap.add_argument("--model", default=None, choices=list(MODELS))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin_linear_bench.jsonl"))
    args = ap.parse_args()
    if args.mode == "sites" and args.model is None:
        raise SystemExit("--mode sites needs --model")
    if not torch.cuda.is_available():
        raise SystemExit("swin_linear_bench needs an MI355X")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        (bench_sites(args.model, args, f) if args.mode == "sites" else bench_backbones(args, f))


if __name__ == "__main__":
    main()
