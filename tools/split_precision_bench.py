#!/usr/bin/env python3
"""Time every distinct call site of the split-bf16 kernels in the default forward (bench.py's model, B = 8 at 1024^2) at the
three inference precisions, alternating the levels in one process.

The sites are found, not listed: one forward runs with the six entry points (ops.token_linear, conv1x1, conv1x1_gn,
conv3x3, conv3x3_stats, stem_conv_pool) wrapped, and the first call of every distinct (function, shapes, epilogue) is kept
with its arguments.  Each site is then replayed on those arguments: warmed at every level, then `rounds` rounds of
highest / high / medium, each a window of `reps` launches between two HIP events (reps sized for a window of about 20 ms).

One JSON line per site: launches per forward, us per launch at each level (the minimum over the rounds, and all rounds),
the ratios to "highest", the MFMA floor with 6, 3 or 1 products (2 M N K flop per product against 2.5 PFLOP/s) and the
share of the launch it explains.  A last line per level: the kernel-timer sum of one traced forward (split sites and all
tagged kernels), and the sum of launches x us over the sites.
usage: split_precision_bench.py [--batch 8] [--size 1024] [--rounds 3] [--out profiles/split_precision_bench.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import weed_instance_segmentation_amd as pkg  # noqa: E402
from weed_instance_segmentation_amd import ops  # noqa: E402

LEVELS = ("highest", "high", "medium")
PRODUCTS = {"highest": 6, "high": 3, "medium": 1}
FUNCS = ("token_linear", "conv1x1", "conv1x1_gn", "conv3x3", "conv3x3_stats", "stem_conv_pool")
PEAK_FLOPS = 2.5e15
SPLIT_PREFIXES = ("conv1x1_K", "conv3x3_C", "stem7x7_pool")


def is_split_tag(tag):
    return tag.startswith(SPLIT_PREFIXES) or (tag.startswith("token_linear_") and "_split" in tag)


def describe(name, args, kwargs):
    """(key, M N K of the GEMM the site runs) from the call's arguments."""
    x, w = args[0], args[1]
    get = lambda i, k, d=None: args[i] if len(args) > i else kwargs.get(k, d)
    if name == "token_linear":
        N, K = w.shape
        M = x.numel() // K
        epi = ("relu" if get(3, "relu", False) else "bias") + ("+ln" if get(5, "ln") is not None else "") + \
              ("+pos" if get(6, "pos") is not None else "") + (f"+g{get(7, 'out_group', 0)}" if get(7, "out_group", 0) else "")
        return f"token_linear K{K} N{N} M{M} {epi}", (M, N, K)
    B, C, H, W = x.shape
    N = w.shape[0]
    if name == "stem_conv_pool":
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return f"stem7x7_pool Cin{C} {H}x{W} B{B}", (B * Hc * Wc, N, 160)
    if name in ("conv1x1", "conv1x1_gn"):
        stride = get(5, "stride", 1) if name == "conv1x1" else get(3, "stride", 1)
        P = ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
        if name == "conv1x1":
            epi = "res" if get(3, "residual") is not None else ("relu" if get(4, "relu", False) else ("bias" if get(2, "bias") is not None else "raw"))
        else:
            epi = "norm" if kwargs.get("norm") is not None else "stats"
        return f"{name} K{C} N{N} P{P} s{stride} B{B} {epi}", (B * P, N, C)
    stride = get(4, "stride", 1) if name == "conv3x3" else get(3, "stride", 1)
    P = ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    epi = "stats" if name == "conv3x3_stats" else ("relu" if get(3, "relu", False) else ("bias" if get(2, "bias") is not None else "raw"))
    return f"{name} C{C} N{N} P{P} s{stride} B{B} {epi}", (B * P, N, 9 * C)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("split_precision_bench.py needs an MI355X")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import build_model
    model = build_model(0).cuda().eval()
    x = torch.randn(a.batch, 3, a.size, a.size, generator=torch.Generator().manual_seed(1000)).cuda()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def forward():
        with torch.no_grad():
            return model(pixel_values=x)

    for _ in range(2):
        forward()
    # ---- find the sites
    sites, real = {}, {name: getattr(ops, name) for name in FUNCS}
    for name in FUNCS:
        def wrapped(*args, _n=name, **kwargs):
            key, mnk = describe(_n, args, kwargs)
            if key not in sites:
                sites[key] = {"name": _n, "args": args, "kwargs": kwargs, "mnk": mnk, "launches": 0}
            sites[key]["launches"] += 1
            return real[_n](*args, **kwargs)
        setattr(ops, name, wrapped)
    try:
        forward()
    finally:
        for name in FUNCS:
            setattr(ops, name, real[name])
    torch.cuda.synchronize()

    # ---- replay each site at the three levels
    totals = {level: 0.0 for level in LEVELS}
    for key, s in sites.items():
        fn = lambda: real[s["name"]](*s["args"], **s["kwargs"])
        try:
            for level in LEVELS:
                with pkg.inference_precision(level):
                    for _ in range(3):
                        fn()
            with pkg.inference_precision("highest"):
                reps = max(5, min(2000, int(20e3 / max(timed(fn, 5), 1.0))))
            us = {level: [] for level in LEVELS}
            for _ in range(a.rounds):
                for level in LEVELS:
                    with pkg.inference_precision(level):
                        us[level].append(round(timed(fn, reps), 2))
        except Exception as e:  # one site must not lose the others
            emit({"site": key, "error": repr(e)})
            continue
        M, N, K = s["mnk"]
        best = {level: min(v) for level, v in us.items()}
        floor = {level: PRODUCTS[level] * 2.0 * M * N * K / PEAK_FLOPS * 1e6 for level in LEVELS}
        for level in LEVELS:
            totals[level] += s["launches"] * best[level]
        emit({"site": key, "launches_per_forward": s["launches"], "reps": reps, "M": M, "N": N, "K": K,
              "us": best, "us_rounds": us,
              "ratio_to_highest": {level: round(best[level] / best["highest"], 3) for level in LEVELS},
              "mfma_floor_us": {level: round(floor[level], 2) for level in LEVELS},
              "mfma_share": {level: round(floor[level] / best[level], 3) for level in LEVELS}})

    # ---- one traced forward per level
    for level in LEVELS:
        with pkg.inference_precision(level):
            forward()
            timer = ops.KernelTimer()
            torch.cuda.synchronize()
            ops.set_kernel_timer(timer)
            try:
                forward()
                torch.cuda.synchronize()
            finally:
                ops.set_kernel_timer(None)
        ks = timer.summary()
        emit({"level": level, "traced_forward_split_kernels_ms": round(sum(n * us for t, (n, us) in ks.items() if is_split_tag(t)) / 1e3, 3),
              "traced_forward_all_tagged_kernels_ms": round(sum(n * us for n, us in ks.values()) / 1e3, 3),
              "sites_launches_x_us_ms": round(totals[level] / 1e3, 3), "batch": a.batch, "size": a.size})
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
