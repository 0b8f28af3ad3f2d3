"""Per-instance statistics on the GPU: the one-launch route against the composed torch route.

    python tools/instance_stats_bench.py [--rounds 7] [--out profiles/instance_stats_bench.jsonl]

Workload: B = 8 fp32 id maps of 1024 x 1024 (-1 background) with 16 and with 100 rectangular instances.  In one process,
alternating per round and timed with HIP events:
- `kernel`: `ops.labelmap_instance_stats` (init + the statistics kernel), `--inner` launches per timing;
- `composed`: per image and instance `seg == id`, `nonzero`, min / max / sum of the coordinates (one host sync per
  instance in `nonzero`) -- what a consumer of the post-processor's map does without the kernel.
One JSON line per shape: median and spread (min, max) over rounds of both, the speed-up, the kernel's bytes per second
(4 B per pixel read, 64 B per (image, id) written) against 8 TB/s, and that both routes gave the same numbers.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from weed_instance_segmentation_amd import ops  # noqa: E402

HBM_BPS = 8e12


def make_maps(B, H, W, n, seed):
    g = torch.Generator().manual_seed(seed)
    maps = torch.full((B, H, W), -1.0)
    for b in range(B):
        for k in range(n):
            y0, x0 = (int(torch.randint(0, H - 16, (1,), generator=g)), int(torch.randint(0, W - 16, (1,), generator=g)))
            h, w = (int(torch.randint(8, 320, (1,), generator=g)), int(torch.randint(8, 320, (1,), generator=g)))
            maps[b, y0:y0 + h, x0:x0 + w] = k
    return maps


def composed(maps, n):
    B, H, W = maps.shape
    out = torch.zeros(B, n, 8, dtype=torch.int64, device=maps.device)
    out[:, :, 1], out[:, :, 2], out[:, :, 3], out[:, :, 4] = W, H, -1, -1
    for b in range(B):
        for k in range(n):
            ys, xs = torch.nonzero(maps[b] == k, as_tuple=True)
            if ys.numel():
                out[b, k, :7] = torch.stack([torch.tensor(ys.numel(), device=maps.device), xs.min(), ys.min(), xs.max(),
                                             ys.max(), xs.sum(), ys.sum()])
    return out


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_stats_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("instance_stats_bench needs an MI355X")
    B, H, W = 8, 1024, 1024
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for n in (16, 100):
            maps = make_maps(B, H, W, n, seed=n).cuda()
            same = bool(torch.equal(ops.labelmap_instance_stats(maps, N=n), composed(maps, n)))
            for _ in range(3):
                ops.labelmap_instance_stats(maps, N=n)
            k_ms, c_ms = [], []
            for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat both alike
                k_ms.append(event_ms(lambda: ops.labelmap_instance_stats(maps, N=n), args.inner))
                c_ms.append(event_ms(lambda: composed(maps, n), 1))
            km, cm = statistics.median(k_ms), statistics.median(c_ms)
            nbytes = maps.numel() * 4 + B * n * 64
            rec = {"B": B, "H": H, "W": W, "instances": n, "rounds": args.rounds, "inner": args.inner,
                   "kernel_us": {"median": round(km * 1e3, 2), "min": round(min(k_ms) * 1e3, 2), "max": round(max(k_ms) * 1e3, 2)},
                   "composed_ms": {"median": round(cm, 2), "min": round(min(c_ms), 2), "max": round(max(c_ms), 2)},
                   "speedup": round(cm / km, 1), "kernel_bytes": nbytes, "kernel_TBps": round(nbytes / (km * 1e-3) / 1e12, 3),
                   "fraction_of_8TBps": round(nbytes / (km * 1e-3) / HBM_BPS, 3), "routes_equal": same}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
