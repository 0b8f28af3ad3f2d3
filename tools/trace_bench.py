"""Tracing id maps into polygons on the GPU: the launch chain against the plain-loop restatement.

    python tools/trace_bench.py [--runs 20] [--out profiles/trace_bench.jsonl] [--skip-baseline | --baseline-only]

Workload: fp32 id maps of 1024 x 1024 (-1 background) with 10, 300 and 3000 elliptic blobs per image (ids k mod 1024,
the kernels' cap), B = 1 and B = 8, pixel coordinates with simplify.  Per case one JSON line:
- `call_ms`: a host clock round `ops.labelmap_trace`, device synchronise before and after (median, min, max of --runs);
- `passes_us`: the HIP-event time of every launch group of the call (`ops.KernelTimer`), medians over the same runs; the
  prefix sums, the sort of the loops and the two device-to-host copies are in `call_ms` only;
- `edges`, `loops`, `points`, `rounds` (jumping launches);
- `bytes`: what the passes move at the least, from the counts -- count: the map and a word per pixel; link: the map, the
  words and 12 B per edge; rank: 36 B per edge and round (three words read at the edge, three at its jump target, three
  written); flags, loops, scatter, emit: 24, 8, 40 and 16 B per edge, 8 B per point -- beside `map_bytes`;
- `baseline_s`: tests/trace_reference.py on the host, once (--baseline-only runs nothing else and needs no GPU;
  --skip-baseline leaves it out), and whether it agrees with the device result when both ran.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from weed_instance_segmentation_amd import _lib, ops  # noqa: E402

PASSES = ("trace_count", "trace_link", "trace_rank", "trace_flags", "trace_loops", "trace_scatter", "trace_emit")


def make_maps(B, H, W, n, seed):
    """n ellipses per image over -1, later ones painting over earlier ones; radii shrink with n so the cover stays alike."""
    rng = np.random.default_rng(seed)
    scale = (H * W / n) ** 0.5
    maps = np.full((B, H, W), -1.0, np.float32)
    for b in range(B):
        for k in range(n):
            cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
            ry, rx = (max(1, int(v)) for v in rng.uniform(0.15, 0.45, 2) * scale)
            y0, y1, x0, x1 = max(0, cy - ry), min(H, cy + ry + 1), max(0, cx - rx), min(W, cx + rx + 1)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            maps[b, y0:y1, x0:x1][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k % _lib.WM2F_RLE_MAX_IDS
    return maps


def spread(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def device_case(maps, N, runs):
    t = torch.from_numpy(maps).cuda()
    B, H, W = maps.shape
    got = ops.labelmap_trace(t, N)  # warm-up: code objects, the allocator's blocks
    ops.labelmap_trace(t, N)
    call_ms, passes = [], {k: [] for k in PASSES}
    for _ in range(runs):
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ops.labelmap_trace(t, N)
            torch.cuda.synchronize()
            call_ms.append((time.perf_counter() - t0) * 1e3)
        finally:
            ops.set_kernel_timer(None)
        for k, (_, us) in timer.summary().items():
            passes[k].append(us)
    # unsimplified crack coordinates give a point per edge
    E = int(ops.labelmap_trace(t, N, 0, False)[0].shape[0])
    P, L = int(got[0].shape[0]), int(got[2].numel())
    rounds = int(_lib.load().wm2f_trace_rounds(E)) if E else 0
    px = B * H * W
    moved = {"trace_count": 8 * px, "trace_link": 8 * px + 12 * E, "trace_rank": 36 * E * rounds, "trace_flags": 24 * E,
             "trace_loops": 8 * E, "trace_scatter": 40 * E, "trace_emit": 16 * E + 8 * P}
    rec = {"edges": E, "loops": L, "points": P, "rounds": rounds, "call_ms": spread(call_ms),
           "passes_us": {k: spread(v, 1) for k, v in passes.items() if v}, "map_bytes": 4 * px, "bytes": moved,
           "bytes_total": sum(moved.values())}
    return rec, [g.cpu().numpy() for g in got]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench.jsonl"))
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    if not args.baseline_only and not torch.cuda.is_available():
        raise SystemExit("trace_bench needs an MI355X (or --baseline-only)")
    H = W = 1024
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for B in (1, 8):
            for n in (10, 300, 3000):
                N = min(n, _lib.WM2F_RLE_MAX_IDS)
                maps = make_maps(B, H, W, n, seed=n)
                rec = {"B": B, "H": H, "W": W, "blobs": n, "N": N, "coords": "pixel", "simplify": True, "runs": args.runs}
                got = None
                if not args.baseline_only:
                    dev, got = device_case(maps, N, args.runs)
                    rec.update(dev)
                if not args.skip_baseline:
                    import trace_reference as R
                    t0 = time.perf_counter()
                    ref = R.csr(maps, N, 1, True)
                    rec["baseline_s"] = round(time.perf_counter() - t0, 2)
                    rec["baseline_loops"], rec["baseline_points"] = int(len(ref[2])), int(len(ref[0]))
                    if got is not None:
                        rec["equal_to_baseline"] = all(np.array_equal(g, r) for g, r in zip(got, ref))
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
