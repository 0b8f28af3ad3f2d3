"""GPU polygon rasterisation on a 1024 x 1024 instance map, against the literal CPU port of
cv2.fillPoly (tests/test_polygons_cpu.py).

    python tools/poly_bench.py [--reps 20] [--out profiles/poly_bench.jsonl] [--oracle-max-edges 200000]

Cases: {10, 300, 3000} star-shaped polygons x {8, 64, 512} vertices, centres uniform over the map, radii about
512 / sqrt(count) (so the painted area stays comparable), overlapping, painted in order on a 255 background.  One JSON
line per case:
- `gpu_ms`: `annotations.polygons_to_instance_map` from host polygons to a device map, synchronised, median of --reps
  (host packing of the tables, one pinned host-to-device copy, the allocation of the map and the three kernels);
- `kernel_ms`: HIP events around the wm2f_poly_fill launches alone (`ops` kernel timer: rank clear, edges + outlines,
  scan fill, resolve);
- `items`: the (polygon, row) pairs of the scan fill, one wave each; `edge_tests`: edges a wave reads over all items;
- `oracle_ms`: the literal Python port, one run, and whether the GPU map equals it; null above --oracle-max-edges.
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

from weed_instance_segmentation_amd import annotations, ops  # noqa: E402

N = 1024


def polygons(count: int, verts: int, seed: int):
    rng = np.random.default_rng(seed)
    out = []
    r0 = 512.0 / np.sqrt(count)
    for _ in range(count):
        cx, cy = rng.uniform(0, N, 2)
        ang = np.sort(rng.uniform(0, 2 * np.pi, verts))
        r = rng.uniform(0.3, 1.0, verts) * r0 * rng.uniform(0.5, 1.0)
        out.append(np.stack([np.round(cx + r * np.cos(ang)), np.round(cy + r * np.sin(ang))], 1).astype(np.int32))
    return out


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_bench.jsonl"))
    ap.add_argument("--oracle-max-edges", type=int, default=200000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("poly_bench needs an MI355X")
    from test_polygons_cpu import paint
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for count in (10, 300, 3000):
            for verts in (8, 64, 512):
                polys = polygons(count, verts, seed=count * 7 + verts)
                ids = list(range(1, count + 1))
                run = lambda: annotations.polygons_to_instance_map(polys, ids, (N, N))  # noqa: E731
                got = run().cpu().numpy()
                for _ in range(3):
                    run()
                gpu_ms = timed(run, args.reps)
                timer = ops.KernelTimer()
                ops.set_kernel_timer(timer)
                for _ in range(args.reps):
                    run()
                torch.cuda.synchronize()
                ops.set_kernel_timer(None)
                k = timer.summary()
                ys = [(max(int(p[:, 1].min()), 0), min(int(p[:, 1].max()), N)) for p in polys]
                items = sum(max(b - a, 0) for a, b in ys)
                oracle_ms, same = None, None
                if count * verts <= args.oracle_max_edges:
                    t = time.perf_counter()
                    exp = paint((N, N), polys, ids)
                    oracle_ms = round((time.perf_counter() - t) * 1e3, 1)
                    same = bool(np.array_equal(got, exp))
                rec = {"case": f"{count}x{verts}", "H": N, "W": N, "polygons": count, "vertices": verts,
                       "covered": round(float((got != 255).mean()), 3), "items": items,
                       "edge_tests": items * verts, "gpu_ms": round(gpu_ms, 3),
                       "kernel_ms": round(sum(v[1] for v in k.values()) / 1e3, 4),
                       "oracle_ms": oracle_ms, "oracle_equal": same}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
                if same is False:
                    raise SystemExit(f"{rec['case']}: GPU map differs from the oracle")


if __name__ == "__main__":
    main()
