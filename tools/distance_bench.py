"""Interior distance maps and aim points on the GPU: times per call, beside the boundary kernel.

    python tools/distance_bench.py [--rounds 5] [--out profiles/distance_bench.jsonl]

Maps (B = 1, int32, -1 background) at 1024 x 1024 and 4096 x 4096:
- `plants`: 300 (at 1024 x 1024: 100) ragged blobs with inscribed radii of 5 .. 150 px, later ones painted over
  earlier ones;
- `speckle`: a random id of 0 .. 255 per pixel -- no walk is longer than a step or two, every pixel attains its
  instance's maximum;
- `one_id`: one id fills the map, the adversarial case: with border="outside" a pixel walks as far as it is from the
  border, with border="inside" g says nothing and every pixel walks its whole row.
Timed with HIP events in one process, the calls alternating per round, median and spread (min, max) over `--rounds`:
- `distance`: `ops.labelmap_distance` (three launches), border outside, and for `one_id` border inside as well;
- `aim`: `ops.labelmap_aim_points` with stats, N = 512 (four launches);
- `boundary`: `ops.labelmap_boundary` at d = 15 on the same map, the yardstick for a two-pass map kernel;
- `cpu_s`: the numpy / scipy restatement (tests/distance_reference.py: one distance transform per id) on the host, once,
  where it ends in reasonable time (not the 4096 x 4096 speckle map: 256 transforms of 16.8 M pixels).
The distance map is checked against the restatement in the run where the restatement was computed.  One JSON line per
map; the bytes a call must move (the map four times, g written, read, rewritten and read, the summaries, d2 written) are
set against 8 TB/s.
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

import distance_reference as R  # noqa: E402
from weed_instance_segmentation_amd import ops  # noqa: E402

HBM_BPS = 8e12
N_IDS = 512


def plants(H, W, seed):
    rng = np.random.default_rng(seed)
    m = np.full((H, W), -1, np.int32)
    n = 300 if H * W >= 4096 * 4096 else 100
    for k in range(n):
        r = int(rng.integers(5, min(151, H // 6)))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        y0, y1, x0, x1 = max(0, cy - 2 * r), min(H, cy + 2 * r), max(0, cx - 2 * r), min(W, cx + 2 * r)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        edge = 1.0 + 0.15 * np.sin(np.arctan2(yy - cy, xx - cx) * int(rng.integers(5, 12)))  # the inscribed radius is 0.85 r
        m[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 < (r / 0.85 * edge) ** 2] = k
    return m


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def stats(ms):
    return {"median": round(statistics.median(ms) * 1e3, 1), "min": round(min(ms) * 1e3, 1), "max": round(max(ms) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distance_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for side in (1024, 4096):
            H = W = side
            for kind in ("plants", "speckle", "one_id"):
                if kind == "plants":
                    m = plants(H, W, side)
                elif kind == "speckle":
                    m = np.random.default_rng(side).integers(0, 256, (H, W)).astype(np.int32)
                else:
                    m = np.zeros((H, W), np.int32)
                dev = torch.from_numpy(m).cuda().unsqueeze(0)
                calls = {"distance": lambda: ops.labelmap_distance(dev, True),
                         "boundary": lambda: ops.labelmap_boundary(dev, 15)}
                if kind == "one_id":
                    calls["distance_inside"] = lambda: ops.labelmap_distance(dev, False)
                d2 = ops.labelmap_distance(dev, True)
                st = ops.labelmap_instance_stats(dev, N=N_IDS)
                calls["aim"] = lambda: ops.labelmap_aim_points(dev, d2, N=N_IDS, stats=st)
                first = {k: event_ms(fn, 1) for k, fn in calls.items()}  # warm-up, and how many calls a timing takes
                inner = {k: max(1, min(20, int(20.0 / max(v, 1e-3)))) for k, v in first.items()}
                times = {k: [] for k in calls}
                for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                    for k, fn in calls.items():
                        times[k].append(event_ms(fn, inner[k]))
                cpu_s, equal = None, None
                if not (kind == "speckle" and side > 1024):
                    t0 = time.perf_counter()
                    want = R.d2_scipy(m, True)
                    cpu_s = round(time.perf_counter() - t0, 3)
                    equal = bool(np.array_equal(d2[0].cpu().numpy(), want))
                chunks = -(-H // 32)  # an upper bound of the summaries
                nbytes = H * W * (4 * 4 + 2 * 4 + 4) + chunks * W * 16 * 3
                rec = {"H": H, "W": W, "map": kind, "rounds": args.rounds, "inner_calls": inner,
                       "d2_max": int(d2.max()), "equals_restatement": equal, "cpu_s": cpu_s,
                       **{k + "_us": stats(v) for k, v in times.items()},
                       "distance_over_boundary": round(statistics.median(times["distance"]) / statistics.median(times["boundary"]), 2),
                       "distance_bytes": nbytes,
                       "distance_share_of_8TBps": round(nbytes / HBM_BPS / (statistics.median(times["distance"]) * 1e-3), 3)}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
