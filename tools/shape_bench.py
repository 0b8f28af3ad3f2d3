"""Per-plant shape sums on the GPU against the one-read statistics kernel and the host loop.

    python tools/shape_bench.py [--rounds 7] [--inner 10] [--no-host] [--out profiles/shape_bench.jsonl]

Workload: one int32 id map (-1 background) of 1024 x 1024 and of 4096 x 4096 with 20, 100 and 1000 instances -- random
rotated ellipses painted over one another, 8 % of the pixels knocked out to background --, and one 4096 x 4096 map whose
single instance is a disc of full height (the longest serial chain the hull kernel can meet at that size).  In one
process, alternating per round and timed with HIP events, `--inner` calls per timing:
- `shape_stats`: `ops.labelmap_shape_stats` (clear, moments, border counts);
- `hull`: `ops.labelmap_hull` with the statistics given (scan, init, rows, chain): the three scalars, no host copy;
- `instance_stats`: `ops.labelmap_instance_stats` on the same map, the cost of one read of the map;
- `host` (once, a host clock): the map copied to the host, scipy.ndimage.find_objects, and per instance on its box the
  sums, the erosion / convolution / bincount of the perimeter and scipy.spatial.ConvexHull of the pixel corners -- what a
  consumer does without the kernels.
One JSON line per map: medians and spreads, the ratios to the two yardsticks, and that the device's areas, sides and hull
areas equal the host loop's.  Kernel times come from a profiler run of this script, not from here."""
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

from weed_instance_segmentation_amd import ops  # noqa: E402


def make_map(H, W, n, seed, knock=0.08):
    rng = np.random.default_rng(seed)
    m = np.full((H, W), -1, np.int32)
    scale = min(H, W) / np.sqrt(max(n, 4))
    for k in range(n):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        a, b = rng.uniform(0.2, 0.9) * scale, rng.uniform(0.08, 0.35) * scale
        t = rng.uniform(0, np.pi)
        r = int(np.ceil(max(a, b))) + 1
        y0, y1, x0, x1 = max(0, int(cy) - r), min(H, int(cy) + r + 1), max(0, int(cx) - r), min(W, int(cx) + r + 1)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        u = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)
        w = -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
        m[y0:y1, x0:x1][(u / a) ** 2 + (w / b) ** 2 <= 1] = k
    m[rng.random((H, W)) < knock] = -1
    return m


def make_disc(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((xx - W / 2 + 0.5) ** 2 + (yy - H / 2 + 0.5) ** 2 <= (min(H, W) / 2) ** 2, 0, -1).astype(np.int32)


def host_loop(dev_map, n):
    """(areas, sides, hull area2) per id on the host, from the device map."""
    from scipy import ndimage
    from scipy.spatial import ConvexHull
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    kernel = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
    m = dev_map.cpu().numpy()
    out = np.zeros((n, 3), np.int64)
    for k, box in enumerate(ndimage.find_objects(m + 1, max_label=n)):
        if box is None:
            continue
        mask = np.pad(m[box] == k, 1)
        ys, xs = np.nonzero(mask)
        sums = (xs.sum(), ys.sum(), (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum())  # the moments' work
        border = mask & ~ndimage.binary_erosion(mask, cross, border_value=0)
        np.bincount(ndimage.convolve(border.astype(np.int64), kernel, mode="constant")[border], minlength=50)
        p = mask.astype(np.int8)
        sides = int(np.abs(np.diff(p, axis=0)).sum() + np.abs(np.diff(p, axis=1)).sum())
        by, bx = np.nonzero(border)  # the corners of the border pixels span the same hull as all corners
        pts = np.unique(np.concatenate([np.stack([bx + dx, by + dy], 1) for dx in (0, 1) for dy in (0, 1)]), axis=0)
        out[k] = [len(ys), sides, int(round(2 * ConvexHull(pts).volume))]
        del sums
    return out


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def spread(ms):
    return {"median": round(statistics.median(ms) * 1e3, 2), "min": round(min(ms) * 1e3, 2), "max": round(max(ms) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the host loop (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shape_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    cases = [(H, H, n, "ellipses") for H in (1024, 4096) for n in (20, 100, 1000)] + [(4096, 4096, 1, "full-height disc")]
    with open(args.out, "a") as f:
        for H, W, n, kind in cases:
            m = make_disc(H, W) if kind != "ellipses" else make_map(H, W, n, seed=H + n)
            maps = torch.from_numpy(m)[None].cuda()
            stats = ops.labelmap_instance_stats(maps, N=n)
            run = {"shape_stats": lambda: ops.labelmap_shape_stats(maps, N=n),
                   "hull": lambda: ops.labelmap_hull(maps, N=n, stats=stats),
                   "instance_stats": lambda: ops.labelmap_instance_stats(maps, N=n)}
            shape, hull = run["shape_stats"](), run["hull"]()
            for fn in run.values():  # warm every shape the timed window uses
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in run}
            for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                for k, fn in run.items():
                    ms[k].append(event_ms(fn, args.inner))
            med = {k: statistics.median(v) for k, v in ms.items()}
            rec = {"H": H, "W": W, "instances": n, "scene": kind, "rounds": args.rounds, "inner": args.inner,
                   "present": int((shape[0, :, 0] > 0).sum()), "largest_hull_vertices": int(hull[0, :, 0].max()),
                   "tallest_box": int((stats[0, :, 4] - stats[0, :, 2] + 1).max()),
                   **{k + "_us": spread(v) for k, v in ms.items()},
                   "shape_stats_over_instance_stats": round(med["shape_stats"] / med["instance_stats"], 2),
                   "hull_over_instance_stats": round(med["hull"] / med["instance_stats"], 2),
                   "map_bytes": int(maps.numel() * 4)}
            if not args.no_host and kind == "ellipses":
                t0 = time.perf_counter()
                ref = host_loop(maps[0], n)
                host_ms = (time.perf_counter() - t0) * 1e3
                got = torch.stack([shape[0, :, 0], shape[0, :, 6], hull[0, :, 1]], 1).cpu().numpy()
                rec.update({"host_ms": round(host_ms, 1), "host_over_device": round(host_ms / (med["shape_stats"] + med["hull"]), 1),
                            "routes_equal": bool(np.array_equal(got, ref))})
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
