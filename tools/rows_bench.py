"""Crop rows on the GPU against the one-read statistics kernel and the numpy restatement.

    python tools/rows_bench.py [--rounds 7] [--inner 10] [--no-host] [--out profiles/rows_bench.jsonl]

Workload: one int32 id map (-1 background) of 1024 x 1024 and of 4096 x 4096 holding a row crop -- discs of radius 9 on
parallel lines 48 pixels apart whose normal points at 30 degrees, about 10 % of the pixels, every plant votes -- with
T = 180 and T = 512 directions and one-pixel bins.  In one process, alternating per round and timed with HIP events,
`--inner` calls per timing:
- `row_votes`: `ops.labelmap_row_votes` (clear, votes, energy);
- `row_bands`: `ops.labelmap_row_bands` with the rows `crop_rows` finds and the zone written;
- `instance_stats`: `ops.labelmap_instance_stats` on the same map, the cost of one read of the map;
- `crop_rows_ms` (a host clock around the whole function, the footprint cached): what a caller waits for;
- `host` (once, a host clock): the restatement's votes and energies (tests/rows_reference.py, one np.bincount per
  direction) on the map copied to the host.
One JSON line per case: medians and spreads, the votes per second, the ratios to the two yardsticks, and that the
device's accumulator equals the restatement's.  Kernel times come from a profiler run of this script, not from here."""
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

from weed_instance_segmentation_amd import RowOptions, crop_rows, ops  # noqa: E402


def make_field(H, W, seed, normal_deg=30.0, spacing=48.0, radius=9, step=50.0, jitter=2.0):
    """(map, n): discs along parallel lines, painted box by box."""
    rng = np.random.default_rng(seed)
    th = np.deg2rad(normal_deg)
    n, d = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], float)
    m = np.full((H, W), -1, np.int32)
    k = 0
    for r in np.arange((corners @ n).min() + spacing / 2, (corners @ n).max(), spacing):
        for a in np.arange((corners @ d).min() + rng.uniform(0, step), (corners @ d).max(), step):
            cx, cy = r * n + a * d + rng.normal(0, jitter, 2)
            if not (radius <= cx <= W - 1 - radius and radius <= cy <= H - 1 - radius):
                continue
            x0, y0 = int(cx) - radius - 1, int(cy) - radius - 1
            yy, xx = np.mgrid[y0:y0 + 2 * radius + 3, x0:x0 + 2 * radius + 3]
            sel = (xx - cx) ** 2 + (yy - cy) ** 2 <= radius ** 2
            m[yy[sel], xx[sel]] = k % 4096
            k += 1
    return m, min(k, 4096)


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
    ap.add_argument("--no-host", action="store_true", help="skip the restatement (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rows_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for H in (1024, 4096):
            m, n = make_field(H, H, seed=H)
            maps = torch.from_numpy(m)[None].cuda()
            vote = torch.ones(1, n, dtype=torch.uint8, device="cuda")
            voters = int((m >= 0).sum())
            for T in (180, 512):
                cs = torch.from_numpy(ops.row_angle_table(T)).cuda()
                opts = RowOptions(vote_labels=[], angles=T)
                rows = crop_rows(maps[0], opts, vote=vote[0])
                line = torch.tensor([[*rows["line"], len(rows["rho_fixed"])]], dtype=torch.int32, device="cuda")
                rho = torch.tensor([rows["rho_fixed"] or [0]], dtype=torch.int32, device="cuda")
                run = {"row_votes": lambda: ops.labelmap_row_votes(maps, vote, cs, 14),
                       "row_bands": lambda: ops.labelmap_row_bands(maps, line, rho, rows["band_fixed"], N=n, zone=True),
                       "instance_stats": lambda: ops.labelmap_instance_stats(maps, N=n)}
                acc, _ = run["row_votes"]()
                for fn in run.values():  # warm every shape the timed window uses
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                ms = {k: [] for k in run}
                whole = []
                for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                    for k, fn in run.items():
                        ms[k].append(event_ms(fn, args.inner))
                    t0 = time.perf_counter()
                    crop_rows(maps[0], opts, vote=vote[0])
                    whole.append((time.perf_counter() - t0) * 1e3)
                med = {k: statistics.median(v) for k, v in ms.items()}
                rec = {"H": H, "W": H, "T": T, "instances": n, "voters": voters, "cover": round(voters / (H * H), 4),
                       "rounds": args.rounds, "inner": args.inner, "found": rows["found"], "t": rows["t"],
                       "rows": len(rows["rho"]), "contrast": round(rows["contrast"], 2),
                       **{k + "_us": spread(v) for k, v in ms.items()},
                       "crop_rows_ms": round(statistics.median(whole), 2),
                       "votes_per_second": round(voters * T / (med["row_votes"] * 1e-3), -6),
                       "row_votes_over_instance_stats": round(med["row_votes"] / med["instance_stats"], 2),
                       "row_bands_over_instance_stats": round(med["row_bands"] / med["instance_stats"], 2),
                       "map_bytes": int(maps.numel() * 4)}
                if not args.no_host:
                    from rows_reference import votes_reference
                    host_map = maps[0].cpu().numpy()
                    t0 = time.perf_counter()
                    want, _ = votes_reference(host_map, np.ones(n, np.uint8), T, 14)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    rec.update({"host_ms": round(host_ms, 1), "host_over_device": round(host_ms / med["row_votes"], 1),
                                "routes_equal": bool(np.array_equal(acc[0].cpu().numpy(), want))})
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
