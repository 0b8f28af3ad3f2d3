"""Nearest-instance maps, cell counts and the treatment grid on the GPU: times per call, beside the
interior distance kernel.

    python tools/treatment_bench.py [--rounds 5] [--out profiles/treatment_bench.jsonl]

Maps (B = 1, int32, -1 background):
- `plants` at 1024 x 1024 and 4096 x 4096: the ragged blobs of tools/distance_bench.py;
- `sparse` at 4096 x 4096: small blobs that cover 1 % of the map -- soil with nothing in range, the case the rows
  pass's prefix count is for.
Even ids are weeds (label 1), odd ids crop (label 0).  Margins 8, 32 and 128.  Timed with HIP events in one process, the
calls alternating per round, median and spread (min, max) over `--rounds`:
- `nearest`: `ops.labelmap_nearest` (two launches), every instance a source, blocked; `nearest_walk_all`: the same with
  the early "none" switched off;
- `cell_counts`: `ops.labelmap_cell_counts` of the grown map with a veto map, 32 x 32 cells, G = 1;
- `treatment_grid`: the whole call, host tables included (wall clock around a synchronised call);
- `distance`: `ops.labelmap_distance` on the same map, for scale;
- `cpu_s`: scipy's `distance_transform_edt(return_indices=True)` of the source mask on the host, once; the nearest map
  is checked against it where the cap allows (distance only: scipy's choice among equally near pixels is its own).
One JSON line per map and margin.  The bytes the passes without walks must move are set against 8 TB/s: the columns
pass reads the map (with its warm-up rows) and writes and rereads 6 bytes per pixel; the cell counts read the map and
the veto map once.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from distance_bench import event_ms, plants, stats  # noqa: E402
from weed_instance_segmentation_amd import TreatmentOptions, ops, treatment_grid  # noqa: E402

HBM_BPS = 8e12
N_IDS = 512
CELL = (32, 32)


def sparse(H, W, seed, cover=0.01):
    """Round blobs of radius 3 .. 12 until `cover` of the map carries an id."""
    rng = np.random.default_rng(seed)
    m = np.full((H, W), -1, np.int32)
    k, filled = 0, 0
    while filled < cover * H * W:
        r = int(rng.integers(3, 13))
        cy, cx = int(rng.integers(r, H - r)), int(rng.integers(r, W - r))
        yy, xx = np.mgrid[cy - r:cy + r + 1, cx - r:cx + r + 1]
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        view = m[cy - r:cy + r + 1, cx - r:cx + r + 1]
        filled += int((disc & (view < 0)).sum())
        view[disc] = k % N_IDS
        k += 1
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "treatment_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("treatment_bench needs an MI355X")
    from scipy import ndimage
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for side, kind in ((1024, "plants"), (4096, "plants"), (4096, "sparse")):
            H = W = side
            m = plants(H, W, side) if kind == "plants" else sparse(H, W, side)
            dev = torch.from_numpy(m).cuda().unsqueeze(0)
            t0 = time.perf_counter()
            edt, (iy, ix) = ndimage.distance_transform_edt(m < 0, return_indices=True)
            cpu_s = round(time.perf_counter() - t0, 3)
            edt2 = np.rint(edt ** 2).astype(np.int64)
            result = {"segmentation": dev[0], "segments_info": [{"id": k, "label_id": 1 - k % 2} for k in range(N_IDS)]}
            crop = torch.from_numpy((np.arange(N_IDS) % 2 == 1).astype(np.uint8)).cuda().unsqueeze(0)
            group = torch.from_numpy(np.where(np.arange(N_IDS) % 2 == 0, 0, 255).astype(np.uint8)).cuda().unsqueeze(0)
            for margin in (8, 32, 128):
                cap = margin * margin
                opt = TreatmentOptions(cell=CELL, margin=margin, protect=margin, target_labels=(1,), protect_labels=(0,))

                def whole():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    treatment_grid(result, opt)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t) * 1e3

                grown, d2 = ops.labelmap_nearest(dev, N_IDS, cap, None, True)
                _, veto = ops.labelmap_nearest(dev, N_IDS, cap, crop, False)
                calls = {"nearest": lambda: ops.labelmap_nearest(dev, N_IDS, cap, None, True),
                         "nearest_walk_all": lambda: ops.labelmap_nearest(dev, N_IDS, cap, None, True, walk_all=True),
                         "cell_counts": lambda: ops.labelmap_cell_counts(grown, group, 1, CELL, (0, 0), veto, cap),
                         "distance": lambda: ops.labelmap_distance(dev, True)}
                first = {k: event_ms(fn, 1) for k, fn in calls.items()}  # warm-up, and how many calls a timing takes
                inner = {k: max(1, min(20, int(20.0 / max(v, 1e-3)))) for k, v in first.items()}
                times = {k: [] for k in calls}
                whole()
                grid_ms = []
                for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                    for k, fn in calls.items():
                        times[k].append(event_ms(fn, inner[k]))
                    grid_ms.append(whole())
                got = d2[0].cpu().numpy().astype(np.int64)
                equal = bool(np.array_equal(np.where(edt2 <= cap, edt2, 2 ** 31 - 1), got))
                claimed = int(((got > 0) & (got <= cap)).sum())
                r = margin
                chunk = max(32, -(-H // -(-2048 // (-(-W // 256) * 4))))
                cols_bytes = H * W * 4 * (2 + 2 * r / chunk) + H * W * 6 * 2  # both marches with warm-up; g and id twice
                rows_bytes = H * W * (6 + 8)
                cell_bytes = H * W * 8
                med = {k: statistics.median(v) for k, v in times.items()}
                rec = {"H": H, "W": W, "map": kind, "cover": round(float((m >= 0).mean()), 4), "margin": margin,
                       "rounds": args.rounds, "inner_calls": inner, "claimed_pixels": claimed,
                       "d2_equals_scipy": equal, "cpu_s": cpu_s,
                       **{k + "_us": stats(v) for k, v in times.items()}, "treatment_grid_us": stats(grid_ms),
                       "walk_all_over_nearest": round(med["nearest_walk_all"] / med["nearest"], 2),
                       "nearest_over_distance": round(med["nearest"] / med["distance"], 2),
                       "nearest_min_bytes": int(cols_bytes + rows_bytes),
                       "nearest_share_of_8TBps": round((cols_bytes + rows_bytes) / HBM_BPS / (med["nearest"] * 1e-3), 3),
                       "cell_counts_bytes": cell_bytes,
                       "cell_counts_share_of_8TBps": round(cell_bytes / HBM_BPS / (med["cell_counts"] * 1e-3), 3),
                       "walk_lds_reads_ceiling": 2 * r * H * W}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
