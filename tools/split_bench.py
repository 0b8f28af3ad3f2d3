"""Splitting touching instances on the GPU: times per call, beside the distance and the clean kernels.

    python tools/split_bench.py [--rounds 5] [--out profiles/split_bench.jsonl]

Maps: those of tools/distance_bench.py (B = 1, int32, -1 background) at 1024 x 1024 and 4096 x 4096 -- `plants` (ragged
blobs painted over one another), `speckle` (a random id of 0 .. 255 per pixel: about as many basins as pixels) and
`one_id` (one id fills the map: the longest ascents there are).
Timed with HIP events in one process, the calls alternating per round, median and spread (min, max) over `--rounds`, at
min_neck_ratio 1/2, 8 merge rounds, N = 512, M = 4096:
- `split`: `ops.labelmap_split` alone on a distance map computed before (8 + 3 * 8 launches);
- `distance_split`: `ops.labelmap_distance` and then the split, what `split_label_maps` runs;
- `distance`, `clean`: `ops.labelmap_distance` and `ops.labelmap_clean` (keep all, no holes: one labelling and a paint) on
  the same map, the nearest existing kernels of the same kind;
- `cpu_s`: the numpy restatement (tests/split_reference.py) on the host at 1024 x 1024, once, and whether out, info and
  status equal it -- not for `speckle`, whose million basins take the restatement's dictionaries minutes.
`status` is the kernel's row [ids wanted, basins, links in the last round, rounds]; `rounds_to_settle` is the first number
of rounds after which a further round links nothing.  The bytes a call must move (16 B per pixel for the ascent, 12 for
every flatten, 16 for the pass and the decisions of a round that runs, 40 for the numbering and the paint) are set
against 8 TB/s.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import split_reference as S  # noqa: E402
from distance_bench import HBM_BPS, N_IDS, event_ms, plants, stats  # noqa: E402
from weed_instance_segmentation_amd import ops  # noqa: E402

M_IDS, NUM, DEN, ROUNDS = 4096, 1, 2, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("split_bench needs an MI355X")
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
                d2 = ops.labelmap_distance(dev, True)

                def split(rounds=ROUNDS):
                    return ops.labelmap_split(dev, d2, N_IDS, M_IDS, NUM, DEN, 0, rounds)

                calls = {"split": split,
                         "distance_split": lambda: ops.labelmap_split(dev, ops.labelmap_distance(dev, True), N_IDS, M_IDS, NUM, DEN, 0, ROUNDS),
                         "distance": lambda: ops.labelmap_distance(dev, True),
                         "clean": lambda: ops.labelmap_clean(dev, N_IDS)}
                first = {k: event_ms(fn, 1) for k, fn in calls.items()}  # warm-up, and how many calls a timing takes
                inner = {k: max(1, min(20, int(20.0 / max(v, 1e-3)))) for k, v in first.items()}
                times = {k: [] for k in calls}
                for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                    for k, fn in calls.items():
                        times[k].append(event_ms(fn, inner[k]))
                out, info, status = split()
                status_h = status[0].cpu().tolist()
                settle = next((r for r in range(1, ROUNDS + 1) if split(r)[2][0, 2].item() == 0), None)
                cpu_s, equal = None, None
                if side == 1024 and kind != "speckle":
                    t0 = time.perf_counter()
                    want = S.split(m, d2[0].cpu().numpy(), N_IDS, M_IDS, NUM, DEN, 0, ROUNDS)
                    cpu_s = round(time.perf_counter() - t0, 3)
                    equal = all(bool(np.array_equal(g[0].cpu().numpy(), w)) for g, w in zip((out, info, status), want))
                run = ROUNDS if settle is None else min(ROUNDS, settle)  # the rounds whose launches do not return at once
                nbytes = H * W * (16 + 12 + run * 28 + 40)
                med = {k: statistics.median(v) for k, v in times.items()}
                rec = {"H": H, "W": W, "map": kind, "rounds": args.rounds, "inner_calls": inner, "ratio": [NUM, DEN],
                       "merge_rounds": ROUNDS, "status": status_h, "ids_in_map": int(len(np.unique(m[m >= 0]))),
                       "rounds_to_settle": settle, "equals_restatement": equal, "cpu_s": cpu_s,
                       **{k + "_us": stats(v) for k, v in times.items()},
                       "split_over_clean": round(med["split"] / med["clean"], 2),
                       "split_over_distance": round(med["split"] / med["distance"], 2),
                       "split_bytes": nbytes, "split_share_of_8TBps": round(nbytes / HBM_BPS / (med["split"] * 1e-3), 3)}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
