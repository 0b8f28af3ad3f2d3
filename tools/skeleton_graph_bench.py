"""Spur pruning and the skeleton graph on the GPU: times per call beside the thinning of the same map.

    python tools/skeleton_graph_bench.py [--rounds 5] [--sides 1024 4096] [--out profiles/skeleton_graph_bench.jsonl]

The maps of tools/skeleton_bench.py (B = 1, int32, -1 background, N = 512): `plants`, `speckle` and `one_id`.  Every
map is thinned first (to its fixed point, or 1024 iterations for the 4096 x 4096 one-id map) and its interior distance
computed; a first prune at 64 rounds says how many rounds remove something.  Timed with HIP events in one process, the
calls alternating per round, median and spread (min, max) over `--rounds`:
- `thin`: `ops.labelmap_skeleton` of the map at the rounds it needs (per_launch at its default);
- `prune`: `ops.labelmap_skeleton_prune` of its skeleton at the defaults (8 rounds, 4 re-thinning iterations);
- `prune_needed`: the same at exactly the rounds that remove something and the one that confirms;
- `graph`: `ops.labelmap_skeleton_graph` of the pruned skeleton;
- `cpu_s`: the numpy restatement (tests/skeleton_graph_reference.py) of `prune_needed` and `graph` on the host, once, for
  the 1024 x 1024 plants map; its results are compared with the kernels'.
One JSON line per map.  The bytes a chain must move are set against 8 TB/s: a round that works reads the state and writes
seven planes in `local`, reads the key plane in `flatten`, `record` and `delete`, writes the state, and the thinning
reads it and writes out -- 56 bytes per pixel; a round after the one that confirms moves only the thinning's 8; the graph
moves 44 (local, flatten, record, and key in, labels out).
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

import skeleton_graph_reference as G  # noqa: E402
from distance_bench import HBM_BPS, N_IDS, event_ms, plants, stats  # noqa: E402
from weed_instance_segmentation_amd import ops  # noqa: E402

MAX_THIN, ROUND_BYTES, QUIET_BYTES, GRAPH_BYTES = 1024, 56, 8, 44


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--maps", nargs="+", default=["plants", "speckle", "one_id"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton_graph_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skeleton_graph_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for side in args.sides:
            H = W = side
            for kind in args.maps:
                if kind == "plants":
                    m = plants(H, W, side)
                elif kind == "speckle":
                    m = np.random.default_rng(side).integers(0, 256, (H, W)).astype(np.int32)
                else:
                    m = np.zeros((H, W), np.int32)
                dev = torch.from_numpy(m).cuda().unsqueeze(0)
                d2 = ops.labelmap_distance(dev, True)
                probe = ops.labelmap_skeleton(dev, N_IDS, MAX_THIN)[1][0].cpu().tolist()
                thin_rounds = probe[1] + 1 if probe[2] == 0 else MAX_THIN
                skel, _ = ops.labelmap_skeleton(dev, N_IDS, thin_rounds)
                busy = ops.labelmap_skeleton_prune(skel, d2, N_IDS, rounds=64)[1][0].cpu().tolist()
                assert busy[2] == 0, "the pruning has not settled within 64 rounds"
                needed = busy[1] + 1
                out, status = ops.labelmap_skeleton_prune(skel, d2, N_IDS)
                short = ops.labelmap_skeleton_prune(skel, d2, N_IDS, rounds=needed)
                assert needed > 8 or (torch.equal(out, short[0]) and torch.equal(status, short[1])), "rounds beyond the fixed point differ"
                labels, sums = ops.labelmap_skeleton_graph(short[0], N=N_IDS)
                calls = {"thin": lambda: ops.labelmap_skeleton(dev, N_IDS, thin_rounds),
                         "prune": lambda: ops.labelmap_skeleton_prune(skel, d2, N_IDS),
                         "prune_needed": lambda: ops.labelmap_skeleton_prune(skel, d2, N_IDS, rounds=needed),
                         "graph": lambda: ops.labelmap_skeleton_graph(short[0], N=N_IDS)}
                first = {k: event_ms(fn, 1) for k, fn in calls.items()}  # warm-up, and how many calls a timing takes
                inner = {k: max(1, min(20, int(20.0 / max(v, 1e-3)))) for k, v in first.items()}
                times = {k: [] for k in calls}
                for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                    for k, fn in calls.items():
                        times[k].append(event_ms(fn, inner[k]))
                cpu_s, equal = None, None
                if side == 1024 and kind == "plants":
                    sk, dd = skel[0].cpu().numpy(), d2[0].cpu().numpy()
                    t0 = time.perf_counter()
                    ref_out, ref_status = G.prune(sk, dd, N_IDS, rounds=needed)
                    ref_labels, ref_sums = G.graph(ref_out, N_IDS)
                    cpu_s = round(time.perf_counter() - t0, 3)
                    equal = bool(np.array_equal(short[0][0].cpu().numpy(), ref_out) and short[1][0].cpu().tolist() == ref_status.tolist()
                                 and np.array_equal(labels[0].cpu().numpy(), ref_labels) and np.array_equal(sums[0].cpu().numpy(), ref_sums))
                med = {k: statistics.median(v) for k, v in times.items()}
                px = H * W
                prune_bytes = (min(needed, 8) * ROUND_BYTES + max(0, 8 - needed) * QUIET_BYTES) * px
                rec = {"H": H, "W": W, "map": kind, "rounds": args.rounds, "inner_calls": inner, "thin_rounds": thin_rounds,
                       "skeleton_pixels": int((skel >= 0).sum()), "prune_status": status[0].cpu().tolist(), "rounds_needed": needed,
                       "graph_totals": sums[0].sum(0).cpu().tolist(), "equals_restatement": equal, "cpu_s": cpu_s,
                       **{k + "_us": stats(v) for k, v in times.items()},
                       "prune_over_thin": round(med["prune"] / med["thin"], 3), "graph_over_thin": round(med["graph"] / med["thin"], 3),
                       "prune_bytes": prune_bytes, "prune_share_of_8TBps": round(prune_bytes / HBM_BPS / (med["prune"] * 1e-3), 3),
                       "prune_needed_share_of_8TBps": round(needed * ROUND_BYTES * px / HBM_BPS / (med["prune_needed"] * 1e-3), 3),
                       "graph_share_of_8TBps": round(GRAPH_BYTES * px / HBM_BPS / (med["graph"] * 1e-3), 3)}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
