"""Skeletons of id maps on the GPU: times per call at every `per_launch`, beside clean and split.

    python tools/skeleton_bench.py [--rounds 5] [--out profiles/skeleton_bench.jsonl]

Maps (B = 1, int32, -1 background) at 1024 x 1024 and 4096 x 4096, those of tools/distance_bench.py:
- `plants`: ragged blobs with inscribed radii of 5 .. 150 px, later ones painted over earlier ones;
- `speckle`: a random id of 0 .. 255 per pixel -- nearly every pixel is its own skeleton, a few iterations settle it;
- `one_id`: one id fills the map: half the side + 1 iterations, the longest chain a map of that size can ask for.
A first call at rounds = 1024 says how many iterations a map needs (status[1] busy iterations and one quiet one).  The
timed calls use exactly that many rounds, so every launch of the chain works except those after the last busy one; the
4096 x 4096 one-id map needs 2049 and is timed as the unsettled rounds = 1024 case.
Timed with HIP events in one process, the calls alternating per round, median and spread (min, max) over `--rounds`:
- `skeleton_p1` .. `skeleton_p8`: `ops.labelmap_skeleton` at per_launch 1, 2, 4 and 8 (identical bits, asserted);
- `stats`: `ops.labelmap_skeleton_stats` with d2 on the result, N = 512;
- `clean`: `ops.labelmap_clean`, `split`: `ops.labelmap_split` at 8 rounds on a distance map computed before;
- `cpu_s`: the numpy restatement (tests/skeleton_reference.py) on the host, once, for the 1024 x 1024 plants and speckle
  maps; its result is compared with the kernel's.
One JSON line per map.  The bytes the chain must move -- a launch that works reads a plane and writes one, 8 bytes per
pixel; launches after a quiet one move nothing -- are set against 8 TB/s for every per_launch.
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

import skeleton_reference as R  # noqa: E402
from distance_bench import HBM_BPS, N_IDS, event_ms, plants, stats  # noqa: E402
from weed_instance_segmentation_amd import ops  # noqa: E402

PER_LAUNCH = (1, 2, 4, 8)
MAX_ROUNDS = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skeleton_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for side in args.sides:
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
                probe = ops.labelmap_skeleton(dev, N_IDS, MAX_ROUNDS, 1)[1][0].cpu().tolist()
                settled = probe[2] == 0
                needed = probe[1] + 1 if settled else None  # the busy iterations and the quiet one that confirms
                rounds = needed if settled else MAX_ROUNDS
                want_out, want_status = ops.labelmap_skeleton(dev, N_IDS, rounds, 1)
                calls = {}
                for per in PER_LAUNCH:
                    got = ops.labelmap_skeleton(dev, N_IDS, rounds, per)
                    assert torch.equal(got[0], want_out) and torch.equal(got[1], want_status), f"per_launch {per} differs"
                    calls[f"skeleton_p{per}"] = lambda per=per: ops.labelmap_skeleton(dev, N_IDS, rounds, per)
                calls["stats"] = lambda: ops.labelmap_skeleton_stats(want_out, N=N_IDS, d2=d2)
                calls["clean"] = lambda: ops.labelmap_clean(dev, N_IDS)
                calls["split"] = lambda: ops.labelmap_split(dev, d2, N_IDS, 4096, 1, 2, 0, 8)
                first = {k: event_ms(fn, 1) for k, fn in calls.items()}  # warm-up, and how many calls a timing takes
                inner = {k: max(1, min(20, int(20.0 / max(v, 1e-3)))) for k, v in first.items()}
                times = {k: [] for k in calls}
                for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                    for k, fn in calls.items():
                        times[k].append(event_ms(fn, inner[k]))
                cpu_s, equal = None, None
                if side == 1024 and kind != "one_id":
                    t0 = time.perf_counter()
                    ref_out, ref_status = R.skeleton(m, N_IDS, rounds)
                    cpu_s = round(time.perf_counter() - t0, 3)
                    equal = bool(np.array_equal(want_out[0].cpu().numpy(), ref_out)) and want_status[0].cpu().tolist() == ref_status.tolist()
                med = {k: statistics.median(v) for k, v in times.items()}
                busy = probe[1] if settled else MAX_ROUNDS
                rec = {"H": H, "W": W, "map": kind, "rounds": args.rounds, "inner_calls": inner, "thin_rounds": rounds,
                       "iterations_needed": needed, "settled": settled, "status": want_status[0].cpu().tolist(),
                       "ids_in_map": int(len(np.unique(m[m >= 0]))), "equals_restatement": equal, "cpu_s": cpu_s,
                       **{k + "_us": stats(v) for k, v in times.items()}}
                for per in PER_LAUNCH:
                    k = f"skeleton_p{per}"
                    working = min(-(-rounds // per), -(-busy // per) + 1)  # the launches with a busy iteration, and one more
                    nbytes = working * 8 * H * W
                    rec[f"p{per}_over_p1"] = round(med[k] / med["skeleton_p1"], 3)
                    rec[f"p{per}_bytes"] = nbytes
                    rec[f"p{per}_share_of_8TBps"] = round(nbytes / HBM_BPS / (med[k] * 1e-3), 3)
                best = min(PER_LAUNCH, key=lambda per: med[f"skeleton_p{per}"])
                rec["fastest_per_launch"] = best
                rec["fastest_over_clean"] = round(med[f"skeleton_p{best}"] / med["clean"], 2)
                rec["fastest_over_split"] = round(med[f"skeleton_p{best}"] / med["split"], 2)
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
