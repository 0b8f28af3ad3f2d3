"""Repair of id maps on the GPU against the host restatement, on 1024 x 1024 int32 maps.

    python tools/clean_bench.py [--reps 20] [--out profiles/clean_bench.jsonl]

Cases: section 16's square blobs at about 10, 300 and 5000 pieces (classes 1-3 taken as the ids 0-2) and its serpentine,
plus the block map of tests/clean_reference.py (3 x 3 cells of six ids with salt); each at B = 1 and B = 8 (the map and
its flips).  Options keep="largest", min_area=16, fill_holes=True.  One JSON line per case and batch size:
- `phases_us`: HIP events around each of the four tagged parts of the chain (pieces: the 8-connected labelling; choose;
  holes: the 4-connected labelling of the free pixels; paint), median of --reps after warm-up;
- `kernel_ms`: their sum; `call_ms`: the whole `ops.labelmap_clean` call on device-resident maps between two HIP events
  (allocations of the outputs and the workspace included), median of --reps;
- `scipy_ms`: the restatement (tests/clean_reference.py) on the same maps, one run;
- `ccl_label_us`: `wm2f_ccl_label` (section 16's label phase: local, merge, flatten, finalize) on the first map taken as
  a class map, median of --reps -- the closest kernel the package had; it labels once and counts nothing.
Every GPU result is checked against the restatement before it is timed.
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

import clean_reference as R  # noqa: E402
from weed_instance_segmentation_amd import _lib, ops  # noqa: E402

N = 1024
OPTIONS = dict(keep="largest", min_area=16, fill_holes=True)


def blobs(n_target: int, seed: int) -> np.ndarray:
    """tools/ccl_bench.py's blobs: squares of class 1..3, here the ids 0..2 on a free background."""
    rng = np.random.default_rng(seed)
    side = max(2, int(0.5 * N / np.sqrt(n_target)))
    m = np.full((N, N), -1, np.int32)
    for _ in range(n_target):
        y, x = rng.integers(0, N - side, 2)
        m[y:y + side, x:x + side] = rng.integers(0, 3)
    return m


def serpentine() -> np.ndarray:
    m = np.full((N, N), -1, np.int32)
    m[::4, 1:N - 1] = 0
    for i, y in enumerate(range(0, N - 4, 4)):
        m[y:y + 5, N - 2 if i % 2 == 0 else 1] = 0
    return m


def batch_of(m: np.ndarray, B: int) -> np.ndarray:
    views = [m, m[::-1], m[:, ::-1], m[::-1, ::-1], m.T, m.T[::-1], m.T[:, ::-1], m.T[::-1, ::-1]]
    return np.ascontiguousarray(np.stack(views[:B]))


def median_events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clean_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clean_bench needs an MI355X")
    cases = [("blobs_10", blobs(10, 1), 3), ("blobs_300", blobs(300, 2), 3), ("blobs_5000", blobs(5000, 3), 3),
             ("serpentine", serpentine(), 1), ("blocks", R.block_map(N, N).astype(np.int32), 6)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name, m, n in cases:
            for B in (1, 8):
                maps = batch_of(m, B)
                dev = torch.from_numpy(maps).cuda()
                t = time.perf_counter()
                want = R.clean(maps, n, **OPTIONS)
                scipy_ms = (time.perf_counter() - t) * 1e3
                got = ops.labelmap_clean(dev, n, **OPTIONS)
                if not all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)):
                    raise SystemExit(f"{name} B={B}: the GPU result differs from the restatement")
                for _ in range(3):
                    ops.labelmap_clean(dev, n, **OPTIONS)
                call_ms = median_events(lambda: ops.labelmap_clean(dev, n, **OPTIONS), args.reps)
                timer = ops.KernelTimer()
                ops.set_kernel_timer(timer)
                for _ in range(args.reps):
                    ops.labelmap_clean(dev, n, **OPTIONS)
                torch.cuda.synchronize()
                ops.set_kernel_timer(None)
                phases = {k: statistics.median(a.elapsed_time(b) for a, b in v) * 1e3 for k, v in timer.records.items()}
                # section 16's label phase on the first map as a class map (id k -> class k + 1, free -> 0)
                cls = torch.from_numpy((maps[0] + 1).astype(np.uint16)).cuda()
                timer = ops.KernelTimer()
                ops.set_kernel_timer(timer)
                for _ in range(args.reps + 3):
                    ops.label_components(cls, _lib.WM2F_CCL_VALUE)
                torch.cuda.synchronize()
                ops.set_kernel_timer(None)
                ccl = statistics.median(a.elapsed_time(b) for a, b in timer.records["ccl_label"][3:]) * 1e3
                stats = want[1]
                rec = {"case": name, "B": B, "H": N, "W": N, "N": n, "options": OPTIONS,
                       "pieces_in": int(stats[:, :, 1].sum()), "pieces_kept": int(stats[:, :, 2].sum()),
                       "holes_filled": int(stats[:, :, 4].sum()), "phases_us": {k: round(v, 1) for k, v in phases.items()},
                       "kernel_ms": round(sum(phases.values()) / 1e3, 4), "call_ms": round(call_ms, 4),
                       "scipy_ms": round(scipy_ms, 1), "ccl_label_us": round(ccl, 1)}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
