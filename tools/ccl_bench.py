"""GPU instance maps from semantic masks against the CPU restatement, per 1024 x 1024 map.

    python tools/ccl_bench.py [--reps 20] [--out profiles/ccl_bench.jsonl]

Cases: uint16 class maps with about 10, 300 and 5000 components (square blobs of classes 1-3 on a background) and one
serpentine component that crosses every tile.  One JSON line per case:
- `gpu_ms`: `annotations.semantic_to_instance_map` on a device-resident map, synchronised, median of --reps (the six
  kernels, the count read-back, torch.sort of the keys and the class copy for the dict);
- `gpu_h2d_ms`: the same with the host-to-device copy of the uint16 map in front;
- `kernel_ms`: HIP events around the label and paint launches alone (`ops` kernel timer);
- `scipy_ms`: the CPU restatement (scipy.ndimage.label per class, renumbered by the first-block rule, vectorised paint);
- `loop_ms`: the reference's own loop shape on the host: one label pass per class and one full-image
  `instance_map[labels == k] = id` pass per component (scipy standing in for cv2, which is not installed), one run.
Every GPU map is checked against the restatement before it is timed.
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
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from weed_instance_segmentation_amd import annotations, ops  # noqa: E402

N = 1024
EIGHT = np.ones((3, 3), dtype=bool)


def blobs(n_target: int, seed: int) -> np.ndarray:
    """Square blobs of random class 1..3; side chosen so that about n_target survive as separate components."""
    rng = np.random.default_rng(seed)
    side = max(2, int(0.5 * N / np.sqrt(n_target)))
    m = np.zeros((N, N), np.uint16)
    for _ in range(n_target):
        y, x = rng.integers(0, N - side, 2)
        m[y:y + side, x:x + side] = rng.integers(1, 4)
    return m


def serpentine() -> np.ndarray:
    m = np.zeros((N, N), np.uint16)
    m[::4, 1:N - 1] = 1
    for i, y in enumerate(range(0, N - 4, 4)):
        m[y:y + 5, N - 2 if i % 2 == 0 else 1] = 1
    return m


def restate(sem: np.ndarray):
    blk = (np.arange(N)[:, None] >> 1) * ((N + 1) // 2) + (np.arange(N)[None, :] >> 1)
    inst = np.full(sem.shape, 255, np.int32)
    d, cur = {}, 1
    for c in np.unique(sem):
        if c == 0:
            continue
        lab, n = ndimage.label(sem == c, structure=EIGHT)
        first = np.full(n + 1, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(first, lab.ravel(), blk.ravel())
        ids = np.zeros(n + 1, np.int32)
        for k in np.argsort(first[1:]) + 1:
            if cur == 255:
                cur += 1
            ids[k] = cur
            d[cur] = int(c)
            cur += 1
        inst = np.where(lab > 0, ids[lab], inst)
    return inst, d


def reference_loop(sem: np.ndarray):
    inst = np.full(sem.shape, 255, np.int32)
    cur = 1
    for c in np.unique(sem):
        if c == 0:
            continue
        lab, n = ndimage.label(sem == c, structure=EIGHT)
        for k in range(1, n + 1):
            if cur == 255:
                cur += 1
            inst[lab == k] = cur
            cur += 1
    return inst


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ccl_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ccl_bench needs an MI355X")
    cases = [("blobs_10", blobs(10, 1)), ("blobs_300", blobs(300, 2)), ("blobs_5000", blobs(5000, 3)),
             ("serpentine", serpentine())]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name, sem in cases:
            dev = torch.from_numpy(sem).cuda()
            exp, exp_d = restate(sem)
            got, d = annotations.semantic_to_instance_map(dev)
            if not (np.array_equal(got.cpu().numpy(), exp) and d == exp_d):
                raise SystemExit(f"{name}: GPU map differs from the restatement")
            for _ in range(3):
                annotations.semantic_to_instance_map(dev)
            gpu_ms = timed(lambda: annotations.semantic_to_instance_map(dev), args.reps)
            h2d_ms = timed(lambda: annotations.semantic_to_instance_map(torch.from_numpy(sem).cuda()), args.reps)
            timer = ops.KernelTimer()
            ops.set_kernel_timer(timer)
            for _ in range(args.reps):
                annotations.semantic_to_instance_map(dev)
            torch.cuda.synchronize()
            ops.set_kernel_timer(None)
            k = timer.summary()
            t = time.perf_counter()
            for _ in range(3):
                restate(sem)
            scipy_ms = (time.perf_counter() - t) * 1e3 / 3
            t = time.perf_counter()
            loop = reference_loop(sem)
            loop_ms = (time.perf_counter() - t) * 1e3
            assert np.array_equal((loop == 255), (exp == 255))
            rec = {"case": name, "H": N, "W": N, "components": len(d), "gpu_ms": round(gpu_ms, 3),
                   "gpu_h2d_ms": round(h2d_ms, 3), "kernel_ms": round(sum(v[1] for v in k.values()) / 1e3, 4),
                   "kernels_us": {kk: round(v[1], 1) for kk, v in k.items()}, "scipy_ms": round(scipy_ms, 2),
                   "loop_ms": round(loop_ms, 1)}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
