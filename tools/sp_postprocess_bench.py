"""Semantic and panoptic post-processing on the GPU against the plain-torch restatement of the
dependency's methods (tests/test_sp_postprocess_cpu.py) run on the same GPU tensors.

    python tools/sp_postprocess_bench.py [--reps 20] [--out profiles/sp_postprocess_bench.jsonl]

Workload: B = 8 images, Q = 100 queries, 256 x 256 mask logits, 1024 x 1024 targets, C = 3 classes (the synthetic
tiled-blob logits of tests/test_sp_postprocess_gpu.py).  One JSON line per method:
- `hip_ms`: the processor method, synchronised, median of --reps (host selection, copies, launches, id assignment);
- `kernel_ms`: HIP events around the method's wm2f launches alone, summed per call (`ops` kernel timer);
- `restatement_ms`: the dependency's algorithm on the same GPU, synchronised, median of --reps;
- agreement: identical segments_info (panoptic) and the fraction of map pixels that differ.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from weed_instance_segmentation_amd import ops  # noqa: E402
from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def kernel_ms(fn, reps):
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ops.set_kernel_timer(None)
    return sum(n * us for n, us in timer.summary().values()) / reps / 1e3, {k: round(v[1], 1) for k, v in timer.summary().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sp_postprocess_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sp_postprocess_bench needs an MI355X")
    from test_sp_postprocess_cpu import panoptic_reference, semantic_reference
    from test_sp_postprocess_gpu import _eval_inputs
    B, Q, C, N = 8, 100, 3, 1024
    cls, m = _eval_inputs(B, Q, C, seed=7)
    outputs = SimpleNamespace(class_queries_logits=cls, masks_queries_logits=m)
    ts = [(N, N)] * B
    P = Mask2FormerInstancePostProcessor()
    shape = {"B": B, "Q": Q, "C": C, "logits": [256, 256], "target": [N, N]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        runs = {
            "semantic": (lambda: P.post_process_semantic_segmentation(outputs, target_sizes=ts),
                         lambda: semantic_reference(cls, m, ts)),
            "panoptic": (lambda: P.post_process_panoptic_segmentation(outputs, label_ids_to_fuse=set(), target_sizes=ts),
                         lambda: panoptic_reference(cls, m, label_ids_to_fuse=set(), target_sizes=ts)),
        }
        for name, (hip, ref) in runs.items():
            got, exp = hip(), ref()
            for _ in range(3):
                hip()
                ref()
            hip_ms = timed(hip, args.reps)
            k_ms, per_kernel = kernel_ms(hip, args.reps)
            ref_ms = timed(ref, max(3, args.reps // 4))
            if name == "semantic":
                diff = sum(int((a != e[0]).sum()) for a, e in zip(got, exp))
                same_info = None
            else:
                diff = sum(int((a["segmentation"] != e["segmentation"]).sum()) for a, e in zip(got, exp))
                same_info = all([(s["id"], s["label_id"], s["was_fused"]) for s in a["segments_info"]] ==
                                [(s["id"], s["label_id"], s["was_fused"]) for s in e["segments_info"]] for a, e in zip(got, exp))
            rec = {"method": name, **shape, "hip_ms": round(hip_ms, 3), "kernel_ms": round(k_ms, 4),
                   "kernel_us_per_launch": per_kernel, "restatement_ms": round(ref_ms, 3),
                   "speedup": round(ref_ms / hip_ms, 2), "map_pixels_differing": diff,
                   "map_fraction_differing": diff / (B * N * N), "segments_info_identical": same_info}
            if name == "panoptic":
                rec["segments"] = sum(len(a["segments_info"]) for a in got)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
