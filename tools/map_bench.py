"""Segmentation mAP timing: `MeanAveragePrecision.update_from_maps` at 1024 x 1024 for B = 2 (the
reference's eval batch) and B = 8, next to the forward of the same batch (bench.py's model) and the oracle on the host
cores (pycocotools' algorithm on mask stacks, oracle/coco_eval.py).  One JSON line per batch size.

    python tools/map_bench.py [--reps 20] [--oracle 1]

The GPU numbers are wall times of the whole call (host-to-device copy of the raw GT maps included, synchronised) and
HIP-event times of the kernels alone; `compute()` is timed once per batch on the same records.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case(B, HW=1024, Q=100, n_gt=60, seed=0):
    """Post-processor-like fp32 id maps (Q kept instances) and raw int32 GT maps (n_gt instances, a 255 band)."""
    rng = np.random.default_rng(seed)
    segs, infos, maps, mappings = [], [], [], []
    for _ in range(B):
        gt = np.zeros((HW, HW), np.int32)
        gt[:32] = 255
        boxes = []
        for k in range(1, n_gt + 1):
            s = int(rng.choice([24, 48, 96, 160]))
            y, x = rng.integers(32, HW - s, 2)
            gt[y:y + s, x:x + s] = k
            boxes.append((y, x, s))
        seg = torch.full((HW, HW), -1.0)
        info = []
        for r in range(Q):
            y, x, s = boxes[int(rng.integers(0, n_gt))]
            dy, dx = rng.integers(-s // 4, s // 4 + 1, 2)
            seg[max(0, y + dy):y + dy + s, max(0, x + dx):x + dx + s] = float(r)
            info.append({"id": r, "label_id": int(rng.integers(0, 2)), "was_fused": False,
                         "score": round(float(rng.random()), 6)})
        segs.append(seg)
        infos.append(info)
        maps.append(gt)
        mappings.append({k: int(rng.integers(0, 2)) for k in range(1, n_gt + 1)})
    return segs, infos, maps, mappings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--oracle", type=int, default=1, help="1: also time the oracle on the host (slow)")
    ap.add_argument("--forward", type=int, default=1)
    a = ap.parse_args()
    from weed_instance_segmentation_amd import ops
    from weed_instance_segmentation_amd.metrics import MeanAveragePrecision
    dev = torch.device("cuda", 0)
    model = None
    if a.forward:
        sys.path.insert(0, ROOT)
        from bench import build_model
        model = build_model().to(dev).eval()
    for B in (2, 8):
        segs, infos, maps, mappings = case(B)
        segs_d = [s.to(dev) for s in segs]
        m = MeanAveragePrecision()
        for _ in range(3):  # warm-up
            m.update_from_maps(segs_d, infos, maps, mappings)
        torch.cuda.synchronize()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            m.update_from_maps(segs_d, infos, maps, mappings)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        for _ in range(a.reps):
            m.update_from_maps(segs_d, infos, maps, mappings)
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        kern = {k: round(v[1], 2) for k, v in timer.summary().items()}
        t0 = time.perf_counter()
        res = m.compute()
        compute_ms = (time.perf_counter() - t0) * 1e3
        n_updates = 3 + 2 * a.reps
        out = {"batch": B, "size": 1024, "queries": 100, "gt_per_image": 60,
               "update_from_maps_ms_median": round(float(np.median(wall)), 3),
               "update_from_maps_ms_min": round(float(np.min(wall)), 3),
               "kernel_us_mean": kern, "compute_ms": round(compute_ms, 2), "compute_images": n_updates * B,
               "map": round(float(res["map"]), 6)}
        hbm_bytes = B * 1024 * 1024 * (4 + 4)  # fp32 prediction map + int32 GT map
        if "labelmap_pair_counts" in kern:
            out["pair_counts_TBps"] = round(hbm_bytes / (kern["labelmap_pair_counts"] * 1e-6) / 1e12, 2)
        if model is not None:
            x = torch.randn(B, 3, 1024, 1024, device=dev)
            with torch.no_grad():
                for _ in range(2):
                    model(pixel_values=x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    model(pixel_values=x)
                torch.cuda.synchronize()
            out["forward_ms"] = round((time.perf_counter() - t0) * 1e3 / 5, 2)
        if a.oracle:
            from oracle import coco_eval as C
            preds = C.preds_from_postprocess([{"segmentation": s, "segments_info": i} for s, i in zip(segs, infos)])
            t0 = time.perf_counter()
            target = C.targets_from_maps(maps, mappings)
            ev = C.CocoSegmEval()
            ev.update(preds, target)
            ev.evaluate(ev.classes())
            out["oracle_host_evaluate_s"] = round(time.perf_counter() - t0, 2)
            ora = MeanAveragePrecision()
            ora.update_from_maps(segs_d, infos, maps, mappings)
            o = C.CocoSegmEval()
            o.update(preds, target)
            out["equals_oracle"] = all(torch.equal(ora.compute()[k], v) for k, v in o.compute().items())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
