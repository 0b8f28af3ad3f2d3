"""Device preprocessing timing: `Mask2FormerImageProcessor` at B = 8 for 1024 x 768 -> 800 x 1088,
1024 x 1024 -> 1024 x 1024 (`size={"height": 1024, "width": 1024}`) and the reference's field-image size 4000 x 3000 ->
800 x 1088, each without and with 16-instance maps.  One JSON line per case, appended to
profiles/r05_preprocess_bench.jsonl.

    python tools/preprocess_bench.py [--reps 20] [--out profiles/r05_preprocess_bench.jsonl] [--tree NAME]

`kernel_ms`: HIP events around the image call of ops.resize_normalize_u8 alone (inputs already on the device);
`gbps`: 3 B/px read at the input size plus 3 B/px written and read for the row-pass intermediate and 12 + 8 B/px
written at the output size, over kernel_ms (the byte count of the two-pass kernels, kept so that records compare).
`label_kernel_ms`: the same around ops.resize_nearest_labels alone, on the lines with maps.  `wall_ms`: the whole
processor call, synchronised, with the uint8 host-to-device copy.  `--tree` adds a `tree` field to every line, for
records that compare two builds.  `dependency_ms`: Mask2FormerImageProcessorPil on the host for the same batch, only where
transformers imports (`host_cores` says how many the host has).
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

from weed_instance_segmentation_amd import Mask2FormerImageProcessor, ops  # noqa: E402
from weed_instance_segmentation_amd import preprocess as P  # noqa: E402


def batch(B, H, W, n_ids, seed=0):
    rng = np.random.default_rng(seed)
    ims = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    maps = None
    if n_ids:
        maps = []
        for _ in range(B):
            m = np.zeros((H, W), np.uint8)
            for i in range(1, n_ids + 1):
                y, x = rng.integers(0, H - 64), rng.integers(0, W - 64)
                m[y:y + rng.integers(32, H // 4), x:x + rng.integers(32, W // 4)] = i
            maps.append(m)
    return ims, maps


def event_ms(call, reps):
    for _ in range(3):
        call()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def label_kernel_ms(maps, size, reps):
    """The label call alone on device-resident maps, index tables built once."""
    H, W = maps[0].shape
    h, w = P.output_size(H, W, size, 32)
    tab = np.concatenate([P.nearest_table(W, w), P.nearest_table(H, h)]).astype(np.int32)
    desc = np.array([[b * H * W, H, W, h, w, 0, w] for b in range(len(maps))], np.int64)
    dev = torch.from_numpy(np.stack(maps).reshape(-1)).cuda()
    t_tab = torch.from_numpy(tab).cuda()
    return event_ms(lambda: ops.resize_nearest_labels(dev, desc, t_tab, h, w, 255), reps)


def kernel_ms(ims, size, reps):
    """The image call alone on device-resident inputs, tables built once."""
    H, W = ims[0].shape[:2]
    h, w = P.output_size(H, W, size, 32)
    bx, cx = P.bilinear_tables(W, w)
    by, cy = P.bilinear_tables(H, h)
    tab = np.concatenate([bx.ravel(), cx.ravel(), by.ravel(), cy.ravel()]).astype(np.int32)
    o = np.cumsum([0, bx.size, cx.size, by.size])
    B = len(ims)
    desc = np.array([[b * H * W * 3, b * H * w * 3, H, W, h, w, o[0], o[1], cx.shape[1], o[2], o[3], cy.shape[1]]
                     for b in range(B)], np.int64)
    img = torch.from_numpy(np.stack(ims).reshape(-1)).cuda()
    t_tab = torch.from_numpy(tab).cuda()
    lut = torch.from_numpy(P.normalize_table(True, 1 / 255, True, P.IMAGENET_DEFAULT_MEAN, P.IMAGENET_DEFAULT_STD)).cuda()
    ms = event_ms(lambda: ops.resize_normalize_u8(img, desc, t_tab, lut, h, w), reps)
    nbytes = B * (H * W * 3 + 2 * H * w * 3 + h * w * (12 + 8))
    return ms, nbytes / ms / 1e6, (h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_preprocess_bench.jsonl"))
    ap.add_argument("--tree", default=None)
    args = ap.parse_args()
    try:
        from transformers.models.mask2former.image_processing_pil_mask2former import Mask2FormerImageProcessorPil
        dep = Mask2FormerImageProcessorPil()
    except Exception:  # noqa: BLE001  (not installed where the GPU runs)
        dep = None
    proc = Mask2FormerImageProcessor()
    B = 8
    recs = []
    for (H, W, size) in [(768, 1024, {"shortest_edge": 800, "longest_edge": 1333}),
                         (1024, 1024, {"height": 1024, "width": 1024}),
                         (3000, 4000, {"shortest_edge": 800, "longest_edge": 1333})]:
        for n_ids in (0, 16):
            ims, maps = batch(B, H, W, n_ids)
            kw = dict(images=ims, segmentation_maps=maps, size=size, ignore_index=255,
                      instance_id_to_semantic_id={i: 1 for i in range(256)} if maps else None)
            k_ms, gbps, (h, w) = kernel_ms(ims, size, args.reps)
            for _ in range(3):
                proc(**kw)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                proc(**kw)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            rec = {"case": f"B{B}_{W}x{H}_to_{w}x{h}_ids{n_ids}", "B": B, "in_hw": [H, W], "out_hw": [h, w],
                   "n_ids": n_ids, "kernel_ms": round(k_ms, 4), "kernel_gbps": round(gbps, 1),
                   "kernel_frac_of_8TBps": round(gbps / 8000, 3), "wall_ms": round(float(np.median(ts)), 3),
                   "device": torch.cuda.get_device_name(0), "reps": args.reps}
            if maps:
                rec["label_kernel_ms"] = round(label_kernel_ms(maps, size, args.reps), 4)
            if args.tree:
                rec["tree"] = args.tree
            if dep is not None:
                t0 = time.perf_counter()
                dep(return_tensors="pt", **kw)
                rec["dependency_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec["host_cores"] = os.cpu_count()
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
