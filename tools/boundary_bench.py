"""Boundary bands on the GPU: the id-map route against a composed stock-ops route.

    python tools/boundary_bench.py [--rounds 7] [--inner 10] [--out profiles/boundary_bench.jsonl]

Workload: B = 8 image pairs -- an fp32 prediction id map (-1 background, the post-processor's) and a uint8 raw GT map
whose instances are the prediction's moved by a few pixels -- at 1024 x 1024 with 20 and with 100 instances, and at
256 x 256 with 20; d = boundary_dilation(H, W) (29 and 7).  Both routes end with the (P, G) band intersections and the
band areas of every image on the device.  Timed with HIP events in one process, alternating per round, median and spread
(min, max) over `--rounds`:
- `new`: two `ops.labelmap_boundary` calls (prediction stack, GT stack) and one `ops.labelmap_pair_counts` on the band
  maps: five launches whatever the number of instances and d;
- `composed`: per image and side, `map == id` for every instance at once, the complement padded with d pixels of
  "outside", `max_pool2d` with kernel 2d+1 (the erosion), AND with the mask, then the intersections as one matrix
  product of the flattened bands and the areas as sums.  One timing is one pass over the batch.
The two band calls alone are timed as well (`--inner` calls per timing) and set against the bytes they must move at
8 TB/s: per pixel the map twice, the one-byte plane written and read, and the int32 result written.
One JSON line per shape; the routes' intersections and areas are checked equal in the run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from weed_instance_segmentation_amd import ops  # noqa: E402
from weed_instance_segmentation_amd.instances import boundary_dilation  # noqa: E402

HBM_BPS = 8e12


def make_pair(B, H, W, n, seed):
    """Elliptical blobs with ragged (sinusoidal) outlines; the GT is the prediction moved by up to 3 px."""
    rng = np.random.default_rng(seed)
    pred = np.full((B, H, W), -1, np.float32)
    gt = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for k in range(n):
            cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
            ry, rx = int(rng.integers(H // 16, H // 5)), int(rng.integers(W // 16, W // 5))
            y0, y1, x0, x1 = max(0, cy - 2 * ry), min(H, cy + 2 * ry), max(0, cx - 2 * rx), min(W, cx + 2 * rx)
            yy, xx = np.mgrid[y0:y1, x0:x1]  # the blob's window: the outline stays within 1.15 radii
            r = 1.0 + 0.15 * np.sin(np.arctan2(yy - cy, xx - cx) * int(rng.integers(5, 12)))
            m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < r ** 2
            pred[b, y0:y1, x0:x1][m] = k
            dy, dx = (int(v) for v in rng.integers(-3, 4, 2))
            full = np.zeros((H, W), bool)
            full[y0:y1, x0:x1] = m
            gt[b][np.roll(full, (dy, dx), (0, 1))] = k + 1
    return pred, gt


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def bands_composed(one_map, ids, d):
    """(N, H, W) bool bands of the listed ids of one (H, W) map with stock ops: N masks, N erosions."""
    masks = one_map.unsqueeze(0) == ids.view(-1, 1, 1).to(one_map.dtype)
    outside = F.pad((~masks).to(torch.float16 if one_map.is_cuda else torch.float32).unsqueeze(1), (d, d, d, d), value=1.0)  # beyond the image is outside
    touched = F.max_pool2d(outside, kernel_size=2 * d + 1, stride=1).squeeze(1) > 0    # some pixel of the square is outside
    return masks & touched


def route_composed(pred, gt, n, d):
    pid = torch.arange(n, device=pred.device)
    gid = torch.arange(1, n + 1, device=pred.device)
    inter, pa, ga = [], [], []
    for b in range(pred.shape[0]):
        pb = bands_composed(pred[b], pid, d).flatten(1).float()
        gb = bands_composed(gt[b], gid, d).flatten(1).float()
        inter.append(pb @ gb.T)  # 0 / 1 products summed in fp32: exact below 2^24 pixels
        pa.append(pb.sum(1))
        ga.append(gb.sum(1))
    return torch.stack(inter).to(torch.int32), torch.stack(pa).to(torch.int32), torch.stack(ga).to(torch.int32)


def route_new(pred, gt, gids, gn, n, d):
    hist = ops.labelmap_pair_counts(ops.labelmap_boundary(pred, d), ops.labelmap_boundary(gt, d), gids, gn, n)
    return hist[:, 1:, 1:], hist[:, 1:, :].sum(2, dtype=torch.int32), hist[:, :, 1:].sum(1, dtype=torch.int32)


def stats(ms):
    return {"median": round(statistics.median(ms) * 1e3, 2), "min": round(min(ms) * 1e3, 2), "max": round(max(ms) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    B = 8
    with open(args.out, "a") as f:
        for H, W, n in ((1024, 1024, 20), (1024, 1024, 100), (256, 256, 20)):
            pred_np, gt_np = make_pair(B, H, W, n, seed=n + H)
            pred, gt = torch.from_numpy(pred_np).cuda(), torch.from_numpy(gt_np).cuda()
            d = boundary_dilation(H, W)
            gids = torch.arange(1, n + 1, dtype=torch.int32).expand(B, n).contiguous().cuda()
            gn = torch.full((B,), n, dtype=torch.int32).cuda()
            new = lambda: route_new(pred, gt, gids, gn, n, d)  # noqa: E731
            composed = lambda: route_composed(pred, gt, n, d)  # noqa: E731
            bands = lambda: (ops.labelmap_boundary(pred, d), ops.labelmap_boundary(gt, d))  # noqa: E731
            same = all(bool(torch.equal(a, b)) for a, b in zip(new(), composed()))
            for _ in range(3):
                new()
            composed()
            times = {"new": [], "composed": [], "bands": []}
            for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                times["new"].append(event_ms(new, args.inner))
                times["composed"].append(event_ms(composed, 1))
                times["bands"].append(event_ms(bands, args.inner))
            band_bytes = B * H * W * ((4 + 1 + 4 + 1 + 4) + (1 + 1 + 1 + 1 + 4))  # the fp32 stack and the uint8 stack
            rec = {"B": B, "H": H, "W": W, "instances": n, "d": d, "rounds": args.rounds, "inner_launches": args.inner,
                   "routes_equal": same, "new_us": stats(times["new"]), "composed_us": stats(times["composed"]),
                   "band_calls_us": stats(times["bands"]), "band_calls_bytes": band_bytes,
                   "band_calls_bytes_per_s": round(band_bytes / (statistics.median(times["bands"]) * 1e-3), 0),
                   "band_calls_share_of_8TBps": round(band_bytes / HBM_BPS / (statistics.median(times["bands"]) * 1e-3), 3)}
            spread = max(rec["new_us"]["max"] - rec["new_us"]["min"], rec["composed_us"]["max"] - rec["composed_us"]["min"])
            rec["speedup_of_medians"] = round(rec["composed_us"]["median"] / rec["new_us"]["median"], 1)
            rec["new_below_composed_by_more_than_spread"] = bool(rec["composed_us"]["median"] - rec["new_us"]["median"] > spread)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
