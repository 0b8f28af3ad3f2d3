"""Overlays and contours on the GPU: the one-launch route against the host routes.

    python tools/overlay_bench.py [--rounds 7] [--inner 20] [--out profiles/overlay_bench.jsonl]

Workload: B = 8 pictures of 1024 x 1024 with 100 rectangular segments each, as an fp32 map (-1 background, the
post-processor's) and as a uint8 map.  Timed with HIP events, `--inner` launches per timing, median and spread over
`--rounds`:
- `kernel`: `ops.labelmap_overlay` at contour widths 2 (inner 1, outer 1: the default), 0 and 8, with the share of the
  HBM floor -- B*H*W*(3 + map bytes + 3) bytes at 8 TB/s -- each reaches.
Timed once with the host clock, on ONE picture:
- `numpy_per_segment`: tests/overlay_reference.py::overlay_painter, one `map == id` pass and two dilations per segment;
- `numpy_per_pixel`: overlay_reference of the same file;
- `matplotlib`: imshow + one contour() per segment + savefig at the picture's size on the Agg canvas, the calls of
  models/model_utils.py::plot_segmentation, when matplotlib is installed.
One JSON line per map dtype; the kernel's output is checked against overlay_reference on the first picture.
"""
from __future__ import annotations

import argparse
import io
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

from overlay_reference import overlay_painter, overlay_reference  # noqa: E402
from weed_instance_segmentation_amd import ops  # noqa: E402
from weed_instance_segmentation_amd.visualize import palette  # noqa: E402

HBM_BPS = 8e12


def make_maps(B, H, W, n, seed):
    rng = np.random.default_rng(seed)
    maps = np.full((B, H, W), -1, np.int64)
    for b in range(B):
        for k in range(n):
            y0, x0 = int(rng.integers(0, H - 16)), int(rng.integers(0, W - 16))
            maps[b, y0:y0 + int(rng.integers(8, 320)), x0:x0 + int(rng.integers(8, 320))] = k
    return maps


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def host_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def matplotlib_ms(image, seg, ids, rgba):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return None

    def draw():
        H, W = seg.shape
        fig, ax = plt.subplots(figsize=(W / 100, H / 100), dpi=100)
        ax.imshow(image)
        colour_mask = np.zeros((H, W, 4))
        masks = []
        for k, c in zip(ids, rgba):
            m = seg == k
            colour_mask[m] = [*(c[:3] / 255.0), 0.4]
            masks.append((m, [*(c[:3] / 255.0), 1.0]))
        ax.imshow(colour_mask)
        for m, c in masks:
            if m.any():
                ax.contour(m, levels=[0.5], colors=[c], linewidths=2)
        ax.axis("off")
        fig.savefig(io.BytesIO(), format="png")
        plt.close(fig)
    return host_ms(draw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_bench needs an MI355X")
    B, H, W, n = 8, 1024, 1024, 100
    raw = make_maps(B, H, W, n, seed=n)
    images = np.random.default_rng(0).integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    ids = np.arange(n, dtype=np.int32)
    rgba = np.concatenate([palette(n), np.full((n, 1), 102, np.uint8)], 1)
    order = np.arange(n, dtype=np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tables = (dev(np.tile(ids, (B, 1))), dev(np.full(B, n, np.int32)), dev(np.tile(rgba, (B, 1, 1))), dev(np.tile(order, (B, 1))))
    pictures = dev(images)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name, np_dt, esz in (("float32", np.float32, 4), ("uint8", np.uint8, 1)):
            maps_np = np.where(raw < 0, 255 if np_dt == np.uint8 else -1, raw).astype(np_dt)
            maps = dev(maps_np)
            run = lambda i, o: ops.labelmap_overlay(pictures, maps, *tables, default_rgba=(0, 0, 0, 0), inner=i, outer=o)  # noqa: E731
            want = overlay_reference(images[0], maps_np[0], ids, rgba, order, (0, 0, 0, 0), 1, 1)
            same = bool(torch.equal(run(1, 1)[0].cpu(), torch.from_numpy(want)))
            floor_bytes = B * H * W * (3 + esz + 3)
            rec = {"B": B, "H": H, "W": W, "segments": n, "map": name, "rounds": args.rounds, "inner_launches": args.inner,
                   "hbm_floor_bytes": floor_bytes, "hbm_floor_us_at_8TBps": round(floor_bytes / HBM_BPS * 1e6, 2),
                   "kernel_equals_reference": same}
            widths = {"width2": (1, 1), "width0": (0, 0), "width8": (4, 4)}
            for i, o in widths.values():
                for _ in range(3):
                    run(i, o)
            times = {k: [] for k in widths}
            for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                for k, (i, o) in widths.items():
                    times[k].append(event_ms(lambda: run(i, o), args.inner))
            for k, ms in times.items():
                med = statistics.median(ms)
                rec[f"kernel_{k}_us"] = {"median": round(med * 1e3, 2), "min": round(min(ms) * 1e3, 2), "max": round(max(ms) * 1e3, 2)}
                rec[f"kernel_{k}_share_of_hbm_floor"] = round(floor_bytes / HBM_BPS / (med * 1e-3), 3)
            one = (images[0], maps_np[0], ids, rgba, order, (0, 0, 0, 0), 1, 1)
            rec["numpy_per_segment_ms_per_image"] = round(host_ms(lambda: overlay_painter(*one)), 1)
            rec["numpy_per_pixel_ms_per_image"] = round(host_ms(lambda: overlay_reference(*one)), 1)
            mpl = matplotlib_ms(images[0], maps_np[0], ids, rgba)
            rec["matplotlib_ms_per_image"] = None if mpl is None else round(mpl, 1)
            rec["kernel_width2_us_per_image"] = round(rec["kernel_width2_us"]["median"] / B, 2)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
