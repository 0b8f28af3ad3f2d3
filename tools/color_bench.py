"""Per-plant colour sums and the vegetation-index kernels on the GPU against the one-read statistics
kernel, the memory floor and the host loop.

    python tools/color_bench.py [--rounds 5] [--inner 10] [--no-host] [--out profiles/color_bench.jsonl]

Workload: `shape_bench.make_map`'s int32 id map (-1 background) of 1024 x 1024 and of 4096 x 4096 with 20, 100 and 1000
instances, and a picture of the same size: plant pixels (60, 140, 50), soil pixels (120, 90, 60), every byte plus uniform
noise in [-25, 25].  In one process, alternating per round and timed with HIP events, `--inner` calls per timing:
- `color_stats`: `ops.labelmap_color_stats` with 12 hue bins; `color_stats_no_hue`: the same without the hue histogram;
- `index_hist`, `index_mask`: `ops.image_index_hist` and `ops.image_index_mask` under "exg";
- `instance_stats`: `ops.labelmap_instance_stats` on the same map, the cost of one read of the map (4 B per pixel);
- `host` (once, a host clock): map and picture copied to the host, then one np.nonzero per id and the fourteen sums of its
  pixels (the Q12 index vectorised, no hue) -- what a consumer does without the kernel.
One JSON line per map: medians and spreads, the ratios to `instance_stats` and to the floor of 7 B per pixel at 8 TB/s,
and that the device's sums equal the host loop's.  Kernel times come from a profiler run of this script, not from here."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from shape_bench import event_ms, make_map, spread  # noqa: E402
from weed_instance_segmentation_amd import ops  # noqa: E402

PEAK_BYTES_PER_S = 8e12
COEF = (-1, 2, -1)
THRESHOLD, DARK, BRIGHT = 70, 32, 250


def make_picture(m, seed):
    rng = np.random.default_rng(seed)
    base = np.where((m >= 0)[..., None], np.array((60, 140, 50)), np.array((120, 90, 60)))
    return np.clip(base + rng.integers(-25, 26, base.shape), 0, 255).astype(np.uint8)


def host_loop(dev_img, dev_map, n):
    """(n, 14) sums on the host, from the device tensors."""
    img, m = dev_img.cpu().numpy(), dev_map.cpu().numpy()
    out = np.zeros((n, 14), np.int64)
    for k in range(n):
        ys, xs = np.nonzero(m == k)
        if len(ys) == 0:
            continue
        px = img[ys, xs].astype(np.int64)
        R, G, B = px[:, 0], px[:, 1], px[:, 2]
        I = COEF[0] * R + COEF[1] * G + COEF[2] * B
        s = R + G + B
        q = np.where(s > 0, (4096 * I) // np.maximum(s, 1), 0)  # numpy's // floors
        mx = px.max(1)
        out[k] = [len(ys), R.sum(), G.sum(), B.sum(), (R * R).sum(), (G * G).sum(), (B * B).sum(), (R * G).sum(),
                  (R * B).sum(), (G * B).sum(), (I > THRESHOLD).sum(), q.sum(), (mx < DARK).sum(), (mx >= BRIGHT).sum()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the host loop (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("color_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:  # one run, one file: a second run replaces the lines
        for H, W, n in [(H, H, n) for H in (1024, 4096) for n in (20, 100, 1000)]:
            m = make_map(H, W, n, seed=H + n)
            maps = torch.from_numpy(m)[None].cuda()
            imgs = torch.from_numpy(make_picture(m, seed=H + n + 1))[None].cuda()
            thr = torch.full((1,), THRESHOLD, dtype=torch.int32, device="cuda")
            kw = dict(N=n, index=COEF, dark=DARK, bright=BRIGHT)
            run = {"color_stats": lambda: ops.labelmap_color_stats(imgs, maps, thr, hue_bins=12, **kw),
                   "color_stats_no_hue": lambda: ops.labelmap_color_stats(imgs, maps, thr, hue_bins=None, **kw),
                   "index_hist": lambda: ops.image_index_hist(imgs, COEF),
                   "index_mask": lambda: ops.image_index_mask(imgs, thr, COEF),
                   "instance_stats": lambda: ops.labelmap_instance_stats(maps, N=n)}
            sums = run["color_stats"]()[0]
            for fn in run.values():  # warm every shape the timed window uses
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in run}
            for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                for k, fn in run.items():
                    ms[k].append(event_ms(fn, args.inner))
            med = {k: statistics.median(v) for k, v in ms.items()}
            floor7_ms, floor4_ms = 7.0 * H * W / PEAK_BYTES_PER_S * 1e3, 4.0 * H * W / PEAK_BYTES_PER_S * 1e3
            rec = {"H": H, "W": W, "instances": n, "rounds": args.rounds, "inner": args.inner,
                   "present": int((sums[0, :, 0] > 0).sum()), "plant_fraction": round(float((m >= 0).mean()), 3),
                   "lds_accumulators": n <= ops.color.COLOR_LDS_MAX_IDS,
                   **{k + "_us": spread(v) for k, v in ms.items()},
                   "color_stats_over_instance_stats": round(med["color_stats"] / med["instance_stats"], 2),
                   "color_stats_no_hue_over_instance_stats": round(med["color_stats_no_hue"] / med["instance_stats"], 2),
                   "floor_7B_per_pixel_us": round(floor7_ms * 1e3, 2),
                   "color_stats_over_floor": round(med["color_stats"] / floor7_ms, 1),
                   "color_stats_no_hue_over_floor": round(med["color_stats_no_hue"] / floor7_ms, 1),
                   "index_hist_over_3B_floor": round(med["index_hist"] / (floor7_ms * 3 / 7), 1),
                   "index_mask_over_4B_floor": round(med["index_mask"] / floor4_ms, 1)}
            if not args.no_host:
                t0 = time.perf_counter()
                ref = host_loop(imgs[0], maps[0], n)
                host_ms = (time.perf_counter() - t0) * 1e3
                rec.update({"host_ms": round(host_ms, 1), "host_over_device": round(host_ms / med["color_stats"], 1),
                            "routes_equal": bool(np.array_equal(sums[0].cpu().numpy(), ref))})
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
