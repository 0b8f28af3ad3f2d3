"""Blending tile scores on the GPU: the one call into csrc/tile_blend.hip against a torch route.

    python tools/tile_blend_bench.py [--rounds 7] [--inner 20] [--out profiles/tile_blend_bench.jsonl]

Workload: a 6000 x 4000 image (H = 4000, W = 6000) in tiles of 1024 with overlap 256 (5 x 8 = 40 tiles), random scores on
the post-processor's 384 x 384 grid, C = 3 and C = 19 classes, F = 1 view and F = 4 views (all four flip codes).  Both
routes start from the (F, T, C, 384, 384) scores on the device and end with the (H, W) map and the (C, H, W) blended
scores on the device.  Timed with HIP events in one process, alternating per round, median and spread (min, max) over
`--rounds`:
- `new`: `ops.tile_blend(..., want_scores=True)`; `new_seg`: the same call for the map alone;
- `torch`: per view and tile `interpolate(bilinear, align_corners=False)` to the tile size, `flip` for a flipped view,
  times the same window, added into a (C, H, W) plane and a weight plane; then one division and one argmax.
The new call's time is set against the bytes it must move at 8 TB/s (`bytes_bound`): the map written once (4 H W), the
scores written once (4 C H W, left out for `new_seg`), the score grids read once (4 F T C 384 384).
One JSON line per workload.  The routes add in different orders and the torch route fuses nothing the same way, so they
are compared with a tolerance: the largest score difference and the share of pixels with another argmax are in the line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from weed_instance_segmentation_amd import ops, tile_windows  # noqa: E402

HBM_BPS = 8e12
GRID = 384


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def window(side, ramp):
    i = torch.arange(side, device="cuda")
    return torch.minimum(torch.minimum(i + 1, side - i), torch.tensor(ramp, device="cuda")).float()


def route_torch(scores, grid, codes, ramp, win):
    F, T, C = scores.shape[:3]
    acc = torch.zeros(C, grid.height, grid.width, device="cuda")
    wsum = torch.zeros(grid.height, grid.width, device="cuda")
    for f, code in enumerate(codes):
        dims = [d for bit, d in ((2, 1), (1, 2)) if code & bit]
        for t, (y0, x0, y1, x1) in enumerate(grid.windows):
            v = torch.nn.functional.interpolate(scores[f, t:t + 1], size=(grid.th, grid.tw), mode="bilinear", align_corners=False)[0]
            if dims:
                v = torch.flip(v, dims)
            acc[:, y0:y1, x0:x1] += win * v
            wsum[y0:y1, x0:x1] += win
    out = acc / wsum
    return out.argmax(0), out


def stats(ms):
    return {"median": round(statistics.median(ms) * 1e3, 2), "min": round(min(ms) * 1e3, 2), "max": round(max(ms) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_blend_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tile_blend_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    H, W, tile, overlap = 4000, 6000, 1024, 256
    grid = tile_windows(H, W, tile, overlap)
    T = grid.n_tiles
    ys = torch.tensor(grid.ys, dtype=torch.int32, device="cuda")
    xs = torch.tensor(grid.xs, dtype=torch.int32, device="cuda")
    ramp = (overlap, overlap)
    win = window(grid.th, ramp[0])[:, None] * window(grid.tw, ramp[1])[None, :]
    with open(args.out, "a") as f:
        for C in (3, 19):
            for codes in ((0,), (0, 1, 2, 3)):
                F = len(codes)
                gen = torch.Generator(device="cuda").manual_seed(1000 * C + F)
                scores = torch.rand(F, T, C, GRID, GRID, device="cuda", generator=gen)
                flips = torch.tensor(codes, dtype=torch.int32, device="cuda")
                new = lambda: ops.tile_blend(scores, ys, xs, flips, (H, W), (grid.th, grid.tw), ramp, want_scores=True)  # noqa: E731
                new_seg = lambda: ops.tile_blend(scores, ys, xs, flips, (H, W), (grid.th, grid.tw), ramp)  # noqa: E731
                ref = lambda: route_torch(scores, grid, codes, ramp, win)  # noqa: E731
                (s1, o1), (s2, o2) = new(), ref()
                score_diff = float((o1 - o2).abs().max())
                other_argmax = float((s1.long() != s2).float().mean())
                del s2, o2
                for _ in range(3):
                    new()
                    new_seg()
                times = {"new": [], "new_seg": [], "torch": []}
                for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                    times["new"].append(event_ms(new, args.inner))
                    times["torch"].append(event_ms(ref, 1))
                    times["new_seg"].append(event_ms(new_seg, args.inner))
                grids = 4 * F * T * C * GRID * GRID
                nbytes, nbytes_seg = 4 * H * W + 4 * C * H * W + grids, 4 * H * W + grids
                new_s, seg_s = statistics.median(times["new"]) * 1e-3, statistics.median(times["new_seg"]) * 1e-3
                rec = {"H": H, "W": W, "tile": tile, "overlap": overlap, "tiles": T, "C": C, "F": F, "grid": GRID,
                       "ramp": list(ramp), "rounds": args.rounds, "inner_launches": args.inner,
                       "largest_score_difference": score_diff, "share_of_pixels_with_another_argmax": other_argmax,
                       "new_us": stats(times["new"]), "new_seg_us": stats(times["new_seg"]), "torch_us": stats(times["torch"]),
                       "bytes_bound": nbytes, "share_of_8TBps": round(nbytes / HBM_BPS / new_s, 3),
                       "bytes_bound_seg": nbytes_seg, "share_of_8TBps_seg": round(nbytes_seg / HBM_BPS / seg_s, 3)}
                spread = max(rec["new_us"]["max"] - rec["new_us"]["min"], rec["torch_us"]["max"] - rec["torch_us"]["min"])
                rec["torch_over_new_medians"] = round(rec["torch_us"]["median"] / rec["new_us"]["median"], 2)
                rec["new_below_torch_by_more_than_spread"] = bool(rec["torch_us"]["median"] - rec["new_us"]["median"] > spread)
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
                del scores, s1, o1
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
