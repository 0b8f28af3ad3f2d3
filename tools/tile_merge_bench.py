"""Merging per-tile instances on the GPU: the four calls into csrc/tiles.hip against a composed
stock-ops route.

    python tools/tile_merge_bench.py [--rounds 7] [--inner 5] [--out profiles/tile_merge_bench.jsonl]

Workloads: a 4096 x 4096 image in tiles of 1024 with overlap 256 (25 tiles, 72 pairs) and N = 100 ids per tile, and an
8192 x 8192 image (121 tiles, 420 pairs) with N = 200.  The scene is a grid of elliptical blobs, one per 128 x 128 (96 x 96)
cell, cut into exact crops that are renumbered per tile, as fp32 maps with -1 background (the post-processor's).  Both
routes start from the stacked tiles and the geometry tables on the device and end with the (H, W) int32 map on the device
and remap and the number of merged ids on the host.  Timed with HIP events in one process, alternating per round, median
and spread (min, max) over `--rounds`:
- `new`: `ops.tile_pair_counts`, `ops.tile_owned_counts`, `ops.tile_link`, `ops.tile_compose`, one device-to-host copy;
- `composed`: per pair one `bincount` of the two copied strips, per tile one `bincount` of its cell, one copy of the
  counts to the host, the link rule and a union-find there, then per tile one gather through its table and one
  slice-assign.
The new route's device time is set against the bytes it must move at 8 TB/s: every cell read twice (owned counts and
compose), every overlap rectangle read from both tiles, the output written once (`bytes_bound`).  The histograms are
traffic of their own, reported apart as `hist_bytes`: P (N+1)^2 int32 bins cleared by the pair counts and read once by the
link; `share_of_8TBps_with_hist` counts both.
One JSON line per workload; the routes' maps, remap tables and counts are checked equal in the run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from weed_instance_segmentation_amd import ops, tile_windows  # noqa: E402

HBM_BPS = 8e12


def make_scene(H, W, cell, seed):
    """(H, W) int32 ids with -1 background on the device: one ellipse per cell, of random size and place inside it."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ny, nx = H // cell, W // cell
    ry = torch.randint(cell // 8, cell // 2 - 2, (ny, nx), generator=g).cuda()
    rx = torch.randint(cell // 8, cell // 2 - 2, (ny, nx), generator=g).cuda()
    yy = torch.arange(H, device="cuda").view(-1, 1)
    xx = torch.arange(W, device="cuda").view(1, -1)
    cy, cx = (yy // cell).clamp(max=ny - 1), (xx // cell).clamp(max=nx - 1)
    dy = (yy - (cy * cell + cell // 2)).float() / ry[cy, cx].float()
    dx = (xx - (cx * cell + cell // 2)).float() / rx[cy, cx].float()
    inside = dy * dy + dx * dx < 1.0
    return torch.where(inside, cy * nx + cx, -1).to(torch.int32)


def cut(scene, grid, N, seed):
    """The scene's exact crops, every tile renumbered at random into [0, N): (T, th, tw) fp32, n_ids, labels."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    tiles, labels = [], torch.zeros(len(grid.windows), N, dtype=torch.int32)
    for t, (y0, x0, y1, x1) in enumerate(grid.windows):
        crop = scene[y0:y1, x0:x1]
        here, inv = torch.unique(crop, return_inverse=True)  # ascending; -1 first when present
        has_bg = int(here[0]) < 0
        n = len(here) - has_bg
        if n > N:
            raise SystemExit(f"tile {t} sees {n} objects, more than N = {N}")
        table = torch.full((len(here),), -1.0)
        new = torch.randperm(N, generator=g)[:n]
        table[has_bg:] = new.float()
        labels[t, new] = (here[has_bg:].cpu() % 2).to(torch.int32)
        tiles.append(table.cuda()[inv])
    return torch.stack(tiles), torch.full((len(grid.windows),), N, dtype=torch.int32).cuda(), labels.cuda()


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def route_new(tiles, n_ids, labels, geom, pairs, N, size):
    hist = ops.tile_pair_counts(tiles, n_ids, pairs, N)
    owned = ops.tile_owned_counts(tiles, n_ids, geom, N)
    remap, n_merged = ops.tile_link(hist, pairs, labels, n_ids, owned, (1, 2))
    out = ops.tile_compose(tiles, n_ids, geom, remap, size)
    host = torch.cat([remap.reshape(-1), n_merged]).cpu()
    return out, host[:-1].view(remap.shape), int(host[-1])


def route_new_device(tiles, n_ids, labels, geom, pairs, N, size):
    hist = ops.tile_pair_counts(tiles, n_ids, pairs, N)
    owned = ops.tile_owned_counts(tiles, n_ids, geom, N)
    remap, _ = ops.tile_link(hist, pairs, labels, n_ids, owned, (1, 2))
    return ops.tile_compose(tiles, n_ids, geom, remap, size)


def route_composed(tiles, labels_host, grid, N, size):
    """Stock ops and a host union-find.  The maps hold exact ids in [-1, N), so slot = value + 1."""
    NB = N + 1
    T = len(grid.windows)
    hists = []
    for a, b, ay, ax, by, bx, h, w in grid.pairs:
        sa = tiles[a, ay:ay + h, ax:ax + w].contiguous().long() + 1  # the copied strips
        sb = tiles[b, by:by + h, bx:bx + w].contiguous().long() + 1
        hists.append(torch.bincount((sa * NB + sb).reshape(-1), minlength=NB * NB))
    owned = []
    for t, (y0, x0, _, _) in enumerate(grid.windows):
        cy0, cy1, cx0, cx1 = grid.owner_cell(t)
        owned.append(torch.bincount((tiles[t, cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0].long() + 1).reshape(-1), minlength=NB)[1:])
    hist = torch.stack(hists).view(-1, NB, NB).cpu().numpy() if hists else np.zeros((0, NB, NB), np.int64)
    owned = torch.stack(owned).cpu().numpy()
    parent = list(range(T * N))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for p, (a, b, *_) in enumerate(grid.pairs):
        h = hist[p]
        area_a, area_b = h.sum(1), h.sum(0)
        for i, j in zip(*np.nonzero(h[1:, 1:])):
            if labels_host[a, i] == labels_host[b, j] and 2 * int(h[i + 1, j + 1]) >= min(int(area_a[i + 1]), int(area_b[j + 1])):
                ra, rb = find(a * N + int(i)), find(b * N + int(j))
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(g) for g in range(T * N)]).reshape(T, N)
    owning = np.unique(roots[owned > 0])
    number = np.full(T * N, -1, np.int32)
    number[owning] = np.arange(len(owning), dtype=np.int32)
    remap = number[roots]
    tables = torch.from_numpy(np.concatenate([np.full((T, 1), -1, np.int32), remap], 1)).cuda()
    out = torch.empty(size, dtype=torch.int32, device="cuda")
    for t, (y0, x0, _, _) in enumerate(grid.windows):
        cy0, cy1, cx0, cx1 = grid.owner_cell(t)
        out[cy0:cy1, cx0:cx1] = tables[t][tiles[t, cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0].long() + 1]
    return out, torch.from_numpy(remap), len(owning)


def stats(ms):
    return {"median": round(statistics.median(ms) * 1e3, 2), "min": round(min(ms) * 1e3, 2), "max": round(max(ms) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_merge_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tile_merge_bench needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for side, N, cell in ((4096, 100, 128), (8192, 200, 96)):
            grid = tile_windows(side, side, 1024, 256)
            scene = make_scene(side, side, cell, seed=side)
            tiles, n_ids, labels = cut(scene, grid, N, seed=N)
            labels_host = labels.cpu().numpy()
            geom, pairs = torch.from_numpy(grid.geom_table()).cuda(), torch.from_numpy(grid.pair_table()).cuda()
            size = (side, side)
            new = lambda: route_new(tiles, n_ids, labels, geom, pairs, N, size)  # noqa: E731
            new_dev = lambda: route_new_device(tiles, n_ids, labels, geom, pairs, N, size)  # noqa: E731
            composed = lambda: route_composed(tiles, labels_host, grid, N, size)  # noqa: E731
            (o1, r1, n1), (o2, r2, n2) = new(), composed()
            same = bool(torch.equal(o1, o2)) and bool(torch.equal(r1, r2)) and n1 == n2
            objects = int(torch.unique(scene).numel()) - 1
            truth_ok = n1 == objects and bool(((o1 < 0) == (scene < 0)).all())
            for _ in range(3):
                new()
            times = {"new": [], "new_dev": [], "composed": []}
            for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                times["new"].append(event_ms(new, args.inner))
                times["composed"].append(event_ms(composed, 1))
                times["new_dev"].append(event_ms(new_dev, args.inner))
            nbytes = 4 * (3 * side * side + 2 * sum(p[6] * p[7] for p in grid.pairs))
            hist_bytes = 2 * 4 * len(grid.pairs) * (N + 1) ** 2  # cleared once, read once by the link
            dev_s = statistics.median(times["new_dev"]) * 1e-3
            rec = {"H": side, "W": side, "tile": 1024, "overlap": 256, "tiles": len(grid.windows), "pairs": len(grid.pairs),
                   "N": N, "objects": objects, "merged": n1, "rounds": args.rounds, "inner_launches": args.inner,
                   "routes_equal": same, "scene_recovered": truth_ok, "new_us": stats(times["new"]),
                   "composed_us": stats(times["composed"]), "new_device_only_us": stats(times["new_dev"]),
                   "bytes_bound": nbytes, "bytes_per_s": round(nbytes / dev_s, 0),
                   "share_of_8TBps": round(nbytes / HBM_BPS / dev_s, 3), "hist_bytes": hist_bytes,
                   "share_of_8TBps_with_hist": round((nbytes + hist_bytes) / HBM_BPS / dev_s, 3)}
            spread = max(rec["new_us"]["max"] - rec["new_us"]["min"], rec["composed_us"]["max"] - rec["composed_us"]["min"])
            rec["speedup_of_medians"] = round(rec["composed_us"]["median"] / rec["new_us"]["median"], 1)
            rec["new_below_composed_by_more_than_spread"] = bool(rec["composed_us"]["median"] - rec["new_us"]["median"] > spread)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            del tiles, scene
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
