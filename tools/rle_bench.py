"""Run-length encoding of id maps on the GPU: the two-launch route against the per-segment route.

    python tools/rle_bench.py [--rounds 7] [--out profiles/rle_bench.jsonl]

Workload: B = 8 fp32 id maps of 1024 x 1024 (-1 background) with about 10, 50 and 100 live instances.  In one process,
alternating per round; every timing is a host clock around work that ends with its result on the host (both routes end
in Python lists), with a device synchronise before and after:
- `parent`: `convert_segmentation_to_rle` per image -- one `torch.unique`, then a `where`, `cat`, `where`, `tolist` per id;
- `hf`: `encode_label_maps(maps, n, format="hf")`, the same lists;
- `coco`: `encode_label_maps(maps, n, format="coco")`, column-major with the string compression.
`count_us` / `write_us` are HIP-event times of the two launches alone (`--inner` per timing).  Bytes: either launch reads
the map once (4 B per pixel); the count launch writes and the write launch reads the per-group table (4 B per group and
slot, `table_bytes`); the write launch stores 4 B per toggle.
One JSON line per shape: medians and spread (min, max) over rounds, the speed-ups, and that the routes gave the same lists.
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

from weed_instance_segmentation_amd import _lib, encode_label_maps, ops  # noqa: E402
from weed_instance_segmentation_amd.postprocess import convert_segmentation_to_rle  # noqa: E402


def make_maps(B, H, W, n, seed):
    """Post-processor-like maps: n ellipses per image over -1, later ones painting over earlier ones."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    maps = torch.full((B, H, W), -1.0)
    for b in range(B):
        for k in range(n):
            cy, cx = (int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g)))
            ry, rx = (int(torch.randint(12, 120, (1,), generator=g)), int(torch.randint(12, 120, (1,), generator=g)))
            maps[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k
    return maps


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_us(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def spread(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rle_bench needs an MI355X")
    B, H, W = 8, 1024, 1024
    lib = _lib.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for n in (10, 50, 100):
            maps = make_maps(B, H, W, n, seed=n).cuda()
            parent = lambda: [convert_segmentation_to_rle(maps[b]) for b in range(B)]
            hf = lambda: encode_label_maps(maps, n=n, format="hf")
            coco = lambda: encode_label_maps(maps, n=n, format="coco")
            want = parent()
            same = [list(d.values()) for d in hf()] == want
            live = sum(len(w) for w in want) - B  # the background is one of the lists
            coco()
            p_ms, h_ms, c_ms = [], [], []
            for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
                p_ms.append(host_ms(parent)[0])
                h_ms.append(host_ms(hf)[0])
                c_ms.append(host_ms(coco)[0])
            rec = {"B": B, "H": H, "W": W, "instances": n, "live_instances_per_image": round(live / B, 1),
                   "rounds": args.rounds, "inner": args.inner, "parent_ms": spread(p_ms), "hf_ms": spread(h_ms),
                   "coco_ms": spread(c_ms), "speedup_hf": round(statistics.median(p_ms) / statistics.median(h_ms), 1),
                   "routes_equal": same}
            for order, name in ((0, "row_major"), (1, "column_major")):
                counts, positions, offsets = ops.labelmap_toggles(maps, n, order)
                offsets_d = torch.from_numpy(offsets.astype(np.int32)).cuda()
                ws = torch.empty(int(lib.wm2f_rle_workspace(B, H, W, n, order)), dtype=torch.uint8, device="cuda")
                cnt = torch.empty(B, n + 1, dtype=torch.int32, device="cuda")
                bad = torch.empty(B, dtype=torch.int32, device="cuda")
                p = lambda t: t.data_ptr()
                stream = torch.cuda.current_stream().cuda_stream
                count = lambda: lib.wm2f_labelmap_toggle_counts(p(maps), _lib.WM2F_F32, p(cnt), p(bad), p(ws), B, H, W, n, order, stream)
                # the write launch consumes the table, so a timed pair is count + write, and write = pair - count
                pair = lambda: (count(), lib.wm2f_labelmap_toggles(p(maps), _lib.WM2F_F32, p(offsets_d), p(positions), p(ws),
                                                                   B, H, W, n, order, stream))
                count(), pair()
                c_us = [event_us(count, args.inner) for _ in range(args.rounds)]
                w_us = [event_us(pair, args.inner) - c for c in c_us]
                rec[name] = {"count_us": spread(c_us), "write_us": spread(w_us), "toggles": int(offsets[-1]),
                             "map_bytes": maps.numel() * 4, "table_bytes": ws.numel(), "position_bytes": int(offsets[-1]) * 4}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
