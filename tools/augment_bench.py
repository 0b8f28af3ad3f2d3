"""Training augmentation timing: the one-call route (`preprocess(..., augment=params)`, kernels of
csrc/augment.hip) against the composed route on the un-augmented kernels: flip of the source, `preprocess` at the whole
(h, w) frame, slice and pad in torch.  Images only (the map path is one small launch on either route).  One JSON line
per case, appended to profiles/augment_bench.jsonl.

    python tools/augment_bench.py [--rounds 15] [--out profiles/augment_bench.jsonl]

Cases: B = 16 sources of 1024 x 1024 under the jitter recipe (crop 1024 x 1024) at f = 0.5, 1.0 and 2.0, and B = 16
sources of 800 x 1333 under the short-edge recipe (edge 800); each with the images already on the device and with the
images in pinned host memory.  The two routes alternate inside every round; times are HIP events around the whole call,
`*_ms` the median over rounds and `*_spread_ms` max - min.  `wins` is the issue's condition: the new median is below
the composed median by more than either spread.  `kernel_ms` is the new image kernel alone (tables and descriptors
built once), `kernel_tbps` its algorithmic bytes (3 B per source pixel the window's taps reach, 12 + 8 B per padded
output pixel) over that time, `roofline_share` of 8 TB/s.
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

from weed_instance_segmentation_amd import AugmentParams, Mask2FormerImageProcessor, ops  # noqa: E402
from weed_instance_segmentation_amd import preprocess as P  # noqa: E402

HBM_TBPS = 8.0


def jitter(H, W, f, crop, flip):
    r = min(crop[0] * f / H, crop[1] * f / W)
    h, w = max(1, round(H * r)), max(1, round(W * r))
    ch, cw = min(crop[0], h), min(crop[1], w)
    return AugmentParams(flip, (h, w), ((h - ch) // 2, (w - cw) // 3), (ch, cw))


def new_route(proc, ims, params, pad):
    return proc.preprocess(ims, augment=params, pad_size=pad)["pixel_values"]


def composed_route(proc, ims, params, pad):
    """Flip, the un-augmented call at the whole frame (one call: every image of a case shares its frame), slice, pad."""
    p = params[0]
    (h, w), (y0, x0), (ch, cw) = p.size, p.origin, p.window
    src = [(torch.flip(im, dims=[1]) if q.flip else im) for im, q in zip(ims, params)]
    r = proc.preprocess(src, size={"height": h, "width": w}, size_divisor=0)
    Hp, Wp = (pad["height"], pad["width"]) if pad else (ch, cw)
    pv = torch.zeros(len(ims), 3, Hp, Wp, device="cuda")
    pm = torch.zeros(len(ims), Hp, Wp, device="cuda", dtype=torch.int64)
    pv[:, :, :ch, :cw] = r["pixel_values"][:, :, y0:y0 + ch, x0:x0 + cw]
    pm[:, :ch, :cw] = r["pixel_mask"][:, y0:y0 + ch, x0:x0 + cw]
    return pv


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def kernel_alone(ims, params, pad, rounds):
    """The new image kernel on device-resident inputs, tables and descriptors built once.  Returns (ms, bytes)."""
    parts, n, rows, off, nbytes = [], 0, [], 0, 0

    def put(a):
        nonlocal n
        a = np.ascontiguousarray(a, np.int32).reshape(-1)
        parts.append(a)
        n += a.size
        return n - a.size

    Hp, Wp = (pad["height"], pad["width"]) if pad else params[0].window
    for im, p in zip(ims, params):
        H, W = im.shape[:2]
        (h, w), (y0, x0), (ch, cw) = p.size, p.origin, p.window
        bx, cx = P.bilinear_tables(W, w)
        by, cy = P.bilinear_tables(H, h)
        rows.append([off, H, W, h, w, put(bx), put(cx), cx.shape[1], put(by), put(cy), cy.shape[1], p.flip, y0, x0, ch, cw])
        off += H * W * 3
        src_rows = by[y0 + ch - 1, 0] + by[y0 + ch - 1, 1] - by[y0, 0]
        src_cols = bx[x0 + cw - 1, 0] + bx[x0 + cw - 1, 1] - bx[x0, 0]
        nbytes += int(src_rows) * int(src_cols) * 3 + Hp * Wp * 20
    img = torch.cat([im.reshape(-1) for im in ims]).cuda()
    tab = torch.from_numpy(np.concatenate(parts)).cuda()
    lut = torch.from_numpy(P.normalize_table(True, 1 / 255, True, P.IMAGENET_DEFAULT_MEAN, P.IMAGENET_DEFAULT_STD)).cuda()
    desc = np.array(rows, np.int64)
    call = lambda: ops.augment_resize_normalize_u8(img, desc, tab, lut, Hp, Wp)  # noqa: E731
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    return statistics.median(timed(call)[0] for _ in range(rounds)), nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs an MI355X: nothing is measured without one")
    proc = Mask2FormerImageProcessor()
    B = 16
    crop, pad = (1024, 1024), {"height": 1024, "width": 1024}
    edge = P.output_size(800, 1333, {"shortest_edge": 800, "longest_edge": 1333}, 32)
    cases = [(f"jitter_f{f}", (1024, 1024), [jitter(1024, 1024, f, crop, b % 2) for b in range(B)], pad)
             for f in (0.5, 1.0, 2.0)]
    cases.append(("short_edge_800", (800, 1333), [AugmentParams(b % 2, edge) for b in range(B)], None))
    rng = np.random.default_rng(0)
    lines = []
    for name, (H, W), params, pd in cases:
        host = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).pin_memory() for _ in range(B)]
        for where, ims in (("device", [t.cuda() for t in host]), ("pinned_host", host)):
            a = new_route(proc, ims, params, pd)
            b = composed_route(proc, ims, params, pd)
            if not torch.equal(a, b):
                raise SystemExit(f"{name} / {where}: the two routes disagree")
            for _ in range(2):
                new_route(proc, ims, params, pd), composed_route(proc, ims, params, pd)
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.rounds):
                t_new.append(timed(lambda: new_route(proc, ims, params, pd))[0])
                t_old.append(timed(lambda: composed_route(proc, ims, params, pd))[0])
            k_ms, nbytes = kernel_alone(ims, params, pd, args.rounds)
            new_ms, old_ms = statistics.median(t_new), statistics.median(t_old)
            s_new, s_old = max(t_new) - min(t_new), max(t_old) - min(t_old)
            line = {"case": name, "images": where, "B": B, "source": [H, W], "frame": list(params[0].size),
                    "window": list(params[0].window), "rounds": args.rounds,
                    "new_ms": round(new_ms, 4), "new_spread_ms": round(s_new, 4),
                    "composed_ms": round(old_ms, 4), "composed_spread_ms": round(s_old, 4),
                    "wins": bool(old_ms - new_ms > max(s_new, s_old)),
                    "kernel_ms": round(k_ms, 4), "kernel_bytes": nbytes,
                    "kernel_tbps": round(nbytes / (k_ms * 1e-3) / 1e12, 3),
                    "roofline_share": round(nbytes / (k_ms * 1e-3) / 1e12 / HBM_TBPS, 3)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
