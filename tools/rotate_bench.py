"""Orientation timing: `ops.orient_u8` alone, what `AugmentParams.rotate` adds to a processor call, and
for scale the same operation in Pillow on the host.  One process, HIP events; one JSON line per case, appended to
profiles/rotate_bench.jsonl.

    python tools/rotate_bench.py [--rounds 15] [--out profiles/rotate_bench.jsonl]
    python tools/rotate_bench.py --call-only rotate          # one processor call with maps, for a kernel trace

Setup: B = 16 device-resident sources of 1024 x 1024 with id maps, under the jitter recipe of section 20 (f = 1, crop
1024 x 1024).  Cases: a pure quarter turn, a pure vertical flip and a rotation by 13.37 degrees.  `op_ms` is
`ops.orient_u8` alone on a packed buffer (median over rounds, `op_spread_ms` its max - min), `op_bytes` one read and one
write of every image (the rotation reads less than the whole image: its corners are fill), `op_tbps` their rate and
`roofline_share` the rate over 8 TB/s; `labels_ms` is `ops.orient_labels` on the uint8 maps.  Inside every round the
processor call with the stage and the same call without it alternate; `added_ms` is the median over rounds of the paired
difference, `added_spread_ms` its max - min.  `pillow_ms` is the median of the same operation on image and map in Pillow
on one core for ONE image.  --call-only runs one warm-up and one processor call of the case and prints nothing: run it
under a kernel trace, which should show one orient_kernel<3> and one orient_kernel<1> per call."""
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

from weed_instance_segmentation_amd import (AugmentParams, Mask2FormerImageProcessor, RotateParams, ops,  # noqa: E402
                                            rotate_images, rotate_maps)

HBM_TBPS = 8.0
B = 16
H = W = 1024
CASES = {"turn": RotateParams(turns=1), "vflip": RotateParams(vflip=True),
         "rotate": RotateParams(angle=13.37, fill=(124, 116, 104), map_fill=255)}


def jitter(flip, rotate=None):
    return AugmentParams(flip, (H, W), (0, 0), (H, W), None, rotate)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def pillow(im: np.ndarray, m: np.ndarray, p: RotateParams):
    from PIL import Image
    out = []
    for a, resample, fill in ((Image.fromarray(im), Image.BILINEAR, p.fill), (Image.fromarray(m), Image.NEAREST, p.map_fill)):
        if p.vflip:
            a = a.transpose(Image.FLIP_TOP_BOTTOM)
        if p.turns:
            a = a.transpose((Image.ROTATE_90, Image.ROTATE_180, Image.ROTATE_270)[p.turns - 1])
        if p.angle % 360.0 != 0:
            a = a.rotate(p.angle, resample=resample, expand=False, fillcolor=fill)
        out.append(np.asarray(a))
    return out


def packed(ts, p, labels):
    off, rows = 0, []
    for t in ts:
        rows.append(p.desc_row(off, t.shape[0], t.shape[1], off, labels=labels))
        off += t.numel()
    src = torch.cat([t.reshape(-1) for t in ts])
    return src, torch.empty_like(src), np.array(rows, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotate_bench.jsonl"))
    ap.add_argument("--call-only", choices=sorted(CASES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rotate_bench needs an MI355X: nothing is measured without one")
    proc = Mask2FormerImageProcessor()
    pad = {"height": H, "width": W}
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    host_m = [np.kron(rng.integers(0, 12, (H // 64, W // 64)), np.ones((64, 64))).astype(np.uint8) for _ in range(B)]
    ims, ms = [torch.from_numpy(a).cuda() for a in host], [torch.from_numpy(a).cuda() for a in host_m]
    id2sem = {i: i % 3 for i in range(12)}
    id2sem[255] = 0
    call = lambda params: proc.preprocess(ims, ms, id2sem, augment=params, pad_size=pad,  # noqa: E731
                                          ignore_index=255)["pixel_values"]
    plain = [jitter(b % 2) for b in range(B)]
    if args.call_only:
        params = [jitter(b % 2, CASES[args.call_only]) for b in range(B)]
        call(params)
        torch.cuda.synchronize()
        call(params)
        torch.cuda.synchronize()
        return
    lines = []
    for name, p in CASES.items():
        params = [jitter(b % 2, p) for b in range(B)]
        src, dst, desc = packed(ims, p, False)
        msrc, mdst, mdesc = packed(ms, p, True)
        op = lambda: ops.orient_u8(src, dst, desc)  # noqa: E731
        lab = lambda: ops.orient_labels(msrc, mdst, mdesc)  # noqa: E731
        want, mwant = pillow(host[0], host_m[0], p)
        if not (torch.equal(rotate_images(ims[0], p), torch.from_numpy(want.copy()).cuda())
                and torch.equal(rotate_maps(ms[0], p), torch.from_numpy(mwant.copy()).cuda())):
            raise SystemExit(f"{name}: the device and Pillow disagree")
        for _ in range(3):
            call(params), call(plain), op(), lab()
        torch.cuda.synchronize()
        added, t_op, t_lab = [], [], []
        for _ in range(args.rounds):
            t1 = timed(lambda: call(params))[0]
            t0 = timed(lambda: call(plain))[0]
            added.append(t1 - t0)
            t_op.append(timed(op)[0])
            t_lab.append(timed(lab)[0])
        t_pil = []
        for _ in range(5):
            t = time.perf_counter()
            pillow(host[0], host_m[0], p)
            t_pil.append((time.perf_counter() - t) * 1e3)
        nbytes = 2 * src.numel()
        add_ms, op_ms, pil_ms = statistics.median(added), statistics.median(t_op), statistics.median(t_pil)
        line = {"case": name, "B": B, "source": [H, W], "rounds": args.rounds,
                "op_ms": round(op_ms, 4), "op_spread_ms": round(max(t_op) - min(t_op), 4), "op_bytes": nbytes,
                "op_tbps": round(nbytes / (op_ms * 1e-3) / 1e12, 3),
                "roofline_share": round(nbytes / (op_ms * 1e-3) / 1e12 / HBM_TBPS, 3),
                "labels_ms": round(statistics.median(t_lab), 4), "labels_spread_ms": round(max(t_lab) - min(t_lab), 4),
                "added_ms": round(add_ms, 4), "added_spread_ms": round(max(added) - min(added), 4),
                "added_per_image_ms": round(add_ms / B, 5),
                "pillow_ms": round(pil_ms, 3), "pillow_spread_ms": round(max(t_pil) - min(t_pil), 3)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
