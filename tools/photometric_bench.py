"""Colour-jitter timing: what `AugmentParams.photometric` adds to a processor call, the op alone, and
for scale the same chain in Pillow on the host.  One process, HIP events; one JSON line per case, appended to
profiles/photometric_bench.jsonl.

    python tools/photometric_bench.py [--rounds 15] [--out profiles/photometric_bench.jsonl]
    python tools/photometric_bench.py --op-only four --source 1024x1024 --iters 20     # for a kernel trace

Cases: B = 16 device-resident sources of 1024 x 1024 and of 966 x 1296 under the jitter recipe of section 20 (f = 1, crop
1024 x 1024), with chains of one step (brightness), three steps without hue (brightness, contrast, saturation) and all
four (brightness, hue, contrast, saturation).  Inside every round the call with the chain and the same call without it
alternate; `added_ms` is the median over rounds of the paired difference, `added_spread_ms` its max - min.
`adjust_ms` is `adjust_colors` alone (it packs the images into a fresh buffer first), `op_ms` is `ops.photometric_u8`
alone on a packed buffer: the clearing of the sums and both launches.  `op_bytes` are the algorithmic bytes of that call
(one read per launch, one write: 2 N without a contrast step, 3 N with one), `op_tbps` their rate and `roofline_share` the
rate over 8 TB/s.  `pillow_ms` is the median of the same chain in Pillow on one core for ONE image, `pillow_spread_ms`
its max - min.  `holds` is the condition of the section: the added device time per image is below Pillow's time for that
image by more than either spread.  --op-only runs one chain's op call `--iters` times and prints nothing else: run it
under a kernel trace to split the call into its launches."""
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

from weed_instance_segmentation_amd import (AugmentParams, Mask2FormerImageProcessor, PhotometricParams,  # noqa: E402
                                            adjust_colors, ops)

HBM_TBPS = 8.0
B = 16
CHAINS = {"one": (("brightness", 1.2),),
          "three": (("brightness", 1.2), ("contrast", 0.8), ("saturation", 1.1)),
          "four": (("brightness", 1.2), ("hue", -0.03), ("contrast", 0.8), ("saturation", 1.1))}
SOURCES = [(1024, 1024), (966, 1296)]


def jitter(H, W, f, crop, flip, photometric=None):
    r = min(crop[0] * f / H, crop[1] * f / W)
    h, w = max(1, round(H * r)), max(1, round(W * r))
    ch, cw = min(crop[0], h), min(crop[1], w)
    return AugmentParams(flip, (h, w), ((h - ch) // 2, (w - cw) // 3), (ch, cw), photometric)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def pillow_chain(im: np.ndarray, chain):
    from PIL import Image, ImageEnhance
    a = Image.fromarray(im)
    for kind, value in chain:
        if kind == "hue":
            h, s, v = a.convert("HSV").split()
            dh = int(value * 255) % 256
            a = Image.merge("HSV", (h.point(lambda x: (x + dh) % 256), s, v)).convert("RGB")
        else:
            enh = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast,
                   "saturation": ImageEnhance.Color}[kind]
            a = enh(a).enhance(value)
    return np.asarray(a)


def packed(ims, p):
    """The images one behind the other and the op's descriptor."""
    off, rows = 0, []
    for im in ims:
        rows.append(p.desc_row(off, im.shape[0], im.shape[1]))
        off += im.numel()
    return torch.cat([im.reshape(-1) for im in ims]), np.array(rows, np.int64)


def op_only(chain_name, source, iters):
    H, W = source
    rng = np.random.default_rng(0)
    ims = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(B)]
    buf, desc = packed(ims, PhotometricParams(CHAINS[chain_name]))
    for _ in range(iters):
        ops.photometric_u8(buf, desc)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_bench.jsonl"))
    ap.add_argument("--op-only", choices=sorted(CHAINS))
    ap.add_argument("--source", default="1024x1024")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_bench needs an MI355X: nothing is measured without one")
    if args.op_only:
        return op_only(args.op_only, tuple(int(v) for v in args.source.split("x")), args.iters)
    proc = Mask2FormerImageProcessor()
    crop, pad = (1024, 1024), {"height": 1024, "width": 1024}
    rng = np.random.default_rng(0)
    lines = []
    for H, W in SOURCES:
        host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
        ims = [torch.from_numpy(a).cuda() for a in host]
        plain = [jitter(H, W, 1.0, crop, b % 2) for b in range(B)]
        without = lambda: proc.preprocess(ims, augment=plain, pad_size=pad)["pixel_values"]  # noqa: E731
        for name, chain in CHAINS.items():
            p = PhotometricParams(chain)
            params = [jitter(H, W, 1.0, crop, b % 2, p) for b in range(B)]
            with_chain = lambda: proc.preprocess(ims, augment=params, pad_size=pad)["pixel_values"]  # noqa: E731
            alone = lambda: adjust_colors(ims, p)  # noqa: E731
            buf, desc = packed(ims, p)
            op = lambda: ops.photometric_u8(buf, desc)  # noqa: E731  (in place, again and again: the time is the same)
            if not torch.equal(alone()[0], torch.from_numpy(pillow_chain(host[0], chain)).cuda()):
                raise SystemExit(f"{name} at {(H, W)}: the device and Pillow disagree")
            for _ in range(3):
                with_chain(), without(), alone(), op()
            torch.cuda.synchronize()
            added, t_alone, t_op = [], [], []
            for _ in range(args.rounds):
                t1 = timed(with_chain)[0]
                t0 = timed(without)[0]
                added.append(t1 - t0)
                t_alone.append(timed(alone)[0])
                t_op.append(timed(op)[0])
            t_pil = []
            for _ in range(5):
                t = time.perf_counter()
                pillow_chain(host[0], chain)
                t_pil.append((time.perf_counter() - t) * 1e3)
            n = sum(im.numel() for im in ims)
            nbytes = n * (3 if any(k == "contrast" for k, _ in chain) else 2)
            add_ms, op_ms, pil_ms = statistics.median(added), statistics.median(t_op), statistics.median(t_pil)
            s_add, s_pil = max(added) - min(added), max(t_pil) - min(t_pil)
            line = {"case": name, "chain": [k for k, _ in chain], "B": B, "source": [H, W], "rounds": args.rounds,
                    "added_ms": round(add_ms, 4), "added_spread_ms": round(s_add, 4),
                    "added_per_image_ms": round(add_ms / B, 5),
                    "adjust_ms": round(statistics.median(t_alone), 4),
                    "adjust_spread_ms": round(max(t_alone) - min(t_alone), 4),
                    "op_ms": round(op_ms, 4), "op_spread_ms": round(max(t_op) - min(t_op), 4), "op_bytes": nbytes,
                    "op_tbps": round(nbytes / (op_ms * 1e-3) / 1e12, 3),
                    "roofline_share": round(nbytes / (op_ms * 1e-3) / 1e12 / HBM_TBPS, 3),
                    "pillow_ms": round(pil_ms, 3), "pillow_spread_ms": round(s_pil, 3),
                    "holds": bool(pil_ms - add_ms / B > max(s_add / B, s_pil))}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
