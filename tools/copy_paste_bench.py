"""Copy-paste timing: the three launches of `ops.copy_paste` and, in the same run and alternating with
them, a composition of stock torch ops that computes the same four results.  One process, HIP events; one JSON line per
case, appended to profiles/copy_paste_bench.jsonl.

    python tools/copy_paste_bench.py [--rounds 15] [--out profiles/copy_paste_bench.jsonl]

Setup: B = 16 images of 1024 x 1024, C = 3, id maps of 64 x 64 blocks of which 39 of 256 are instances (15.2 % of the
pixels), every image pasting all instances of its neighbour, min_visible = 1/4 so that all three steps run.  Cases:
`aligned` (shift (32, 36): the source side is read 16 bytes wide) and `unaligned` (shift (32, 37): pixel by pixel where
pasted).  The shifts clip a little of the pasted blocks at the frame's edge: `pasted_share` is what was pasted.

`select_ms`, `paste_ms`, `prune_ms`: each entry point alone, bracketed by events through the ops' kernel timer (median
over rounds; the select bracket holds its clearing and its two kernels).  `paste_bytes` are the algorithmic bytes of the
paste from the shapes: per pixel one map read, one source-map read, one map write, one read and one write of C floats
(where a pixel is pasted the read is the source's instead of the destination's) = 12 + 8 C bytes; `paste_tbps` their
rate, `paste_roofline_share` the rate over 8 TB/s.  `select_bytes` and `prune_bytes` are one map read each.  `op_ms` is
the whole `ops.copy_paste` call between two events -- allocations, the LUT's upload and all launches -- and `torch_ms` the
stock composition between two events; inside every round the two alternate.  `*_spread_ms` is max - min over rounds.
Before anything is timed the two are compared with torch.equal; the tool stops if they differ."""
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

from weed_instance_segmentation_amd import ops  # noqa: E402

HBM_TBPS = 8.0
B, C = 16, 3
H = W = 1024
IG = 255
NUM, DEN = 1, 4
CASES = {"aligned": (32, 36), "unaligned": (32, 37)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def hist(ids, weight):
    """(B, 256) int64 counts of the ids 0 .. 254 where `weight`; other values are not counted."""
    ok = (ids >= 0) & (ids <= 254) & weight
    rows = torch.arange(B, device=ids.device).view(B, 1, 1) * 256
    out = torch.bincount((torch.where(ok, ids, torch.full_like(ids, 255)) + rows).view(-1), minlength=B * 256).view(B, 256)
    out[:, 255] = 0
    return out


def stock(pix, maps, source, lut, shift, ignore_index=IG):
    """The same four results from stock torch ops, batched over the images (the four histograms are torch.bincount, which
    sizes its output on the host).  Every image has a source here."""
    dev = pix.device
    src = torch.as_tensor(source, device=dev)
    smaps, spix = maps[src], pix[src]
    at = torch.full_like(maps, -1)
    moved = torch.zeros_like(pix)
    for b, (dy, dx) in enumerate(shift):
        ys0, ys1, xs0, xs1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        at[b, ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx] = smaps[b, ys0:ys1, xs0:xs1]
        moved[b, :, ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx] = spix[b, :, ys0:ys1, xs0:xs1]
    lut64 = lut.long()
    sel = lambda ids, table: table.gather(1, ids.clamp(0, 255).view(B, -1).long()).view(ids.shape)  # noqa: E731
    selected = (lut64 >= 0) & (lut64 <= 254)
    original = hist(smaps, sel(smaps, selected.long()) > 0)
    landed = hist(at, sel(at, selected.long()) > 0)
    live = selected & (landed > 0) & (landed * DEN >= NUM * original)
    live[:, 255] = False
    lut_final = torch.where(live, lut64, torch.full_like(lut64, -1))
    take = (at >= 0) & (at <= 254) & (sel(at, lut_final) >= 0)
    new = torch.where(take, sel(at, lut_final).int(), maps)
    out = torch.where(take[:, None], moved, pix)
    everywhere = torch.ones_like(take)
    before, after = hist(maps, everywhere), hist(new, everywhere)
    kill = (after > 0) & (after * DEN < NUM * before)
    new = torch.where((new >= 0) & (new <= 254) & (sel(new, kill.long()) > 0), torch.full_like(new, ignore_index), new)
    areas = torch.stack([before, after, original * selected], 1).int()
    return out, new, lut_final.int(), areas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_paste_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("copy_paste_bench needs an MI355X: nothing is measured without one")
    rng = np.random.default_rng(0)
    blocks = np.full((B, 256), IG, dtype=np.int32)
    for b in range(B):
        blocks[b, rng.choice(256, 39, replace=False)] = np.arange(1, 40)
    maps = torch.from_numpy(np.kron(blocks.reshape(B, 16, 16), np.ones((64, 64), dtype=np.int32)).astype(np.int32)).cuda()
    pix = torch.randn(B, C, H, W, device="cuda")
    source = [(b + 1) % B for b in range(B)]
    lut_host = np.full((B, 256), -1, dtype=np.int32)
    lut_host[:, 1:40] = [0] + list(range(40, 78))  # the free ids of a destination that uses 1 .. 39
    lut = torch.from_numpy(lut_host).cuda()
    px = B * H * W
    paste_bytes = px * (12 + 8 * C)
    lines = []
    for name, sh in CASES.items():
        shift = [sh] * B
        op = lambda: ops.copy_paste(pix, maps, source, lut, shift, None, (NUM, DEN), IG)  # noqa: E731
        ref = lambda: stock(pix, maps, source, lut, shift)  # noqa: E731
        got, want = op(), ref()
        for g, w, what in zip(got, want, ("pixels", "maps", "lut_final", "areas")):
            if not torch.equal(g.view(torch.int32), w.view(torch.int32)):
                raise SystemExit(f"{name}: {what}: the kernels and the stock composition disagree")
        pasted_share = float(((got[1] == 0) | ((got[1] >= 40) & (got[1] <= 77))).sum().item()) / px  # the new ids
        del got, want
        for _ in range(3):
            op(), ref()
        torch.cuda.synchronize()
        t_op, t_ref = [], []
        for _ in range(args.rounds):
            t_op.append(timed(op)[0])
            t_ref.append(timed(ref)[0])
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        for _ in range(args.rounds):
            op()
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        steps = {k: [a.elapsed_time(b) for a, b in v] for k, v in timer.records.items()}
        sel_ms, paste_ms, prune_ms = (statistics.median(steps[k]) for k in ("copy_paste_select", "copy_paste", "copy_paste_prune"))
        op_ms, ref_ms = statistics.median(t_op), statistics.median(t_ref)
        line = {"case": name, "B": B, "C": C, "frame": [H, W], "shift": list(sh), "min_visible": [NUM, DEN],
                "rounds": args.rounds, "pasted_share": round(pasted_share, 4),
                "select_ms": round(sel_ms, 4), "select_spread_ms": round(max(steps["copy_paste_select"]) - min(steps["copy_paste_select"]), 4),
                "select_bytes": px * 4,
                "paste_ms": round(paste_ms, 4), "paste_spread_ms": round(max(steps["copy_paste"]) - min(steps["copy_paste"]), 4),
                "paste_bytes": paste_bytes, "paste_tbps": round(paste_bytes / (paste_ms * 1e-3) / 1e12, 3),
                "paste_roofline_share": round(paste_bytes / (paste_ms * 1e-3) / 1e12 / HBM_TBPS, 3),
                "prune_ms": round(prune_ms, 4), "prune_spread_ms": round(max(steps["copy_paste_prune"]) - min(steps["copy_paste_prune"]), 4),
                "prune_bytes": px * 4,
                "op_ms": round(op_ms, 4), "op_spread_ms": round(max(t_op) - min(t_op), 4),
                "torch_ms": round(ref_ms, 4), "torch_spread_ms": round(max(t_ref) - min(t_ref), 4),
                "torch_over_op": round(ref_ms / op_ms, 2)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
