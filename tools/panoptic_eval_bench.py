"""Panoptic quality and semantic mIoU on the GPU: the two kernels, the whole metric calls, and a
torch restatement on the same GPU.

    python tools/panoptic_eval_bench.py [--rounds 7] [--out profiles/panoptic_eval_bench.jsonl]

Workload: B = 8 maps of 1024 x 1024 from `post_process_panoptic_segmentation` / `post_process_semantic_segmentation` on the
tiled-blob logits of the post-processing tests (Q = 100, 3 classes, 256 x 256 logits).  The GT is the panoptic map moved
8 pixels to the right with its segments renamed to raw ids.  In one process, alternating per round, HIP events:
- `match_kernel`: `ops.panoptic_match` on the merged histograms; `confusion_kernel`: `ops.semantic_confusion_` on the
  (8, 1024, 1024) int64 stack against the raw-id GT (`--inner` launches per timing);
- `pq_call` / `miou_call`: whole `update_from_maps` calls, wall clock to the end of the device work, with the time inside
  wm2f kernels (pair counts, matching, confusion) taken by `ops.KernelTimer` in separate calls; the rest of a call is
  host work, copies and torch glue;
- `torch_pairs`: the colour pairs of PQ per image as `torch.unique(pred * K + gt, return_counts=True)`;
  `torch_bincount`: the confusion matrix as `bincount(gt_class * C + pred)` after a table lookup of the raw ids.
One JSON line: medians and spreads (min, max) over rounds, and that the restatements gave the same counts.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from weed_instance_segmentation_amd import ops  # noqa: E402
from weed_instance_segmentation_amd.metrics import MeanIoU, PanopticQuality  # noqa: E402
from weed_instance_segmentation_amd.postprocess import Mask2FormerInstancePostProcessor  # noqa: E402


def tiled_blob_logits(B, Q, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    owner = torch.randint(0, Q, (B, 1, 16, 16), generator=g)
    low = torch.where(owner == torch.arange(Q).view(1, Q, 1, 1), 6.0, -6.0) + torch.randn(B, Q, 16, 16, generator=g)
    m = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)
    m += 0.2 * torch.randn(B, Q, h, w, generator=g)
    cls = torch.randn(B, Q, C + 1, generator=g)
    strong = torch.rand(B, Q, generator=g) < 0.2
    lab = torch.randint(0, C, (B, Q), generator=g)
    cls.scatter_(2, lab.unsqueeze(-1), torch.where(strong, 6.0 + torch.rand(B, Q, generator=g), torch.zeros(B, Q)).unsqueeze(-1))
    cls[..., C] += torch.where(strong, torch.zeros(B, Q), torch.full((B, Q), 4.0))
    return cls.cuda(), m.cuda()


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def kernels_ms(fn):
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    return sum(n * us for n, us in timer.summary().values()) / 1e3


def spread(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panoptic_eval_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("panoptic_eval_bench needs an MI355X")
    B, H, W, C = 8, 1024, 1024, 3
    things, stuffs = {0, 1}, {2}
    cls, m = tiled_blob_logits(B, 100, C, 256, 256, seed=0)
    out = SimpleNamespace(class_queries_logits=cls, masks_queries_logits=m)
    proc = Mask2FormerInstancePostProcessor()
    pan = proc.post_process_panoptic_segmentation(out, label_ids_to_fuse=set(), target_sizes=[(H, W)] * B)
    sem = proc.post_process_semantic_segmentation(out, target_sizes=[(H, W)] * B)
    segs, infos = [r["segmentation"] for r in pan], [r["segments_info"] for r in pan]
    gts, mappings = [], []
    for r in pan:  # GT maps on the host, as a data loader hands them over
        seg = r["segmentation"].to(torch.int32)
        gt = torch.full_like(seg, 255)
        gt[:, 8:] = torch.where(seg[:, :-8] > 0, seg[:, :-8] * 3 + 250, 255)
        gts.append(gt.cpu().numpy())
        mappings.append({s["id"] * 3 + 250: s["label_id"] for s in r["segments_info"]})

    def pq_call():
        metric = PanopticQuality(things, stuffs, void_as_background=True)
        metric.update_from_maps(segs, infos, gts, mappings)
        return metric

    def miou_call():
        metric = MeanIoU(C, background_label=2)
        metric.update_from_maps(sem, gts, mappings)
        return metric

    # the kernels' own inputs
    metric = pq_call()
    rec0 = metric._records[0]
    P, G = rec0[4].shape[1], rec0[2].shape[1]
    gt_dev = torch.stack([torch.from_numpy(g) for g in gts]).cuda()
    seg_dev = torch.stack([s.to(torch.int32) for s in segs])
    G_raw = max(len(mp) for mp in mappings)
    ids = torch.zeros(B, G_raw, dtype=torch.int32)
    gcls = torch.zeros(B, G_raw, dtype=torch.int32)
    for i, mp in enumerate(mappings):
        ks = sorted(mp)
        ids[i, :len(ks)] = torch.tensor(ks, dtype=torch.int32)
        gcls[i, :len(ks)] = torch.tensor([mp[k] for k in ks], dtype=torch.int32)
    ids, gcls = ids.cuda(), gcls.cuda()
    n_ids = torch.tensor([len(mp) for mp in mappings], dtype=torch.int32).cuda()
    P_raw = max(max((s["id"] for s in info), default=0) for info in infos) + 1
    hist = ops.labelmap_pair_counts(seg_dev, gt_dev, ids, n_ids, P_raw)
    plab = torch.full((B, P_raw), -2 ** 31, dtype=torch.int32)
    for i, info in enumerate(infos):
        for s in info:
            plab[i, s["id"]] = s["label_id"]
    plab = plab.cuda()
    n_pred = torch.full((B,), P_raw, dtype=torch.int32).cuda()
    sem_dev = torch.stack(sem)
    conf = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    n_out = torch.zeros(1, dtype=torch.int64, device="cuda")
    match_kernel = lambda: ops.panoptic_match(hist, plab, gcls, n_pred, n_ids, True)
    confusion_kernel = lambda: ops.semantic_confusion_(conf, n_out, sem_dev, gt_dev, gt_ids=ids, gt_cls=gcls, n_ids=n_ids,
                                                       background_label=2)

    # the torch restatement
    K = 4096

    def torch_pairs():
        res = []
        for i in range(B):
            keys, counts = torch.unique(seg_dev[i].to(torch.int64).view(-1) * K + gt_dev[i].to(torch.int64).view(-1),
                                        return_counts=True)
            res.append((keys, counts))
        return res

    lut = torch.full((B, K), 2, dtype=torch.int64)
    for i, mp in enumerate(mappings):
        for k, v in mp.items():
            lut[i, k] = v
    lut = lut.cuda()

    def torch_bincount():
        total = torch.zeros(C * C, dtype=torch.int64, device="cuda")
        for i in range(B):
            g = lut[i][gt_dev[i].to(torch.int64).view(-1)]
            total += torch.bincount(g * C + sem_dev[i].view(-1), minlength=C * C)
        return total.view(C, C)

    # both restatements count what the kernels count
    pairs_equal = True
    for i, (keys, counts) in enumerate(torch_pairs()):
        h = hist[i].cpu()
        col = {int(v): j + 1 for j, v in enumerate(ids[i, :int(n_ids[i])].tolist())}
        for key, n in zip(keys.tolist(), counts.tolist()):
            pairs_equal &= int(h[key // K + 1, col.get(key % K, 0)]) == n  # every map value is in [0, P_raw)
    conf_equal = bool(torch.equal(miou_call().confusion_matrix(), torch_bincount().cpu()))

    for fn in (match_kernel, confusion_kernel, pq_call, miou_call, torch_pairs, torch_bincount):
        fn()
    t = {k: [] for k in ("match_kernel_us", "confusion_kernel_us", "pq_call_ms", "pq_call_wm2f_kernels_ms", "miou_call_ms",
                         "miou_call_wm2f_kernels_ms", "torch_pairs_ms", "torch_bincount_ms")}
    for _ in range(args.rounds):  # alternate, so that clocks and neighbours treat all alike
        t["match_kernel_us"].append(event_ms(match_kernel, args.inner) * 1e3)
        t["confusion_kernel_us"].append(event_ms(confusion_kernel, args.inner) * 1e3)
        t["pq_call_ms"].append(wall_ms(pq_call))
        t["pq_call_wm2f_kernels_ms"].append(kernels_ms(pq_call))
        t["miou_call_ms"].append(wall_ms(miou_call))
        t["miou_call_wm2f_kernels_ms"].append(kernels_ms(miou_call))
        t["torch_pairs_ms"].append(event_ms(torch_pairs, 1))
        t["torch_bincount_ms"].append(event_ms(torch_bincount, 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    conf_bytes = sem_dev.numel() * 8 + gt_dev.numel() * 4
    rec = {"B": B, "H": H, "W": W, "classes": C, "merged_pred_rows": P, "merged_gt_columns": G, "raw_pred_rows": P_raw,
           "raw_gt_ids": G_raw, "rounds": args.rounds, "inner": args.inner, **{k: spread(v) for k, v in t.items()},
           "confusion_kernel_TBps": round(conf_bytes / (med["confusion_kernel_us"] * 1e-6) / 1e12, 3),
           "pq_call_share_outside_wm2f_kernels": round(1 - med["pq_call_wm2f_kernels_ms"] / med["pq_call_ms"], 3),
           "miou_call_share_outside_wm2f_kernels": round(1 - med["miou_call_wm2f_kernels_ms"] / med["miou_call_ms"], 3),
           "torch_pairs_equal": bool(pairs_equal), "torch_bincount_equal": conf_equal}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
