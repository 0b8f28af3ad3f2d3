#!/usr/bin/env python3
"""Time wm2f_conv1x1_split_fwd at every 1x1 site of the benchmark (B = 8, 1024^2) under each entry of its tile table and
under the kernel's own choice (config -1); one JSON line per site.  usage: conv1x1_configs.py [reps] [--dual [rounds]]
--dual: the four conv3 + projection-shortcut sites on wm2f_conv1x1_split_dual_fwd_p (ops.conv1x1_dual) instead, each entry
timed `rounds` times (default 5) in interleaved rounds: a list of µs per entry, whose spread is the bar a pick has to clear."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from weed_instance_segmentation_amd import _lib, ops  # noqa: E402

NT = [256, 256, 256, 128, 64]
# (K, N, H, W, stride, epilogue), in forward order of first appearance
SITES = [(64, 64, 256, 256, 1, "relu"), (64, 256, 256, 256, 1, "raw"), (64, 256, 256, 256, 1, "res"), (256, 64, 256, 256, 1, "relu"),
         (256, 128, 256, 256, 1, "relu"), (256, 512, 256, 256, 2, "raw"), (128, 512, 128, 128, 1, "res"), (512, 128, 128, 128, 1, "relu"),
         (512, 256, 128, 128, 1, "relu"), (512, 1024, 128, 128, 2, "raw"), (256, 1024, 64, 64, 1, "res"), (1024, 256, 64, 64, 1, "relu"),
         (1024, 512, 64, 64, 1, "relu"), (1024, 2048, 64, 64, 2, "raw"), (512, 2048, 32, 32, 1, "res"), (2048, 512, 32, 32, 1, "relu"),
         (2048, 256, 32, 32, 1, "raw"), (1024, 256, 64, 64, 1, "raw"), (512, 256, 128, 128, 1, "raw"), (256, 256, 256, 256, 1, "raw"),
         (256, 256, 256, 256, 1, "bias")]
# (K1, K2, N, Ho, Wo, stride2): conv3 + projection shortcut of the first block of each ResNet-50 stage
DUAL_SITES = [(64, 64, 256, 256, 256, 1), (128, 256, 512, 128, 128, 2), (256, 512, 1024, 64, 64, 2), (512, 1024, 2048, 32, 32, 2)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 1)


def dual(reps, rounds):
    B = 8
    for K1, K2, N, Ho, Wo, s in DUAL_SITES:
        x1 = torch.randn(B, K1, Ho, Wo, device="cuda")
        x2 = torch.randn(B, K2, s * Ho, s * Wo, device="cuda")
        w1, w2 = torch.randn(N, K1, device="cuda") / K1 ** 0.5, torch.randn(N, K2, device="cuda") / K2 ** 0.5
        b = torch.randn(N, device="cuda")
        ws1, ws2 = ops.split_weight(w1), ops.split_weight(w2)
        cfgs = [-1] + [ci for ci in range(len(NT)) if N % NT[ci] == 0]
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        res = {"K1": K1, "K2": K2, "N": N, "P": Ho * Wo, "stride2": s,
               "rule_picks": int(_lib.load().wm2f_conv1x1_split_config(N, Ho * Wo, B, n_cu))}
        for ci in cfgs:
            res["auto" if ci < 0 else f"cfg{ci}"] = []
        for _ in range(rounds):  # interleaved: a drift of the clock lands on every entry alike
            for ci in cfgs:
                run = lambda: ops.conv1x1_dual(x1, w1, x2, w2, b, s, w1_split=ws1, w2_split=ws2, config=ci)
                run(), run()
                res["auto" if ci < 0 else f"cfg{ci}"].append(timed(run, reps))
        print(json.dumps(res), flush=True)
        del x1, x2


def main():
    args = [a for a in sys.argv[1:] if a != "--dual"]
    reps = int(args[0]) if args else 10
    if "--dual" in sys.argv:
        return dual(reps, int(args[1]) if len(args) > 1 else 5)
    B = 8
    for K, N, H, W, s, epi in SITES:
        x = torch.randn(B, K, H, W, device="cuda")
        w = torch.randn(N, K, device="cuda") / K ** 0.5
        b = torch.randn(N, device="cuda") if epi != "raw" else None
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        r = torch.randn(B, N, Ho, Wo, device="cuda") if epi == "res" else None
        relu = epi in ("relu", "res")
        ws = ops.split_weight(w)
        res = {"K": K, "N": N, "P": Ho * Wo, "stride": s, "epi": epi}
        for ci in [-1] + list(range(len(NT))):
            if ci >= 0 and N % NT[ci]:
                continue
            run = lambda: ops.conv1x1(x, w, b, r, relu, s, w_split=ws, config=ci)
            run(), run()
            res["auto" if ci < 0 else f"cfg{ci}"] = timed(run, reps)
        print(json.dumps(res), flush=True)
        del x, r


if __name__ == "__main__":
    main()
