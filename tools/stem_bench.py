#!/usr/bin/env python3
"""Time the ResNet stem, ops.stem_conv_pool (wm2f_stem7x7_pool_fwd) against its split=False route (the library's 7x7
convolution + bias_relu_maxpool), alternating in one process, at the benchmark's B = 8 1024^2 and at B = 2 800 x 1088; one
JSON line per shape: us per launch of both (HIP events), the kernel's MFMA FLOP/s (6 x 2 x 64 x 160 per conv pixel) against
2.5 PFLOP/s, its HBM bytes/s (x read once, out written once) against 8 TB/s, and the bound that applies.
usage: stem_bench.py [reps] [rounds]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from weed_instance_segmentation_amd import ops  # noqa: E402

SHAPES = [(8, 3, 1024, 1024), (2, 3, 800, 1088)]
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for B, C, H, W in SHAPES:
        x = torch.randn(B, C, H, W, device="cuda")
        w = torch.randn(64, C, 7, 7, device="cuda") / (49 * C) ** 0.5
        b = torch.randn(64, device="cuda") * 0.1
        ws = ops.split_weight_stem(w)
        routes = {"split": lambda: ops.stem_conv_pool(x, w, b, w_split=ws),
                  "library": lambda: ops.stem_conv_pool(x, w, b, split=False)}
        for fn in routes.values():
            for _ in range(3):
                fn()
        us = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                us[k].append(round(timed(fn, reps), 1))
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
        flop = 6 * 2 * 64 * 160 * B * Hc * Wc
        nbytes = 4 * (B * C * H * W + B * 64 * Hp * Wp)
        t = min(us["split"]) * 1e-6
        floor_mfma, floor_hbm = flop / PEAK_FLOPS, nbytes / PEAK_BYTES
        print(json.dumps({"B": B, "Cin": C, "H": H, "W": W, "split_us": us["split"], "library_us": us["library"],
                          "mfma_flop": flop, "mfma_flops_achieved": round(flop / t / 1e12, 1),
                          "mfma_share_of_2.5PF": round(floor_mfma / t, 3), "hbm_bytes": nbytes,
                          "hbm_TBps_achieved": round(nbytes / t / 1e12, 3), "hbm_share_of_8TBps": round(floor_hbm / t, 3),
                          "bound": "mfma" if floor_mfma > floor_hbm else "hbm"}), flush=True)
        del x


if __name__ == "__main__":
    main()
