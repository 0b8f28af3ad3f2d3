#!/usr/bin/env python3
"""Time wm2f_conv3x3_split_fwd at every 3x3 site of the benchmark (B = 8, 1024^2) under each entry of its tile table and
under the kernel's own choice (config -1); one JSON line per site.  usage: conv3x3_configs.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from weed_instance_segmentation_amd import _lib, ops  # noqa: E402

NT = [256, 256, 256, 128, 64]
# (Cin = N, H, W, stride, epilogue), in forward order of first appearance
SITES = [(64, 256, 256, 1, "relu"), (128, 256, 256, 2, "relu"), (128, 128, 128, 1, "relu"), (256, 128, 128, 2, "relu"),
         (256, 64, 64, 1, "relu"), (512, 64, 64, 2, "relu"), (512, 32, 32, 1, "relu"), (256, 256, 256, 1, "raw")]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    B = 8
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for C, H, W, s, epi in SITES:
        x = torch.randn(B, C, H, W, device="cuda")
        w = torch.randn(C, C, 3, 3, device="cuda") / (9 * C) ** 0.5
        b = torch.randn(C, device="cuda") if epi != "raw" else None
        relu = epi == "relu"
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        ws = ops.split_weight_3x3(w)
        res = {"Cin": C, "N": C, "H": H, "W": W, "stride": s, "P": Ho * Wo, "epi": epi,
               "pick": _lib.load().wm2f_conv3x3_split_config(C, Ho * Wo, B, n_cu)}
        for ci in [-1] + list(range(len(NT))):
            if ci >= 0 and C % NT[ci]:
                continue
            for _ in range(2):
                ops.conv3x3(x, w, b, relu, s, w_split=ws, config=ci)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.conv3x3(x, w, b, relu, s, w_split=ws, config=ci)
            e1.record()
            torch.cuda.synchronize()
            res["auto" if ci < 0 else f"cfg{ci}"] = round(e0.elapsed_time(e1) * 1e3 / reps, 1)
        print(json.dumps(res), flush=True)
        del x


if __name__ == "__main__":
    main()
