#!/usr/bin/env python3
"""Time wm2f_conv3x3_split_fwd at every 3x3 site of the benchmark (B = 8, 1024^2) under each entry of its tile table and
under the kernel's own choice (config -1); one JSON line per site.  usage: conv3x3_configs.py [reps]

conv3x3_configs.py --ablation [reps]: the profiling library's timing ablations of the kernel (WM2F_C3_ABL, OUTPUTS NOT
VALID; include/wm2f_prof.h) against the shipped kernel under the kernel's own choice, five interleaved rounds in one
process; one JSON line per site with the median, the spread (max - min) and the rounds of each variant, and
`ceiling_us` = shipped - ablation medians: what a kernel that splits (and loads) each x element once per channel block
instead of once per tap could save at most.  `launches` is the site's count in one forward.

conv3x3_configs.py --staged [reps]: the direct kernel (route 0) against the staged kernel (route 1) at the stride-1 sites
under every WN = 1 entry that divides N, five interleaved rounds in one process; per entry the median, the spread and the
rounds of both routes, `gain_us` = direct - staged medians and whether the two outputs are bit-equal; `rule_entry` and
`rule_route` are what wm2f_conv3x3_split_route picks."""
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
LAUNCHES = [3, 1, 3, 1, 5, 1, 2, 1]  # of each site in one forward of the benchmark's model
ABLATIONS = [("shipped", None), ("split_once_INVALID", "1"), ("split_and_load_once_INVALID", "2")]
ROUNDS = 5


def site_tensors(C, H, W, epi, B):
    x = torch.randn(B, C, H, W, device="cuda")
    w = torch.randn(C, C, 3, 3, device="cuda") / (9 * C) ** 0.5
    b = torch.randn(C, device="cuda") if epi != "raw" else None
    return x, w, b, ops.split_weight_3x3(w)


def time_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def ablation(reps):
    _lib.use_profiling_library()
    B = 8
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for (C, H, W, s, epi), launches in zip(SITES, LAUNCHES):
        x, w, b, ws = site_tensors(C, H, W, epi, B)
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        fn = lambda: ops.conv3x3(x, w, b, epi == "relu", s, w_split=ws)  # noqa: E731
        res = {"Cin": C, "N": C, "H": H, "W": W, "stride": s, "P": Ho * Wo, "epi": epi, "launches": launches,
               "pick": _lib.load().wm2f_conv3x3_split_config(C, Ho * Wo, B, n_cu)}
        rounds = {v: [] for v, _ in ABLATIONS}
        try:
            for r in range(ROUNDS + 1):  # round 0 warms up
                for v, env in ABLATIONS:
                    os.environ.pop("WM2F_C3_ABL", None)
                    if env:
                        os.environ["WM2F_C3_ABL"] = env
                    t = time_us(fn, reps)
                    if r:
                        rounds[v].append(t)
        finally:
            os.environ.pop("WM2F_C3_ABL", None)
        for v, _ in ABLATIONS:
            ts = sorted(rounds[v])
            res[v] = dict(med_us=round(ts[len(ts) // 2], 1), spread_us=round(ts[-1] - ts[0], 1),
                          rounds_us=[round(t, 1) for t in rounds[v]])
        for v, _ in ABLATIONS[1:]:
            res[v]["ceiling_us"] = round(res["shipped"]["med_us"] - res[v]["med_us"], 1)
        print(json.dumps(res), flush=True)
        del x


def staged(reps):
    """Direct against staged at the stride-1 sites, under every WN = 1 entry that divides N: five interleaved rounds."""
    import ctypes
    B = 8
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    entry = ctypes.c_int(-1)
    for (C, H, W, s, epi), launches in zip(SITES, LAUNCHES):
        if s != 1:
            continue
        x, w, b, ws = site_tensors(C, H, W, epi, B)
        rule = _lib.load().wm2f_conv3x3_split_route(C, H, W, s, B, n_cu, 3, ctypes.byref(entry))
        res = {"Cin": C, "N": C, "H": H, "W": W, "stride": s, "epi": epi, "launches": launches, "rule_entry": entry.value,
               "rule_route": rule}
        for ci in (0, 3, 4):  # (16, 1), (8, 1), (4, 1)
            if C % NT[ci]:
                continue
            fns = {r: (lambda r=r: ops.conv3x3_route(x, w, r, b, epi == "relu", s, w_split=ws, config=ci)) for r in (0, 1)}
            try:
                same = torch.equal(fns[0](), fns[1]())
            except _lib.Wm2fError as e:  # the staged kernel does not fit this entry on this device
                res[f"cfg{ci}"] = {"refused": str(e)[:120]}
                continue
            rounds = {0: [], 1: []}
            for k in range(ROUNDS + 1):  # round 0 warms up
                for r in (0, 1):
                    t = time_us(fns[r], reps)
                    if k:
                        rounds[r].append(t)
            out = {"bit_equal": same}
            for r, name in ((0, "direct"), (1, "staged")):
                ts = sorted(rounds[r])
                out[name] = dict(med_us=round(ts[len(ts) // 2], 1), spread_us=round(ts[-1] - ts[0], 1),
                                 rounds_us=[round(t, 1) for t in rounds[r]])
            out["gain_us"] = round(out["direct"]["med_us"] - out["staged"]["med_us"], 1)
            res[f"cfg{ci}"] = out
        print(json.dumps(res), flush=True)
        del x


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 10
    if "--ablation" in sys.argv[1:]:
        return ablation(reps)
    if "--staged" in sys.argv[1:]:
        return staged(reps)
    B = 8
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for C, H, W, s, epi in SITES:
        x, w, b, ws = site_tensors(C, H, W, epi, B)
        relu = epi == "relu"
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        res = {"Cin": C, "N": C, "H": H, "W": W, "stride": s, "P": Ho * Wo, "epi": epi,
               "pick": _lib.load().wm2f_conv3x3_split_config(C, Ho * Wo, B, n_cu)}
        for ci in [-1] + list(range(len(NT))):
            if ci >= 0 and C % NT[ci]:
                continue
            fn = lambda: ops.conv3x3(x, w, b, relu, s, w_split=ws, config=ci)  # noqa: E731
            time_us(fn, 2)
            res["auto" if ci < 0 else f"cfg{ci}"] = round(time_us(fn, reps), 1)
        print(json.dumps(res), flush=True)
        del x


if __name__ == "__main__":
    main()
