#!/usr/bin/env python3
"""Times pose_resnet (experiments/bench/res50_256.yaml: ResNet-50, 256 x 256, three k4 deconvs of 256, 11 joints) on the engine in
bf16 at batch 64 and 256, and, in the same run on the same device, the restatement of the module (tests/pose_resnet_restated.py,
BatchNorm folded once) under torch in the same dtype -- what a user would otherwise run.

    python tools_dev/time_pose_resnet.py [--batches 64 256] [--repeats 10] [--out profiles/pose_resnet_timing.json]

Per batch: ms per forward (median of --repeats, HIP events around each), the per-op-class split of one profiled forward (launches,
ms, executed FLOP/s and bytes/s from the engine's own work figures), executed FLOP/s of the whole forward against the MFMA ceilings
recorded in profiles/round6_final_bench.json, and for every launch of the three new kernels (stem, transposed conv, 1x1 stride 2) the
same layer under torch.  Engine input: uint8 NHWC (normalisation is in its stem); torch input: the normalised tensor in bf16."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_ms(fn, warmup, repeats, torch):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "repeats": repeats}


def find_keys(node, keys, out=None):
    """first value of each of `keys` anywhere in a loaded JSON tree"""
    out = {} if out is None else out
    if isinstance(node, dict):
        for k, v in node.items():
            if k in keys and k not in out and isinstance(v, (int, float)):
                out[k] = float(v)
            find_keys(v, keys, out)
    elif isinstance(node, list):
        for v in node:
            find_keys(v, keys, out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_resnet_timing.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import scpose  # noqa: F401
    from importlib import import_module
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    syn = import_module("spacecraft-pose-estimation_amd.synthetic")
    config = import_module("spacecraft-pose-estimation_amd.config")
    import pose_resnet_restated as PR

    cfg = config.cfg.clone()
    cfg.merge_from_file(os.path.join(ROOT, "landmark_regression", "experiments", "bench", "res50_256.yaml"))
    sd = syn.pose_resnet_checkpoint(cfg, seed=0)
    h, w = int(cfg.MODEL.IMAGE_SIZE[1]), int(cfg.MODEL.IMAGE_SIZE[0])
    with open(os.path.join(ROOT, "profiles", "round6_final_bench.json")) as f:
        ceil = find_keys(json.load(f), ("peak", "peak_sustained_measured"))
    eng = ops.HrnetEngine(cfg, sd, dtype="bf16")
    sd_dev = {k: v.cuda().to(torch.bfloat16) if torch.is_floating_point(v) else v for k, v in sd.items()}
    cache = {}
    names = {9: "stem conv7x7 s2 + maxpool", 10: "gather (deconv / 1x1 s2)", 1: "conv", 6: "fused Bottleneck"}
    out = {"model": "pose_resnet R50 %dx%d, deconv 3 x k4 x 256, J=11" % (h, w), "dtype": "bf16", "device": torch.cuda.get_device_name(0),
           "mfma_ceiling_tflops": ceil, "batches": {}}
    for n in args.batches:
        g = torch.Generator().manual_seed(n)
        u8 = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).cuda()
        xt = torch.randn(n, 3, h, w, generator=g).cuda().to(torch.bfloat16)
        rec = {"engine": device_ms(lambda: eng(u8), 3, args.repeats, torch)}
        with torch.no_grad():
            rec["torch"] = device_ms(lambda: PR.forward(sd_dev, cfg, xt, cache=cache), 3, args.repeats, torch)
        st = eng.executed_stats(h, w)
        rec["engine"]["tflops"] = st["flops_per_frame"] * n / rec["engine"]["median_ms"] / 1e9
        rec["engine"]["share_of_peak"] = rec["engine"]["tflops"] / ceil["peak"]
        rec["engine"]["share_of_sustained"] = rec["engine"]["tflops"] / ceil["peak_sustained_measured"]
        rec["torch"]["tflops"] = st["flops_per_frame"] * n / rec["torch"]["median_ms"] / 1e9
        rec["engine_over_torch_speed"] = rec["torch"]["median_ms"] / rec["engine"]["median_ms"]
        eng.forward(u8, profile=True)
        torch.cuda.synchronize()
        recs = eng.profile_read()
        classes = {}
        for c, r in zip(eng.kernel_classes(recs), recs):
            k = classes.setdefault(c, {"what": names.get(r["kind"], str(r["kind"])), "launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            k["launches"] += 1; k["ms"] += r["ms"]; k["flops"] += r["flops_per_frame"] * n; k["bytes"] += r["bytes_per_frame"] * n
        for k in classes.values():
            k["tflops"] = k["flops"] / k["ms"] / 1e9 if k["ms"] > 0 else 0.0
            k["tbytes_per_s"] = k["bytes"] / k["ms"] / 1e9 if k["ms"] > 0 else 0.0
        rec["profiled_total_ms"] = sum(r["ms"] for r in recs)
        rec["classes"] = dict(sorted(classes.items(), key=lambda kv: -kv[1]["ms"]))
        by_kind = {}
        for r in recs:
            by_kind[names.get(r["kind"], str(r["kind"]))] = by_kind.get(names.get(r["kind"], str(r["kind"])), 0.0) + r["ms"]
        rec["ms_by_kernel_family"] = by_kind
        # the three new kernels, launch by launch, next to the same layer under torch
        new = []
        with torch.no_grad():
            for c, r in zip(eng.kernel_classes(recs), recs):
                if r["kind"] not in (9, 10):
                    continue
                if r["kind"] == 9:
                    wt = torch.randn(64, 3, 7, 7, device="cuda", dtype=torch.bfloat16); b = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
                    fn = lambda: F.max_pool2d(torch.relu(F.conv2d(xt, wt, b, 2, 3)), 3, 2, 1)
                    what = "stem %dx%d" % (h, w)
                elif r["a"] == 12:
                    px = r["flops_per_frame"] / (2.0 * r["cin"] * r["cout"])
                    s = int(round(px ** 0.5))
                    xi = torch.randn(n, r["cin"], 2 * s, 2 * s, device="cuda", dtype=torch.bfloat16)
                    wt = torch.randn(r["cout"], r["cin"], 1, 1, device="cuda", dtype=torch.bfloat16)
                    fn = lambda xi=xi, wt=wt: F.conv2d(xi, wt, None, 2)
                    what = "1x1 s2 %d->%d @%d -> %d" % (r["cin"], r["cout"], 2 * s, s)
                else:
                    kk = (r["a"] - 202) // 10
                    px = r["flops_per_frame"] / (2.0 * r["cin"] * r["cout"] * kk * kk)
                    s = int(round(px ** 0.5))
                    xi = torch.randn(n, r["cin"], s, s, device="cuda", dtype=torch.bfloat16)
                    wt = torch.randn(r["cin"], r["cout"], kk, kk, device="cuda", dtype=torch.bfloat16)
                    pad, opad = PR.DECONV[kk]
                    fn = lambda xi=xi, wt=wt, pad=pad, opad=opad: torch.relu(F.conv_transpose2d(xi, wt, None, 2, pad, opad))
                    what = "deconv k%d %d->%d @%d -> %d" % (kk, r["cin"], r["cout"], s, 2 * s)
                t = device_ms(fn, 2, 5, torch)
                new.append({"layer": what, "class": c, "engine_ms": r["ms"], "torch_ms": t["median_ms"],
                            "engine_tflops": r["flops_per_frame"] * n / r["ms"] / 1e9, "engine_tbytes_per_s": r["bytes_per_frame"] * n / r["ms"] / 1e9,
                            "engine_slower_than_torch": r["ms"] > t["median_ms"]})
        rec["new_kernels"] = new
        out["batches"][str(n)] = rec
        print("batch %d: engine %.2f ms (%.0f TFLOP/s, %.2f of the sustained ceiling), torch %.2f ms; engine %.2fx torch" % (
            n, rec["engine"]["median_ms"], rec["engine"]["tflops"], rec["engine"]["share_of_sustained"], rec["torch"]["median_ms"],
            rec["engine_over_torch_speed"]))
        for k, v in rec["ms_by_kernel_family"].items():
            print("   %-28s %8.3f ms" % (k, v))
        for e in new:
            print("   %-32s engine %7.3f ms  torch %7.3f ms  %6.1f TFLOP/s %5.2f TB/s%s" % (
                e["layer"], e["engine_ms"], e["torch_ms"], e["engine_tflops"], e["engine_tbytes_per_s"], "  SLOWER" if e["engine_slower_than_torch"] else ""))
    eng.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
