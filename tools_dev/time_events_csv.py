"""Cost of reading events.csv: the parent's reader (pandas.read_csv + four uploads) against the device parser
(csrc/events_csv.hip, ops.parse_events_csv).

    python tools_dev/time_events_csv.py --keep-dir <files> --generate-only
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/time_events_csv.py --child trace --dir <files>   (per-kernel)
    python tools_dev/time_events_csv.py --keep-dir <files> [--events 3000000] [--reps 5] [--rounds 2]
                                        [--kernel-stats <the run's kernel_stats.csv>] [--out profiles/events_csv_timing.json]

Rows: two files of --events events at 640 x 480 generated from fixed seeds: "comma" (aedat_to_csv.py style, 't,x,y,p' integers)
and "white" (v2e text style, '%f %d %d %d' under a '#' header line, read with --delim_whitespace --swap_xy).
Child processes alternate, parent reader then device reader, --rounds times; each child does 2 warm-up reads per file (the file
is then in the page cache for both), then --reps timed ones.  Every time is the host clock around work that ends in a device
synchronise, except `kernels_us` (device events around scpose_events_csv_parse alone).
  per row   file -> four device arrays: parent (read_events_csv + the uploads render_scene did) and new (parse_events_csv on the
            path); the new path split into file read, H2D copy, kernels; the kernels against their HBM floor (n_bytes read once +
            17 bytes written per row, at 6.29 TB/s, the copy rate the microarchitecture guide measured on this chip);
            ops.render_events on the parsed stream (324 frames at 10 000 ticks for 3 M events, with undistortion) -- the
            renderer is the parent's, unchanged; per kernel, from the separate rocprofv3 run, split by row (--kernel-trace)
  scene     the comma row only: the steps of event_render.render_scene restated in the child (not a convert_aedats.py
            process), without the distorted copies: read / render / D2H / BMP writing, with the parent reader and with the
            device reader; the renderer is warmed in both children first, so the split compares the readers alone
  C1  the new file -> arrays median is below the parent's on both rows
  C2  kernels_us median <= the render_events call's median on the same stream
The JSON holds every sample and the medians over all rounds."""
import argparse
import csv
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HW = (480, 640)
HBM_BYTES_PER_S = 6.29e12
ROWS = [("comma", {"delim_whitespace": False, "swap_xy": False}), ("white", {"delim_whitespace": True, "swap_xy": True})]
TICKS_PER_EVENT = 1.083      # a 3 M-event stream then spans 324 written frames of 10 000 ticks


def generate(folder, events):
    """Plain files (no padding or noise lines): what the two writers produce.  Stamps are rescaled to ~325 frames per 3 M."""
    import numpy as np
    import events_csv_restated as R
    out = {}
    for name, _ in ROWS:
        path = os.path.join(folder, name + ".csv")
        if os.path.exists(path + ".done"):          # left by --generate-only
            out[name] = {"path": path, "bytes": os.path.getsize(path), "events": events}
            continue
        rng = np.random.default_rng(1 if name == "comma" else 2)
        t = np.cumsum(rng.random(events) * 2 * TICKS_PER_EVENT).astype(np.int64) + 5000000
        x = rng.integers(0, HW[1], events); y = rng.integers(0, HW[0], events); p = rng.integers(0, 2, events)
        if name == "comma":
            body = "".join("%d,%d,%d,%d\n" % r for r in zip(t.tolist(), x.tolist(), y.tolist(), p.tolist()))
        else:       # t, y, x, p with a float stamp of six decimals: the integer part is the tick
            body = "# v2e text events\n" + "".join("%d.%06d %d %d %d\n" % (a, (a * 7919) % 1000000, c, b, 2 * d - 1)
                                                   for a, b, c, d in zip(t.tolist(), x.tolist(), y.tolist(), p.tolist()))
        data = body.encode()
        assert not isinstance(R.parse(data[:200000].rsplit(b"\n", 1)[0], **dict(ROWS)[name]), str)
        with open(path, "wb") as f:
            f.write(data)
        open(path + ".done", "w").close()
        out[name] = {"path": path, "bytes": len(data), "events": events}
    return out


def _sync_time(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, r


def child(which, folder, reps, scene):
    import ctypes
    import numpy as np
    import torch
    import scpose  # noqa: F401
    from importlib import import_module
    nat = import_module("spacecraft-pose-estimation_amd._native")
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    er = import_module("spacecraft-pose-estimation_amd.event_render")
    syn = import_module("spacecraft-pose-estimation_amd.synthetic")
    lib = nat.lib()
    dev = torch.device("cuda:0")
    h, w = HW
    K = syn.SPEEDPLUS_K.copy(); K[0] *= w / 1920.0; K[1] *= h / 1200.0; dist = syn.SPEEDPLUS_DIST.copy()
    P = lambda v: ctypes.c_void_p(v.data_ptr())      # noqa: E731
    res = {}
    for name, flags in ROWS:
        path = os.path.join(folder, name + ".csv")
        row = {}

        def parent_read():
            t, x, y, p = er.read_events_csv(path, **flags)
            return (torch.from_numpy(t).to(dev), torch.from_numpy(x.astype(np.int32)).to(dev),
                    torch.from_numpy(y.astype(np.int32)).to(dev))

        def new_read():
            return ops.parse_events_csv(path, device=dev, **flags)[:3]

        read = parent_read if which == "parent" else new_read
        if which == "trace":
            for _ in range(5):
                new_read()
            torch.cuda.synchronize()
            continue
        for _ in range(2):
            read()
        row["file_to_arrays_us"] = []
        for _ in range(reps):
            us, cols = _sync_time(torch, read)
            row["file_to_arrays_us"].append(round(us, 1))
        row["rows"] = int(cols[0].numel())
        if which == "new":
            row["file_read_us"], row["h2d_us"], row["kernels_us"], row["render_events_us"] = [], [], [], []
            for _ in range(reps):
                us, host = _sync_time(torch, lambda: np.fromfile(path, dtype=np.uint8))
                row["file_read_us"].append(round(us, 1))
                us, buf = _sync_time(torch, lambda: torch.from_numpy(host).to(dev))
                row["h2d_us"].append(round(us, 1))
            n = buf.numel(); cap = (n + 1) // 8
            ws = ctypes.c_size_t()
            nat.check(lib.scpose_events_csv_workspace_bytes(n, ctypes.byref(ws)))
            outs = [torch.empty(cap, dtype=d, device=dev) for d in (torch.int64, torch.int32, torch.int32, torch.int8)]
            cs = torch.empty(2, dtype=torch.int64, device=dev); work = torch.empty(ws.value, dtype=torch.uint8, device=dev)

            def kernels():
                nat.check(lib.scpose_events_csv_parse(P(buf), n, int(flags["delim_whitespace"]), int(flags["swap_xy"]), 0.0, P(outs[0]),
                                                      P(outs[1]), P(outs[2]), P(outs[3]), cap, P(cs), P(work), ws.value,
                                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            for _ in range(3):
                kernels()
            torch.cuda.synchronize()
            for _ in range(reps):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); kernels(); e1.record(); e1.synchronize()
                row["kernels_us"].append(round(e0.elapsed_time(e1) * 1e3, 1))
            assert cs.tolist() == [row["rows"], 0]
            del outs, work, buf
            for _ in range(3):
                ops.render_events(cols[0], cols[1], cols[2], None, HW, K=K, dist=dist)
            for _ in range(reps):
                us, r = _sync_time(torch, lambda: ops.render_events(cols[0], cols[1], cols[2], None, HW, K=K, dist=dist))
                row["render_events_us"].append(round(us, 1))
            row["frames"] = len(r[1])
            del r
        if scene and name == "comma":
            tmp = tempfile.mkdtemp(prefix="scene_", dir=folder)
            try:
                for _ in range(3):          # both children: the renderer and the D2H path warm before the timed scene
                    ops.render_events(cols[0], cols[1], cols[2], None, HW, K=K, dist=dist)[0]["flat"][:h * w * 3].cpu()
                st = {}
                st["read_us"], cols = _sync_time(torch, read)
                st["render_us"], (frames, names) = _sync_time(
                    torch, lambda: ops.render_events(cols[0], cols[1], cols[2], None, HW, K=K, dist=dist))
                und = frames["flat"].view(-1, h, w, 3)
                st["d2h_us"] = 0.0; st["bmp_us"] = 0.0
                for k0 in range(0, len(names), 256):
                    us, host = _sync_time(torch, lambda: und[k0:k0 + 256].cpu().numpy())
                    st["d2h_us"] += us
                    t0 = time.perf_counter()
                    for i, nm in enumerate(names[k0:k0 + 256]):
                        er.write_bmp(os.path.join(tmp, nm + ".bmp"), host[i])
                    st["bmp_us"] += (time.perf_counter() - t0) * 1e6
                st = {k: round(v, 1) for k, v in st.items()}
                st["total_us"] = round(sum(st.values()), 1); st["frames"] = len(names)
                row["scene"] = st
                del frames
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        del cols
        torch.cuda.empty_cache()
        res[name] = row
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=3000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--kernel-trace", default="", help="the same run's kernel_trace.csv: per-kernel medians split by row")
    ap.add_argument("--out", default="")
    ap.add_argument("--dir", default="")
    ap.add_argument("--keep-dir", default="", help="generate the files here and keep them (for the rocprofv3 run)")
    ap.add_argument("--generate-only", action="store_true", help="write the files into --keep-dir and stop")
    ap.add_argument("--child", default="")
    ap.add_argument("--scene", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.dir, a.reps, bool(a.scene))
    folder = a.keep_dir or tempfile.mkdtemp(prefix="events_csv_")
    os.makedirs(folder, exist_ok=True)
    if a.generate_only:
        return print(json.dumps(generate(folder, a.events)))
    try:
        files = generate(folder, a.events)
        keys = ("file_to_arrays_us", "file_read_us", "h2d_us", "kernels_us", "render_events_us")
        samples = {wh: {name: {k: [] for k in keys} for name, _ in ROWS} for wh in ("parent", "new")}
        meta = {wh: {name: {} for name, _ in ROWS} for wh in ("parent", "new")}
        for rnd in range(a.rounds):
            for which in ("parent", "new"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--dir", folder, "--reps", str(a.reps),
                                    "--scene", str(int(rnd == 0))], capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    sys.exit("child %s failed (%d): %s" % (which, r.returncode, r.stderr[-3000:]))
                got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
                for name, row in got.items():
                    for k, v in row.items():
                        if k in keys:
                            samples[which][name][k] += v
                        else:
                            meta[which][name][k] = v
                print("round %d %s done" % (rnd, which), flush=True)
    finally:
        if not a.keep_dir:
            shutil.rmtree(folder, ignore_errors=True)
    res = {"events": a.events, "hw": list(HW), "reps_per_round": a.reps, "rounds": a.rounds, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "rows": []}
    try:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    c1 = c2 = True
    for name, flags in ROWS:
        med = {wh: {k: statistics.median(v) for k, v in samples[wh][name].items() if v} for wh in ("parent", "new")}
        assert meta["parent"][name]["rows"] == meta["new"][name]["rows"] == a.events
        floor_us = (files[name]["bytes"] + 17 * a.events) / HBM_BYTES_PER_S * 1e6
        row = {"row": name, "flags": flags, "file_bytes": files[name]["bytes"], "rows": a.events, "frames": meta["new"][name]["frames"],
               "parent_file_to_arrays_median_us": med["parent"]["file_to_arrays_us"],
               "new_file_to_arrays_median_us": med["new"]["file_to_arrays_us"],
               "ratio_parent_over_new": round(med["parent"]["file_to_arrays_us"] / med["new"]["file_to_arrays_us"], 2),
               "new_file_read_median_us": med["new"]["file_read_us"], "new_h2d_median_us": med["new"]["h2d_us"],
               "new_kernels_median_us": med["new"]["kernels_us"], "kernels_hbm_floor_us": round(floor_us, 1),
               "kernels_hbm_floor_share": round(floor_us / med["new"]["kernels_us"], 3),
               "render_events_median_us": med["new"]["render_events_us"],
               "kernels_over_render_events": round(med["new"]["kernels_us"] / med["new"]["render_events_us"], 3),
               "samples": {wh: samples[wh][name] for wh in ("parent", "new")}}
        if "scene" in meta["parent"][name]:
            row["scene_parent_reader"] = meta["parent"][name]["scene"]
            row["scene_device_reader"] = meta["new"][name]["scene"]
        c1 = c1 and row["new_file_to_arrays_median_us"] < row["parent_file_to_arrays_median_us"]
        c2 = c2 and row["new_kernels_median_us"] <= row["render_events_median_us"]
        res["rows"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "samples"}), flush=True)
    res["C1_new_below_parent_on_both_rows"] = c1
    res["C2_kernels_within_render_events_call"] = c2
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            res["kernel_stats_rocprofv3"] = [r for r in csv.DictReader(f) if "csv_" in (r.get("Name") or r.get("KernelName") or "")]
        res["kernel_stats_note"] = ("one separate rocprofv3 --kernel-trace --stats run: 5 parses of the comma file, then 5 of the "
                                    "white file; kernel_trace_per_row splits the dispatches by that order")
    if a.kernel_trace:
        with open(a.kernel_trace) as f:
            disp = [r for r in csv.DictReader(f) if "csv_" in r.get("Kernel_Name", "")]
        disp.sort(key=lambda r: int(r["Start_Timestamp"]))
        per = {}
        for kern in ("csv_count_kernel", "csv_scan_kernel", "csv_parse_kernel", "csv_finish_kernel"):
            d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in disp if kern in r["Kernel_Name"]]
            half = len(d) // 2                      # the trace child parses the comma file 5 times, then the white file 5 times
            if half:
                per[kern] = {"comma_median_us": round(statistics.median(d[:half]), 1),
                             "white_median_us": round(statistics.median(d[half:]), 1), "dispatches": len(d)}
        res["kernel_trace_per_row"] = per
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("rows", "kernel_stats_rocprofv3")}), flush=True)


if __name__ == "__main__":
    main()
