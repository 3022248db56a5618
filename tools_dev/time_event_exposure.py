"""Cost of the COUNT and AREA_COUNT exposure modes (csrc/events_exposure.hip) against the parent's DURATION renderer.

    python tools_dev/time_event_exposure.py --parent-lib <parent's libscpose_hip.so> [--reps 9] [--rounds 2]
                                            [--bench-json <bench.py's result line>] [--out profiles/event_exposure_timing.json]

Rows: the streams of tests/test_gpu_event_exposure.py (uniform_stream): 640 x 480, 3 M events, D = 64, M = 150 with
undistortion (and without); the same with 10 % of the events on 16 hot pixels, M = 240; 64 x 48, 2^20 events, D = 8, M = 2;
COUNT N = 9 216 at 640 x 480 with undistortion.  For every row the baseline is the DURATION call of the parent library on the
SAME stream with the interval chosen so that its frame count is within 1 % of the row's (equal n, F, H, W, undistortion).

The parent library and this tree's library are loaded by child processes of their own (one library per process, through
SCPOSE_DEV=1 SCPOSE_LIB), alternated --rounds times: parent, new, parent, new, ...  Each child times every row: 3 warm-up
calls, then --reps calls one by one with device events around (a) the bounds step alone (scpose_events_area_bounds /
scpose_events_count_bounds; the parent: scpose_events_frame_bounds) and (b) the whole ops.render_events call, host
read-backs included.  The JSON holds every sample and the medians over all rounds.
  C1  whole-call median of every row <= 3 x the parent's duration call of the same row
  C2  area_count frames/s at 640 x 480, ~9 216 events per frame, with undistortion >= 10 x bench.py's poses/s (--bench-json)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS = [  # name, (h, w), n, hot fraction, mode, M or N, D, undistort
    ("area_vga_d64_m150_undist", (480, 640), 3000000, 0.0, "area_count", 150, 64, True),
    ("area_vga_d64_m150", (480, 640), 3000000, 0.0, "area_count", 150, 64, False),
    ("area_vga_hot_m240", (480, 640), 3000000, 0.1, "area_count", 240, 64, False),
    ("area_64x48_d8_m2", (48, 64), 2 ** 20, 0.0, "area_count", 2, 8, False),
    ("count_vga_9216_undist", (480, 640), 3000000, 0.0, "count", 9216, None, True),
]
SEEDS = {"area_vga_d64_m150_undist": 1, "area_vga_d64_m150": 1, "area_vga_hot_m240": 2, "area_64x48_d8_m2": 0,
         "count_vga_9216_undist": 3}


def stream(name):
    import numpy as np
    from test_gpu_event_exposure import uniform_stream
    row = [r for r in ROWS if r[0] == name][0]
    return uniform_stream(row[2], row[1], SEEDS[name], row[3])


def plan():
    """Per row: the exposure's frame count (NumPy restatement) and the matching DURATION interval."""
    import event_exposure_restated as X
    from importlib import import_module
    import scpose  # noqa: F401
    er = import_module("spacecraft-pose-estimation_amd.event_render")
    out = {}
    for name, hw, n, hot, mode, v, D, undist in ROWS:
        t, x, y = stream(name)
        F = len(X.area_bounds_suffix_min(x, y, hw, v, D)) if mode == "area_count" else len(X.serial_count_bounds(n, v))
        span = float(t[n - 2] - t[0])
        interval = span / (F + 0.5)
        fd = len(er.frame_schedule(t[0], t[n - 2], t[n - 1], interval)[1])
        assert abs(fd - F) <= 0.01 * F, (name, F, fd)
        out[name] = {"frames": F, "duration_interval": interval, "duration_frames": fd, "events_per_frame": round(n / F, 1)}
        print(json.dumps({"row": name, **out[name]}), flush=True)
    return out


def child(which, plan_json, reps):
    import ctypes
    import numpy as np
    import torch
    import scpose  # noqa: F401
    from importlib import import_module
    nat = import_module("spacecraft-pose-estimation_amd._native")
    if which == "parent":        # the parent's library exports the parent's symbols only
        probe = ctypes.CDLL(nat.LIB_PATH)
        for name in list(nat.SYMBOLS):
            if not hasattr(probe, name):
                del nat.SYMBOLS[name]
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    er = import_module("spacecraft-pose-estimation_amd.event_render")
    syn = import_module("spacecraft-pose-estimation_amd.synthetic")
    lib = nat.lib()
    pl = json.loads(plan_json)
    dev = torch.device("cuda:0")
    P = lambda v: ctypes.c_void_p(v.data_ptr())      # noqa: E731
    res = {}
    for name, (h, w), n, hot, mode, v, D, undist in ROWS:
        t, x, y = stream(name)
        td = torch.from_numpy(t).to(dev); xd = torch.from_numpy(x.astype(np.int32)).to(dev); yd = torch.from_numpy(y.astype(np.int32)).to(dev)
        K = dist = None
        if undist:
            K = syn.SPEEDPLUS_K.copy(); K[0] *= w / 1920.0; K[1] *= h / 1200.0; dist = syn.SPEEDPLUS_DIST.copy()
        st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
        if which == "parent":
            interval = pl[name]["duration_interval"]
            first, before_last, last = t[0], t[n - 2], t[n - 1]
            starts, names = er.frame_schedule(first, before_last, last, interval)
            F = len(names)
            starts_d = torch.from_numpy(starts).to(dev); bounds = torch.empty((F, 2), dtype=torch.int64, device=dev)

            def bounds_step():
                nat.check(lib.scpose_events_frame_bounds(P(td), n, P(starts_d), F, P(bounds), st()), "events_frame_bounds")

            def whole():
                return ops.render_events(td, xd, yd, None, (h, w), interval=interval, K=K, dist=dist)
        else:
            if mode == "area_count":
                ws = ctypes.c_size_t()
                nat.check(lib.scpose_events_area_bounds_workspace_bytes(n, v, D, h, w, ctypes.byref(ws)))
                cap = (n - 2) // (v - 1)
                bounds = torch.empty((cap, 2), dtype=torch.int64, device=dev); cs = torch.empty(2, dtype=torch.int64, device=dev)
                work = torch.empty(ws.value, dtype=torch.uint8, device=dev)

                def bounds_step():
                    nat.check(lib.scpose_events_area_bounds(P(xd), P(yd), n, v, D, h, w, P(bounds), cap, P(cs), P(work), ws.value, st()))
                kw = {"exposure": "area_count", "area_count": v, "area_dimension": D}
            else:
                F = (n - 2) // v
                bounds = torch.empty((F, 2), dtype=torch.int64, device=dev)

                def bounds_step():
                    nat.check(lib.scpose_events_count_bounds(n, v, F, P(bounds), st()))
                kw = {"exposure": "count", "event_count": v}

            def whole():
                return ops.render_events(td, xd, yd, None, (h, w), K=K, dist=dist, **kw)
        row = {}
        for label, fn in (("bounds_us", bounds_step), ("whole_us", whole)):
            for _ in range(3):
                r = fn()
            torch.cuda.synchronize()
            samples = []
            for _ in range(reps):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); r = fn(); e1.record(); e1.synchronize()
                samples.append(round(e0.elapsed_time(e1) * 1e3, 1))
            row[label] = samples
            if label == "whole_us":
                row["frames"] = len(r[1])
            del r
        res[name] = row
        del td, xd, yd, bounds
        torch.cuda.empty_cache()
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench-json", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--plan", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.plan, a.reps)
    pl = plan()
    samples = {w: {r[0]: {"bounds_us": [], "whole_us": []} for r in ROWS} for w in ("parent", "new")}
    frames = {w: {} for w in ("parent", "new")}
    for rnd in range(a.rounds):
        for which in ("parent", "new"):
            env = dict(os.environ)
            if which == "parent":
                env.update({"SCPOSE_DEV": "1", "SCPOSE_LIB": os.path.abspath(a.parent_lib)})
            else:
                env.pop("SCPOSE_DEV", None); env.pop("SCPOSE_LIB", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--plan", json.dumps(pl), "--reps",
                                str(a.reps)], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("child %s failed (%d): %s" % (which, r.returncode, r.stderr[-3000:]))
            got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
            for name, row in got.items():
                for k in ("bounds_us", "whole_us"):
                    samples[which][name][k] += row[k]
                frames[which][name] = row["frames"]
            print("round %d %s done" % (rnd, which), flush=True)
    res = {"reps_per_round": a.reps, "rounds": a.rounds, "rows": []}
    try:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    ok1 = True
    for name, hw, n, hot, mode, v, D, undist in ROWS:
        med = {w: {k: statistics.median(samples[w][name][k]) for k in ("bounds_us", "whole_us")} for w in ("parent", "new")}
        ratio = med["new"]["whole_us"] / med["parent"]["whole_us"]
        ok1 = ok1 and ratio <= 3.0
        row = {"row": name, "hw": list(hw), "n": n, "hot_fraction": hot, "mode": mode, "value": v, "area_dimension": D,
               "undistort": undist, "frames": frames["new"][name], "parent_duration_frames": frames["parent"][name],
               "parent_duration_interval": pl[name]["duration_interval"], "events_per_frame": pl[name]["events_per_frame"],
               "new_bounds_median_us": med["new"]["bounds_us"], "new_whole_median_us": med["new"]["whole_us"],
               "parent_bounds_median_us": med["parent"]["bounds_us"], "parent_whole_median_us": med["parent"]["whole_us"],
               "ratio_whole_new_over_parent": round(ratio, 3),
               "new_frames_per_s": round(frames["new"][name] / med["new"]["whole_us"] * 1e6, 1),
               "samples": {w: samples[w][name] for w in ("parent", "new")}}
        assert frames["new"][name] == pl[name]["frames"]
        res["rows"].append(row)
        print(json.dumps({k: v2 for k, v2 in row.items() if k != "samples"}), flush=True)
    res["C1_all_rows_within_3x_parent"] = ok1
    if a.bench_json:
        line = [ln for ln in open(a.bench_json).read().splitlines() if ln.strip().startswith("{")][-1]
        poses = float(json.loads(line)["value"])
        head = [r for r in res["rows"] if r["row"] == "area_vga_d64_m150_undist"][0]
        res["engine_poses_per_s_same_call"] = poses
        res["C2_area_frames_per_s_over_poses_per_s"] = round(head["new_frames_per_s"] / poses, 2)
        res["C2_at_least_10x"] = bool(head["new_frames_per_s"] >= 10 * poses)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v2 for k, v2 in res.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
