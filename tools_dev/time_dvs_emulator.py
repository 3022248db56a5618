"""Cost of the device DVS emulator (csrc/dvs_emulator.hip, ops.dvs_emulator) against the torch restatement of the reference's
emulator run on the same card (tests/dvs_emulator_restated.py with device="cuda": the reference's own tensor expressions,
sub-iteration loop, nonzero and host synchronises included).

    python tools_dev/time_dvs_emulator.py [--frames 64] [--reps 9] [--out profiles/dvs_emulator_timing.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/time_dvs_emulator.py --child 640x480:dense:plain --trace 1

Rows: 640 x 480 and 1280 x 720, --frames frames per call (the first one initialises), a sparse stream (about 1 % of the pixels
step per frame) and a dense one (every pixel alternates between two levels 5 thresholds apart), each without options
("plain") and with cutoff_hz = 30, leak_rate_hz = 0.1 over a log-normal noise-rate array and refractory_period_s = 1 ms ("all").
One child process per row, one after the other under a time limit each; the parent stops at the first child that fails.  In a
child: 3 warm-up calls, then --reps timed ones, device events around the call (state re-initialised by the first frame of every
call; the output columns are sized by the warm-ups, so no timed call repeats itself).
  C1  the device call takes no longer than the restatement on every row (ratio restated / device reported)
  C2  floor per call = (frames - 1) * H * W * 33 bytes (1 input byte, four float32 state planes read and written) + 21 bytes per
      event, at 6.29 TB/s (the copy rate the microarchitecture guide gives for this chip); share = floor / measured
  C3  640 x 480 sparse plain: events emitted per second > events ops.render_events consumes per second on that stream"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 6.29e12
SIZES = ((480, 640), (720, 1280))


def make_frames(kind, f, h, w, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    if kind == "dense":                      # ln(110 / 40) = 1.01: five events per pixel and frame at threshold 0.2
        a = np.where(rng.random((h, w)) < 0.5, 40, 110).astype(np.uint8)
        b = (150 - a).astype(np.uint8)
        return np.stack([a if k % 2 == 0 else b for k in range(f)])
    cur = rng.integers(30, 200, (h, w)).astype(np.uint8)
    out = [cur.copy()]
    for _ in range(f - 1):
        m = rng.random((h, w)) < 0.01
        cur = np.where(m, rng.integers(10, 250, (h, w)), cur).astype(np.uint8)
        out.append(cur.copy())
    return np.stack(out)


def options(opt, h, w):
    import numpy as np
    if opt == "plain":
        return dict(pos_thres=0.2, neg_thres=0.2)
    nra = np.exp(np.log(10) * 0.1 * np.random.default_rng(5).standard_normal((h, w))).astype(np.float32)
    return dict(pos_thres=0.2, neg_thres=0.2, cutoff_hz=30.0, leak_rate_hz=0.1, noise_rate_array=nra, refractory_period_s=0.001)


def child(spec, frames_n, reps, trace):
    import numpy as np
    import torch
    import scpose  # noqa: F401
    from importlib import import_module
    import dvs_emulator_restated as R
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    size, kind, opt = spec.split(":")
    w, h = (int(v) for v in size.split("x"))
    dev = torch.device("cuda:0")
    fr = torch.from_numpy(make_frames(kind, frames_n, h, w)).to(dev)
    t_host = 0.01 * np.arange(frames_n, dtype=np.float64)
    t = torch.from_numpy(t_host).to(dev)
    kw = options(opt, h, w)
    emu = ops.dvs_emulator(h, w, **kw)

    def timed(fn, warm, n):
        for _ in range(warm):
            r = fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(n):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); r = fn(); e1.record(); e1.synchronize()
            out.append(round(e0.elapsed_time(e1) * 1e3, 1))
        return out, r

    def device_call():
        emu.reset()
        return emu.emulate(fr, t_host)

    dev_us, cols = timed(device_call, 3, reps)
    n_events = int(cols[0].numel())
    res = {"row": spec, "h": h, "w": w, "frames": frames_n, "events": n_events, "device_us": dev_us}
    if trace:
        print("CHILD " + json.dumps(res), flush=True)
        return
    rest = R.RestatedEmulator(device=dev, **kw)

    def restated_call():
        rest.reset()
        n = 0
        for k in range(frames_n):
            r = rest.frame(fr[k], t_host[k])
            n += 0 if r is None else int(r[0].numel())
        return n

    rest_us, n_rest = timed(restated_call, 1 if kind == "dense" else 3, reps)
    assert n_rest == n_events, (n_rest, n_events)
    res["restated_us"] = rest_us
    res["num_iters_max"] = max(rest.num_iters)
    if spec == "640x480:sparse:plain":
        tt, x, y, p, _ = cols
        res["render_events_us"], (_, names) = timed(lambda: ops.render_events(tt, x, y, p, (h, w), interval=10000.0), 3, reps)
        res["render_frames"] = len(names)
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames, a.reps, bool(a.trace))
    res = {"frames_per_call": a.frames, "reps": a.reps, "warm_ups": 3, "hbm_bytes_per_s": HBM_BYTES_PER_S, "rows": []}
    c1 = True
    for h, w in SIZES:
        for kind in ("sparse", "dense"):
            for opt in ("plain", "all"):
                spec = "%dx%d:%s:%s" % (w, h, kind, opt)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, "--frames", str(a.frames), "--reps", str(a.reps)],
                                   capture_output=True, text=True, timeout=a.timeout)
                if r.returncode != 0:
                    sys.exit("child %s failed (%d): %s" % (spec, r.returncode, r.stderr[-3000:]))
                row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
                d = statistics.median(row["device_us"]); b = statistics.median(row["restated_us"])
                floor = ((a.frames - 1) * h * w * 33 + 21 * row["events"]) / HBM_BYTES_PER_S * 1e6
                row.update(device_median_us=d, restated_median_us=b, ratio_restated_over_device=round(b / d, 2),
                           floor_us=round(floor, 1), floor_share=round(floor / d, 3), events_per_s=round(row["events"] / d * 1e6))
                if "render_events_us" in row:
                    rm = statistics.median(row["render_events_us"])
                    row.update(render_events_median_us=rm, render_events_per_s=round(row["events"] / rm * 1e6))
                    res["C3_emits_faster_than_render_events_consumes"] = row["events_per_s"] > row["render_events_per_s"]
                c1 = c1 and d <= b
                res["rows"].append(row)
                print(json.dumps({k: v for k, v in row.items() if not k.endswith("_us") or "median" in k or k == "floor_us"}), flush=True)
    res["C1_device_not_slower_on_every_row"] = c1
    try:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
