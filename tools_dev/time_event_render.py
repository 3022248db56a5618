"""Cost of rendering event frames on the device (scpose_events_frame_bounds + scpose_events_render) over a sweep.

    python tools_dev/time_event_render.py [--frames 256] [--reps 9] [--bench-json <bench.py's result line>]
                                          [--out profiles/event_render_timing.json] [--quick]

Sweep: 640 x 480 and 1280 x 720; 256 frames per call; 9 216 / 100 000 / 1 000 000 events per frame; uniform pixels and
10 % of the events on 16 hot pixels; with and without undistortion.  The stream is generated on the device from a seed.  Every
point: 3 warm-up calls, then --reps calls timed one by one with device events; the JSON holds the medians and the samples.
Per point also: the traffic floor of the output pass, F*H*W*(3 + 4*counter_bytes) bytes (counter_bytes = 1: the gray plane
the undistortion samples; without undistortion the floor is the 3 output bytes) over the 4 TB/s the project's bandwidth-bound
kernels reach, and the fraction of it reached; and the NumPy restatement (tests/event_render_restated.py) on the host on the
first --host-frames frames of the same uniform stream, per frame, as the CPU comparison.  With --bench-json the condition of
the feature is evaluated: frames/s at 640 x 480, 9 216 events per frame, with undistortion, must exceed the engine's poses/s."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_REACHED = 4.0e12     # bytes/s: what the project's bandwidth-bound kernels reach


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--bench-json", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--quick", action="store_true", help="640 x 480 and 9 216 / 100 000 events per frame only")
    a = ap.parse_args()
    import ctypes
    import numpy as np
    import torch
    import scpose  # noqa: F401
    from importlib import import_module
    import event_render_restated as R
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    er = import_module("spacecraft-pose-estimation_amd.event_render")
    syn = import_module("spacecraft-pose-estimation_amd.synthetic")
    nat = ops.nat; lib = nat.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    F, interval, t0 = a.frames, 10000, 1000000
    P = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames_per_call": F, "reps": a.reps,
           "hbm_bytes_per_s_reached_by_project": HBM_REACHED, "points": []}
    sizes = [(480, 640)] if a.quick else [(480, 640), (720, 1280)]
    densities = [9216, 100000] if a.quick else [9216, 100000, 1000000]
    lut = torch.from_numpy(er.gray_table(2)).to(dev)
    for h, w in sizes:
        K = syn.SPEEDPLUS_K.copy(); K[0] *= w / 1920.0; K[1] *= h / 1200.0
        Kd = torch.from_numpy(K).to(dev); dd = torch.from_numpy(syn.SPEEDPLUS_DIST).to(dev)
        frames = torch.empty((F, h, w, 3), dtype=torch.uint8, device=dev)
        work = torch.empty(F * h * w, dtype=torch.uint8, device=dev)
        for epf in densities:
            g = torch.Generator(device=dev).manual_seed(epf + h)
            n = epf * F + epf // 2 + 2
            t = torch.sort(torch.randint(t0, t0 + interval * F + interval // 2, (n,), generator=g, device=dev, dtype=torch.int64)).values
            t[0] = t0
            x = torch.randint(0, w, (n,), generator=g, device=dev, dtype=torch.int32)
            y = torch.randint(0, h, (n,), generator=g, device=dev, dtype=torch.int32)
            first, before_last, last = t[torch.tensor([0, n - 2, n - 1], device=dev)].tolist()
            starts, names = er.frame_schedule(first, before_last, last, float(interval), max_frames=F)
            assert len(names) == F, len(names)
            starts_d = torch.from_numpy(starts).to(dev)
            bounds = torch.empty((F, 2), dtype=torch.int64, device=dev)
            for hot in (False, True):
                if hot:                  # 10 % of the events on 16 hot pixels
                    sel = torch.rand((n,), generator=g, device=dev) < 0.1
                    which = torch.randint(0, 16, (n,), generator=g, device=dev, dtype=torch.int32)
                    x = torch.where(sel, (which * 37 + 11) % w, x).to(torch.int32)
                    y = torch.where(sel, (which * 23 + 5) % h, y).to(torch.int32)
                    del sel, which
                host = None
                for undist in (True, False):
                    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

                    def call():
                        nat.check(lib.scpose_events_frame_bounds(P(t), n, P(starts_d), F, P(bounds), st), "events_frame_bounds")
                        nat.check(lib.scpose_events_render(P(x), P(y), None, 0, P(bounds), F, h, w, 2, 1, P(lut), P(Kd) if undist else None,
                                                           P(dd) if undist else None, P(frames), None, P(work), work.numel(), st),
                                  "events_render")
                    for _ in range(3):
                        call()
                    torch.cuda.synchronize()
                    samples = []
                    for _ in range(a.reps):
                        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(); call(); e1.record(); e1.synchronize()
                        samples.append(e0.elapsed_time(e1) * 1e3)
                    med = statistics.median(samples)
                    floor_bytes = F * h * w * (3 + 4 * 1) if undist else F * h * w * 3
                    floor_us = floor_bytes / HBM_REACHED * 1e6
                    pt = {"hw": [h, w], "events_per_frame": epf, "hot_pixels": hot, "undistort": undist, "median_us_per_call": round(med, 1),
                          "min_us": round(min(samples), 1), "max_us": round(max(samples), 1), "frames_per_s": round(F / med * 1e6, 1),
                          "events_per_s": round(n / med * 1e6, 0), "floor_bytes": floor_bytes, "floor_us": round(floor_us, 1),
                          "fraction_of_floor_rate": round(floor_us / med, 4), "samples_us": [round(s, 1) for s in samples]}
                    if not hot:          # the NumPy restatement on the host, first frames of the same stream
                        if host is None:
                            hf = min(a.host_frames, F)
                            b = bounds[:hf].cpu().numpy()
                            hx = x[:int(b[-1, 1])].cpu().numpy(); hy = y[:int(b[-1, 1])].cpu().numpy()
                            c0 = time.perf_counter()
                            imgs = [R.gray(R.counts(hx[b0:b1], hy[b0:b1], None, (h, w)), 2) for b0, b1 in b]
                            c1 = time.perf_counter()
                            und = [R.undistort(im, K, syn.SPEEDPLUS_DIST) for im in imgs]
                            c2 = time.perf_counter()
                            host = ((c1 - c0) / hf * 1e6, (c2 - c1) / hf * 1e6)
                            assert np.array_equal(np.stack(und)[..., None].repeat(3, 3), frames[:hf].cpu().numpy()) if undist else True
                        host_us = host[0] + (host[1] if undist else 0.0)
                        pt["numpy_host_us_per_frame"] = round(host_us, 1)
                        pt["speedup_vs_numpy_host"] = round(host_us / (med / F), 1)
                    res["points"].append(pt)
                    print(json.dumps({k: v for k, v in pt.items() if k != "samples_us"}), flush=True)
            del t, x, y
            torch.cuda.empty_cache()
    head = [p for p in res["points"] if p["hw"] == [480, 640] and p["events_per_frame"] == 9216 and p["undistort"] and not p["hot_pixels"]][0]
    res["headline_frames_per_s"] = head["frames_per_s"]
    if a.bench_json:
        line = [ln for ln in open(a.bench_json).read().splitlines() if ln.strip().startswith("{")][-1]
        poses = float(json.loads(line)["value"])
        res["engine_poses_per_s_same_box"] = poses
        res["margin_over_engine"] = round(head["frames_per_s"] / poses, 2)
        res["condition_stage0_faster_than_engine"] = bool(head["frames_per_s"] > poses)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if a.bench_json and not res["condition_stage0_faster_than_engine"]:
        sys.exit("stage 0 renders %.0f frames/s, the engine %.0f poses/s: the condition is not met" % (head["frames_per_s"], poses))


if __name__ == "__main__":
    main()
