"""Cost of the Levenberg-Marquardt pose refinement (scpose_pnp_epnp_ransac_refine) next to the unrefined PnP.

    python tools_dev/pnp_refine_timing.py [--sizes 256,2048] [--reps 25] [--out profiles/pnp_refine_timing.json]
    python tools_dev/pnp_refine_timing.py --stats <rocprofv3 results .db> --out profiles/pnp_refine_kernel_trace.json

Key points: the package's own synthetic.keypoints (1 px noise, 10 % outliers), as bench.py builds its PnP input.  Per size, one
process alternates refine_iters = 0 and 20 (rows form, the entry bench.py uses for 0), timing every call alone with device events;
the JSON holds the medians over --reps repetitions and the per-repetition samples.  The --stats form condenses the kernel
trace of one `rocprofv3 --kernel-trace --stats` run of this script (its SQLite output) to the two PnP kernel instantiations.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def condense_stats(path):
    """The PnP dispatches of a rocprofv3 run (its rocpd SQLite output, `kernels` view): per kernel instantiation and batch size,
    duration statistics and the resources the runtime reports for the code object."""
    import sqlite3
    import statistics
    con = sqlite3.connect(path)
    groups = {}
    for name, gx, wx, dur, vgpr, agpr, sgpr, scratch, lds in con.execute(
            "select name, grid_x, workgroup_x, duration, vgpr_count, accum_vgpr_count, sgpr_count, scratch_size, lds_size "
            "from kernels where name like '%pnp_kernel%' order by start"):
        g = groups.setdefault((name, gx // 64), {"durations_ns": [], "vgpr": vgpr, "agpr": agpr, "sgpr": sgpr,
                                                 "scratch_bytes_per_lane": scratch, "lds_bytes": lds, "workgroup": wx})
        g["durations_ns"].append(int(dur))
    out = []
    for (name, frames), g in sorted(groups.items()):
        d = g.pop("durations_ns")
        out.append(dict(kernel=name, frames=frames, calls=len(d), median_ns=statistics.median(d), min_ns=min(d), max_ns=max(d), **g))
    return {"source": "rocprofv3 --kernel-trace --stats of tools_dev/pnp_refine_timing.py --reps 5 (warm-up calls included)",
            "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,2048")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--stats", default="", help="condense this rocprofv3 results database instead of timing")
    a = ap.parse_args()
    if a.stats:
        res = condense_stats(a.stats)
    else:
        import numpy as np
        import torch
        import scpose  # noqa: F401
        from importlib import import_module
        ops = import_module("spacecraft-pose-estimation_amd.ops")
        syn = import_module("spacecraft-pose-estimation_amd.synthetic")
        dev = torch.device("cuda:0")
        d = lambda x: torch.from_numpy(x).to(dev)   # noqa: E731
        res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "refine_iters": a.iters,
               "input": "synthetic.keypoints, 1 px noise, 10 % outliers, seed 2000", "sizes": {}}
        for n in (int(s) for s in a.sizes.split(",")):
            kp, _, _ = syn.keypoints(n, np.random.default_rng(2000), 1.0, 0.1)
            args = (d(kp), d(syn.TANGO_LANDMARKS), d(syn.SPEEDPLUS_K), d(syn.SPEEDPLUS_DIST))
            rows = torch.empty((n, 13), dtype=torch.float64, device=dev)
            times = {0: [], a.iters: []}
            for it in (0, a.iters, 0, a.iters):       # warm-up: code objects, LDS opt-in
                ops.pnp_epnp_ransac(*args, rows=rows, refine_iters=it)
            torch.cuda.synchronize()
            for _ in range(a.reps):
                for it in (0, a.iters):
                    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    st.record()
                    ops.pnp_epnp_ransac(*args, rows=rows, refine_iters=it)
                    en.record()
                    torch.cuda.synchronize()
                    times[it].append(st.elapsed_time(en))
            m0, m1 = float(np.median(times[0])), float(np.median(times[a.iters]))
            res["sizes"][str(n)] = {"refine_off_ms_median": m0, "refine_on_ms_median": m1, "added_ms": m1 - m0,
                                    "added_rel": (m1 - m0) / m0, "refine_off_ms": times[0], "refine_on_ms": times[a.iters]}
            print("N=%d: refine off %.3f ms, refine_iters=%d %.3f ms (+%.3f ms, %+.1f %%)" % (n, m0, a.iters, m1, m1 - m0,
                                                                                          100 * (m1 - m0) / m0), flush=True)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
