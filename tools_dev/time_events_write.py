#!/usr/bin/env python3
"""Times the device event writers (csrc/events_write.hip, event_write.py) against the Python loop they replace and writes
profiles/events_write_timing.json.

    python tools_dev/time_events_write.py                 # the whole table: one child process per row
    python tools_dev/time_events_write.py --row NAME      # one row, one JSON line on stdout (what the children run)

Workload: 3 000 000 events of a 640 x 480 sensor, the size profiles/events_csv_timing.json uses.  Rows:
    text_space, text_comma, aedat2     columns -> bytes on the device: kernels only (HIP events around the C ABI calls on
                                       preallocated buffers) and with the read-back (the ops call plus .cpu()); columns -> file
                                       through the chunked writer (default chunk size, wall clock, file in --dir)
    parent_write_text                  the body of v2e/v2e.py:write_text before the device writer: four .cpu().numpy() copies
                                       and `"%d %d %d %d\\n" % row` per event, restated here
    parent_pandas_to_csv               pandas.DataFrame.to_csv(index=False, header=False) on the same host columns, where pandas
                                       imports
    csv_parse                          the device reader's kernels on the text_space / text_comma bytes (criterion C3)
Every figure is the median of 9 after 3 warm-ups.  Each child runs under its own `timeout -k 10`; the first failure stops the
table.  Criteria, as ratios: C1 new columns -> file below the parent's on every row; C2 the share of the HBM floor
((17 B read + bytes written per row) at 6.29 TB/s) the kernels reach; C3 format kernels over parse kernels on the same text.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, HW = 3000000, (480, 640)
WARMUP, REPS = 3, 9
HBM = 6.29e12
ROWS = ("text_space", "text_comma", "aedat2", "parent_write_text", "parent_pandas_to_csv", "csv_parse")
LIMIT_S = {"parent_write_text": 240, "parent_pandas_to_csv": 300}


def columns():
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    t = np.sort(rng.integers(0, 30000000, N)).astype(np.int64)
    cols = (t, rng.integers(0, HW[1], N).astype(np.int32), rng.integers(0, HW[0], N).astype(np.int32), rng.integers(0, 2, N).astype(np.int8))
    return tuple(torch.from_numpy(c).cuda() for c in cols)


def median_us(fn, sync=None):
    out = []
    for k in range(WARMUP + REPS):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        if k >= WARMUP:
            out.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(out), 1), [round(v, 1) for v in out]


def device_us(launch):
    """Median device time of launch() between two HIP events on the current stream."""
    import torch
    out = []
    for k in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        launch()
        b.record()
        b.synchronize()
        if k >= WARMUP:
            out.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(out), 1), [round(v, 1) for v in out]


def run_row(row, folder):
    import torch
    import scpose  # noqa: F401
    from importlib import import_module
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    ew = import_module("spacecraft-pose-estimation_amd.event_write")
    lib, ptr = ops.nat.lib(), lambda x: ctypes.c_void_p(x.data_ptr())
    t, x, y, p = columns()
    sync = torch.cuda.synchronize
    res = {"row": row, "events": N}
    path = os.path.join(folder, "events_write_timing." + row)
    seps = {"text_space": " ", "text_comma": ","}
    if row in seps or row == "csv_parse":
        ws = ctypes.c_size_t()
        ops.nat.check(lib.scpose_events_text_workspace_bytes(N, ctypes.byref(ws)))
        work = torch.empty(ws.value, dtype=torch.uint8, device="cuda")
        cs = torch.empty(2, dtype=torch.int64, device="cuda")
    if row in seps:
        sep = seps[row]
        n_bytes = int(ops.format_events_text(t, x, y, p, sep=sep).numel())
        out = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")

        def kernels():
            ops.nat.check(lib.scpose_events_text_measure(ptr(t), ptr(x), ptr(y), ptr(p), N, ptr(cs), ptr(work), ws.value, ops._stream()))
            ops.nat.check(lib.scpose_events_text_emit(ptr(t), ptr(x), ptr(y), ptr(p), N, ord(sep), 0, ptr(out), n_bytes, ptr(cs), ptr(work),
                                                      ws.value, ops._stream()))
        res["bytes"] = n_bytes
        res["kernels_us"], res["kernels_samples_us"] = device_us(kernels)
        res["emit_only_us"] = device_us(lambda: ops.nat.check(lib.scpose_events_text_emit(
            ptr(t), ptr(x), ptr(y), ptr(p), N, ord(sep), 0, ptr(out), n_bytes, ptr(cs), ptr(work), ws.value, ops._stream())))[0]
        res["to_host_us"], _ = median_us(lambda: ops.format_events_text(t, x, y, p, sep=sep).cpu(), sync)
        res["to_file_us"], res["to_file_samples_us"] = median_us(lambda: ew.write_events_text(path, t, x, y, p, sep=sep), sync)
        res["hbm_floor_us"] = round((17.0 * N + n_bytes) / HBM * 1e6, 1)
    elif row == "aedat2":
        out = torch.empty(8 * N, dtype=torch.uint8, device="cuda")
        cs3 = torch.empty(3, dtype=torch.int64, device="cuda")
        res["bytes"] = 8 * N
        res["kernels_us"], res["kernels_samples_us"] = device_us(lambda: ops.nat.check(lib.scpose_events_aedat2_pack(
            ptr(t), ptr(x), ptr(y), ptr(p), N, HW[0], HW[1], ptr(out), ptr(cs3), ops._stream())))
        res["to_host_us"], _ = median_us(lambda: ops.pack_events_aedat2(t, x, y, p, HW)[0].cpu(), sync)
        res["to_file_us"], res["to_file_samples_us"] = median_us(lambda: ew.write_events_aedat2(path, t, x, y, p, HW), sync)
        res["hbm_floor_us"] = round((17.0 * N + 8.0 * N) / HBM * 1e6, 1)
    elif row == "parent_write_text":
        def parent():
            th, xh, yh, ph = t.cpu().numpy(), x.cpu().numpy(), y.cpu().numpy(), p.cpu().numpy()
            with open(path, "w") as f:
                for r in zip(th.tolist(), xh.tolist(), yh.tolist(), ph.tolist()):
                    f.write("%d %d %d %d\n" % r)
        res["to_file_us"], res["to_file_samples_us"] = median_us(parent, sync)
    elif row == "parent_pandas_to_csv":
        try:
            import pandas as pd
        except ImportError:
            res["skipped"] = "pandas does not import"
            return res
        def parent():
            pd.DataFrame({"t": t.cpu().numpy(), "x": x.cpu().numpy(), "y": y.cpu().numpy(), "p": p.cpu().numpy()}).to_csv(
                path, index=False, header=False)
        res["to_file_us"], res["to_file_samples_us"] = median_us(parent, sync)
    elif row == "csv_parse":
        for name, sep in seps.items():
            text = ops.format_events_text(t, x, y, p, sep=sep)
            nb = int(text.numel())
            w2 = ctypes.c_size_t()
            ops.nat.check(lib.scpose_events_csv_workspace_bytes(nb, ctypes.byref(w2)))
            work2 = torch.empty(w2.value, dtype=torch.uint8, device="cuda")
            cols = (torch.empty_like(t), torch.empty_like(x), torch.empty_like(y), torch.empty_like(p))
            res[name + "_parse_kernels_us"] = device_us(lambda: ops.nat.check(lib.scpose_events_csv_parse(
                ptr(text), nb, int(sep == " "), 0, ctypes.c_double(0.0), ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), ptr(cols[3]), N, ptr(cs),
                ptr(work2), w2.value, ops._stream())))[0]
            assert cs.tolist() == [N, 0] and all(torch.equal(a, b) for a, b in zip(cols, (t, x, y, p)))
    if os.path.exists(path):
        res["file_bytes"] = os.path.getsize(path)
        os.remove(path)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--row", choices=ROWS, default=None)
    ap.add_argument("--dir", default=None, help="where the timed files go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_write_timing.json"))
    args = ap.parse_args()
    if args.row:
        with tempfile.TemporaryDirectory(dir=args.dir) as d:
            print(json.dumps(run_row(args.row, d)))
        return 0
    rows = {}
    for row in ROWS:
        cmd = ["timeout", "-k", "10", str(LIMIT_S.get(row, 120)), sys.executable, os.path.abspath(__file__), "--row", row]
        if args.dir:
            cmd += ["--dir", args.dir]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("time_events_write: row %s ended with status %d; nothing after it was run" % (row, r.returncode))
        rows[row] = json.loads(r.stdout.strip().splitlines()[-1])
        print(row, {k: v for k, v in rows[row].items() if not k.endswith("samples_us")}, flush=True)
    parents = [rows[k]["to_file_us"] for k in ("parent_write_text", "parent_pandas_to_csv") if "to_file_us" in rows[k]]
    new = ("text_space", "text_comma", "aedat2")
    result = {
        "events": N, "hw": list(HW), "warmup": WARMUP, "reps": REPS, "hbm_bytes_per_s": HBM, "rows": rows,
        "C1_parent_over_new_to_file": {k: round(min(parents) / rows[k]["to_file_us"], 2) for k in new},
        "C1_new_below_parent_on_every_row": all(rows[k]["to_file_us"] < min(parents) for k in new),
        "C2_hbm_floor_share_of_kernels": {k: round(rows[k]["hbm_floor_us"] / rows[k]["kernels_us"], 3) for k in new},
        "C3_format_kernels_over_parse_kernels": {k: round(rows[k]["kernels_us"] / rows["csv_parse"][k + "_parse_kernels_us"], 3)
                                                 for k in ("text_space", "text_comma")},
    }
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
