"""Cost of decoding AEDAT-2.0 records on the device (scpose_events_aedat2_unpack), from bytes on the device to columns on the device.

    python tools_dev/time_events_aedat2_read.py [--records 16777216] [--reps 9] [--out profiles/events_aedat2_read_timing.json]

Three rows on the same bytes, 346 x 260, DAVIS layout:
    device   the three launches of scpose_events_aedat2_unpack on preallocated columns and workspace (no allocation and no
             read-back inside the timed region), for a stream of polarity events only and for the mix of about 30 % bit-31 and
             5 % bit-10 records; the columns are compared with the restatement once, before anything is timed
    host     the NumPy restatement (tests/events_aedat2_read_restated.py) on the same bytes
    copy     a plain device-to-device copy of 33 bytes per record: the traffic floor (16 B read and 17 B written per record by
             the decoder; the copy reads 33 and writes 33, so its GB/s counts both directions and so does the decoder's)
Every device point: 3 warm-up calls, then --reps calls timed one by one with device events; the JSON holds the medians and the
samples.  GB/s of the decoder: (16 * n + 17 * kept) bytes over the median."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import scpose  # noqa: F401
    from importlib import import_module
    import events_aedat2_read_restated as R
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    nat = ops.nat; lib = nat.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n, hw = a.records, (260, 346)
    P = lambda v: ctypes.c_void_p(v.data_ptr())                       # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "records": n, "reps": a.reps, "warmup": 3, "points": []}

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), ms

    ws = ctypes.c_size_t()
    nat.check(lib.scpose_events_aedat2_unpack_workspace_bytes(n, ctypes.byref(ws)), "workspace_bytes")
    work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
    t = torch.empty(n, dtype=torch.int64, device=dev); x = torch.empty(n, dtype=torch.int32, device=dev)
    y = torch.empty(n, dtype=torch.int32, device=dev); p = torch.empty(n, dtype=torch.int8, device=dev)
    cs = torch.empty(6, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.empty(33 * n, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    copy_ms, copy_samples = timed(lambda: dst.copy_(src))
    res["copy_33_bytes_per_record"] = {"ms": copy_ms, "samples_ms": copy_samples, "gb_per_s_read_plus_write": 2 * 33 * n / copy_ms / 1e6}
    del src, dst
    for pattern in ("all", "mix"):
        aw, u = R.stream(n, hw, pattern, seed=1, t0=2 ** 32 - 5000)
        body = R.records(aw, u)
        t0 = time.perf_counter()
        want, info, status = R.unpack(body, hw)
        host_ms = (time.perf_counter() - t0) * 1e3
        buf = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).to(dev)

        def call():
            nat.check(lib.scpose_events_aedat2_unpack(P(buf), n, hw[0], hw[1], nat.AEDAT2_LAYOUT_DAVIS, 1, 1, 1, ctypes.c_double(0.0),
                                                      P(t), P(x), P(y), P(p), n, P(cs), P(work), ws.value, stream), "unpack")
        call()
        got = cs.tolist()
        k = info["n_events"]
        assert status == 0 and got == [k, 0, info["n_other"], info["n_special"], info["n_wraps"], info["n_backward"]], (got, info)
        for d, h in zip((t, x, y, p), want):
            assert np.array_equal(d[:k].cpu().numpy(), h)
        ms, samples = timed(call)
        moved = 16 * n + 17 * k
        res["points"].append({"pattern": pattern, "kept": k, "device_ms": ms, "device_samples_ms": samples, "bytes_moved": moved,
                              "device_gb_per_s": moved / ms / 1e6, "share_of_copy": (moved / ms) / (2 * 33 * n / copy_ms),
                              "host_numpy_ms": host_ms, "records_per_s_device": n / ms * 1e3})
        print(json.dumps(res["points"][-1]), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
