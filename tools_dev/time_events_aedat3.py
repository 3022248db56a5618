#!/usr/bin/env python3
"""Times the AEDAT-3.1 reader on synthetic DAVIS346 recordings: file -> columns (event_read.read_events_aedat3, upload included),
its two calls alone between HIP events (count + the count scan, unpack), the share of the device's copy bandwidth the two calls
reach, and the same events through the AEDAT-4.0 reader (NONE packets) and through the NumPy restatement on the host.

    python tools_dev/time_events_aedat3.py [--events 1000000 10000000 50000000] [--packet 4096 512]
                                           [--out profiles/events_aedat3_timing.json]

The recordings come from the tests' writer (tests/aedat3_stream_writer.py: its header and its event words; the packet headers are
laid out in one NumPy array, and the first packet is compared with the writer's own bytes), all events valid.  Bytes: count reads 8 B per event; unpack reads 8 B and
writes 17 B per event.  The copy reference is a device-to-device copy that moves as many bytes in all (read + written) as the
call it is compared with, timed in the same run: share = copy time / call time.  Warm-up runs, then the median and the minimum of
--repeats runs."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, warmup, repeats, sync):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "repeats": repeats}


def timed_device(fn, warmup, repeats, torch):
    """The same with HIP events on the current stream around fn: device time between them, not the host's launch and wait."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "repeats": repeats, "clock": "HIP events"}


def recording(W, np, cols, per):
    """The bytes of an AEDAT-3.1 recording of the events, `per` of them in each polarity packet (all valid, source 1)."""
    n = len(cols[0])
    assert n % per == 0 and int(cols[0][-1]) < 1 << 31
    data, ts = W.polarity_words(*cols)
    body = np.zeros(n // per, dtype=[("head", "<i2", 2), ("fields", "<i4", 6), ("ev", "<u4", (per, 2))])
    body["head"] = (W.POLARITY, 1)
    body["fields"] = (8, 4, 0, per, per, per)                       # eventSize, eventTSOffset, eventTSOverflow, capacity, number, valid
    body["ev"][:, :, 0] = data.reshape(-1, per)
    body["ev"][:, :, 1] = ts.astype(np.uint32).reshape(-1, per)
    out = W.header({1: "DAVIS346"}) + body.tobytes()
    first = W.polarity_packet(*(c[:per] for c in cols))
    assert out[len(W.header({1: "DAVIS346"})):][:len(first)] == first
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, nargs="+", default=[1_000_000, 10_000_000, 50_000_000])
    ap.add_argument("--packet", type=int, nargs="+", default=[4096, 512])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import scpose  # noqa: F401
    from importlib import import_module
    import aedat3_stream_writer as W
    import aedat4_stream_writer as W4
    import events_aedat3_restated as R
    er = import_module("spacecraft-pose-estimation_amd.event_read")
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    nat = ops.nat
    hw = (260, 346)
    sync = torch.cuda.synchronize
    lib, P, S = nat.lib(), ops._ptr, ops._stream
    result = {"device": torch.cuda.get_device_name(0), "sensor": [346, 260], "bytes_per_event": {"count": 8, "unpack": 25},
              "recordings": []}

    def copy_ms(traffic):
        """A device-to-device copy that reads and writes `traffic` bytes in all."""
        src = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda").fill_(1)
        dst = torch.empty_like(src)
        return timed_device(lambda: dst.copy_(src), args.warmup, args.repeats, torch)

    for events in args.events:
        for per in args.packet:
            n_ev = events // per * per
            cols = W.random_events(n_ev, hw, seed=0, step=40)
            data = recording(W, np, cols, per)
            row = {"events": n_ev, "events_per_packet": per, "packets": n_ev // per, "file_bytes": len(data)}
            row["read_events_aedat3"] = timed(lambda: er.read_events_aedat3(data), args.warmup, args.repeats, sync)
            t, x, y, p, info = er.read_events_aedat3(data)
            assert info["n_events"] == n_ev and info["n_backward"] == 0
            assert np.array_equal(t.cpu().numpy(), cols[0] - cols[0][0]) and np.array_equal(x.cpu().numpy(), cols[1])
            del t, x, y, p
            # the two calls one by one, on the uploaded file
            head = er.parse_aedat3(data)
            pk = torch.from_numpy(np.stack([head.packet_offset, head.packet_events, head.packet_overflow], axis=1)).cuda()
            buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
            n = int(pk.shape[0])
            ws = ops._query_bytes("events_aedat3_workspace_bytes", n)
            work = torch.empty(ws, dtype=torch.uint8, device="cuda")
            cs = torch.empty(6, dtype=torch.int64, device="cuda")
            count = lambda: nat.check(lib.scpose_events_aedat3_count(P(buf), P(pk), n, P(cs), P(work), ws, S()))
            count()
            rows = int(cs.tolist()[0])
            assert rows == n_ev, (rows, cs.tolist())
            tc, xc, yc, pc = ops._empty_event_columns(rows, buf.device)
            unpack = lambda: nat.check(lib.scpose_events_aedat3_unpack(P(buf), P(pk), n, hw[0], hw[1], 1, P(tc), P(xc), P(yc), P(pc), rows,
                                                                       P(cs), P(work), ws, S()))
            calls = {}
            for name, fn, per_event in (("count", count, 8), ("unpack", unpack, 25)):
                count()                                                  # a fresh count_status: the counters of unpack add up otherwise
                c = timed_device(fn, args.warmup, args.repeats, torch)
                ref = copy_ms(per_event * n_ev)
                c.update(events_per_s=n_ev / (c["median_ms"] * 1e-3), gbytes_per_s=per_event * n_ev / (c["median_ms"] * 1e-3) / 1e9,
                         copy_same_bytes_median_ms=ref["median_ms"], copy_gbytes_per_s=per_event * n_ev / (ref["median_ms"] * 1e-3) / 1e9,
                         share_of_copy_bandwidth=ref["median_ms"] / c["median_ms"])
                calls[name] = c
            row["calls"] = calls
            row["upload"] = timed(lambda: torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda(), args.warmup, args.repeats,
                                  sync)
            row["parse_aedat3_host"] = timed(lambda: er.parse_aedat3(data), 1, 3, lambda: None)
            row["read_events_aedat3"]["events_per_s"] = n_ev / (row["read_events_aedat3"]["median_ms"] * 1e-3)
            del buf, tc, xc, yc, pc, work
            if per == args.packet[0]:                                    # the other two routes once per size
                four = W4.write_aedat4([(0, W4.evts_payload(*(c[k:k + per] for c in cols))) for k in range(0, n_ev, per)],
                                       {0: ("EVTS", 346, 260)}, W4.NONE)
                row["read_events_aedat4_none"] = timed(lambda: er.read_events_aedat4(four), args.warmup, args.repeats, sync)
                row["read_events_aedat4_none"]["events_per_s"] = n_ev / (row["read_events_aedat4_none"]["median_ms"] * 1e-3)
                row["read_events_aedat4_none"]["file_bytes"] = len(four)
                del four
                row["numpy_restatement_host"] = timed(lambda: R.read(data), 0, 2 if n_ev > 20_000_000 else 3, lambda: None)
                row["numpy_restatement_host"]["events_per_s"] = n_ev / (row["numpy_restatement_host"]["median_ms"] * 1e-3)
            result["recordings"].append(row)
            print(json.dumps(row), flush=True)
            del data, cols
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
