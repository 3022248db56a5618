"""AEDAT-3.1 recordings read on the device (csrc/events_aedat3_read.hip through event_read.read_events_aedat3,
ops.unpack_events_aedat3 and the command lines) against the restated reader (tests/events_aedat3_restated.py).  Files come from
tests/aedat3_stream_writer.py.  Everything is integer: every comparison is exact equality of the four columns and of info."""
import json
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

import aedat3_stream_writer as W
import aedat4_stream_writer as W4
import events_aedat3_restated as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HW = (48, 64)
SOURCES = {1: "TestSensor64x48"}                # no camera this reader knows: every read gives hw


@pytest.fixture(scope="module")
def er(gpu_ops):
    return import_module("spacecraft-pose-estimation_amd.event_read")


def check(er, data, what="", hw=HW, **kw):
    """The device read of `data` equals the restatement: columns (dtype and value) and info."""
    *want, info = R.read(data, hw=hw, **kw)
    *got, ginfo = er.read_events_aedat3(data, hw=hw, **kw)
    got = [c.cpu().numpy() for c in got]
    assert ginfo == info, (what, ginfo, info)
    for name, a, b in zip("txyp", got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0])
            raise AssertionError("%s: column %s differs first at row %d: %d != %d" % (what, name, i, a[i], b[i]))
    return want, info


def mask(pattern, n, seed=0):
    if pattern == "all":
        return np.ones(n, dtype=bool)
    if pattern == "none":
        return np.zeros(n, dtype=bool)
    if pattern == "alternating":
        return np.arange(n) % 2 == 0
    return np.random.default_rng(seed).random(n) < 0.6


SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "random"])
def test_packet_sizes_and_valid_patterns(er, pattern):
    cols = W.random_events(sum(SIZES), HW, 1)
    valid = mask(pattern, sum(SIZES), seed=2)
    data = W.write_aedat3(W.split(cols, SIZES, valid=valid, fillers=True), SOURCES)
    want, info = check(er, data, pattern)
    kept = int(valid.sum())
    assert info["n_events"] == kept and info["n_invalid"] == sum(SIZES) - kept and info["n_packets"] == len(SIZES)
    assert info["other_packets"] == {W.SPECIAL: 3, W.FRAME: 3, W.IMU6: 3} and info["hw"] == HW
    assert np.array_equal(want[1], cols[1][valid]) and np.array_equal(want[3], cols[3][valid])
    if kept:
        assert info["t0"] == cols[0][valid][0] and np.array_equal(want[0], cols[0][valid] - info["t0"])
    want, _ = check(er, data, pattern + ", no rebase", rebase=False)
    assert np.array_equal(want[0], cols[0][valid])
    for size, start in zip(SIZES, np.cumsum((0,) + SIZES[:-1])):         # each size alone, as the only packet of its file
        part = [c[start:start + size] for c in cols]
        check(er, W.write_aedat3(W.split(part, (size,), valid=valid[start:start + size]), SOURCES), "%s, %d alone" % (pattern, size))


@pytest.mark.parametrize("n_packets", [1, 255, 256, 257, 300])
def test_packet_counts_at_the_scan_tile_edges(er, n_packets):
    rng = np.random.default_rng(n_packets)
    counts = rng.integers(0, 9, n_packets)
    cols = W.random_events(int(counts.sum()), HW, 3)
    valid = mask("random", int(counts.sum()), seed=4)
    _, info = check(er, W.write_aedat3(W.split(cols, counts, valid=valid), SOURCES), "%d packets" % n_packets)
    assert info["n_packets"] == n_packets and info["n_events"] == int(valid.sum())


def test_long_runs_of_empty_packets(er):
    """More packets without a valid event in a row than one step of the scans takes: the first event and each packet's predecessor
    are still found.  Some of the empty packets hold events, all of them invalid."""
    counts = [0] * 300 + [3] + [0, 2] * 300 + [4, 0, 0, 5] + [0] * 20
    n = sum(counts)
    valid = np.zeros(n, dtype=bool)
    valid[:3] = True
    valid[-9:] = True
    cols = list(W.random_events(n, HW, 5))
    t = cols[0].copy()
    t[603] = t[2] - 1                                                     # a step back across the 600 packets in between
    t[n - 5] = t[n - 6] - 1                                               # and one across two
    cols[0] = t
    _, info = check(er, W.write_aedat3(W.split(cols, counts, valid=valid), SOURCES), "empty runs")
    assert info["n_backward"] == 2 and info["t0"] == t[0] and info["n_packets"] == len(counts) and info["n_events"] == 12
    _, info = check(er, W.write_aedat3(W.split([c[:0] for c in cols], [0] * 5), SOURCES), "no events at all")
    assert info["n_events"] == 0 and info["t0"] == 0
    check(er, W.write_aedat3([W.filler_packet(W.IMU6, 1, 2)], SOURCES), "no polarity packet at all")


def test_capacity_above_number_and_a_cut_off_tail(er):
    cols = W.random_events(40, HW, 6)
    tail = b"\xff" * 80                                                   # would be ten valid events at (32767, 32767) with ts -1
    packets = [W.polarity_packet(*(c[:10] for c in cols), tail=tail), W.polarity_packet(*(c[10:] for c in cols))]
    data = W.write_aedat3(packets, SOURCES)
    _, info = check(er, data, "garbage tail")
    assert info["n_events"] == 40
    _, info = check(er, data[:-1], "cut off")
    assert info["n_events"] == 10 and info["trailing_bytes"] == 28 + 30 * 8 - 1


def test_time_stamp_overflow(er):
    """eventTSOverflow 0 then 1 with ts wrapping from 2^31 - 1 to 0, and a packet deep into the overflow count."""
    top = (1 << 31) - 1
    t = np.array([top - 2, top - 1, top, top + 1, top + 2, (5 << 31) + 7, (5 << 31) + 8], dtype=np.int64)
    x, y, p = np.arange(7, dtype=np.int32), np.arange(7, dtype=np.int32) + 1, (np.arange(7) % 2).astype(np.int8)
    cols = (t, x, y, p)
    data = W.write_aedat3(W.split(cols, (3, 2, 2)), SOURCES)
    assert er.parse_aedat3(data).packet_overflow.tolist() == [0, 1, 5]
    want, info = check(er, data, "overflow")
    assert info["t0"] == top - 2 and info["n_backward"] == 0 and want[0].tolist() == (t - t[0]).tolist()
    want, _ = check(er, data, "overflow, no rebase", rebase=False)
    assert want[0].tolist() == t.tolist()
    stale = W.write_aedat3(W.split(cols, (3, 2, 2), overflow=0), SOURCES)   # the wrap without the overflow count: a step back
    _, info = check(er, stale, "stale overflow", rebase=False)
    assert info["n_backward"] == 1                                          # 2^31 - 1 -> 0; 1 -> 7 is forward again


def test_sensor_edges(er):
    t = np.arange(1, 7, dtype=np.int64)
    x = np.array([0, 63, 0, 63, 31, 5], dtype=np.int32)
    y = np.array([0, 0, 47, 47, 20, 7], dtype=np.int32)
    p = np.array([0, 1, 0, 1, 1, 0], dtype=np.int8)
    want, _ = check(er, W.write_aedat3(W.split((t, x, y, p), (6,)), SOURCES), "corners")
    assert want[1].tolist() == x.tolist() and want[2].tolist() == y.tolist()
    big = (np.array([32767, 0, 32767], dtype=np.int32), np.array([0, 32767, 32767], dtype=np.int32))
    want, info = check(er, W.write_aedat3(W.split((t[:3], *big, p[:3]), (3,)), SOURCES), "15-bit fields", hw=(32768, 32768))
    assert want[1].tolist() == [32767, 0, 32767] and want[2].tolist() == [0, 32767, 32767] and info["hw"] == (32768, 32768)
    for far_x, far_y in ((64, 0), (0, 48)):
        xx, yy = x.copy(), y.copy()
        xx[4], yy[4] = far_x, far_y
        data = W.write_aedat3(W.split((t, xx, yy, p), (4, 2)), SOURCES)
        with pytest.raises(ValueError, match="RANGE"):
            R.read(data, hw=HW)
        with pytest.raises(ValueError, match=r"outside the 64 x 48 sensor \(status RANGE\)"):
            er.read_events_aedat3(data, hw=HW)
        check(er, data, "large enough", hw=(49, 65))
    xx = x.copy()
    xx[4] = 64                                                            # out of range and invalid: dropped, not an error
    valid = np.array([1, 1, 1, 1, 0, 1], dtype=bool)
    _, info = check(er, W.write_aedat3(W.split((t, xx, y, p), (6,), valid=valid), SOURCES), "invalid and far")
    assert info["n_events"] == 5 and info["n_invalid"] == 1


def test_one_event_outside_the_sensor_is_tallied(er, gpu_ops):
    """A recording whose only polarity packet holds exactly one valid event, outside the sensor: one chunk, one lane with anything
    to add, so the tally's own barrier is all that orders the zeroing of its LDS pair before the one atomic."""
    import torch
    cols = (np.array([9], dtype=np.int64), np.array([64], dtype=np.int32), np.array([3], dtype=np.int32), np.array([1], dtype=np.int8))
    data = W.write_aedat3(W.split(cols, (1,)), SOURCES)
    with pytest.raises(ValueError, match=r"outside the 64 x 48 sensor \(status RANGE\)"):
        er.read_events_aedat3(data, hw=HW)
    ops, nat = gpu_ops, gpu_ops.nat
    head = er.parse_aedat3(data)
    pk = torch.from_numpy(np.stack([head.packet_offset, head.packet_events, head.packet_overflow], axis=1)).cuda()
    buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    ws = ops._query_bytes("events_aedat3_workspace_bytes", 1)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    cs = torch.empty(6, dtype=torch.int64, device="cuda")
    lib, P, S = nat.lib(), ops._ptr, ops._stream
    nat.check(lib.scpose_events_aedat3_count(P(buf), P(pk), 1, P(cs), P(work), ws, S()), "count")
    assert cs.tolist() == [1, 0, 9, 0, 0, 0]
    t = torch.empty(1, dtype=torch.int64, device="cuda")
    x, y, p = (torch.empty(1, dtype=d, device="cuda") for d in (torch.int32, torch.int32, torch.int8))
    nat.check(lib.scpose_events_aedat3_unpack(P(buf), P(pk), 1, HW[0], HW[1], 0, P(t), P(x), P(y), P(p), 1, P(cs), P(work), ws, S()),
              "unpack")
    assert cs.tolist() == [1, nat.AEDAT3_RANGE, 9, 0, 1, 0]              # n_backward 0, n_out_of_range 1
    assert (t.item(), x.item(), y.item(), p.item()) == (9, 64, 3, 1)


def test_backward_time_stamps_are_counted(er):
    cols = list(W.random_events(700, HW, 7))
    t = cols[0].copy()
    valid = np.ones(700, dtype=bool)
    t[100] = t[99] - 1                                                    # inside a wavefront
    t[128] = t[127] - 1                                                   # across two wavefronts
    t[256] = t[255] - 1                                                   # across two chunks of 256
    t[400] = t[399] - 1                                                   # across two packets
    valid[500:580] = False
    t[580] = t[499] - 1                                                   # across 80 invalid events
    t[581] = t[580] + 1
    t[540] = 0                                                            # invalid: not a step back
    cols[0] = t
    _, info = check(er, W.write_aedat3(W.split(cols, (400, 300), valid=valid), SOURCES), "backward")
    assert info["n_backward"] == int(np.count_nonzero(np.diff(t[valid]) < 0)) == 5


def test_status_words(er, gpu_ops):
    import torch
    cols = W.random_events(300, HW, 8)
    good = W.write_aedat3(W.split(cols, (100, 200)), SOURCES)
    check(er, good, "undamaged")
    for where, valid in ((150, None), (299, np.arange(300) < 290)):       # a negative ts on a valid and on an invalid event
        ts = cols[0] & 0x7FFFFFFF
        ts[where] = -5
        data = W.write_aedat3(W.split([c[:100] for c in cols], (100,)) + [
            W.polarity_packet(*(c[100:] for c in cols), ts=ts[100:], valid=None if valid is None else valid[100:])], SOURCES)
        with pytest.raises(ValueError, match="CORRUPT"):
            R.read(data, hw=HW)
        with pytest.raises(ValueError, match=r"negative time stamp.*\(status CORRUPT\)"):
            er.read_events_aedat3(data, hw=HW)
    for off in (-1, 1):
        data = W.write_aedat3([W.polarity_packet(*(c[:100] for c in cols)),
                               W.polarity_packet(*(c[100:] for c in cols), valid=np.arange(200) != 7, event_valid=199 + off)], SOURCES)
        with pytest.raises(ValueError, match="VALID_MISMATCH"):
            R.read(data, hw=HW)
        with pytest.raises(ValueError, match=r"do not add up to the eventValid.*\(status VALID_MISMATCH\)"):
            er.read_events_aedat3(data, hw=HW)
    # columns one row short, through the C ABI: CAPACITY, and the columns stay as they were
    ops, nat = gpu_ops, gpu_ops.nat
    head = er.parse_aedat3(good)
    pk = torch.from_numpy(np.stack([head.packet_offset, head.packet_events, head.packet_overflow], axis=1)).cuda()
    buf = torch.from_numpy(np.frombuffer(good, dtype=np.uint8).copy()).cuda()
    ws = ops._query_bytes("events_aedat3_workspace_bytes", 2)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    cs = torch.empty(6, dtype=torch.int64, device="cuda")
    lib, P, S = nat.lib(), ops._ptr, ops._stream
    nat.check(lib.scpose_events_aedat3_count(P(buf), P(pk), 2, P(cs), P(work), ws, S()), "count")
    assert cs.tolist()[:3] == [300, 0, int(cols[0][0])]
    t = torch.full((300,), -7, dtype=torch.int64, device="cuda")
    x = torch.full((300,), -7, dtype=torch.int32, device="cuda")
    y, p = x.clone(), torch.full((300,), -7, dtype=torch.int8, device="cuda")
    nat.check(lib.scpose_events_aedat3_unpack(P(buf), P(pk), 2, HW[0], HW[1], 1, P(t), P(x), P(y), P(p), 299, P(cs), P(work), ws, S()),
              "unpack")
    assert cs.tolist()[1] == nat.AEDAT3_CAPACITY
    for col in (t, x, y, p):
        assert bool((col == -7).all())
    check(er, good, "still fine")                                          # the device is in order after all of that


def test_two_runs_are_bitwise_equal(er):
    cols = W.random_events(5000, HW, 9)
    valid = mask("random", 5000, seed=10)
    data = W.write_aedat3(W.split(cols, (1000, 0, 2500, 1500), valid=valid, fillers=True), SOURCES)
    *a, ia = er.read_events_aedat3(data, hw=HW)
    *b, ib = er.read_events_aedat3(data, hw=HW)
    assert ia == ib
    for u, v in zip(a, b):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


def test_two_sources_and_the_camera_name(er):
    a, b = W.random_events(90, (260, 346), 11), W.random_events(70, (180, 240), 12)
    pa, pb = W.split(a, (40, 50), source=1), W.split(b, (30, 40), source=2)
    data = W.write_aedat3([pa[0], pb[0], pa[1], pb[1]], {1: "DAVIS346B", 2: "DAVIS240C"})
    want, info = check(er, data, "source 2", hw=None, source=2)
    assert info["hw"] == (180, 240) and info["sources"] == (2,) and info["n_events"] == 70 and np.array_equal(want[1], b[1])
    _, info = check(er, data, "source 1", hw=None, source=1)
    assert info["hw"] == (260, 346) and info["n_events"] == 90
    with pytest.raises(er.UnsupportedAedat3, match="sources 1, 2 all carry polarity packets"):
        er.read_events_aedat3(data)


# ------------------------------------------------------------------ command lines
def run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "v2e", script), *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """A DVS128 recording of 3000 events over 50 ms named like a 2.0 file, some events invalid, next to an AEDAT-4.0 recording of
    the events it keeps and the CSV text of those."""
    d = tmp_path_factory.mktemp("aedat3")
    rng = np.random.default_rng(13)
    t = 5_000_000 + np.sort(rng.integers(0, 50000, 3000)).astype(np.int64)
    x, y, p = rng.integers(0, 128, 3000), rng.integers(0, 128, 3000), rng.integers(0, 2, 3000)
    valid = rng.random(3000) < 0.9
    path = d / "rec.aedat"
    path.write_bytes(W.write_aedat3(W.split((t, x, y, p), (1000, 0, 1500, 500), valid=valid, fillers=True), {1: "DVS128"}))
    t, x, y, p = t[valid], x[valid], y[valid], p[valid]
    four = d / "rec.aedat4"
    four.write_bytes(W4.write_aedat4([(0, W4.evts_payload(t, x, y, p))], {0: ("EVTS", 128, 128)}, W4.NONE))
    text = "".join("%d,%d,%d,%d\n" % row for row in zip(t - t[0], x, y, p))
    return path, four, text


def test_aedat_to_csv_writes_the_same_bytes_as_for_the_4_0_recording(gpu_ops, recording):
    path, four, text = recording
    out3, out4 = path.parent / "out3.csv", path.parent / "out4.csv"
    r = run("aedat_to_csv.py", "--events_file", str(path), "--output_file", str(out3))
    assert r.returncode == 0, r.stderr
    r = run("aedat_to_csv.py", "--events_file", str(four), "--output_file", str(out4))
    assert r.returncode == 0, r.stderr
    assert out3.read_bytes() == out4.read_bytes() == text.encode()
    r = run("aedat_to_csv.py", "--events_file", str(path), "--output_file", str(out3), "--width", "100", "--height", "128")
    assert r.returncode != 0 and "outside the 100 x 128 sensor" in r.stderr


def test_e2v_renders_the_same_frames_from_aedat3_and_csv(gpu_ops, recording):
    path, _, text = recording
    csv = path.parent / "events.csv"
    csv.write_text(text)
    a, b = path.parent / "from_aedat3", path.parent / "from_csv"
    r = run("e2v.py", "--events_file", str(path), "--dvs_exposure", "duration", "10000", "--output_folder", str(a))
    assert r.returncode == 0, r.stderr
    r = run("e2v.py", "--events_file", str(csv), "--dvs_exposure", "duration", "10000", "--output_folder", str(b), "--output_width", "128",
            "--output_height", "128")
    assert r.returncode == 0, r.stderr
    names = sorted(os.listdir(a / "event-frames"))
    assert names == sorted(os.listdir(b / "event-frames")) and len(names) >= 4
    for name in names:
        assert (a / "event-frames" / name).read_bytes() == (b / "event-frames" / name).read_bytes(), name
    r = run("e2v.py", "--events_file", str(path), "--swap_xy", "--output_folder", str(a))
    assert r.returncode != 0 and "--swap_xy" in r.stderr and "AEDAT-3.1" in r.stderr


def test_events_convert_takes_a_3_1_input(gpu_ops, recording):
    path, _, text = recording
    out = path.parent / "converted.csv"
    r = run("events_convert.py", "--events_file", str(path), "--output", str(out))
    assert r.returncode == 0, r.stderr
    assert out.read_text() == text
    r = run("events_convert.py", "--events_file", str(path), "--output", str(out), "--aedat_layout", "v2e")
    assert r.returncode != 0 and "AEDAT-3.1" in r.stderr


def test_convert_aedats_takes_a_scene_with_only_a_3_1_file(gpu_ops, recording):
    path, _, _ = recording
    scenes = path.parent / "scenes"
    os.makedirs(scenes / "s0")
    (scenes / "s0" / "rec.aedat").write_bytes(path.read_bytes())
    calib = path.parent / "calib.json"
    calib.write_text(json.dumps({"intrinsics": {"camera_matrix": [[120.0, 0, 64.0], [0, 120.0, 64.0], [0, 0, 1.0]],
                                                "distortion_coefficients": [-0.1, 0.01, 0.0, 0.0, 0.0]}}))
    r = run("convert_aedats.py", "--scenes_dir", str(scenes), "--calibration_file_path", str(calib), "--image_height", "128",
            "--image_width", "128")
    assert r.returncode == 0, r.stderr
    assert "s0: " in r.stdout
    frames = sorted(os.listdir(scenes / "s0" / "event-frames"))
    assert len(frames) >= 4 and frames == sorted(os.listdir(scenes / "s0" / "event-frames-distorted"))
