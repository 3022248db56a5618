"""AEDAT-4.0 recordings read on the device (csrc/events_aedat4_read.hip through event_read.read_events_aedat4,
ops.unpack_events_aedat4 and the command lines) against the restated reader (tests/events_aedat4_restated.py).  Files come from
tests/aedat4_stream_writer.py.  Everything is integer: every comparison is exact equality of the four columns and of info."""
import json
import os
import struct
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

import aedat4_stream_writer as W
import events_aedat4_restated as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HW = (48, 64)
STREAMS = {0: ("EVTS", 64, 48), 1: ("FRME", 64, 48), 2: ("IMUS", None, None), 3: ("EVTS", 64, 48)}
HEAD = 36                                      # a size-prefixed event payload: the first struct's position


@pytest.fixture(scope="module")
def er(gpu_ops):
    return import_module("spacecraft-pose-estimation_amd.event_read")


def check(er, data, what="", **kw):
    """The device read of `data` equals the restatement: columns (dtype and value) and info."""
    *want, info = R.read(data, **kw)
    *got, ginfo = er.read_events_aedat4(data, **kw)
    got = [c.cpu().numpy() for c in got]
    assert ginfo == info, (what, ginfo, info)
    for name, a, b in zip("txyp", got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0])
            raise AssertionError("%s: column %s differs first at row %d: %d != %d" % (what, name, i, a[i], b[i]))
    return want, info


def split(cols, counts, sid=0, prefixed=True, fillers=True):
    """[(stream, payload)]: the columns cut into event packets of `counts` events, filler packets of other streams between them."""
    packets, at = [], 0
    for k, c in enumerate(counts):
        packets.append((sid, W.evts_payload(*(col[at:at + c] for col in cols), prefixed=prefixed, omit_empty=k % 2 == 1)))
        if fillers:
            packets.append((1 + k % 2, W.filler_payload("FRME" if k % 2 == 0 else "IMUS", 60 + 13 * (k % 7), seed=k)))
        at += c
    assert at == len(cols[0])
    return packets


def zero_led(n_zero, n_rest, seed=0):
    """n_zero events that are all zero bytes (t = x = y = p = 0), then n_rest random ones with small increasing time stamps: a run
    of 16 * n_zero zero bytes from HEAD on, in which every offset and every match length is a valid LZ4 match."""
    t, x, y, p = W.random_events(n_rest, HW, seed, t_start=1, step=300)
    z = np.zeros(n_zero, dtype=np.int64)
    return (np.concatenate([z, t]), np.concatenate([z.astype(np.int32), x]), np.concatenate([z.astype(np.int32), y]),
            np.concatenate([z.astype(np.int8), p]))


def plan(sequences, start=0):
    """[(literal run, match length, offset)] from `start` on -> the matches of lz4_block_planned."""
    matches, at = [], start
    for lit, ml, off in sequences:
        matches.append((at + lit, off, ml))
        at += lit + ml
    return matches


@pytest.mark.parametrize("compression", [W.NONE, W.LZ4])
@pytest.mark.parametrize("prefixed", [True, False])
def test_packet_sizes(er, compression, prefixed):
    counts = (0, 1, 63, 64, 65, 0, 7)
    cols = W.random_events(sum(counts), HW, 1)
    data = W.write_aedat4(split(cols, counts, prefixed=prefixed), STREAMS, compression, ftab=prefixed)
    want, info = check(er, data, "sizes")
    assert info["n_events"] == 200 and info["n_packets"] == 7 and info["hw"] == HW and info["t0"] == cols[0][0]
    assert np.array_equal(want[0], cols[0] - cols[0][0]) and np.array_equal(want[1], cols[1])
    want, _ = check(er, data, "no rebase", rebase=False)
    assert np.array_equal(want[0], cols[0])
    check(er, data, "hw given", hw=(50, 70))


@pytest.mark.parametrize("compression", [W.NONE, W.LZ4_HIGH])
def test_300_packets(er, compression):
    rng = np.random.default_rng(2)
    counts = rng.integers(0, 12, 300)
    cols = W.random_events(int(counts.sum()), HW, 2)
    data = W.write_aedat4(split(cols, counts, fillers=False), STREAMS, compression)
    _, info = check(er, data, "300 packets")
    assert info["n_packets"] == 300 and info["n_events"] == counts.sum()


def test_two_event_streams_and_stream_selection(er):
    a, b = W.random_events(90, HW, 3), W.random_events(70, HW, 4, t_start=1_600_000_000_000_500)
    pa, pb = split(a, (40, 50), sid=0), split(b, (30, 40), sid=3)
    packets = [pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3]]
    for compression in (W.NONE, W.LZ4):
        data = W.write_aedat4(packets, STREAMS, compression)
        _, info = check(er, data, "both")
        assert info["n_events"] == 160 and info["streams"] == (0, 3) and info["n_backward"] > 0
        want, info = check(er, data, "stream 3", stream=3)
        assert info["n_events"] == 70 and info["streams"] == (3,) and np.array_equal(want[1], b[1])
        want, info = check(er, data, "stream 0", stream=0)
        assert info["n_events"] == 90 and info["n_backward"] == 0
    with pytest.raises(er.UnsupportedAedat4, match="no event stream 1"):
        er.read_events_aedat4(data, stream=1)


def test_dictated_sequences(er):
    """Literal runs of 14, 15, 270, 271; match lengths 4, 18, 19, 273, 274; offsets 1, 2, 3, 63, 64, 65: all inside the zero run."""
    cols = zero_led(90, 30)
    payload = W.evts_payload(*cols)
    seqs = [(271, 4, 1), (14, 18, 2), (15, 19, 3), (270, 273, 63), (14, 274, 64), (15, 4, 65)]
    matches = plan(seqs)
    assert matches[0][0] - matches[0][1] >= HEAD and matches[-1][0] + matches[-1][2] <= HEAD + 16 * 90
    frame = W.lz4_frame(payload, plans={0: matches})
    assert R.lz4_frame(frame) == payload
    data = W.write_aedat4([(0, payload)], STREAMS, W.LZ4, compress=lambda k, pl: frame)
    _, info = check(er, data, "dictated")
    assert info["n_events"] == 120


@pytest.mark.parametrize("flags", [{}, {"block_checksum": True}, {"content_checksum": True}, {"content_size": True},
                                   {"block_checksum": True, "content_checksum": True, "content_size": True}, {"linked": False},
                                   {"stored": True}, {"stored": True, "block_checksum": True, "content_checksum": True},
                                   {"stored": (1,), "block_bytes": 700}, {"block_code": 7, "content_checksum": True}])
def test_frame_flags(er, flags):
    cols = W.random_events(150, HW, 5)
    kw = dict(flags)
    kw.setdefault("block_bytes", 1000)
    data = W.write_aedat4(split(cols, (100, 50)), STREAMS, W.LZ4, compress=lambda k, pl: W.lz4_frame(pl, **kw))
    _, info = check(er, data, str(flags))
    assert info["n_events"] == 150
    check(er, data, "unverified", verify=False)


def test_match_across_a_linked_block_boundary(er):
    cols = zero_led(100, 20)
    payload = W.evts_payload(*cols)
    frame = W.lz4_frame(payload, block_bytes=1000, plans={1: [(1000, 10, 40), (1100, 900, 30)]})
    assert R.lz4_frame(frame) == payload
    check(er, W.write_aedat4([(0, payload)], STREAMS, W.LZ4, compress=lambda k, pl: frame), "linked")
    with pytest.raises(ValueError, match="CORRUPT"):                      # the same block in a frame of independent blocks
        er.read_events_aedat4(W.write_aedat4([(0, payload)], STREAMS, W.LZ4, compress=lambda k, pl: W.lz4_frame(
            payload, block_bytes=1000, linked=False, overrides={1: W.lz4_block_planned(payload, 1000, 2000, [(1000, 10, 40)])})))


def test_5000_events_in_one_packet(er):
    """80 KB: two 64 KiB blocks; in the second a match at offset 10 into the first block and one at offset 65535, whose source
    lies where a 64 KiB ring would already have wrapped."""
    cols = zero_led(4200, 800, seed=6)
    payload = W.evts_payload(*cols)
    assert len(payload) == HEAD + 80000
    frame = W.lz4_frame(payload, content_checksum=True, plans={1: [(65536, 10, 40), (65636, 65535, 50)]})
    assert R.lz4_frame(frame) == payload
    _, info = check(er, W.write_aedat4([(0, payload)], STREAMS, W.LZ4, compress=lambda k, pl: frame), "5000 planned")
    assert info["n_events"] == 5000
    cols = W.random_events(5000, HW, 7)
    for compression in (W.NONE, W.LZ4):
        check(er, W.write_aedat4(split(cols, (5000,)), STREAMS, compression), "5000 greedy")


def test_long_runs_of_empty_packets(er):
    """More empty packets in a row than one step of the scans takes: the first event and each packet's predecessor are still found."""
    counts = [0] * 300 + [3] + [0] * 600 + [4, 0, 0, 5] + [0] * 20
    cols = list(W.random_events(12, HW, 10))
    cols[0] = cols[0].copy()
    cols[0][3] = cols[0][2] - 1                                           # a step back across the 600 empty packets
    cols[0][7] = cols[0][6] - 1                                           # and one across two
    for compression in (W.NONE, W.LZ4):
        _, info = check(er, W.write_aedat4(split(cols, counts, fillers=False), STREAMS, compression), "empty runs")
        assert info["n_backward"] == 2 and info["t0"] == cols[0][0] and info["n_packets"] == len(counts)
    check(er, W.write_aedat4(split([c[:0] for c in cols], [0] * 5, fillers=False), STREAMS, W.LZ4), "no events at all")


def zeros_frame(head, total):
    """An LZ4 frame of 4 MiB blocks that decodes to `head` followed by zero bytes, `total` bytes in all: per block one match at
    offset 1 and the five last literals."""
    out = bytearray(W.lz4_header(block_code=7))
    at = 0
    while at < total:
        n = min(1 << 22, total - at)
        lit = head + b"\0" if at == 0 else b""
        body = W.lz4_sequence(lit, 1, n - len(lit) - 5) + W.lz4_sequence(b"\0" * 5)
        out += struct.pack("<I", len(body)) + body
        at += n
    return bytes(out + struct.pack("<I", 0))


def test_largest_packet_and_one_byte_more(er):
    """A packet may decode to 2^23 - 16 bytes: its size rounded up to 16 is what the device sums, 256 at a time, in an int32."""
    most = (1 << 23) - 16
    n = (most - HEAD) // 16
    head = W.evts_payload(*(np.zeros(n, dtype=np.int64),) * 4)[:HEAD]
    _, info = check(er, W.write_aedat4([(0, b"")], STREAMS, W.LZ4, compress=lambda k, pl: zeros_frame(head, most)), "largest")
    assert info["n_events"] == n
    for total in (most + 1, most + 15, most + 16, 3 << 22):
        damaged(er, W.write_aedat4([(0, b"")], STREAMS, W.LZ4, compress=lambda k, pl: zeros_frame(head, total)), "CORRUPT")


def damaged(er, data, word):
    with pytest.raises(ValueError):
        R.read(data)
    with pytest.raises(ValueError, match=word):
        er.read_events_aedat4(data)


def test_damaged_files_raise(er):
    cols = W.random_events(40, HW, 8)
    payload = W.evts_payload(*cols)
    good = W.write_aedat4([(0, payload)], STREAMS, W.LZ4)
    check(er, good, "undamaged")

    def one(frame):
        return W.write_aedat4([(0, payload)], STREAMS, W.LZ4, compress=lambda k, pl: frame)
    frame = bytearray(W.lz4_frame(payload, content_checksum=True, stored=True))
    frame[7 + 4 + HEAD + 16 * 5 + 1] ^= 0x10                              # a time stamp byte of event 5, in the stored block
    damaged(er, one(bytes(frame)), "CHECKSUM")
    check(er, one(bytes(frame)), "flipped byte, unverified", verify=False)
    body = W.lz4_block_planned(payload, 0, len(payload), [])             # one run of literals: the block's last byte is a pad byte
    frame = bytearray(W.lz4_frame(payload, block_checksum=True, overrides={0: body}))
    assert frame[7 + 4 + len(body) - 1] == payload[-1] == 0
    frame[7 + 4 + len(body) - 1] ^= 0x01                                  # changes no event: only the block checksum can tell
    damaged(er, one(bytes(frame)), "CHECKSUM")
    check(er, one(bytes(frame)), "flipped pad byte, unverified", verify=False)
    tail = W.lz4_sequence(payload[8:])
    damaged(er, one(W.lz4_frame(payload, overrides={0: W.lz4_sequence(payload[:4], 0, 4) + tail})), "CORRUPT")      # offset 0
    damaged(er, one(W.lz4_frame(payload, overrides={0: W.lz4_sequence(payload[:4], 5, 4) + tail})), "CORRUPT")      # before the output
    damaged(er, one(W.lz4_frame(payload, overrides={0: bytes([0xF0, 40]) + payload[:20]})), "CORRUPT")              # literals past the block
    damaged(er, one(W.lz4_frame(payload, overrides={0: W.lz4_sequence(payload[:8], 4, 8)[:-1]})), "CORRUPT")        # ends inside an offset
    damaged(er, one(W.lz4_frame(payload, bad_hc=True)), "CORRUPT")
    damaged(er, one(W.lz4_frame(payload, dict_id=True)), "CORRUPT")
    damaged(er, one(W.lz4_frame(payload, version=0)), "CORRUPT")
    damaged(er, one(b"\x04\x22\x4d\x19" + W.lz4_frame(payload)[4:]), "CORRUPT")
    sized = W.lz4_frame(payload, content_size=True)
    check(er, one(sized), "content size")
    for wrong in (len(payload) + 1, len(payload) - 1, len(payload) | 1 << 63, 1 << 63, 2 ** 64 - 1):
        damaged(er, one(W.lz4_header(content_size=wrong) + sized[15:]), "CORRUPT")
    big = bytearray(payload)
    struct.pack_into("<I", big, HEAD - 4, 41)                             # one event more than the payload holds
    damaged(er, W.write_aedat4([(0, bytes(big))], STREAMS, W.NONE), "FLATBUFFER")
    damaged(er, W.write_aedat4([(0, bytes(big))], STREAMS, W.LZ4), "FLATBUFFER")
    damaged(er, W.write_aedat4([(0, payload[:4] + payload[4:8] + b"EVTX" + payload[12:])], STREAMS, W.NONE), "FLATBUFFER")
    far = list(cols)
    far[1] = far[1].copy()
    far[1][17] = 64
    damaged(er, W.write_aedat4(split(far, (30, 10)), STREAMS, W.NONE), "RANGE")
    check(er, W.write_aedat4(split(far, (30, 10)), STREAMS, W.NONE), "wide enough", hw=(48, 65))
    check(er, good, "still fine")                                          # the device is in order after all of that


# ------------------------------------------------------------------ the measure / decode pair alone, on the staging buffer
def test_nothing_stored_past_the_measured_size(gpu_ops):
    """LZ4 frames that decode to 0, 1, 15, 16 and 17 bytes (the head of an event payload, cut there: an empty slot, slots that
    end 15, 1 and 15 bytes before a multiple of 16, and one that ends on it) and a two-block linked frame whose second block
    matches into the first (436 bytes, 4 past a multiple of 16), in one launch on a staging buffer of 0xA5: every slot holds its
    bytes at its 16-byte-rounded offset, and the pad behind it is untouched."""
    from aedat4_payload_driver import decode_payloads, padded
    payload = W.evts_payload(*zero_led(20, 5))
    planned = [payload[:n] for n in (0, 1, 15, 16, 17)] + [payload]
    frames = [W.lz4_frame(d, content_checksum=bool(k & 1)) for k, d in enumerate(planned[:-1])]
    frames.append(W.lz4_frame(payload, block_bytes=256, plans={1: [(256, 10, 40)]}))
    assert len(payload) == 436 and all(R.lz4_frame(f) == d for f, d in zip(frames, planned))
    total, st_measure, st, staging = decode_payloads(frames, codec="lz4")
    assert st_measure == 0 and total == sum(padded(len(d)) for d in planned) == 80 + 448
    at = 0
    for d in planned:
        assert staging[at:at + len(d)].tobytes() == d, len(d)
        assert (staging[at + len(d):at + padded(len(d))] == 0xA5).all(), len(d)
        at += padded(len(d))
    assert st & ~gpu_ops.nat.AEDAT4_FLATBUFFER == 0                       # the cut payloads are no event packets: only that bit may be set


def test_damaged_packet_between_good_ones(gpu_ops):
    """A frame whose first match has offset 0, between two good frames: CORRUPT, the packet gets no slot, the neighbours decode."""
    from aedat4_payload_driver import decode_payloads, padded
    nat = gpu_ops.nat
    payload = W.evts_payload(*W.random_events(12, HW, 11))
    good = W.lz4_frame(payload, content_checksum=True)
    bad = W.lz4_frame(payload, overrides={0: W.lz4_sequence(payload[:4], 0, 4) + W.lz4_sequence(payload[8:])})
    for verify in (True, False):
        total, st_measure, st, staging = decode_payloads([good, bad, good], verify, codec="lz4")
        assert (st_measure | st) & (nat.AEDAT4_CORRUPT | nat.AEDAT4_CHECKSUM) == nat.AEDAT4_CORRUPT
        assert st_measure & nat.AEDAT4_CORRUPT and total == 2 * padded(len(payload))
        for at in (0, padded(len(payload))):
            assert staging[at:at + len(payload)].tobytes() == payload
            assert (staging[at + len(payload):at + padded(len(payload))] == 0xA5).all()


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_staging_shorter_than_measured(gpu_ops, codec):
    """DECODE told that the staging buffer ends 16 bytes before what MEASURE asked for (the tensor itself is whole): the last
    packet's slot no longer lies inside, so it is refused as CORRUPT and nothing of it is stored; the two before it decode."""
    from aedat4_payload_driver import decode_payloads, padded
    nat = gpu_ops.nat
    if codec == "lz4":
        planned = [W.evts_payload(*W.random_events(n, HW, 12 + n)) for n in (3, 1, 2)]
        frames = [W.lz4_frame(d) for d in planned]
    else:
        import zstd_cases as C
        frames, planned = zip(*(C.valid()["sequences_fse"][:2] for _ in range(3)))
    assert all(len(d) > 0 for d in planned)
    total, st_measure, st, staging = decode_payloads(list(frames), codec=codec)
    assert st_measure == 0 and st & nat.AEDAT4_CORRUPT == 0 and total == sum(padded(len(d)) for d in planned)
    short = decode_payloads(list(frames), codec=codec, staging_bytes=total - 16)
    assert short[:2] == (total, 0) and short[2] & nat.AEDAT4_CORRUPT and len(short[3]) == total
    last = total - padded(len(planned[2]))
    assert np.array_equal(short[3][:last], staging[:last])               # the first two slots, pads included, as in the whole buffer
    assert short[3][:len(planned[0])].tobytes() == planned[0]
    assert (short[3][last:] == 0xA5).all()


def test_one_event_outside_the_sensor_is_tallied(er, gpu_ops):
    """A NONE recording whose only packet holds exactly one event, outside the sensor: one lane with anything to add, so the
    tally's own barrier is all that orders the zeroing of its LDS pair before the one atomic."""
    import torch
    cols = (np.array([9], dtype=np.int64), np.array([64], dtype=np.int32), np.array([3], dtype=np.int32), np.array([1], dtype=np.int8))
    data = W.write_aedat4([(0, W.evts_payload(*cols))], STREAMS, W.NONE)
    with pytest.raises(ValueError, match=r"outside the 64 x 48 sensor \(status RANGE\)"):
        er.read_events_aedat4(data)
    ops, nat = gpu_ops, gpu_ops.nat
    head = er.parse_aedat4(data)
    pk = torch.from_numpy(np.stack([head.packet_offset, head.packet_size], axis=1)).cuda()
    buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    ws = ops._query_bytes("events_aedat4_workspace_bytes", 1)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    cs = torch.empty(6, dtype=torch.int64, device="cuda")
    lib, P, S = nat.lib(), ops._ptr, ops._stream
    nat.check(lib.scpose_events_aedat4_count(P(buf), P(pk), 1, 0, P(cs), P(work), ws, S()), "count")
    assert cs.tolist() == [1, 0, 9, 0, 0, 0]
    t = torch.empty(1, dtype=torch.int64, device="cuda")
    x, y, p = (torch.empty(1, dtype=d, device="cuda") for d in (torch.int32, torch.int32, torch.int8))
    nat.check(lib.scpose_events_aedat4_unpack(P(buf), 1, HW[0], HW[1], 0, P(t), P(x), P(y), P(p), 1, P(cs), P(work), ws, S()), "unpack")
    assert cs.tolist() == [1, nat.AEDAT4_RANGE, 9, 0, 1, 0]              # n_backward 0, n_out_of_range 1
    assert (t.item(), x.item(), y.item(), p.item()) == (9, 64, 3, 1)


# ------------------------------------------------------------------ command lines
def run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "v2e", script), *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """A 64 x 48 LZ4 recording of 3000 events over 50 ms, next to the CSV text the reference's aedat_to_csv.py would write."""
    d = tmp_path_factory.mktemp("aedat4")
    rng = np.random.default_rng(9)
    t = 1_700_000_000_000_000 + np.sort(rng.integers(0, 50000, 3000)).astype(np.int64)
    x, y, p = rng.integers(0, 64, 3000), rng.integers(0, 48, 3000), rng.integers(0, 2, 3000)
    path = d / "rec.aedat4"
    path.write_bytes(W.write_aedat4(split((t, x, y, p), (1000, 0, 1500, 500)), STREAMS, W.LZ4, ftab=True))
    text = "".join("%d,%d,%d,%d\n" % row for row in zip(t - t[0], x, y, p))
    return path, text


def test_aedat_to_csv(gpu_ops, recording):
    path, text = recording
    out = path.parent / "out.csv"
    r = run("aedat_to_csv.py", "--events_file", str(path), "--output_file", str(out))
    assert r.returncode == 0, r.stderr
    assert out.read_text() == text


def test_e2v_renders_the_same_frames_from_aedat4_and_csv(gpu_ops, recording):
    path, text = recording
    csv = path.parent / "events.csv"
    csv.write_text(text)
    a, b = path.parent / "from_aedat4", path.parent / "from_csv"
    r = run("e2v.py", "--events_file", str(path), "--dvs_exposure", "duration", "10000", "--output_folder", str(a))
    assert r.returncode == 0, r.stderr
    r = run("e2v.py", "--events_file", str(csv), "--dvs_exposure", "duration", "10000", "--output_folder", str(b), "--output_width", "64",
            "--output_height", "48")
    assert r.returncode == 0, r.stderr
    names = sorted(os.listdir(a / "event-frames"))
    assert names == sorted(os.listdir(b / "event-frames")) and len(names) >= 4
    for name in names:
        assert (a / "event-frames" / name).read_bytes() == (b / "event-frames" / name).read_bytes(), name
    r = run("e2v.py", "--events_file", str(path), "--swap_xy", "--output_folder", str(a))
    assert r.returncode != 0 and "--swap_xy" in r.stderr and "AEDAT-4.0" in r.stderr
    r = run("e2v.py", "--events_file", str(path), "--aedat_layout", "v2e", "--output_folder", str(a))
    assert r.returncode != 0 and "--aedat_layout" in r.stderr


def test_convert_aedats_takes_a_scene_with_only_an_aedat4_file(gpu_ops, recording):
    path, _ = recording
    scenes = path.parent / "scenes"
    os.makedirs(scenes / "s0")
    (scenes / "s0" / "rec.aedat4").write_bytes(path.read_bytes())
    calib = path.parent / "calib.json"
    calib.write_text(json.dumps({"intrinsics": {"camera_matrix": [[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1.0]],
                                                "distortion_coefficients": [-0.1, 0.01, 0.0, 0.0, 0.0]}}))
    r = run("convert_aedats.py", "--scenes_dir", str(scenes), "--calibration_file_path", str(calib), "--image_height", "48",
            "--image_width", "64")
    assert r.returncode == 0, r.stderr
    assert "s0: " in r.stdout
    frames = sorted(os.listdir(scenes / "s0" / "event-frames"))
    assert len(frames) >= 4 and frames == sorted(os.listdir(scenes / "s0" / "event-frames-distorted"))
