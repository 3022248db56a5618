"""A hand-written AEDAT-3.1 file writer for the tests (not collected), from the format statement at the head of
csrc/events_aedat3_read.hip and independent of event_read.py.  Every field of the text header and of the 28-byte packet header has
a knob, so that damaged files can be made.  All integers little-endian."""
import struct

import numpy as np

SPECIAL, POLARITY, FRAME, IMU6, IMU9 = 0, 1, 2, 3, 4
EVENT_SIZE = {SPECIAL: 8, POLARITY: 8, IMU6: 36, IMU9: 48}
TS_OFFSET = {SPECIAL: 4, POLARITY: 4, FRAME: 12, IMU6: 4, IMU9: 4}


def header(sources=None, version=b"3.1", fmt=b"RAW", extra=(), end=True, eol=b"\r\n"):
    """The text header.  sources: {id: name} (default one DAVIS346 as source 1).  extra: further lines (bytes, with their '#')
    put between the source lines and the end mark.  end: write '#!END-HEADER'."""
    sources = {1: "DAVIS346"} if sources is None else sources
    lines = [b"#!AER-DAT" + version]
    if fmt is not None:
        lines.append(b"#Format: " + fmt)
    lines += [("#Source %d: %s" % (sid, name)).encode() for sid, name in sources.items()]
    lines.append(b"#Start-Time: 2019-03-07 11:32:04 (TZ+0100)")
    lines += list(extra)
    if end:
        lines.append(b"#!END-HEADER")
    return b"".join(line + eol for line in lines)


def polarity_words(t, x, y, p, valid=None):
    """(data uint32, ts int64) per event: data bit 0 valid, bit 1 polarity, bits 2..16 y, bits 17..31 x; ts the low 31 bits of t."""
    t = np.asarray(t, dtype=np.int64)
    valid = np.ones(len(t), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    data = ((np.asarray(x, dtype=np.int64) & 0x7FFF) << 17) | ((np.asarray(y, dtype=np.int64) & 0x7FFF) << 2) | \
        ((np.asarray(p, dtype=np.int64) & 1) << 1) | valid.astype(np.int64)
    return data.astype(np.uint32), t & 0x7FFFFFFF


def polarity_payload(t, x, y, p, valid=None, ts=None):
    """The 8-byte events.  ts: the int32 time stamps as stored, in place of t's low 31 bits (a negative one can be written)."""
    data, low = polarity_words(t, x, y, p, valid)
    rec = np.empty(len(data), dtype=[("data", "<u4"), ("ts", "<i4")])
    rec["data"] = data
    rec["ts"] = low if ts is None else np.asarray(ts, dtype=np.int64)
    return rec.tobytes()


def packet(etype, source, payload, number, size=None, ts_offset=None, overflow=0, capacity=None, event_valid=None, tail=b""):
    """One packet: the 28-byte header, `payload` (the events), `tail` (what lies between eventNumber and eventCapacity).  Every
    header field can be overridden; by default capacity = number + len(tail) / size and event_valid = number."""
    size = EVENT_SIZE.get(etype, 8) if size is None else size
    ts_offset = TS_OFFSET.get(etype, 4) if ts_offset is None else ts_offset
    if capacity is None:
        capacity = number + (len(tail) // size if size > 0 else 0)
    event_valid = number if event_valid is None else event_valid
    return struct.pack("<hhiiiiii", etype, source, size, ts_offset, overflow, capacity, number, event_valid) + payload + tail


def polarity_packet(t, x, y, p, valid=None, source=1, overflow=None, ts=None, **kw):
    """A polarity packet of the events; overflow defaults to t >> 31 of its first event, eventValid to the number of valid bits."""
    t = np.asarray(t, dtype=np.int64)
    if overflow is None:
        overflow = int(t[0] >> 31) if len(t) else 0
    n_valid = len(t) if valid is None else int(np.count_nonzero(valid))
    kw.setdefault("event_valid", n_valid)
    return packet(POLARITY, source, polarity_payload(t, x, y, p, valid, ts), len(t), overflow=overflow, **kw)


def filler_packet(etype, source, number, seed=0, size=None, **kw):
    """A packet of another type (special, frame, IMU6, ...): `number` events of half-random bytes, never parsed."""
    size = EVENT_SIZE.get(etype, 36 + 2 * 6 * 4) if size is None else size
    rng = np.random.default_rng(seed)
    return packet(etype, source, rng.integers(0, 256, number * size, dtype=np.uint8).tobytes(), number, size=size, **kw)


def write_aedat3(packets, sources=None, cut=0, **header_kw):
    """The bytes of a recording: the header, the packets (bytes, in file order); cut: drop that many bytes from the end."""
    data = header(sources, **header_kw) + b"".join(packets)
    return data[:len(data) - cut] if cut else data


def random_events(n, hw, seed=0, t_start=1000, step=40):
    """n events on an hw sensor: increasing time stamps in microseconds from the camera's start, random x, y and p."""
    rng = np.random.default_rng(seed)
    t = t_start + np.cumsum(rng.integers(0, step, n, dtype=np.int64))
    return (t, rng.integers(0, hw[1], n).astype(np.int32), rng.integers(0, hw[0], n).astype(np.int32),
            rng.integers(0, 2, n).astype(np.int8))


def split(cols, counts, valid=None, source=1, fillers=False, **kw):
    """[packet bytes]: the columns cut into polarity packets of `counts` events, packets of other types between them on request."""
    out, at = [], 0
    for k, c in enumerate(counts):
        c = int(c)
        v = None if valid is None else valid[at:at + c]
        out.append(polarity_packet(*(col[at:at + c] for col in cols), valid=v, source=source, **kw))
        if fillers:
            out.append(filler_packet((SPECIAL, FRAME, IMU6)[k % 3], source, 1 + k % 3, seed=k))
        at += c
    assert at == len(cols[0])
    return out
