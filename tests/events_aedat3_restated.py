"""The AEDAT-3.1 reader restated in plain Python and NumPy for the tests (not collected): written from the format statement at the
head of csrc/events_aedat3_read.hip, independently of event_read.py.  read() returns what event_read.read_events_aedat3 returns,
with NumPy columns; every file that reader refuses raises ValueError here."""
import struct

import numpy as np

SENSORS = {"DVS128": (128, 128), "DAVIS240": (180, 240), "DAVIS346": (260, 346), "DAVIS640": (480, 640)}
MAX_HEADER = 1 << 20


def sensor_hw(name):
    for prefix, hw in SENSORS.items():
        if name.upper().startswith(prefix):
            return hw
    return None


def text_header(data):
    """-> ({source id: name}, position of the first packet)"""
    data = bytes(data)
    if not data.startswith(b"#!AER-DAT3.1\r\n"):
        raise ValueError("not AEDAT-3.1")
    stop = data.find(b"#!END-HEADER\r\n", 0, MAX_HEADER)
    if stop < 0 or data[stop - 2:stop] != b"\r\n":
        raise ValueError("no end of header")
    sources, fmt = {}, None
    for line in data[:stop].decode("latin-1").split("\r\n"):
        if line.startswith("#Format:"):
            fmt = line.split(":", 1)[1].strip()
        elif line.startswith("#Source "):
            sid, name = line[len("#Source "):].split(":", 1)
            sources[int(sid)] = name.strip()
    if fmt != "RAW":
        raise ValueError("format %r" % fmt)
    return sources, stop + len(b"#!END-HEADER\r\n")


def packets(data):
    """-> ({source id: name}, [(type, source, overflow, number, valid, payload position)], {type: count} of the others, trailing)"""
    data = bytes(data)
    sources, pos = text_header(data)
    table, other, trailing = [], {}, 0
    while pos < len(data):
        if len(data) - pos < 28:
            trailing = len(data) - pos
            break
        etype, source, size, ts_at, overflow, capacity, number, valid = struct.unpack_from("<hhiiiiii", data, pos)
        if min(etype, source, size, ts_at, overflow, capacity, number, valid) < 0 or size == 0:
            raise ValueError("packet %d: a field is negative or the size 0" % len(table))
        if number > capacity or valid > number:
            raise ValueError("packet %d: counts out of order" % len(table))
        if etype == 1 and (size, ts_at) != (8, 4):
            raise ValueError("packet %d: polarity events of another shape" % len(table))
        if pos + 28 + capacity * size > len(data):
            trailing = len(data) - pos
            break
        table.append((etype, source, overflow, number, valid, pos + 28))
        if etype != 1:
            other[etype] = other.get(etype, 0) + 1
        pos += 28 + capacity * size
    return sources, table, other, trailing


def read(data, hw=None, source=None, rebase=True):
    data = bytes(data)
    sources, table, other, trailing = packets(data)
    carrying = sorted({s for e, s, *_ in table if e == 1})
    if source is None:
        if len(carrying) > 1:
            raise ValueError("several polarity sources")
        source = carrying[0] if carrying else min(sources)
    elif source not in sources and source not in carrying:
        raise ValueError("no such source")
    if hw is None:
        hw = sensor_hw(sources.get(source, ""))
        if hw is None:
            raise ValueError("unknown sensor")
    ts, xs, ys, ps, n_packets, n_all = [], [], [], [], 0, 0
    for etype, src, overflow, number, valid, at in table:
        if etype != 1 or src != source:
            continue
        n_packets += 1
        n_all += number
        words = np.frombuffer(data, dtype="<u4", count=2 * number, offset=at).reshape(-1, 2).astype(np.int64)
        d, stamp = words[:, 0], words[:, 1]
        if np.any(stamp >= 1 << 31):
            raise ValueError("CORRUPT: a negative time stamp")
        keep = (d & 1) == 1
        if int(keep.sum()) != valid:
            raise ValueError("VALID_MISMATCH")
        ts.append(((np.int64(overflow) << 31) | stamp)[keep])
        xs.append((d >> 17)[keep])
        ys.append(((d >> 2) & 0x7FFF)[keep])
        ps.append(((d >> 1) & 1)[keep])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    t, x, y, p = cat(ts), cat(xs), cat(ys), cat(ps)
    n_out = int(np.count_nonzero((x >= hw[1]) | (y >= hw[0])))
    if n_out:
        raise ValueError("RANGE: %d events outside the sensor" % n_out)
    t0 = int(t[0]) if len(t) else 0
    info = {"n_events": int(len(t)), "n_packets": n_packets, "n_invalid": n_all - int(len(t)), "t0": t0,
            "n_backward": int(np.count_nonzero(t[1:] < t[:-1])), "n_out_of_range": 0, "sources": (source,), "other_packets": other,
            "trailing_bytes": trailing, "hw": (int(hw[0]), int(hw[1]))}
    return (t - t0 if rebase else t).astype(np.int64), x.astype(np.int32), y.astype(np.int32), p.astype(np.int8), info
