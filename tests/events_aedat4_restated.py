"""The AEDAT-4.0 reader said again in NumPy / Python: what the device reader (event_read.read_events_aedat4, csrc/events_aedat4_read.hip)
is compared against, column for column and counter for counter.  It shares no code with the package; xxh32 comes from the writer
helper, whose known answers tests/test_events_aedat4.py pins."""
import re
import struct

import numpy as np

from aedat4_stream_writer import xxh32

MAGIC = b"#!AER-DAT4.0\r\n"
BLOCK_BYTES = {4: 1 << 16, 5: 1 << 18, 6: 1 << 20, 7: 1 << 22}
MAX_DECODED = (1 << 23) - 16                   # rounded up to 16, 256 of them sum within int32


class Corrupt(ValueError):
    pass


class Checksum(ValueError):
    pass


class Flatbuffer(ValueError):
    pass


class Range(ValueError):
    pass


def _table_field(buf, table, index):
    """Position of field `index` of the table at `table`, or None when the vtable has no slot for it."""
    vt = table - struct.unpack_from("<i", buf, table)[0]
    vsize = struct.unpack_from("<H", buf, vt)[0]
    if 4 + 2 * index + 2 > vsize:
        return None
    slot = struct.unpack_from("<H", buf, vt + 4 + 2 * index)[0]
    return table + slot if slot else None


def parse_header(data):
    """-> (compression, data_table_position, {id: (type, sizeX, sizeY)}, offset of the first packet)"""
    assert data[:14] == MAGIC
    n = struct.unpack_from("<I", data, 14)[0]
    head = data[18:18 + n]
    if head[4:8] != b"IOHE":
        raise ValueError("no IOHE identifier")
    root = struct.unpack_from("<I", head, 0)[0]
    f = _table_field(head, root, 0)
    compression = struct.unpack_from("<i", head, f)[0] if f is not None else 0
    f = _table_field(head, root, 1)
    table_at = struct.unpack_from("<q", head, f)[0] if f is not None else -1
    f = _table_field(head, root, 2)
    xml = b""
    if f is not None:
        s = f + struct.unpack_from("<I", head, f)[0]
        xml = head[s + 4:s + 4 + struct.unpack_from("<I", head, s)[0]]
    streams = {}
    text = xml.decode("utf-8", "replace")
    m = re.search(r'<node name="outInfo"[^>]*>', text)
    pos = m.end() if m else len(text)
    for node in re.finditer(r'<node name="(\d+)"[^>]*>', text[pos:]):
        rest = text[pos + node.end():]
        nxt = re.search(r'<node name="\d+"', rest)
        part = rest[:nxt.start()] if nxt else rest
        kind = re.search(r'<attr key="typeIdentifier"[^>]*>([^<]*)</attr>', part)
        sx = re.search(r'<attr key="sizeX"[^>]*>(-?\d+)</attr>', part)
        sy = re.search(r'<attr key="sizeY"[^>]*>(-?\d+)</attr>', part)
        streams[int(node.group(1))] = (kind.group(1) if kind else None, int(sx.group(1)) if sx else None,
                                       int(sy.group(1)) if sy else None)
    return compression, table_at, streams, 18 + n


def lz4_block(src, out, first, limit):
    """Appends what the block `src` decodes to onto the bytearray `out`; matches reach back to out[first] at the most."""
    ip, n = 0, len(src)
    while True:
        if ip >= n:
            raise Corrupt("block ends before a token")
        token = src[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= n:
                    raise Corrupt("block ends inside a literal length")
                b = src[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        if ip + lit > n or len(out) + lit > limit:
            raise Corrupt("literals overrun")
        out += src[ip:ip + lit]
        ip += lit
        if ip == n:
            return
        if ip + 2 > n:
            raise Corrupt("block ends inside an offset")
        offset = src[ip] | (src[ip + 1] << 8)
        ip += 2
        ml = token & 15
        if ml == 15:
            while True:
                if ip >= n:
                    raise Corrupt("block ends inside a match length")
                b = src[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if offset == 0 or offset > len(out) - first or len(out) + ml > limit:
            raise Corrupt("offset %d with %d bytes of output" % (offset, len(out) - first))
        start = len(out) - offset
        if offset >= ml:
            out += out[start:start + ml]
        else:
            pattern = bytes(out[start:])
            out += (pattern * (ml // offset + 1))[:ml]


def lz4_frame(src, verify=True):
    """One LZ4 frame -> bytes.  Raises Corrupt / Checksum."""
    src = bytes(src)
    if len(src) < 7 or src[:4] != b"\x04\x22\x4d\x18":
        raise Corrupt("magic")
    flg, bd = src[4], src[5]
    if flg >> 6 != 1 or flg & 3 or bd & 0x8F or (bd >> 4) < 4:
        raise Corrupt("descriptor")
    bmax = BLOCK_BYTES[bd >> 4]
    linked, bsum = not flg & 0x20, bool(flg & 0x10)
    hc_at = 6 + (8 if flg & 8 else 0)
    if len(src) < hc_at + 1:
        raise Corrupt("descriptor cut")
    if (xxh32(src[4:hc_at]) >> 8) & 0xFF != src[hc_at]:
        raise Corrupt("HC")
    content = struct.unpack_from("<Q", src, 6)[0] if flg & 8 else None
    pos = hc_at + 1
    out = bytearray()
    bad_sum = False
    while True:
        if pos + 4 > len(src):
            raise Corrupt("no end mark")
        word = struct.unpack_from("<I", src, pos)[0]
        pos += 4
        if word == 0:
            break
        bs = word & 0x7FFFFFFF
        if bs > bmax or pos + bs + (4 if bsum else 0) > len(src):
            raise Corrupt("block overruns the frame")
        body = src[pos:pos + bs]
        if bsum and verify and xxh32(body) != struct.unpack_from("<I", src, pos + bs)[0]:
            bad_sum = True
        limit = min(len(out) + bmax, MAX_DECODED)
        if word >> 31:
            if len(out) + bs > limit:
                raise Corrupt("stored block too long")
            out += body
        else:
            lz4_block(body, out, 0 if linked else len(out), limit)
        pos += bs + (4 if bsum else 0)
    if flg & 4:
        if pos + 4 > len(src):
            raise Corrupt("no content checksum")
        if verify and xxh32(out) != struct.unpack_from("<I", src, pos)[0]:
            bad_sum = True
    if content is not None and content != len(out):
        raise Corrupt("content size")
    if bad_sum:
        raise Checksum("xxh32 differs")
    return bytes(out)


EVENT = np.dtype([("t", "<i8"), ("x", "<i2"), ("y", "<i2"), ("on", "u1"), ("pad", "u1", 3)])


def event_vector(payload):
    """The structs of an EventPacket flatbuffer (prefixed or not) as a NumPy record array.  Raises Flatbuffer."""
    b = bytes(payload)
    if len(b) >= 12 and b[8:12] == b"EVTS":
        b = b[4:]
    elif not (len(b) >= 8 and b[4:8] == b"EVTS"):
        raise Flatbuffer("no EVTS identifier")
    n = len(b)
    root = struct.unpack_from("<I", b, 0)[0]
    if root < 4 or root + 4 > n:
        raise Flatbuffer("root")
    vt = root - struct.unpack_from("<i", b, root)[0]
    if vt < 0 or vt + 4 > n:
        raise Flatbuffer("vtable")
    vsize = struct.unpack_from("<H", b, vt)[0]
    if vsize < 4 or vt + vsize > n:
        raise Flatbuffer("vtable size")
    slot = struct.unpack_from("<H", b, vt + 4)[0] if vsize >= 6 else 0
    if slot == 0:
        return np.zeros(0, dtype=EVENT)
    fpos = root + slot
    if fpos + 4 > n:
        raise Flatbuffer("field")
    vec = fpos + struct.unpack_from("<I", b, fpos)[0]
    if vec + 4 > n:
        raise Flatbuffer("vector")
    count = struct.unpack_from("<I", b, vec)[0]
    if count >= 1 << 23 or vec + 4 + 16 * count > n:
        raise Flatbuffer("count %d" % count)
    return np.frombuffer(b, dtype=EVENT, count=count, offset=vec + 4)


def read(data, hw=None, stream=None, rebase=True, verify=True):
    """-> (t int64, x int32, y int32, p int8, info) as NumPy arrays, what event_read.read_events_aedat4 returns on the device."""
    data = bytes(data)
    compression, table_at, streams, pos = parse_header(data)
    if compression not in (0, 1, 2):
        raise ValueError("compression %d" % compression)
    end = table_at if table_at >= 0 else len(data)
    end = min(end, len(data))
    ids = [sid for sid, s in streams.items() if s[0] == "EVTS"] if stream is None else [stream]
    if not ids or any(sid not in streams or streams[sid][0] != "EVTS" for sid in ids):
        raise ValueError("no event stream")
    if hw is None:
        hw = (streams[ids[0]][2], streams[ids[0]][1])
    chunks, trailing, n_packets = [], 0, 0
    while pos < end:
        if pos + 8 > end:
            trailing = end - pos
            break
        sid, size = struct.unpack_from("<ii", data, pos)
        if size < 0 or pos + 8 + size > end:
            trailing = end - pos
            break
        if sid in ids:
            payload = data[pos + 8:pos + 8 + size]
            chunks.append(event_vector(lz4_frame(payload, verify) if compression else payload))
            n_packets += 1
        pos += 8 + size
    ev = np.concatenate(chunks) if chunks else np.zeros(0, dtype=EVENT)
    t = ev["t"].astype(np.int64)
    x, y = ev["x"].astype(np.int32), ev["y"].astype(np.int32)
    out = int(((x < 0) | (x >= hw[1]) | (y < 0) | (y >= hw[0])).sum())
    if out:
        raise Range("%d events outside the sensor" % out)
    t0 = int(t[0]) if len(t) else 0
    info = {"n_events": int(len(t)), "n_packets": n_packets, "t0": t0, "n_backward": int((t[1:] < t[:-1]).sum()),
            "n_out_of_range": 0, "compression": compression, "hw": (int(hw[0]), int(hw[1])), "streams": tuple(ids),
            "trailing_bytes": int(trailing)}
    return (t - t0 if rebase else t), x, y, (ev["on"] != 0).astype(np.int8), info
