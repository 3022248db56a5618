"""Writes AEDAT-4.0 recordings from event arrays, for the tests of the device reader (csrc/events_aedat4_read.hip states the format).

Nothing here is shared with the reader under test: the flatbuffers are laid out by hand, the LZ4 frames come from a plain-Python
encoder, and xxh32 is restated (cross-checked against the `xxhash` module only when that imports).  The encoder has a greedy hash
matcher and a PLANNED entry point, where the test dictates the matches (position, offset, length) and the literals are what lies
between them, so literal runs, match lengths and offsets can be set exactly; the plan is verified against the data.
"""
import struct

import numpy as np

MAGIC = b"#!AER-DAT4.0\r\n"
NONE, LZ4, LZ4_HIGH, ZSTD, ZSTD_HIGH = 0, 1, 2, 3, 4
P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
M32 = 0xFFFFFFFF


def _rotl(v, r):
    return ((v << r) | (v >> (32 - r))) & M32


def xxh32(data, seed=0):
    data = bytes(data)
    n = len(data)
    i = 0
    if n >= 16:
        acc = [(seed + P1 + P2) & M32, (seed + P2) & M32, seed & M32, (seed - P1) & M32]
        while i + 16 <= n:
            for k, w in enumerate(struct.unpack_from("<4I", data, i)):
                acc[k] = (_rotl((acc[k] + w * P2) & M32, 13) * P1) & M32
            i += 16
        h = (_rotl(acc[0], 1) + _rotl(acc[1], 7) + _rotl(acc[2], 12) + _rotl(acc[3], 18)) & M32
    else:
        h = (seed + P5) & M32
    h = (h + n) & M32
    while i + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, i)[0] * P3) & M32, 17) * P4) & M32
        i += 4
    while i < n:
        h = (_rotl((h + data[i] * P5) & M32, 11) * P1) & M32
        i += 1
    h ^= h >> 15
    h = (h * P2) & M32
    h ^= h >> 13
    h = (h * P3) & M32
    h ^= h >> 16
    return h


try:                                                                  # a second opinion where one is installed
    import xxhash as _xxhash
    for _probe in (b"", b"a" * 20, bytes(range(256)) * 3 + b"xyz"):
        assert _xxhash.xxh32(_probe).intdigest() == xxh32(_probe)
except ImportError:
    pass


# ------------------------------------------------------------------ LZ4 block
def _length_bytes(n):
    """The extension bytes of a length nibble of 15 whose remainder is n."""
    out = bytearray()
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def lz4_sequence(literals, offset=None, match_len=None):
    """One sequence: token, literal length extension, literals and -- unless it is a block's last -- offset and match length."""
    lit = len(literals)
    ml = 0 if offset is None else match_len - 4
    assert offset is None or (match_len >= 4 and 0 <= offset <= 65535)
    out = bytearray([(min(lit, 15) << 4) | min(ml, 15)])
    if lit >= 15:
        out += _length_bytes(lit - 15)
    out += literals
    if offset is not None:
        out += struct.pack("<H", offset)
        if ml >= 15:
            out += _length_bytes(ml - 15)
    return bytes(out)


def lz4_block_planned(data, start, end, matches, first=0):
    """data[start:end] as one block whose matches are exactly `matches`, a sorted list of (position, offset, length); the literal
    runs are what lies between them.  Every match is checked: inside the block, at least 4 long, an offset that stays at or after
    `first`, and bytes that an LZ4 copy (overlapping included) would reproduce."""
    out = bytearray()
    at = start
    for pos, offset, length in matches:
        assert start <= at <= pos and pos + length <= end and length >= 4, (pos, offset, length)
        assert 1 <= offset <= 65535 and pos - offset >= first, (pos, offset, first)
        for i in range(length):
            assert data[pos + i] == data[pos - offset + (i % offset)], "planned match does not reproduce the data at %d" % (pos + i)
        out += lz4_sequence(data[at:pos], offset, length)
        at = pos + length
    out += lz4_sequence(data[at:end])
    return bytes(out)


def lz4_block_greedy(data, start, end, first=0):
    """data[start:end] as one block: a greedy matcher on a hash of 4 bytes, matches reaching back to `first` at the most and 65535
    bytes; the last 12 bytes stay literals, as the reference encoder leaves them."""
    table = {}
    for i in range(max(first, start - 65535), start):
        table[data[i:i + 4]] = i
    matches = []
    i = start
    last = end - 12
    while i < last:
        key = data[i:i + 4]
        j = table.get(key)
        table[key] = i
        if j is not None and i - j <= 65535 and j >= first:
            n = 4
            while i + n < end - 5 and data[i + n] == data[j + n]:
                n += 1
            matches.append((i, i - j, n))
            for k in range(i + 1, min(i + n, last), 7):
                table[data[k:k + 4]] = k
            i += n
        else:
            i += 1
    return lz4_block_planned(data, start, end, matches, first)


# ------------------------------------------------------------------ LZ4 frame
BLOCK_BYTES = {4: 1 << 16, 5: 1 << 18, 6: 1 << 20, 7: 1 << 22}


def lz4_header(block_code=4, linked=True, block_checksum=False, content_checksum=False, content_size=None, version=1, dict_id=False,
               bad_hc=False, magic=b"\x04\x22\x4d\x18"):
    flg = (version << 6) | (0 if linked else 0x20) | (0x10 if block_checksum else 0) | (8 if content_size is not None else 0) | \
        (4 if content_checksum else 0) | (1 if dict_id else 0)
    desc = bytes([flg, block_code << 4])
    if content_size is not None:
        desc += struct.pack("<Q", content_size)
    if dict_id:
        desc += b"\0\0\0\0"
    hc = (xxh32(desc) >> 8) & 0xFF
    return magic + desc + bytes([hc ^ (0x55 if bad_hc else 0)])


def lz4_frame(data, block_code=4, linked=True, block_checksum=False, content_checksum=False, content_size=False, stored=(),
              plans=None, overrides=None, block_bytes=None, **header_kwargs):
    """One LZ4 frame of `data`.  stored: indices of blocks written uncompressed (True: all).  plans: {block index: matches} for
    lz4_block_planned, positions counted in `data`; other blocks go through the greedy matcher.  overrides: {block index: bytes}
    puts those bytes in place of the block's compressed form (damaged blocks).  block_bytes: cut blocks shorter than the maximum."""
    data = bytes(data)
    size = block_bytes or BLOCK_BYTES[block_code]
    assert size <= BLOCK_BYTES[block_code]
    out = bytearray(lz4_header(block_code, linked, block_checksum, content_checksum, len(data) if content_size else None,
                               **header_kwargs))
    for k, start in enumerate(range(0, len(data), size)):
        end = min(start + size, len(data))
        first = 0 if linked else start
        if stored is True or k in stored:
            body, word = data[start:end], (end - start) | 0x80000000
        else:
            if overrides and k in overrides:
                body = overrides[k]
            elif plans and k in plans:
                body = lz4_block_planned(data, start, end, plans[k], first)
            else:
                body = lz4_block_greedy(data, start, end, first)
            word = len(body)
        out += struct.pack("<I", word) + body
        if block_checksum:
            out += struct.pack("<I", xxh32(body))
    out += struct.pack("<I", 0)
    if content_checksum:
        out += struct.pack("<I", xxh32(data))
    return bytes(out)


# ------------------------------------------------------------------ flatbuffers, by hand
def evts_payload(t, x, y, p, prefixed=True, omit_empty=False):
    """An EventPacket flatbuffer: root offset, "EVTS", a vtable of one field, the table, the vector of 16-byte structs (8-byte
    aligned).  prefixed: with the uint32 size in front, as writers emit it.  omit_empty: no events -> the field is absent."""
    n = len(t)
    ev = np.zeros(n, dtype=np.dtype([("t", "<i8"), ("x", "<i2"), ("y", "<i2"), ("on", "u1"), ("pad", "u1", 3)]))
    ev["t"], ev["x"], ev["y"], ev["on"] = t, x, y, p
    if n == 0 and omit_empty:
        body = struct.pack("<I4s", 12, b"EVTS") + struct.pack("<HH", 4, 4) + struct.pack("<i", 4)
    else:
        body = struct.pack("<I4s", 16, b"EVTS") + struct.pack("<HHH", 6, 8, 4) + b"\0\0" + struct.pack("<iI", 8, 8) + b"\0\0\0\0" + \
            struct.pack("<I", n) + ev.tobytes()
        assert (len(body) - 16 * n) == 32
    return (struct.pack("<I", len(body)) + body) if prefixed else body


def filler_payload(kind, nbytes, seed=0):
    """A size-prefixed packet of another stream (FRME / IMUS / TRIG): identifier and half-compressible bytes, never parsed."""
    rng = np.random.default_rng(seed)
    junk = np.repeat(rng.integers(0, 256, (nbytes + 3) // 4, dtype=np.uint8), 4)[:nbytes].tobytes()
    body = struct.pack("<I4s", 8, kind.encode()) + junk
    return struct.pack("<I", len(body)) + body


def info_node(streams):
    out = ['<dv version="2.0"><node name="outInfo" path="/mainloop/output_file/outInfo/">']
    for sid, (kind, sx, sy) in streams.items():
        out.append('<node name="%d" path="/mainloop/output_file/outInfo/%d/">' % (sid, sid))
        out.append('<attr key="compression" type="int">0</attr><attr key="originalModuleName" type="string">capture</attr>')
        out.append('<attr key="typeIdentifier" type="string">%s</attr>' % kind)
        out.append('<node name="info" path="/mainloop/output_file/outInfo/%d/info/">' % sid)
        if sx is not None:
            out.append('<attr key="sizeX" type="int">%d</attr><attr key="sizeY" type="int">%d</attr>' % (sx, sy))
        out.append('<attr key="source" type="string">DVXplorer_DXA00093</attr></node></node>')
    out.append("</node></dv>")
    return "".join(out).encode()


def io_header(compression, data_table_position, info, identifier=b"IOHE"):
    """The IOHeader flatbuffer: vtable of three fields at 8, table at 24 (compression, dataTablePosition, infoNode), string at 44."""
    return struct.pack("<I4s", 24, identifier) + struct.pack("<HHHHH", 10, 20, 4, 8, 16) + b"\0" * 6 + \
        struct.pack("<iiqI", 16, compression, data_table_position, 4) + struct.pack("<I", len(info)) + info + b"\0"


def write_aedat4(packets, streams, compression=NONE, ftab=False, compress=None, identifier=b"IOHE", cut=0):
    """The bytes of a recording.  packets: [(stream id, payload bytes)] in file order.  streams: {id: (type, sizeX, sizeY)}.
    compression: the header's value; under LZ4 / LZ4_HIGH every payload becomes compress(index, payload) (default: lz4_frame).
    ftab: append a file data table and point dataTablePosition at it.  cut: drop that many bytes from the end."""
    body = bytearray()
    for k, (sid, payload) in enumerate(packets):
        if compression in (LZ4, LZ4_HIGH):
            payload = compress(k, payload) if compress else lz4_frame(payload)
        body += struct.pack("<ii", sid, len(payload)) + payload
    info = info_node(streams)
    head_len = len(io_header(compression, -1, info, identifier))
    table_at = len(MAGIC) + 4 + head_len + len(body) if ftab else -1
    head = io_header(compression, table_at, info, identifier)
    out = MAGIC + struct.pack("<I", len(head)) + head + bytes(body)
    if ftab:
        # what lies there is never read: a size prefix, "FTAB", and bytes that would be a broken packet header if they were
        out += struct.pack("<I4s", 4, b"FTAB") + struct.pack("<ii", 0, 1 << 30) + b"\xff" * 24
    return out[:len(out) - cut] if cut else out


def random_events(n, hw, seed=0, t_start=1_600_000_000_000_000, step=40):
    """n events on an hw sensor: increasing time stamps (64-bit microseconds, as a camera's epoch clock gives), x and y in bursts."""
    rng = np.random.default_rng(seed)
    t = t_start + np.cumsum(rng.integers(0, step, n, dtype=np.int64))
    x = (rng.integers(0, hw[1], n) // 4 * 4 + rng.integers(0, 2, n)).clip(0, hw[1] - 1)
    y = rng.integers(0, hw[0], n)
    p = rng.integers(0, 2, n)
    return t.astype(np.int64), x.astype(np.int32), y.astype(np.int32), p.astype(np.int8)
