"""The AEDAT-4.0 writer (event_write.write_events_aedat4, csrc/events_aedat4_write.hip) restated in plain Python.

Nothing here is shared with the code under test.  The LZ4 blocks of `write` come from aedat4_stream_writer.lz4_block_greedy, the
plain greedy encoder, so the files differ from the device's in their compressed bytes and agree in everything else: header,
flatbuffers, framing, checksums, file data table.  lz4_block_wave is a second encoder, the device's matcher lane by lane (64
positions hashed at once, candidates read before the round's positions are entered, the first verified position by ballot, the
later lanes keeping their candidates): its bytes are what the device must give.
"""
import struct

import numpy as np

import aedat4_stream_writer as W

MAGIC = b"#!AER-DAT4.0\r\n"
BLOCK = 1 << 16
FB_HEAD = 48
FRAME_FIXED = 7 + 8                                 # magic FLG BD HC; end mark, content checksum
TABLE_POSITION_AT = 14 + 4 + 32
MAX_PACKET_EVENTS = ((1 << 23) - 16 - FB_HEAD) // 16


def evts_flatbuffer(t, x, y, p):
    """The size-prefixed EventPacket flatbuffer as written: the structs start at byte 48."""
    n = len(t)
    ev = np.zeros(n, dtype=np.dtype([("t", "<i8"), ("x", "<i2"), ("y", "<i2"), ("on", "u1"), ("pad", "u1", 3)]))
    ev["t"], ev["x"], ev["y"], ev["on"] = t, x, y, p
    body = struct.pack("<I4s", 16, b"EVTS") + struct.pack("<HHHH", 6, 8, 4, 0) + struct.pack("<iI", 8, 20) + b"\0" * 16 + \
        struct.pack("<I", n) + ev.tobytes()
    assert len(body) + 4 == FB_HEAD + 16 * n
    return struct.pack("<I", len(body)) + body


def lz4_frame(data, block=W.lz4_block_greedy):
    """One frame as written: independent 64 KiB blocks, content checksum, no content size; a block that is not smaller is stored."""
    data = bytes(data)
    out = bytearray(W.lz4_header(block_code=4, linked=False, content_checksum=True))
    assert out[4] == 0x64 and out[5] == 0x40
    for start in range(0, len(data), BLOCK):
        end = min(start + BLOCK, len(data))
        body = block(data, start, end, start)
        if len(body) >= end - start:
            out += struct.pack("<I", (end - start) | 0x80000000) + data[start:end]
        else:
            out += struct.pack("<I", len(body)) + body
    return bytes(out + struct.pack("<II", 0, W.xxh32(data)))


def block_words(frame):
    """The size words of a frame written by lz4_frame or the device."""
    pos, words = 7, []
    while True:
        w = struct.unpack_from("<I", frame, pos)[0]
        if w == 0:
            return words
        words.append(w)
        pos += 4 + (w & 0x7FFFFFFF)


def lz4_block_wave(data, start, end, first=None):
    """data[start:end] as the device's wavefront encodes it."""
    src = bytes(data[start:end])
    n = len(src)
    u32 = lambda i: struct.unpack_from("<I", src, i)[0]
    table = [0] * 4096
    out = bytearray()
    anchor = pos = 0
    mflimit, matchlimit = n - 12, n - 5
    while pos < mflimit:
        base = pos
        lanes = [i for i in range(base, base + 64) if i < mflimit]
        seq = {i: u32(i) for i in lanes}
        hsh = {i: ((seq[i] * 2654435761) & 0xFFFFFFFF) >> 20 for i in lanes}
        cand = {i: table[hsh[i]] for i in lanes}                     # all read before any is entered
        for i in lanes:
            table[hsh[i]] = max(table[hsh[i]], i)
        ok = [i for i in lanes if cand[i] < i and u32(cand[i]) == seq[i]]
        cur = base
        while True:
            hit = [i for i in ok if i >= cur]
            if not hit:
                break
            mpos, mc = hit[0], cand[hit[0]]
            length = 4
            while mpos + length < matchlimit and src[mpos + length] == src[mc + length]:
                length += 1
            out += W.lz4_sequence(src[anchor:mpos], mpos - mc, length)
            anchor = cur = mpos + length
            if cur >= base + 64:
                break
        pos = max(cur, base + 64)
    return bytes(out + W.lz4_sequence(src[anchor:]))


def info_node(hw, stream_name="events", source="scpose"):
    p = "/mainloop/output_file/outInfo/"
    return "".join([
        '<dv version="2.0"><node name="outInfo" path="%s">' % p, '<node name="0" path="%s0/">' % p,
        '<attr key="compression" type="int">0</attr>', '<attr key="originalModuleName" type="string">%s</attr>' % source,
        '<attr key="originalOutputName" type="string">%s</attr>' % stream_name,
        '<attr key="typeDescription" type="string">Array of events (polarity ON/OFF).</attr>',
        '<attr key="typeIdentifier" type="string">EVTS</attr>', '<node name="info" path="%s0/info/">' % p,
        '<attr key="sizeX" type="int">%d</attr>' % hw[1], '<attr key="sizeY" type="int">%d</attr>' % hw[0],
        '<attr key="source" type="string">%s</attr>' % source, "</node></node></node></dv>"]).encode()


def file_data_table(rows):
    """The size-prefixed FTAB flatbuffer, one definition at a time.  rows: (byte offset, size, events, first t, last t)."""
    n = len(rows)
    t0 = (48 + 4 * n + 7) // 8 * 8
    b = bytearray(struct.pack("<II4s", 0, 16, b"FTAB"))
    b += struct.pack("<HHHH", 6, 8, 4, 0)                            # 12: the root's vtable
    b += struct.pack("<iI", 8, 20)                                   # 20: the root table -> the vector at 44
    b += struct.pack("<HHHHHHHH", 14, 48, 16, 4, 24, 32, 40, 0)      # 28: the definitions' vtable
    b += struct.pack("<I", n)                                        # 44
    for k in range(n):
        b += struct.pack("<I", t0 + 48 * k - (48 + 4 * k))
    b += b"\0" * (t0 - len(b))
    for k, (off, size, cnt, ts, te) in enumerate(rows):
        b += struct.pack("<iiiiqqqq", t0 + 48 * k - 28, 0, int(size), 0, int(off), int(cnt), int(ts), int(te))
    struct.pack_into("<I", b, 0, len(b) - 4)
    return bytes(b)


def read_file_data_table(fb):
    """The rows of a size-prefixed FTAB flatbuffer, walked the flatbuffer way: [(offset, stream, size, events, first, last)]."""
    assert struct.unpack_from("<I", fb, 0)[0] == len(fb) - 4 and fb[8:12] == b"FTAB"
    b = fb[4:]
    field = lambda table, k: table + struct.unpack_from("<H", b, table - struct.unpack_from("<i", b, table)[0] + 4 + 2 * k)[0]
    root = struct.unpack_from("<I", b, 0)[0]
    f = field(root, 0)
    vec = f + struct.unpack_from("<I", b, f)[0]
    rows = []
    for k in range(struct.unpack_from("<I", b, vec)[0]):
        e = vec + 4 + 4 * k
        tab = e + struct.unpack_from("<I", b, e)[0]
        q = lambda j: struct.unpack_from("<q", b, field(tab, j))[0]
        sid, size = struct.unpack_from("<ii", b, field(tab, 1))
        rows.append((q(0), sid, size, q(2), q(3), q(4)))
    return rows


def packet_bounds(n, packet_events):
    return list(range(0, n, packet_events)) + [n]


def write(t, x, y, p, hw, compression="lz4", packet_events=10000, stream_name="events", source="scpose", block=W.lz4_block_greedy):
    """The bytes of the file."""
    code = {"none": W.NONE, "lz4": W.LZ4}[compression]
    squeeze = (lambda d: lz4_frame(d, block)) if code else (lambda d: d)
    head = W.io_header(code, -1, info_node(hw, stream_name, source))
    out = bytearray(MAGIC + struct.pack("<I", len(head)) + head)
    rows = []
    b = packet_bounds(len(t), packet_events)
    for lo, hi in zip(b[:-1], b[1:]):
        payload = squeeze(evts_flatbuffer(t[lo:hi], x[lo:hi], y[lo:hi], p[lo:hi]))
        rows.append((len(out), len(payload), hi - lo, t[lo] if hi > lo else 0, t[hi - 1] if hi > lo else 0))
        out += struct.pack("<ii", 0, len(payload)) + payload
    struct.pack_into("<q", out, TABLE_POSITION_AT, len(out))
    return bytes(out + squeeze(file_data_table(rows)))


def table_of(data):
    """The file data table of a file's bytes -> rows, decompressed and walked."""
    import events_aedat4_restated as RD
    compression, table_at, _, _ = RD.parse_header(data)
    raw = data[table_at:]
    return read_file_data_table(RD.lz4_frame(raw) if compression else raw)
