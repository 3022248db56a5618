"""Device columns from AEDAT-2.0, AEDAT-3.1 and AEDAT-4.0 event files: the mirror of event_write.py.

An AEDAT-2.0 file is a text header, the run of lines that start with '#' and end with '\\n', whose first line is
`#!AER-DAT2.0`, followed by 8-byte records of two big-endian 32-bit words (address, time stamp).  The header is split off on the
host (a few lines); the records are uploaded in one piece and decoded on the device (csrc/events_aedat2_read.hip through
ops.unpack_events_aedat2).  Both jAER's DAVIS recordings (layout 'davis') and the files event_write.write_events_aedat2 and the
reference's AEDat2Output write (layout 'v2e') are read.  AEDAT-1.0 and 3.x are other formats and are refused by name; so is 4.0 by
the AEDAT-2.0 entry points: callers sniff the first 14 bytes (is_aedat4_path) and dispatch before them.

An AEDAT-4.0 file (a DVXplorer / DV recording) is `#!AER-DAT4.0\r\n`, a length-prefixed IOHeader flatbuffer (compression, the
position of the file data table, an XML node that names the streams), then packets: int32 stream id, int32 size, the payload, a
flatbuffer that is raw, one LZ4 frame or Zstandard frames.  parse_aedat4 reads the header and walks the packet headers on the host (eight bytes
per packet); read_events_aedat4 uploads the file in one piece and the payloads of the event streams are decompressed and
unpacked on the device (csrc/events_aedat4_read.hip and, for ZSTD, csrc/events_aedat4_zstd.hip, which state the formats, through
ops.unpack_events_aedat4).

An AEDAT-3.1 file (a cAER / early DV recording of a DAVIS or DVS128 camera) is a '#' text header with '\\r\\n' line ends that
starts with `#!AER-DAT3.1` and ends with `#!END-HEADER`, then packets: a 28-byte header and eventCapacity * eventSize payload bytes.
parse_aedat3 reads the text and walks the packet headers on the host; read_events_aedat3 uploads the file in one piece and the
polarity packets of one source are unpacked on the device (csrc/events_aedat3_read.hip, which states the format, through
ops.unpack_events_aedat3).  Such a file usually carries the .aedat name: callers sniff it (is_aedat3_path) before the AEDAT-2.0
entry points, which still refuse it by name, as parse_aedat4 does.  AEDAT-3.0, formats other than RAW and the decoding of frame,
IMU and special events stay out; there is no 3.1 writer.
"""
import re
import struct

import numpy as np

AEDAT2_MAGIC = b"#!AER-DAT"
AEDAT3_MAGIC = b"#!AER-DAT3."
AEDAT4_MAGIC = b"#!AER-DAT4.0\r\n"
MAX_HEADER_BYTES = 1 << 20


class UnsupportedAedat(ValueError):
    """The file is not AEDAT-2.0: another version of the format, no version line, or a header that does not end."""


def split_aedat2_header(prefix):
    """The offset of the first record in `prefix`, the first bytes of an AEDAT-2.0 file (or all of it).  The header is the run
    of lines that start with '#' and end with '\\n' ('\\r\\n' included); its first line must be `#!AER-DAT2.0`.  Raises
    UnsupportedAedat naming the version for `#!AER-DAT1.0`, `3.x` and `4.0`; a file without a version line is what jAER takes
    for AEDAT-1.0 and is refused as such; so is a header that has not ended after 1 MiB."""
    data = bytes(prefix[:MAX_HEADER_BYTES + 1]) if not isinstance(prefix, bytes) else prefix
    if not data.startswith(AEDAT2_MAGIC):
        raise UnsupportedAedat("no '#!AER-DAT' version line: jAER reads such a file as AEDAT-1.0, which is not supported "
                               "(only AEDAT-2.0 is)")
    end = data.find(b"\n", 0, MAX_HEADER_BYTES)
    first = data[:end if end >= 0 else 64].rstrip(b"\r")
    m = re.match(rb"#!AER-DAT(\d+(?:\.\d+)?)", first)
    version = m.group(1).decode() if m else first[len(AEDAT2_MAGIC):len(AEDAT2_MAGIC) + 16].decode("latin-1")
    if first != b"#!AER-DAT2.0":
        raise UnsupportedAedat("AEDAT-%s is not supported (only AEDAT-2.0 is): the first line is %r" % (version, first[:40]))
    off = 0
    while off < len(data) and data[off:off + 1] == b"#":
        if off >= MAX_HEADER_BYTES:
            raise UnsupportedAedat("the '#' header has not ended after %d bytes: not an AEDAT-2.0 file" % MAX_HEADER_BYTES)
        nl = data.find(b"\n", off, MAX_HEADER_BYTES + 1)
        if nl < 0:
            if len(data) > MAX_HEADER_BYTES:
                raise UnsupportedAedat("the '#' header has not ended after %d bytes: not an AEDAT-2.0 file" % MAX_HEADER_BYTES)
            break                                                    # a '#' without a line end: the first record's byte
        off = nl + 1
    return off


# (key, name suffixes, first bytes), in the order they are tested: a suffix or the magic decides.  An AEDAT-3.1 recording usually
# carries the .aedat name of a 2.0 one, so its magic is looked at before that suffix.
EVENT_FORMATS = (("aedat4", (".aedat4",), AEDAT4_MAGIC),
                 ("aedat3", (".aedat3",), AEDAT3_MAGIC),
                 ("aedat2", (".aedat", ".aedat2"), AEDAT2_MAGIC))


def _sniff(path, suffixes, magic):
    if str(path).lower().endswith(suffixes):
        return True
    try:
        with open(path, "rb") as f:
            return f.read(len(magic)) == magic
    except OSError:
        return False


def events_format(path):
    """'aedat4', 'aedat3' or 'aedat2' for an event file of that format, by its name or its first bytes (EVENT_FORMATS, tested in
    that order); None for anything else: text, or a path that cannot be read."""
    return next((key for key, suffixes, magic in EVENT_FORMATS if _sniff(path, suffixes, magic)), None)


def is_aedat_path(path):
    """True for a path that ends in .aedat / .aedat2 or a file whose first bytes are '#!AER-DAT'."""
    return _sniff(path, *EVENT_FORMATS[2][1:])


def is_aedat4_path(path):
    """True for a path that ends in .aedat4 or a file whose first 14 bytes are the AEDAT-4.0 version line."""
    return _sniff(path, *EVENT_FORMATS[0][1:])


def is_aedat3_path(path):
    """True for a path that ends in .aedat3 or a file whose first bytes are '#!AER-DAT3.' (a 3.1 recording usually carries the
    .aedat name of a 2.0 one: look here first)."""
    return _sniff(path, *EVENT_FORMATS[1][1:])


def _load(path_or_bytes):
    """A path, or a file's bytes -> the file as a uint8 NumPy array (read-only when it views the caller's bytes)."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return np.frombuffer(path_or_bytes, dtype=np.uint8)
    return np.fromfile(path_or_bytes, dtype=np.uint8)


def _device(device):
    import torch
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _upload(host, dev):
    """The whole file to the device in one piece; only a read-only buffer is copied first."""
    import torch
    return torch.from_numpy(host.copy() if not host.flags.writeable else host).to(dev)


def read_events_file(path, hw=None, device=None, **kw):
    """An event file of any EVENT_FORMATS format -> the (t, x, y, p, info) of its reader (read_events_aedat4 / _aedat3 / _aedat2,
    which takes kw); None for a path events_format does not know: text."""
    fmt = events_format(path)
    return READERS[fmt](path, hw=hw, device=device, **kw) if fmt else None


def read_events_aedat2(path_or_bytes, hw, device=None, **unpack_kwargs):
    """An AEDAT-2.0 file (a path, or its bytes) -> (t int64, x int32, y int32, p int8, info) on `device` (default: the current
    one), the kept events in file order.  hw = (height, width) of the sensor; unpack_kwargs are ops.unpack_events_aedat2's
    (layout, flip_x, flip_y, unwrap, t_divisor).  The body is uploaded in one piece, as ops.parse_events_csv uploads its text.
    A trailing partial record is ignored and reported as info['trailing_bytes']; info holds the decoder's counters as well."""
    from . import ops
    host = _load(path_or_bytes)
    off = split_aedat2_header(host[:MAX_HEADER_BYTES + 1].tobytes())
    n = (len(host) - off) // 8
    body = host[off:off + 8 * n]
    buf = _upload(body.copy(), _device(device))                      # the copy starts the records on an aligned address
    t, x, y, p, info = ops.unpack_events_aedat2(buf, hw, **unpack_kwargs)
    info["trailing_bytes"] = int(len(host) - off - 8 * n)
    return t, x, y, p, info


# ------------------------------------------------------------------ AEDAT-4.0
AEDAT4_COMPRESSION = {0: "NONE", 1: "LZ4", 2: "LZ4_HIGH", 3: "ZSTD", 4: "ZSTD_HIGH"}


class UnsupportedAedat4(ValueError):
    """An AEDAT-4.0 file this reader does not take: ZSTD packets where no ZSTD decoder is on offer, an unknown compression, no
    IOHeader, no event stream."""


class Aedat4Header:
    """What parse_aedat4 found: compression (the IOHeader's value), streams {id: (type, sizeX, sizeY)}, data_table_position,
    the packet table as NumPy arrays (packet_offset: payload offset in the file, packet_size, packet_stream), trailing_bytes."""

    def __init__(self, compression, streams, data_table_position, packet_offset, packet_size, packet_stream, trailing_bytes):
        self.compression = compression
        self.streams = streams
        self.data_table_position = data_table_position
        self.packet_offset = packet_offset
        self.packet_size = packet_size
        self.packet_stream = packet_stream
        self.trailing_bytes = trailing_bytes

    def event_streams(self):
        """The ids of the EVTS streams, in the header's order."""
        return [sid for sid, s in self.streams.items() if s[0] == "EVTS"]


def _fb_field(buf, table, index):
    """Position of field `index` of the flatbuffer table at `table`, None when it is absent; every step inside buf."""
    if table < 0 or table + 4 > len(buf):
        raise UnsupportedAedat4("the IOHeader flatbuffer is damaged: table at %d of %d bytes" % (table, len(buf)))
    vt = table - struct.unpack_from("<i", buf, table)[0]
    if vt < 0 or vt + 4 > len(buf):
        raise UnsupportedAedat4("the IOHeader flatbuffer is damaged: vtable at %d of %d bytes" % (vt, len(buf)))
    vsize = struct.unpack_from("<H", buf, vt)[0]
    if vt + vsize > len(buf):
        raise UnsupportedAedat4("the IOHeader flatbuffer is damaged: vtable of %d bytes at %d" % (vsize, vt))
    if 4 + 2 * index + 2 > vsize:
        return None
    slot = struct.unpack_from("<H", buf, vt + 4 + 2 * index)[0]
    return table + slot if slot else None


def _aedat4_streams(xml):
    """{id: (typeIdentifier, sizeX, sizeY)} of the nodes under <node name="outInfo"> of the IOHeader's infoNode."""
    import xml.etree.ElementTree as ET
    streams = {}
    try:
        root = ET.fromstring(xml)
    except ET.ParseError as e:
        raise UnsupportedAedat4("the IOHeader's infoNode is not XML: %s" % e)
    for out in root.iter("node"):
        if out.get("name") != "outInfo":
            continue
        for node in out.findall("node"):
            try:
                sid = int(node.get("name"))
            except (TypeError, ValueError):
                continue
            kind = next((a.text for a in node.findall("attr") if a.get("key") == "typeIdentifier"), None)
            size = {}
            for info in node.findall("node"):
                if info.get("name") == "info":
                    for a in info.findall("attr"):
                        if a.get("key") in ("sizeX", "sizeY"):
                            try:
                                size[a.get("key")] = int(a.text)
                            except (TypeError, ValueError):
                                raise UnsupportedAedat4("stream %d: %s is %r in the IOHeader, not an integer" % (sid, a.get("key"), a.text))
            streams[sid] = (kind, size.get("sizeX"), size.get("sizeY"))
    return streams


def parse_aedat4(data, zstd=False):
    """The header and packet table of an AEDAT-4.0 file (its bytes) -> Aedat4Header.  Packets run to dataTablePosition when that is
    >= 0, else to the end; a last packet whose header or payload is cut off is dropped and reported as trailing_bytes, as the
    AEDAT-2.0 reader reports a partial record.  zstd: whether the caller has a ZSTD decoder on offer (read_events_aedat4 has the
    device's); without one, raises UnsupportedAedat4 for ZSTD / ZSTD_HIGH (there is no host fallback: no zstd module is at hand).
    Raises it too for an unknown compression value, a missing IOHE identifier and a file without an event stream."""
    buf = data if isinstance(data, (bytes, bytearray, memoryview)) else bytes(data)       # a memoryview is walked, not copied
    if buf[:len(AEDAT4_MAGIC)] != AEDAT4_MAGIC:
        raise UnsupportedAedat4("not an AEDAT-4.0 file: the first 14 bytes are %r" % bytes(buf[:14]))
    at = len(AEDAT4_MAGIC)
    if at + 4 > len(buf):
        raise UnsupportedAedat4("the file ends before the IOHeader")
    n = struct.unpack_from("<I", buf, at)[0]
    head = bytes(buf[at + 4:at + 4 + n])
    if len(head) < n or n < 8 or head[4:8] != b"IOHE":
        raise UnsupportedAedat4("no IOHE identifier: the %d bytes after the version line are not an IOHeader" % n)
    root = struct.unpack_from("<I", head, 0)[0]
    f = _fb_field(head, root, 0)
    compression = struct.unpack_from("<i", head, f)[0] if f is not None and f + 4 <= n else 0
    f = _fb_field(head, root, 1)
    table_at = struct.unpack_from("<q", head, f)[0] if f is not None and f + 8 <= n else -1
    f = _fb_field(head, root, 2)
    xml = b""
    if f is not None and f + 4 <= n:
        spos = f + struct.unpack_from("<I", head, f)[0]
        if spos + 4 <= n:
            xml = head[spos + 4:spos + 4 + struct.unpack_from("<I", head, spos)[0]]
    if compression in (3, 4) and not zstd:
        raise UnsupportedAedat4("the packets are %s compressed: only NONE, LZ4 and LZ4_HIGH are read, and there is no host "
                                "fallback (no zstd module)" % AEDAT4_COMPRESSION[compression])
    if compression not in AEDAT4_COMPRESSION:
        raise UnsupportedAedat4("unknown compression value %d in the IOHeader (0 NONE, 1 LZ4, 2 LZ4_HIGH)" % compression)
    streams = _aedat4_streams(xml) if xml else {}
    if not any(s[0] == "EVTS" for s in streams.values()):
        raise UnsupportedAedat4("no event stream: the IOHeader names %s" % (sorted((k, v[0]) for k, v in streams.items()) or "no streams"))
    pos = at + 4 + n
    end = min(table_at, len(buf)) if table_at >= 0 else len(buf)
    offs, sizes, sids, trailing = [], [], [], 0
    while pos < end:
        if pos + 8 > end:
            trailing = end - pos
            break
        sid, size = struct.unpack_from("<ii", buf, pos)
        if size < 0 or pos + 8 + size > end:
            trailing = end - pos
            break
        offs.append(pos + 8)
        sizes.append(size)
        sids.append(sid)
        pos += 8 + size
    return Aedat4Header(compression, streams, table_at, np.asarray(offs, dtype=np.int64), np.asarray(sizes, dtype=np.int64),
                        np.asarray(sids, dtype=np.int32), int(trailing))


def read_events_aedat4(path_or_bytes, hw=None, stream=None, rebase=True, verify=True, device=None):
    """An AEDAT-4.0 file (a path, or its bytes) -> (t int64, x int32, y int32, p int8, info) on `device` (default: the current
    one), the events of the file's EVTS streams in file order -- what the reference's aedat_to_csv.py loop collects.  hw defaults
    to the stream's (sizeY, sizeX); stream: one stream id, default every EVTS stream; rebase: subtract the first event's time
    stamp, as the reference does; verify: check the LZ4 block and content checksums or ZSTD content checksums the file carries.  The file is uploaded
    once, as ops.parse_events_csv uploads its text.  info: n_events, n_packets, t0, n_backward, n_out_of_range, compression, hw,
    streams, trailing_bytes.  Raises UnsupportedAedat4 (parse_aedat4) and ValueError (ops.unpack_events_aedat4)."""
    from . import ops
    host = _load(path_or_bytes)
    head = parse_aedat4(memoryview(host), zstd=True)
    if stream is None:
        ids = head.event_streams()
    else:
        ids = [int(stream)]
        if ids[0] not in head.streams or head.streams[ids[0]][0] != "EVTS":
            raise UnsupportedAedat4("no event stream %r: the IOHeader names %s" % (stream, sorted((k, v[0]) for k, v in head.streams.items())))
    if hw is None:
        _, sx, sy = head.streams[ids[0]]
        if sx is None or sy is None:
            raise UnsupportedAedat4("stream %d has no sizeX / sizeY in the IOHeader: give hw" % ids[0])
        hw = (sy, sx)
    keep = np.isin(head.packet_stream, ids)
    packets = np.stack([head.packet_offset[keep], head.packet_size[keep]], axis=1)
    t, x, y, p, info = ops.unpack_events_aedat4(_upload(host, _device(device)), packets, head.compression, hw, rebase=rebase, verify=verify)
    info.update(compression=int(head.compression), hw=(int(hw[0]), int(hw[1])), streams=tuple(ids),
                trailing_bytes=int(head.trailing_bytes))
    return t, x, y, p, info


# ------------------------------------------------------------------ AEDAT-3.1
AEDAT3_PACKET_HEADER = 28
AEDAT3_TYPES = {0: "special", 1: "polarity", 2: "frame", 3: "IMU6", 4: "IMU9"}
AEDAT3_POLARITY = 1
# (prefix of the '#Source' name, (height, width)); the longest prefix that matches wins
AEDAT3_SENSORS = (("DVS128", (128, 128)), ("DAVIS240", (180, 240)), ("DAVIS346", (260, 346)), ("DAVIS640", (480, 640)))


class UnsupportedAedat3(ValueError):
    """An AEDAT-3.1 file this reader does not take: AEDAT-3.0, a format other than RAW, a header that does not end, a packet
    header that contradicts itself, a source whose sensor size is not known, several polarity sources and none chosen."""


class Aedat3Header:
    """What parse_aedat3 found: sources {id: name}, the packet table as NumPy arrays (packet_offset: payload offset in the file,
    packet_events: eventNumber, packet_valid: eventValid, packet_overflow: eventTSOverflow, packet_source, packet_type) with one
    row per packet of ANY type, other_packets {type: count} of the packets that are not polarity packets, trailing_bytes."""

    def __init__(self, sources, packet_offset, packet_events, packet_valid, packet_overflow, packet_source, packet_type, other_packets,
                 trailing_bytes):
        self.sources = sources
        self.packet_offset = packet_offset
        self.packet_events = packet_events
        self.packet_valid = packet_valid
        self.packet_overflow = packet_overflow
        self.packet_source = packet_source
        self.packet_type = packet_type
        self.other_packets = other_packets
        self.trailing_bytes = trailing_bytes

    def polarity_sources(self):
        """The ids of the sources that carry polarity packets, ascending."""
        return sorted(set(int(s) for s in self.packet_source[self.packet_type == AEDAT3_POLARITY]))


def aedat3_sensor_hw(name):
    """(height, width) of the camera a '#Source' line names: DVS128, DAVIS240*, DAVIS346*, DAVIS640; None for any other name."""
    for prefix, hw in AEDAT3_SENSORS:
        if str(name).strip().upper().startswith(prefix):
            return hw
    return None


def _aedat3_header(buf):
    """The text header of an AEDAT-3.1 file -> ({source id: name}, offset of the first packet)."""
    first = bytes(buf[:64]).split(b"\n", 1)[0].rstrip(b"\r")
    if not first.startswith(b"#!AER-DAT"):
        raise UnsupportedAedat3("not an AEDAT-3.1 file: the first bytes are %r" % bytes(buf[:14]))
    if first == b"#!AER-DAT3.0":
        raise UnsupportedAedat3("AEDAT-3.0 is not supported (only AEDAT-3.1 is): its packet header differs")
    if first != b"#!AER-DAT3.1":
        raise UnsupportedAedat3("not an AEDAT-3.1 file: the first line is %r" % first[:40])
    head = bytes(buf[:MAX_HEADER_BYTES])
    mark = b"#!END-HEADER\r\n"
    end = head.find(b"\r\n" + mark)
    if end < 0:
        raise UnsupportedAedat3("no '#!END-HEADER' line in the first %d bytes: not an AEDAT-3.1 file" % MAX_HEADER_BYTES)
    sources, fmt = {}, None
    for line in head[:end].split(b"\r\n")[1:]:
        if not line.startswith(b"#"):
            raise UnsupportedAedat3("a header line does not start with '#': %r" % line[:40])
        text = line.decode("latin-1")
        if text.startswith("#Format:"):
            fmt = text[len("#Format:"):].strip()
        m = re.match(r"#Source\s+(-?\d+):\s*(.*)$", text)
        if m:
            sources[int(m.group(1))] = m.group(2).strip()
    if fmt != "RAW":
        raise UnsupportedAedat3("the format is %s: only '#Format: RAW' is read" % ("%r" % fmt if fmt is not None else "not stated"))
    if not sources:
        raise UnsupportedAedat3("the header names no '#Source <id>: <name>'")
    return sources, end + 2 + len(mark)


def parse_aedat3(data):
    """The header and packet table of an AEDAT-3.1 file (its bytes) -> Aedat3Header.  Packets run to the end of the file; a last
    packet whose header or payload is cut off is dropped and reported as trailing_bytes, as parse_aedat4 does.  Packets that are not
    polarity packets (special, frame, IMU6, IMU9, anything else) are stepped over by eventCapacity * eventSize and counted per type.
    Raises UnsupportedAedat3 for AEDAT-3.0, a '#Format:' other than RAW, a header without '#!END-HEADER' in its first 1 MiB, and,
    naming the packet's index, for a packet header with a negative field, eventSize <= 0, eventNumber > eventCapacity, eventValid >
    eventNumber, a payload size beyond int64, or a polarity packet whose eventSize is not 8 or whose eventTSOffset is not 4."""
    buf = data if isinstance(data, (bytes, bytearray, memoryview)) else bytes(data)       # a memoryview is walked, not copied
    sources, pos = _aedat3_header(buf)
    end = len(buf)
    offs, nums, valids, overs, srcs, types, other, trailing = [], [], [], [], [], [], {}, 0
    k = 0
    while pos < end:
        if pos + AEDAT3_PACKET_HEADER > end:
            trailing = end - pos
            break
        etype, source, size, ts_at, overflow, capacity, number, valid = struct.unpack_from("<hhiiiiii", buf, pos)
        fields = (("eventType", etype), ("eventSource", source), ("eventSize", size), ("eventTSOffset", ts_at),
                  ("eventTSOverflow", overflow), ("eventCapacity", capacity), ("eventNumber", number), ("eventValid", valid))
        for name, value in fields:
            if value < 0:
                raise UnsupportedAedat3("packet %d at byte %d: %s is negative (%d)" % (k, pos, name, value))
        if size <= 0:
            raise UnsupportedAedat3("packet %d at byte %d: eventSize is %d" % (k, pos, size))
        if number > capacity:
            raise UnsupportedAedat3("packet %d at byte %d: eventNumber %d exceeds eventCapacity %d" % (k, pos, number, capacity))
        if valid > number:
            raise UnsupportedAedat3("packet %d at byte %d: eventValid %d exceeds eventNumber %d" % (k, pos, valid, number))
        payload = capacity * size                                        # Python integers: the product itself cannot wrap
        if payload > (1 << 63) - 1:
            raise UnsupportedAedat3("packet %d at byte %d: eventCapacity * eventSize does not fit in int64" % (k, pos))
        if etype == AEDAT3_POLARITY and (size != 8 or ts_at != 4):
            raise UnsupportedAedat3("packet %d at byte %d: a polarity packet with eventSize %d and eventTSOffset %d (8 and 4 are read)"
                                    % (k, pos, size, ts_at))
        if pos + AEDAT3_PACKET_HEADER + payload > end:
            trailing = end - pos
            break
        offs.append(pos + AEDAT3_PACKET_HEADER)
        nums.append(number)
        valids.append(valid)
        overs.append(overflow)
        srcs.append(source)
        types.append(etype)
        if etype != AEDAT3_POLARITY:
            other[etype] = other.get(etype, 0) + 1
        pos += AEDAT3_PACKET_HEADER + payload
        k += 1
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    return Aedat3Header(sources, i64(offs), i64(nums), i64(valids), i64(overs), np.asarray(srcs, dtype=np.int32),
                        np.asarray(types, dtype=np.int32), other, int(trailing))


def read_events_aedat3(path_or_bytes, hw=None, source=None, rebase=True, device=None):
    """An AEDAT-3.1 file (a path, or its bytes) -> (t int64, x int32, y int32, p int8, info) on `device` (default: the current
    one), the valid polarity events of one source in file order, t in microseconds.  hw defaults to the size of the camera the
    '#Source' line names (aedat3_sensor_hw); source: the source id, needed only when several sources carry polarity packets;
    rebase: subtract the first event's time stamp, as the AEDAT-4.0 reader does.  The file is uploaded once and the device gets one
    descriptor per polarity packet of the source (csrc/events_aedat3_read.hip through ops.unpack_events_aedat3).  info: n_events,
    n_packets, n_invalid (events dropped because their valid bit is clear), t0, n_backward, n_out_of_range, sources (the ids
    read), other_packets {type: count}, trailing_bytes, hw.  Raises UnsupportedAedat3 (parse_aedat3, the source, the size) and
    ValueError (ops.unpack_events_aedat3).  Frame, IMU and special events are counted and not decoded."""
    from . import ops
    host = _load(path_or_bytes)
    head = parse_aedat3(memoryview(host))
    carrying = head.polarity_sources()
    if source is None:
        if len(carrying) > 1:
            raise UnsupportedAedat3("sources %s all carry polarity packets: give source, one of them (%s)" % (
                ", ".join(str(s) for s in carrying), ", ".join("%d: %s" % (s, head.sources.get(s, "?")) for s in carrying)))
        sid = carrying[0] if carrying else min(head.sources)
    else:
        sid = int(source)
        if sid not in head.sources and sid not in carrying:
            raise UnsupportedAedat3("no source %r: the header names %s" % (source, sorted(head.sources.items())))
    if hw is None:
        hw = aedat3_sensor_hw(head.sources.get(sid, ""))
        if hw is None:
            raise UnsupportedAedat3("source %d is %r, a camera whose sensor size is not known here (DVS128, DAVIS240, DAVIS346, "
                                    "DAVIS640 are): give the size, hw = (height, width)" % (sid, head.sources.get(sid)))
    keep = (head.packet_type == AEDAT3_POLARITY) & (head.packet_source == sid)
    packets = np.stack([head.packet_offset[keep], head.packet_events[keep], head.packet_overflow[keep]], axis=1)
    t, x, y, p, info = ops.unpack_events_aedat3(_upload(host, _device(device)), packets, hw, rebase=rebase)
    info.update(n_invalid=int(packets[:, 1].sum()) - info["n_events"], sources=(sid,), other_packets=dict(head.other_packets),
                trailing_bytes=int(head.trailing_bytes), hw=(int(hw[0]), int(hw[1])))
    return t, x, y, p, info


READERS = {"aedat4": read_events_aedat4, "aedat3": read_events_aedat3, "aedat2": read_events_aedat2}
