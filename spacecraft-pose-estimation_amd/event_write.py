"""Event files from device columns: text / CSV (the grammar ops.parse_events_csv reads), AEDAT-2.0 for jAER and AEDAT-4.0 for DV.

The bytes are made on the device (csrc/events_write.hip through ops.format_events_text / ops.pack_events_aedat2), a chunk of
rows at a time: while the file takes chunk k - 1 from one of two pinned host buffers, chunk k is formatted and copied into the
other on a side stream, and an event per buffer orders the two.  Rows are independent, so the concatenated chunks are the file.

AEDAT-2.0 follows the reference's v2ecore/output/aedat2_output.py (AEDat2Output): records of two big-endian 32-bit words, both
axes flipped, and from the first non-empty write the leading records whose first byte is '#' dropped, because a reader would take
them for header lines.  The header here holds no date, time or user line: two runs give identical files.

AEDAT-4.0 is what DV and dv-processing read (csrc/events_aedat4_read.hip states the format, csrc/events_aedat4_write.hip what is
written): the version line, a uint32 length and the IOHeader flatbuffer, one packet per `packet_events` events -- each the
packet's EVTS flatbuffer, raw or as one LZ4 frame made on the device -- and the FTAB file data table, to which the IOHeader's
dataTablePosition points.  Two deviations, as above: no date or user fields, so two runs give identical files, and the time
stamps are written as given (microseconds), without a rebase.
"""
import struct

import numpy as np

AEDAT2_SIZES = ((346, 260), (692, 520), (1280, 720), (640, 480), (240, 180))      # (width, height): the reference's five
AEDAT2_HEADER = (b"#!AER-DAT2.0\r\n"
                 b"# Polarity events written from device event columns by the scpose event writer\r\n"
                 b"# Each event is 8 bytes, two big-endian signed 32-bit words: the address, then the time stamp\r\n"
                 b"# Address word: polarity in bit 11 (1 = ON), x in bits 12-21, y in bits 22-31, both axes flipped (origin bottom right)\r\n"
                 b"# One time stamp tick is 1 us\r\n")
DEFAULT_CHUNK_ROWS = 1 << 20


def _ops():
    from . import ops
    return ops


class _Pipe:
    """Two pinned host buffers behind a side stream: put() queues the copy of a device chunk, the chunk before it goes to the
    file meanwhile."""

    def __init__(self, f, device):
        import torch
        self.torch = torch
        self.f = f
        self.device = device
        self.side = torch.cuda.Stream(device=device)
        self.side.wait_stream(torch.cuda.current_stream(device))     # the columns are complete before the side stream reads them
        self.host = [None, None]
        self.done = [torch.cuda.Event(), torch.cuda.Event()]
        self.pending = None                                          # (buffer index, bytes) of the chunk still to be written
        self.k = 0

    def put(self, make):
        """make() -> (uint8 device tensor, first byte to keep); runs on the side stream."""
        torch = self.torch
        b = self.k & 1
        with torch.cuda.stream(self.side):
            dev, skip = make()
            n = int(dev.numel()) - skip
            if n > 0:
                if self.host[b] is None or self.host[b].numel() < n:
                    self.host[b] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
                self.host[b][:n].copy_(dev[skip:], non_blocking=True)
                self.done[b].record(self.side)
        self.flush()                                                 # chunk k - 1 goes to the file while chunk k is copied
        if n > 0:
            self.pending = (b, n, dev)                               # dev: kept alive until its copy has been waited for
            self.k += 1

    def flush(self):
        if self.pending is not None:
            b, n, _ = self.pending
            self.done[b].synchronize()
            self.f.write(memoryview(self.host[b].numpy())[:n])
            self.pending = None

    def close(self):
        self.flush()
        self.torch.cuda.current_stream(self.device).wait_stream(self.side)


def _chunks(n, chunk_rows):
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be at least 1 (got %d)" % chunk_rows)
    return [(lo, min(lo + chunk_rows, n)) for lo in range(0, n, chunk_rows)]


def write_events_text(path, t, x, y, p, sep=" ", swap_xy=False, header=b"", chunk_rows=DEFAULT_CHUNK_ROWS):
    """Writes `header` and then one `t SEP x SEP y SEP p` line per event (ops.format_events_text) to `path`; the columns are
    device tensors and are never copied to the host.  Returns the number of bytes written."""
    ops = _ops()
    ops._sep_byte(sep)
    t, x, y, p, dev, n = ops._event_columns("write_events_text", t, x, y, p)
    with open(path, "wb") as f:
        f.write(header)
        pipe = _Pipe(f, dev)
        for lo, hi in _chunks(n, chunk_rows):
            pipe.put(lambda: (ops.format_events_text(t[lo:hi], x[lo:hi], y[lo:hi], p[lo:hi], sep=sep, swap_xy=swap_xy), 0))
        pipe.close()
        return f.tell()


def check_aedat2_size(hw):
    """(height, width) as integers; ValueError naming the sizes AEDAT-2.0 output exists for when it is none of them."""
    h, w = int(hw[0]), int(hw[1])
    if (w, h) not in AEDAT2_SIZES:
        raise ValueError("AEDAT-2.0 output: width=%d height=%d is not supported; the sizes are %s"
                         % (w, h, ", ".join("%dx%d" % s for s in AEDAT2_SIZES)))
    return h, w


def write_events_aedat2(path, t, x, y, p, hw, chunk_rows=DEFAULT_CHUNK_ROWS):
    """Writes an AEDAT-2.0 file of the events (t in microseconds, p in {0, 1}) for a sensor of hw = (height, width), one of
    AEDAT2_SIZES.  Returns the number of records written: the events minus the leading '#' records of the first chunk."""
    ops = _ops()
    h, w = check_aedat2_size(hw)
    t, x, y, p, dev, n = ops._event_columns("write_events_aedat2", t, x, y, p)
    state = {"first": True, "records": 0}

    def make(lo, hi):
        out, lead = ops.pack_events_aedat2(t[lo:hi], x[lo:hi], y[lo:hi], p[lo:hi], (h, w))
        skip = lead if state["first"] else 0                         # the chop: the first non-empty chunk only
        state["first"] = False
        state["records"] += hi - lo - skip
        return out, 8 * skip

    with open(path, "wb") as f:
        f.write(AEDAT2_HEADER)
        pipe = _Pipe(f, dev)
        for lo, hi in _chunks(n, chunk_rows):
            pipe.put(lambda: make(lo, hi))
        pipe.close()
    return state["records"]



AEDAT4_MAGIC = b"#!AER-DAT4.0\r\n"
AEDAT4_COMPRESSION = {"none": 0, "lz4": 1}                             # the IOHeader's value
AEDAT4_PACKET_EVENTS = 10000       # DV cuts a camera's stream by time into packets of this order; 160 KB, three LZ4 blocks
AEDAT4_TABLE_POSITION_AT = len(AEDAT4_MAGIC) + 4 + 32                  # dataTablePosition in the file (aedat4_io_header)
AEDAT4_STREAM_ID = 0


def aedat4_info_node(hw, stream_name="events", source="scpose", stream_id=AEDAT4_STREAM_ID):
    """The IOHeader's infoNode: XML that names one EVTS stream with its sizeX / sizeY, in the shape DV writes and
    event_read._aedat4_streams parses."""
    from xml.sax.saxutils import escape
    path = "/mainloop/output_file/outInfo/"
    return ('<dv version="2.0"><node name="outInfo" path="%s">'
            '<node name="%d" path="%s%d/">'
            '<attr key="compression" type="int">0</attr><attr key="originalModuleName" type="string">%s</attr>'
            '<attr key="originalOutputName" type="string">%s</attr><attr key="typeDescription" type="string">Array of events '
            '(polarity ON/OFF).</attr><attr key="typeIdentifier" type="string">EVTS</attr>'
            '<node name="info" path="%s%d/info/">'
            '<attr key="sizeX" type="int">%d</attr><attr key="sizeY" type="int">%d</attr><attr key="source" type="string">%s</attr>'
            '</node></node></node></dv>'
            % (path, stream_id, path, stream_id, escape(source), escape(stream_name), path, stream_id, int(hw[1]), int(hw[0]),
               escape(source))).encode()


def aedat4_io_header(compression, data_table_position, info):
    """The IOHeader flatbuffer (identifier IOHE): the vtable of three fields at 8, the table at 24 -- compression int32 at 28,
    dataTablePosition int64 at 32, the uoffset of infoNode at 40 -- and the string at 44."""
    return struct.pack("<I4s", 24, b"IOHE") + struct.pack("<HHHHH", 10, 20, 4, 8, 16) + b"\0" * 6 + \
        struct.pack("<iiqI", 16, compression, data_table_position, 4) + struct.pack("<I", len(info)) + info + b"\0"


def aedat4_packet_bounds(n, packet_events):
    """Row boundaries of the packets of n events, `packet_events` to a packet and the rest in the last: int64, n_packets + 1."""
    packet_events = int(packet_events)
    if not 1 <= packet_events <= 524284:
        raise ValueError("packet_events must be 1 .. 524284, the events of the largest packet the reader takes (got %d)" % packet_events)
    b = np.arange(0, n, packet_events, dtype=np.int64)
    return np.append(b, np.int64(n)) if n else np.zeros(1, dtype=np.int64)


def aedat4_file_data_table(rows, stream_id=AEDAT4_STREAM_ID):
    """The size-prefixed FTAB flatbuffer of DV's FileDataTable.  rows: (n, 5) int64, per packet the byte offset of its header in
    the file, the payload size, the number of events, the first and the last time stamp.  Positions from the size prefix: root
    offset at 4, "FTAB" at 8, the root's vtable at 12 and table at 20, the one vtable all definitions share at 28 (ByteOffset at
    16, PacketInfo {StreamID, Size} at 4, NumElements 24, TimestampStart 32, TimestampEnd 40 of a 48-byte table), the vector's
    count at 44, its uoffsets from 48, the tables from the next multiple of 8."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    n = rows.shape[0]
    t0 = (48 + 4 * n + 7) & ~7
    head = struct.pack("<I4s", 16, b"FTAB") + struct.pack("<HHHH", 6, 8, 4, 0) + struct.pack("<iI", 8, 20) + \
        struct.pack("<HHHHHHHH", 14, 48, 16, 4, 24, 32, 40, 0) + struct.pack("<I", n)
    at = t0 + 48 * np.arange(n, dtype=np.int64)
    offs = (at - (48 + 4 * np.arange(n, dtype=np.int64))).astype("<u4").tobytes()
    tab = np.zeros(n, dtype=np.dtype([("so", "<i4"), ("sid", "<i4"), ("size", "<i4"), ("pad", "<i4"), ("off", "<i8"), ("cnt", "<i8"),
                                      ("ts", "<i8"), ("te", "<i8")]))
    tab["so"], tab["sid"], tab["size"], tab["off"] = at - 28, stream_id, rows[:, 1], rows[:, 0]
    tab["cnt"], tab["ts"], tab["te"] = rows[:, 2], rows[:, 3], rows[:, 4]
    body = head + offs + b"\0" * (t0 - 48 - 4 * n) + tab.tobytes()
    return struct.pack("<I", len(body)) + body


def write_events_aedat4(path, t, x, y, p, hw, compression="lz4", packet_events=AEDAT4_PACKET_EVENTS, chunk_rows=DEFAULT_CHUNK_ROWS,
                        stream_name="events", source="scpose"):
    """Writes an AEDAT-4.0 file of the events (t in microseconds, written as given; p in {0, 1}) for a sensor of hw = (height,
    width), any size up to 32767 each.  compression: 'lz4' (what DV writes; the default) or 'none'.  One packet per
    `packet_events` events; the packets are made on the device (ops.pack_events_aedat4), a whole number of them per call and at
    most chunk_rows rows (one packet where chunk_rows is smaller), so the file does not depend on chunk_rows.  The file data
    table follows the packets, under the file's compression, and dataTablePosition is patched to point at it.  An empty stream
    gives a file with the header and an empty table.  Returns the number of packets."""
    ops = _ops()
    ops._aedat4_compression("write_events_aedat4", compression)
    h, w = int(hw[0]), int(hw[1])
    if not (1 <= h <= 32767 and 1 <= w <= 32767):
        raise ValueError("AEDAT-4.0 output: width=%d height=%d is not supported: each 1 .. 32767" % (w, h))
    t, x, y, p, dev, n = ops._event_columns("write_events_aedat4", t, x, y, p)
    packet_events = int(packet_events)
    aedat4_packet_bounds(0, packet_events)
    rows_per_call = max(int(chunk_rows) // packet_events, 1) * packet_events
    head = aedat4_io_header(AEDAT4_COMPRESSION[compression], -1, aedat4_info_node((h, w), stream_name, source))
    start = len(AEDAT4_MAGIC) + 4 + len(head)
    state = {"at": start, "rows": []}

    def make(lo, hi):
        out, table = ops.pack_events_aedat4(t[lo:hi], x[lo:hi], y[lo:hi], p[lo:hi], (h, w), aedat4_packet_bounds(hi - lo, packet_events),
                                            compression=compression, stream_id=AEDAT4_STREAM_ID)
        table[:, 0] += state["at"]
        state["at"] += int(out.numel())
        state["rows"].append(table)
        return out, 0

    with open(path, "wb") as f:
        f.write(AEDAT4_MAGIC + struct.pack("<I", len(head)) + head)
        pipe = _Pipe(f, dev)
        for lo, hi in _chunks(n, rows_per_call):
            pipe.put(lambda: make(lo, hi))
        pipe.close()
        rows = np.concatenate(state["rows"]) if state["rows"] else np.zeros((0, 5), dtype=np.int64)
        ftab = aedat4_file_data_table(rows)
        if compression == "lz4":
            import torch
            with torch.cuda.device(dev):
                framed, _ = ops.lz4_frame_bytes(torch.from_numpy(np.frombuffer(ftab, dtype=np.uint8).copy()).to(dev))
            ftab = framed[8:].cpu().numpy().tobytes()                  # the frame without the record header
        table_at = f.tell()
        assert table_at == state["at"], (table_at, state["at"])
        f.write(ftab)
        f.seek(AEDAT4_TABLE_POSITION_AT)
        f.write(struct.pack("<q", table_at))
    return int(rows.shape[0])
