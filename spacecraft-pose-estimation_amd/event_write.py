"""Event files from device columns: text / CSV (the grammar ops.parse_events_csv reads) and AEDAT-2.0 for jAER.

The bytes are made on the device (csrc/events_write.hip through ops.format_events_text / ops.pack_events_aedat2), a chunk of
rows at a time: while the file takes chunk k - 1 from one of two pinned host buffers, chunk k is formatted and copied into the
other on a side stream, and an event per buffer orders the two.  Rows are independent, so the concatenated chunks are the file.

AEDAT-2.0 follows the reference's v2ecore/output/aedat2_output.py (AEDat2Output): records of two big-endian 32-bit words, both
axes flipped, and from the first non-empty write the leading records whose first byte is '#' dropped, because a reader would take
them for header lines.  The header here holds no date, time or user line: two runs give identical files.
"""
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

