"""Device columns from AEDAT-2.0 event files: the mirror of event_write.py.

An AEDAT-2.0 file is a text header, the run of lines that start with '#' and end with '\\n', whose first line is
`#!AER-DAT2.0`, followed by 8-byte records of two big-endian 32-bit words (address, time stamp).  The header is split off on the
host (a few lines); the records are uploaded in one piece and decoded on the device (csrc/events_aedat2_read.hip through
ops.unpack_events_aedat2).  Both jAER's DAVIS recordings (layout 'davis') and the files event_write.write_events_aedat2 and the
reference's AEDat2Output write (layout 'v2e') are read.  AEDAT-1.0, 3.x and 4.0 are other formats and are refused by name.
"""
import re

import numpy as np

AEDAT2_MAGIC = b"#!AER-DAT"
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


def is_aedat_path(path):
    """True for a path that ends in .aedat / .aedat2 or a file whose first bytes are '#!AER-DAT'."""
    name = str(path).lower()
    if name.endswith(".aedat") or name.endswith(".aedat2"):
        return True
    try:
        with open(path, "rb") as f:
            return f.read(len(AEDAT2_MAGIC)) == AEDAT2_MAGIC
    except OSError:
        return False


def read_events_aedat2(path_or_bytes, hw, device=None, **unpack_kwargs):
    """An AEDAT-2.0 file (a path, or its bytes) -> (t int64, x int32, y int32, p int8, info) on `device` (default: the current
    one), the kept events in file order.  hw = (height, width) of the sensor; unpack_kwargs are ops.unpack_events_aedat2's
    (layout, flip_x, flip_y, unwrap, t_divisor).  The body is uploaded in one piece, as ops.parse_events_csv uploads its text.
    A trailing partial record is ignored and reported as info['trailing_bytes']; info holds the decoder's counters as well."""
    import torch
    from . import ops
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        host = np.frombuffer(path_or_bytes, dtype=np.uint8)
    else:
        host = np.fromfile(path_or_bytes, dtype=np.uint8)
    off = split_aedat2_header(host[:MAX_HEADER_BYTES + 1].tobytes())
    n = (len(host) - off) // 8
    body = host[off:off + 8 * n]
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    buf = torch.from_numpy(body.copy()).to(dev)                      # the copy starts the records on an aligned address
    t, x, y, p, info = ops.unpack_events_aedat2(buf, hw, **unpack_kwargs)
    info["trailing_bytes"] = int(len(host) - off - 8 * n)
    return t, x, y, p, info
