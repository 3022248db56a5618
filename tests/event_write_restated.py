"""NumPy / Python restatement of the two event file formats the device writes (csrc/events_write.hip), and the inputs the tests
share.

Text: a row is `"%d<sep>%d<sep>%d<sep>%d\\n" % (t, a, b, p)`, (a, b) = (x, y) or (y, x) with swap_xy: Python's "%d" of an int
is C's -- '-' for negatives, no '+', no leading zeros.

AEDAT-2.0, written from the lines of the reference's v2ecore/output/aedat2_output.py (AEDat2Output.appendEvents): per event the
int32 pair (address, time stamp), address = xf << 12 | yf << 22 | p << 11 with both axes flipped, the array byte-swapped to big
endian; from the first non-empty write to a file, records are dropped from the front while the first byte is '#'.  The address
is formed in uint32 here; the reference's int32 shifts wrap to the same bits.
"""
import numpy as np

SIZES = ((346, 260), (692, 520), (1280, 720), (640, 480), (240, 180))      # (width, height)
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def text(t, x, y, p, sep=" ", swap_xy=False):
    a, b = (y, x) if swap_xy else (x, y)
    fmt = "%d" + sep + "%d" + sep + "%d" + sep + "%d\n"
    return "".join(fmt % row for row in zip(np.asarray(t).tolist(), np.asarray(a).tolist(), np.asarray(b).tolist(),
                                            np.asarray(p).tolist())).encode()


def aedat2_records(t, x, y, p, hw):
    """uint8 (8 * n,): the records of the events, nothing dropped."""
    h, w = hw
    xf = (w - 1 - np.asarray(x, np.int64)).astype(np.uint32)
    yf = (h - 1 - np.asarray(y, np.int64)).astype(np.uint32)
    a = (xf << np.uint32(12)) | (yf << np.uint32(22)) | (np.asarray(p).astype(np.uint32) << np.uint32(11))
    out = np.empty(2 * len(a), dtype=">u4")
    out[0::2] = a
    out[1::2] = np.asarray(t, np.int64).astype(np.int32).view(np.uint32)
    return out.view(np.uint8)


def lead(records):
    """How many leading records start with '#'."""
    first = np.asarray(records).reshape(-1, 8)[:, 0]
    other = np.flatnonzero(first != 0x23)
    return int(other[0]) if len(other) else len(first)


def aedat2_body(chunks, hw):
    """The bytes after the header of a file to which the chunks, each (t, x, y, p), are written in turn."""
    parts, written = [], 0
    for t, x, y, p in chunks:
        if len(t) == 0:
            continue
        r = aedat2_records(t, x, y, p, hw)
        if written == 0:
            r = r[8 * lead(r):]
        parts.append(r.tobytes())
        written += len(t)          # the reference counts the events it was given, dropped ones included
    return b"".join(parts)


def boundary_values_64():
    """int64 values at every change of the printed length, and the extremes."""
    v = [0, -1, 1, INT64_MIN, INT64_MAX, INT32_MIN, INT32_MAX, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, -(2 ** 32)]
    for k in range(1, 19):
        v += [10 ** k - 1, 10 ** k, -(10 ** k - 1), -(10 ** k)]
    return v


def boundary_values_32():
    v = [0, -1, 1, INT32_MIN, INT32_MAX, INT32_MIN + 1]
    for k in range(1, 10):
        v += [10 ** k - 1, 10 ** k, -(10 ** k - 1), -(10 ** k)]
    return v


def text_columns(n, seed=0, parseable=False):
    """n rows for the text formatter: the boundary values of every column first (cycled against each other), then blocks of
    shortest (8 bytes) and longest (50 bytes) rows next to each other, so that tile start offsets take every residue mod 16,
    then random rows of every length.  parseable: only values the device reader takes back unchanged -- it accepts any int64 /
    int32 / int8 written without a '.', so the columns are the same; the flag keeps the 15-digit rule of its header visible by
    limiting t to 15 digits."""
    rng = np.random.default_rng(seed)
    b64, b32 = boundary_values_64(), boundary_values_32()
    if parseable:
        b64 = [v for v in b64 if abs(v) < 10 ** 15]
    bp = [-128, 0, 1, 127, -1, 9, 10, -9, -10, 99, 100, -99, -100]
    t = np.empty(n, np.int64); x = np.empty(n, np.int32); y = np.empty(n, np.int32); p = np.empty(n, np.int8)
    for i in range(n):
        if i < 160:
            t[i], x[i], y[i], p[i] = b64[i % len(b64)], b32[(3 * i) % len(b32)], b32[(5 * i + 1) % len(b32)], bp[i % len(bp)]
        elif i % 97 < 48:
            # runs of 1 ... 16 longest rows between shortest ones: 50 = 2 mod 16, 8 = 8 mod 16
            long_row = (i % 97) % 17 != 0
            if long_row:
                t[i], x[i], y[i], p[i] = (-(10 ** 14) - i if parseable else INT64_MIN + i), INT32_MIN + i, INT32_MIN + 2 * i, -128
            else:
                t[i], x[i], y[i], p[i] = i % 10, (i // 10) % 10, 3, 1
        else:
            mag = 10 ** int(rng.integers(0, 15 if parseable else 19))
            t[i] = int(rng.integers(-mag, mag + 1))
            x[i] = int(rng.integers(-10 ** int(rng.integers(0, 10)), 10 ** int(rng.integers(0, 10))))
            y[i] = int(rng.integers(0, 1000))
            p[i] = int(rng.integers(-128, 128))
    return t, x, y, p


def aedat2_columns(n, hw, seed=0):
    """n random in-range events (t increasing, below 2^31)."""
    h, w = hw
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, 2 ** 31, n)).astype(np.int64)
    return (t, rng.integers(0, w, n).astype(np.int32), rng.integers(0, h, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int8))
