"""NumPy restatement of the AEDAT-2.0 record decoder (csrc/events_aedat2_read.hip; the contract is in include/scpose.h at
scpose_events_aedat2_unpack), and the inputs its tests share.

A record is two big-endian uint32 words (address, time stamp).  DAVIS layout: bit 31 set -> "other" (APS / IMU), dropped; bit 31
clear and bit 10 set -> "special", dropped; else a polarity event, p = bit 11, x field = bits 12-21, y field = bits 22-30.  V2E
layout: every record is a polarity event and the y field is bits 22-31.  x = w - 1 - field when flipped, else the field.  With u
the time stamp words of ALL records, wraps = cumsum(u[j-1] > u[j] and u[j-1] - u[j] > 2^31) and t = u + 2^32 * wraps (unwrap) or
the sign-extended word; a divisor applies (int64)((double)t / d) afterwards.  n_backward counts kept events whose final t is
below the previous kept event's.
"""
import numpy as np

TILE = 4096
DAVIS, V2E = "davis", "v2e"
RANGE, CAPACITY = 1, 2
MAX_HW = {DAVIS: (512, 1024), V2E: (1024, 1024)}
INFO = ("n_events", "n_other", "n_special", "n_wraps", "n_backward")


def check_size(hw, layout):
    h, w = int(hw[0]), int(hw[1])
    mh, mw = MAX_HW[layout]
    if not (1 <= h <= mh and 1 <= w <= mw):
        raise ValueError("frame %dx%d (HxW) not supported under the %s layout" % (h, w, layout))
    return h, w


def unpack(body, hw, layout=DAVIS, flip_x=True, flip_y=True, unwrap=True, t_divisor=0.0):
    """-> ((t int64, x int32, y int32, p int8), info dict, status)."""
    h, w = check_size(hw, layout)
    if t_divisor not in (0.0, 1e3, 1e6):
        raise ValueError("t_divisor")
    words = np.frombuffer(bytes(body), dtype=">u4").astype(np.uint32)
    a, u = words[0::2], words[1::2]
    n = len(a)
    if layout == DAVIS:
        other = (a >> np.uint32(31)) != 0
        special = ~other & (((a >> np.uint32(10)) & np.uint32(1)) != 0)
        yf = ((a >> np.uint32(22)) & np.uint32(0x1ff)).astype(np.int64)
    else:
        other = np.zeros(n, bool)
        special = np.zeros(n, bool)
        yf = (a >> np.uint32(22)).astype(np.int64)
    keep = ~other & ~special
    xf = ((a >> np.uint32(12)) & np.uint32(0x3ff)).astype(np.int64)
    p = ((a >> np.uint32(11)) & np.uint32(1)).astype(np.int8)
    u64 = u.astype(np.int64)
    flag = np.zeros(n, bool)
    flag[1:] = (u64[:-1] > u64[1:]) & (u64[:-1] - u64[1:] > 2 ** 31)
    wraps = np.cumsum(flag).astype(np.int64)
    t = u64 + (wraps << 32) if unwrap else u.view(np.int32).astype(np.int64)
    if t_divisor:
        t = (t.astype(np.float64) / t_divisor).astype(np.int64)
    status = RANGE if bool((keep & ((xf >= w) | (yf >= h))).any()) else 0
    x = (w - 1 - xf if flip_x else xf).astype(np.int32)
    y = (h - 1 - yf if flip_y else yf).astype(np.int32)
    tk = t[keep]
    info = {"n_events": int(keep.sum()), "n_other": int(other.sum()), "n_special": int(special.sum()),
            "n_wraps": int(flag.sum()), "n_backward": int((tk[1:] < tk[:-1]).sum())}
    return (tk, x[keep], y[keep], p[keep]), info, status


def records(a, u):
    """bytes of the records with address words a and time stamp words u (uint32)."""
    out = np.empty(2 * len(a), dtype=">u4")
    out[0::2] = np.asarray(a, dtype=np.uint32)
    out[1::2] = np.asarray(u, dtype=np.uint32)
    return out.tobytes()


def address(x, y, p, hw, flip=True):
    """The polarity-event word both writers make (bit 31 clear for y fields below 512)."""
    h, w = hw
    xf = (w - 1 - np.asarray(x, np.int64)) if flip else np.asarray(x, np.int64)
    yf = (h - 1 - np.asarray(y, np.int64)) if flip else np.asarray(y, np.int64)
    return ((xf << 12) | (yf << 22) | (np.asarray(p, np.int64) << 11)).astype(np.uint32)


def stream(n, hw, pattern, seed=0, t0=0, step=3):
    """(a, u) of n records on a sensor hw (h <= 512) under the DAVIS layout.  pattern: 'all' kept, 'none' kept (other and special
    records), 'mix' (about 30 % bit-31 and 5 % bit-10 records), 'ends' (only the first and the last record of every tile of 4096
    kept).  Time stamps increase by 0 .. step from t0 (mod 2^32)."""
    h, w = hw
    rng = np.random.default_rng(seed)
    a = address(rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, 2, n), hw)
    junk = rng.integers(0, 2 ** 31, n).astype(np.uint32)             # the payload bits of a dropped record are arbitrary
    r = rng.random(n)
    idx = np.arange(n)
    if pattern == "all":
        other = special = np.zeros(n, bool)
    elif pattern == "none":
        other, special = r < 0.5, r >= 0.5
    elif pattern == "mix":
        other, special = r < 0.30, (r >= 0.30) & (r < 0.35)
    elif pattern == "ends":
        kept = (idx % TILE == 0) | (idx % TILE == TILE - 1)
        other, special = ~kept & (r < 0.5), ~kept & (r >= 0.5)
    else:
        raise ValueError(pattern)
    a = np.where(other, junk | np.uint32(1 << 31), a)
    a = np.where(special, (junk | np.uint32(1 << 10)) & np.uint32(0x7fffffff), a).astype(np.uint32)
    u = ((t0 + np.cumsum(rng.integers(0, step + 1, n))) % (2 ** 32)).astype(np.uint32)
    return a, u
