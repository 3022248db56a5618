"""A coefficient-domain baseline JPEG writer for tests, from ITU T.81 alone: quantised coefficients in, a file out.  Nothing
here is an encoder's habit -- component ids, table ids, tables, restart interval and every coefficient are the caller's.

write(...) takes the blocks in scan order (MCU after MCU; inside a 4:2:0 MCU Y00 Y01 Y10 Y11 Cb Cr), each 64 quantised
coefficients in zig-zag order with the DC value absolute (the writer codes the differences and resets the prediction at every
restart).  It emits SOI, an optional JFIF segment, DQT, SOF0, DHT, DRI, SOS, the entropy-coded bytes with FF 00 stuffing, RSTn
(D0 .. D7 and round again) and EOI; every restart segment ends with fill bits of ones.  It returns the bytes and a Written:
per restart segment the data bits and the fill bits, and the code lengths that were emitted per table.
"""
import struct

import numpy as np

# T.81 figure 5: natural index of the i-th coefficient in zig-zag order
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
SAMPLING = {"gray": ((1, 1),), "444": ((1, 1),) * 3, "420": ((2, 2), (1, 1), (1, 1))}
AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]


def table(lengths):
    """{symbol: code length} -> (bits[17], huffval) as DHT carries them (T.81 annex C assigns the codes in this order).  The
    Kraft sum stays below 1, so that no code is all ones (T.81 annex K.2)."""
    assert all(1 <= l <= 16 for l in lengths.values())
    assert sum(1 << (16 - l) for l in lengths.values()) < (1 << 16), "the code would use the all-ones word"
    order = sorted(lengths, key=lambda s: lengths[s])                  # stable: the caller's order inside one length
    bits = [0] * 17
    for s in order:
        bits[lengths[s]] += 1
    assert max(bits) <= 255
    return bits, order


def dc_table(lengths):
    """code lengths of the size categories 0 .. 11"""
    assert len(lengths) == 12
    return table(dict(enumerate(lengths)))


def ac_table(first, rest=16):
    """{symbol: length} for the symbols named, `rest` bits for every other of the 162 baseline AC symbols"""
    lengths = dict(first)
    for s in AC_SYMBOLS:
        lengths.setdefault(s, rest)
    return table(lengths)


def codes(tab):
    """(bits, huffval) -> {symbol: (code, length)}, T.81 annex C"""
    bits, vals = tab
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            out[vals[p]] = (code, l)
            code += 1; p += 1
        code <<= 1
    return out


def size_of(v):
    return int(abs(int(v))).bit_length()


def value_bits(v, s):
    """T.81 F.1.2.1.1: the s low bits of v, of v - 1 when v is negative"""
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):
        self.acc = (self.acc << n) | v
        self.n += n


def code_block(out, block, pred, dc, ac, used_dc, used_ac):
    """one block (zig-zag order, DC absolute) after prediction `pred` -> appended to `out`"""
    diff = int(block[0]) - pred
    s = size_of(diff)
    assert s <= 11, "DC difference %d" % diff
    c, l = dc[s]
    out.put(c, l); used_dc.add(l)
    if s:
        out.put(value_bits(diff, s), s)
    run = 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            c, l = ac[0xF0]
            out.put(c, l); used_ac.add(l)
            run -= 16
        s = size_of(v)
        assert s <= 10, "AC coefficient %d" % v
        c, l = ac[(run << 4) | s]
        out.put(c, l); used_ac.add(l)
        out.put(value_bits(v, s), s)
        run = 0
    if run:
        c, l = ac[0x00]
        out.put(c, l); used_ac.add(l)


class Written:
    """data_bits, fill_bits: per restart segment; dc_lengths, ac_lengths: {table id: set of emitted code lengths};
    entropy: the raw bytes of every restart segment (stuffing included, markers not)"""


def write(height, width, mode, blocks, qtables, dc_tables, ac_tables, comp_ids=None, comp_q=None, comp_dc=None, comp_ac=None,
          restart_interval=0, jfif=True):
    """qtables {id: 64 values in natural order}; dc_tables / ac_tables {id: (bits[17], huffval)} -> (bytes, Written)"""
    samp = SAMPLING[mode]
    nc = len(samp)
    comp_ids = list(comp_ids or range(1, nc + 1))
    comp_q, comp_dc, comp_ac = list(comp_q or [0] * nc), list(comp_dc or [0] * nc), list(comp_ac or [0] * nc)
    hmax, vmax = samp[0]
    mcus = -(-width // (8 * hmax)) * -(-height // (8 * vmax))
    comp_of = [0] * (hmax * vmax) + list(range(1, nc))
    blocks = np.asarray(blocks)
    assert blocks.shape == (mcus * len(comp_of), 64), (blocks.shape, mcus, len(comp_of))
    dcc = {t: codes(dc_tables[t]) for t in set(comp_dc)}
    acc = {t: codes(ac_tables[t]) for t in set(comp_ac)}
    w = Written()
    w.data_bits, w.fill_bits, w.entropy = [], [], []
    w.dc_lengths, w.ac_lengths = {t: set() for t in dcc}, {t: set() for t in acc}

    f = bytearray(b"\xff\xd8")
    seg = lambda marker, body: f.extend(b"\xff" + bytes([marker]) + struct.pack(">H", len(body) + 2) + bytes(body))
    if jfif:
        seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in sorted(set(comp_q)):
        q = np.asarray(qtables[t]).reshape(64)
        assert q.min() >= 1 and q.max() <= 255
        seg(0xDB, bytes([t]) + bytes(int(q[n]) for n in ZIGZAG))
    seg(0xC0, struct.pack(">BHHB", 8, height, width, nc) +
        b"".join(bytes([comp_ids[c], (samp[c][0] << 4) | samp[c][1], comp_q[c]]) for c in range(nc)))
    for cls, tabs, sel in ((0, dc_tables, comp_dc), (1, ac_tables, comp_ac)):
        for t in sorted(set(sel)):
            bits, vals = tabs[t]
            seg(0xC4, bytes([(cls << 4) | t]) + bytes(bits[1:17]) + bytes(vals))
    if restart_interval:
        seg(0xDD, struct.pack(">H", restart_interval))
    seg(0xDA, bytes([nc]) + b"".join(bytes([comp_ids[c], (comp_dc[c] << 4) | comp_ac[c]]) for c in range(nc)) + b"\x00\x3f\x00")

    per = restart_interval or mcus
    for si, m0 in enumerate(range(0, mcus, per)):
        if si:
            f.extend(bytes([0xFF, 0xD0 + (si - 1) % 8]))
        out, pred = Bits(), [0] * nc
        for b in range(m0 * len(comp_of), min(m0 + per, mcus) * len(comp_of)):
            c = comp_of[b % len(comp_of)]
            code_block(out, blocks[b], pred[c], dcc[comp_dc[c]], acc[comp_ac[c]], w.dc_lengths[comp_dc[c]], w.ac_lengths[comp_ac[c]])
            pred[c] = int(blocks[b][0])
        fill = -out.n % 8
        w.data_bits.append(out.n); w.fill_bits.append(fill)
        out.put((1 << fill) - 1, fill)
        raw = out.acc.to_bytes(out.n // 8, "big").replace(b"\xff", b"\xff\x00")
        w.entropy.append(raw)
        f.extend(raw)
    f.extend(b"\xff\xd9")
    return bytes(f), w
