"""Writes PNG files from raw pixels with every choice a test wants to make itself: the filter of each row, the deflate form, the block
and IDAT boundaries, the palette -- and assembles by hand the deflate forms no zlib call is certain to emit.  No decoder is involved:
what a file means is left to PIL (tests/test_png_decode.py)."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(kind, body, crc_xor=0):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) ^ crc_xor)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(samples, bpp, filters):
    """samples uint8 (h, w bpp), filters one type per row -> the filtered scan lines (bytes, h x (1 + w bpp)).  A type above 4 is written
    as it stands with the row unfiltered."""
    h, stride = samples.shape
    rows = samples.astype(np.int32)
    out = bytearray()
    for r in range(h):
        f = int(filters[r])
        cur = rows[r]
        up = rows[r - 1] if r else np.zeros(stride, dtype=np.int32)
        left = np.concatenate([np.zeros(bpp, dtype=np.int32), cur[:-bpp]]) if stride > bpp else np.zeros(stride, dtype=np.int32)
        ul = np.concatenate([np.zeros(bpp, dtype=np.int32), up[:-bpp]]) if stride > bpp else np.zeros(stride, dtype=np.int32)
        if f == 1:
            pred = left
        elif f == 2:
            pred = up
        elif f == 3:
            pred = (left + up) >> 1
        elif f == 4:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, ul)], dtype=np.int32)
        else:
            pred = 0
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw, level=6, wbits=15, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    """zlib stream of raw; flush_every > 0: Z_FULL_FLUSH after every that many bytes (many blocks, empty stored blocks between them)."""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem_level, strategy)
    if flush_every <= 0:
        return c.compress(raw) + c.flush()
    out = b""
    for i in range(0, len(raw), flush_every):
        out += c.compress(raw[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


DEFLATE_FORMS = {
    "stored": dict(level=0),
    "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "huffman_only": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": dict(level=6, strategy=zlib.Z_RLE),
    "default": dict(level=6),
    "best": dict(level=9, mem_level=9),
    "fast_small_mem": dict(level=1, mem_level=1),
    "flushed": dict(level=6, flush_every=37),
    "flushed_stored": dict(level=0, flush_every=50),
    "wbits9": dict(level=6, wbits=9),
    "wbits12": dict(level=9, wbits=12),
}


def split_points(stream, pattern):
    """Names of the IDAT split patterns -> the sorted cut offsets into the stream (a repeated offset makes an empty chunk)."""
    n = len(stream)
    if pattern == "one":
        return []
    if pattern == "every_byte":
        return list(range(1, n))
    if pattern == "header":
        return [1]                              # between the two zlib header bytes
    if pattern == "empty_chunks":
        return [0, 0, n // 2, n // 2, n // 2, n]
    if pattern == "thirds":
        return [n // 3, 2 * n // 3]
    if pattern == "trailer":
        return [max(n - 2, 0)]                  # inside the Adler-32
    if pattern == "stored_len":
        return [3, 4, 5, 6]                     # a level-0 stream: its first stored block's LEN / NLEN are bytes 3 .. 6
    raise KeyError(pattern)


SPLIT_PATTERNS = ("one", "every_byte", "header", "empty_chunks", "thirds", "trailer", "stored_len")


def assemble(h, w, color_type, stream, cuts=(), palette=None, trns=None, interlace=0, depth=8, extra=(), idat_crc_xor=0):
    """A PNG file around a zlib stream cut into IDAT chunks at `cuts`."""
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace))
    for kind, body in extra:
        out += chunk(kind, body)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, dtype=np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    edges = [0] + sorted(cuts) + [len(stream)]
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        out += chunk(b"IDAT", stream[a:b], idat_crc_xor if k == 0 else 0)
    return out + chunk(b"IEND", b"")


def write_png(pixels, color_type, filters=0, form="default", split="one", palette=None, trns=None, rng=None):
    """pixels uint8 (h, w) or (h, w, channels of color_type) -> (file bytes, raw filtered scan lines, zlib stream).  filters: one type
    for every row, a list, or "random" (needs rng; row 0 then takes Up, Avg or Paeth)."""
    px = np.asarray(pixels, dtype=np.uint8)
    h, w = px.shape[:2]
    bpp = CHANNELS[color_type]
    samples = px.reshape(h, w * bpp)
    if isinstance(filters, str):
        filters = [int(rng.integers(2, 5))] + [int(v) for v in rng.integers(0, 5, h - 1)]
    elif np.isscalar(filters):
        filters = [int(filters)] * h
    raw = filter_rows(samples, bpp, filters)
    params = DEFLATE_FORMS[form] if isinstance(form, str) else form
    stream = deflate(raw, **params)
    return assemble(h, w, color_type, stream, split_points(stream, split), palette, trns), raw, stream


# ---------------------------------------------------------------- deflate by hand
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, count):            # LSB first: header fields and extra bits
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):            # a Huffman code: most significant bit first
        for k in range(count - 1, -1, -1):
            self.bits((value >> k) & 1, 1)

    def at(self):                            # bits written so far
        return 8 * len(self.out) + self.n

    def done(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


_FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_DIST_LENS = [5] * 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
DEFAULT_CL_LENS = [4] * 13 + [5] * 6             # a complete code over all nineteen code-length symbols


def canonical_codes(lens):
    """code lengths -> {symbol: (code, length)} as RFC 1951 3.2.2 assigns them.  The set is taken as it stands: an over-subscribed or
    incomplete one still gets its numbers (the damaged cases need them written)."""
    count = [0] * 17
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for ln in range(1, 17):
        code = (code + count[ln - 1]) << 1
        nxt[ln] = code
    out = {}
    for s, ln in enumerate(lens):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


def is_complete(lens):
    return sum(1 << (15 - ln) for ln in lens if ln) == 1 << 15


def _match_symbols(op):
    """An op that stands for a match -> (length symbol, extra, distance symbol or None, extra)."""
    if op[0] == "len":
        return op[1:]
    ln, d = op
    li = 28 if ln == 258 else max(i for i in range(28) if _LEN_BASE[i] <= ln)
    di = max(i for i in range(30) if _DIST_BASE[i] <= d)
    return 257 + li, ln - _LEN_BASE[li], di, d - _DIST_BASE[di]


def _write_ops(bw, ops, lit, dist, rec):
    """ops with the codes lit / dist ({symbol: (code, length)}): an int is a literal, (length, distance) a match in its usual spelling,
    ("len", symbol, extra, distance symbol or None, extra) a match spelled out -- symbols 286 / 287 and 30 / 31 included, which carry
    no extra bits --, ("bits", value, count) a pattern that is no code.  rec takes the code lengths written and where each op began."""
    for op in ops:
        rec["op_at"].append(bw.at())
        if not isinstance(op, tuple):
            bw.code(*lit[op])
            rec["lit_used"].add(lit[op][1])
        elif op[0] == "bits":
            bw.bits(op[1], op[2])
        else:
            ls, le, ds, de = _match_symbols(op)
            rec["matches"].append((ls, le, ds, de))
            bw.code(*lit[ls])
            rec["lit_used"].add(lit[ls][1])
            bw.bits(le, _LEN_EXTRA[ls - 257] if ls <= 285 else 0)
            if ds is not None:
                bw.code(*dist[ds])
                rec["dist_used"].add(dist[ds][1])
                bw.bits(de, _DIST_EXTRA[ds] if ds <= 29 else 0)
    rec["eob_at"] = bw.at()
    if 256 in lit:
        bw.code(*lit[256])


def _new_record():
    return {"lit_used": set(), "dist_used": set(), "op_at": [], "matches": []}


def fixed_block(ops, final=True, bw=None):
    """One fixed-Huffman block from ops (see _write_ops), then the end-of-block code.  -> BitWriter"""
    bw = bw or BitWriter()
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    _write_ops(bw, ops, canonical_codes(_FIXED_LIT_LENS), canonical_codes(_FIXED_DIST_LENS), _new_record())
    return bw


def stored_block(data, final=True, bw=None):
    """One stored block wherever the writer stands: the header's three bits, zeros up to the byte, LEN, NLEN, the bytes."""
    bw = bw or BitWriter()
    bw.bits(1 if final else 0, 1)
    bw.bits(0, 2)
    if bw.n:
        bw.bits(0, 8 - bw.n)
    bw.bits(len(data), 16)
    bw.bits(len(data) ^ 0xFFFF, 16)
    for v in data:
        bw.bits(v, 8)
    return bw


def expand_seq(seq):
    """What a length sequence of literal lengths and (16 | 17 | 18, repeat) items stands for."""
    out = []
    for item in seq:
        if isinstance(item, tuple):
            out += [out[-1] if item[0] == 16 else 0] * item[1]
        else:
            out.append(item)
    return out


def dynamic_block(ops, lit_lens, dist_lens, cl_lens=None, length_seq=None, final=True, bw=None, raw_header=None):
    """One dynamic-Huffman block: BFINAL / BTYPE, HLIT / HDIST / HCLEN (raw_header: the three FIELD values, None keeps the one that
    follows from the lengths), the code-length code's lengths in CL_ORDER, the length sequence -- length_seq as given, literal lengths
    and (16 | 17 | 18, repeat) items, whether or not it spells lit_lens + dist_lens; without it one symbol per length --, then ops
    (see _write_ops) in the canonical codes of lit_lens and dist_lens, then the end-of-block code if it has one.
    -> (BitWriter, record): what was actually written.  lit_used / dist_used / cl_used: the lengths of the codes the ops (the
    sequence) used; matches: every match as (length symbol, extra, distance symbol, extra); seq: per item (item, first slot, slot
    after its last); the bit offsets (of this BitWriter: the zlib header is 16 more) at which the block, each
    HCLEN field, each item, each item's extra bits, each op and the end-of-block code begin."""
    bw = bw or BitWriter()
    rec = _new_record()
    cl_lens = list(DEFAULT_CL_LENS if cl_lens is None else cl_lens)
    seq = list(lit_lens) + list(dist_lens) if length_seq is None else list(length_seq)
    hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
    fields = [len(lit_lens) - 257, len(dist_lens) - 1, hclen - 4]
    for k, v in enumerate(raw_header or ()):
        if v is not None:
            fields[k] = v
    rec.update(block_at=bw.at(), hlit=fields[0] + 257, hdist=fields[1] + 1, hclen=fields[2] + 4, final=final, lit_lens=list(lit_lens),
               dist_lens=list(dist_lens), cl_lens=cl_lens)
    bw.bits(1 if final else 0, 1)
    bw.bits(2, 2)
    bw.bits(fields[0], 5)
    bw.bits(fields[1], 5)
    bw.bits(fields[2], 4)
    rec["hclen_at"] = []
    for i in range(fields[2] + 4):
        rec["hclen_at"].append(bw.at())
        bw.bits(cl_lens[CL_ORDER[i]], 3)
    cl = canonical_codes(cl_lens)
    rec.update(seq=[], item_at=[], extra_at=[], cl_used=set())
    slot = 0
    for item in seq:
        sym, rep = item if isinstance(item, tuple) else (item, 1)
        rec["item_at"].append(bw.at())
        bw.code(*cl[sym])
        rec["cl_used"].add(cl[sym][1])
        rec["extra_at"].append(bw.at())
        if sym >= 16:
            bw.bits(rep - (3, 3, 11)[sym - 16], (2, 3, 7)[sym - 16])
        rec["seq"].append((item, slot, slot + rep))
        slot += rep
    rec["seq_end_at"] = bw.at()
    _write_ops(bw, ops, canonical_codes(lit_lens), canonical_codes(dist_lens), rec)
    rec["end_at"] = bw.at()
    return bw, rec


def run_ops(ops, out=None):
    out = bytearray() if out is None else out
    for op in ops:
        if not isinstance(op, tuple):
            out.append(op)
        elif op[0] != "bits":
            ls, le, ds, de = _match_symbols(op)
            for _ in range(_LEN_BASE[ls - 257] + le):
                out.append(out[-(_DIST_BASE[ds] + de)])
    return out


def zlib_wrap(deflate_bytes, raw):
    return b"\x78\x9c" + deflate_bytes + struct.pack(">I", zlib.adler32(bytes(raw)))


def hand_fixed_png():
    """A 1 x 593 gray frame (594 raw bytes, the first the row's filter type: Sub) as ONE hand-made fixed-Huffman block that holds a match
    of length 258 at distance 1, matches of lengths 3 and 4, and a match whose distance reaches exactly to byte 0.  -> (file, raw)."""
    ops = [1, 7, (258, 1), 9, 200, 255, (3, 2), (4, 265), 143, 144]
    ops.append((258, len(run_ops(ops))))         # distance == bytes so far: reaches exactly to byte 0
    ops.append((594 - len(run_ops(ops)), 300))
    raw = run_ops(ops)
    assert len(raw) == 594
    return assemble(1, 593, 0, zlib_wrap(fixed_block(ops).done(), raw)), bytes(raw)


def stored_stream(raw, sizes):
    """A zlib stream of stored blocks of the given sizes (0 and 65 535 included), the last one final."""
    out, pos = bytearray(b"\x78\x01"), 0
    for k, n in enumerate(sizes):
        out.append(1 if k == len(sizes) - 1 else 0)
        out += struct.pack("<HH", n, n ^ 0xFFFF) + raw[pos:pos + n]
        pos += n
    assert pos == len(raw)
    return bytes(out) + struct.pack(">I", zlib.adler32(raw))


def hand_far_matches_png(rng):
    """A 131 x 255 gray frame (33 536 raw bytes): a stored block of 33 020 bytes, then ONE hand-made fixed-Huffman block of two matches
    of length 258, at distance 32 768 -- the whole window -- and at 32 768 - 10, where a decoder whose ring is exactly the window
    loads from the slots the same match stores to.  -> (file, raw)."""
    prefix = bytearray(rng.integers(0, 256, 33020, dtype=np.uint8).tobytes())
    for r in range(0, 33020, 256):
        prefix[r] = int(rng.integers(0, 5))      # the filter bytes of rows 0 .. 128
    prefix[33280 - 32758] = 3                    # the byte the second match copies into row 130's filter byte
    ops = [(258, 32768), (258, 32758)]
    raw = run_ops(ops, bytearray(prefix))
    assert len(raw) == 131 * 256 and all(raw[r] <= 4 for r in range(0, len(raw), 256))
    stream = b"\x78\x01" + b"\x00" + struct.pack("<HH", 33020, 33020 ^ 0xFFFF) + bytes(prefix) + fixed_block(ops).done()
    return assemble(131, 255, 0, stream + struct.pack(">I", zlib.adler32(bytes(raw)))), bytes(raw)


def hand_stored_png(rng):
    """A 260 x 255 gray frame (66 560 raw bytes) as stored blocks of 0, 65 535, 0, 1 025 and 0 bytes.  -> (file, raw)."""
    px = rng.integers(0, 256, (260, 255), dtype=np.uint8)
    raw = filter_rows(px, 1, [int(v) for v in rng.integers(0, 5, 260)])
    return assemble(260, 255, 0, stored_stream(raw, [0, 65535, 0, 1025, 0])), raw


# ---------------------------------------------------------------- dynamic-Huffman blocks no zlib writes
WINDOW_BITS = 4096 * 8                           # the device's input window (csrc/png_decode.hip: kInWords words), counted from the zlib header


def lens_of(n, by_symbol):
    """n code lengths, zero but for {symbol: length}"""
    out = [0] * n
    for s, ln in by_symbol.items():
        out[s] = ln
    return out


def flat_lens(n, symbols):
    """n code lengths: a complete code over `symbols` (two or more) whose lengths differ by one at the most, the short ones first"""
    symbols = list(symbols)
    m = (len(symbols) - 1).bit_length()
    short = (1 << m) - len(symbols)
    return lens_of(n, {s: m - 1 if k < short else m for k, s in enumerate(symbols)})


LADDER = list(range(1, 16)) + [15]               # 1, 2, ..., 14, 15, 15: complete, with two 15-bit codes
# dyn_long_codes: the ladder over sixteen literal/length symbols (in this order) and over the distance symbols 0 .. 15
_LONG_LIT = lens_of(286, dict(zip((65, 1, 66, 257, 67, 260, 266, 68, 285, 69, 70, 273, 256, 71, 72, 284), LADDER)))
_LONG_OPS = [1, 65, 66, 67, 68, 69, 70, 71, 72,                  # literals of 2, 1, 3, 5, 8, 10, 11, 14 and 15 bits
             (3, 3), (6, 5), (14, 9), 69, (258, 15),             # distance codes of 3, 5, 7 and 8 bits (symbols 2, 4, 6, 7)
             70, (40, 22), 71, (250, 60),                        # 9 bits (symbol 8: 17 .. 24), 12 bits (symbol 11: 49 .. 64); length 284 is 15 bits
             72, (13, 192), (3, 250), 68, (6, 30), (14, 256),    # 15 bits twice (symbols 14 and 15), 10 bits (symbol 9), the last distance
             ("len", 284, 30, 15, 0), 70, 71, 72]


def _one_row(ops, blocks_of):
    """A 1 x (n - 1) gray frame whose n raw bytes are what ops produce (the first one the row's filter type)."""
    raw = bytes(run_ops(ops))
    assert raw[0] <= 4
    bw, recs = blocks_of(ops)
    stream = zlib_wrap(bw.done(), raw)
    return assemble(1, len(raw) - 1, 0, stream), raw, recs, stream


def dyn_long_codes(dist_count=16, cl_lens=None, length_seq=None):
    """1 x 880 gray in one block.  dist_count 30, _EXTREME_CL and _EXTREME_SEQ make it dyn_counts_extremes_286_30."""
    assert length_seq is None or expand_seq(length_seq) == _LONG_LIT + LADDER + [0] * (dist_count - 16)

    def blocks(ops):
        bw, rec = dynamic_block(ops, _LONG_LIT, LADDER + [0] * (dist_count - 16), cl_lens, length_seq)
        return bw, [rec]
    return _one_row(_LONG_OPS, blocks)


# dyn_counts_extremes_286_30: the tables of dyn_long_codes, every length 0 .. 15 and every repeat symbol in the sequence, and a
# code-length code over all nineteen symbols whose 7-bit codes (for 2 and 18) the sequence uses
_EXTREME_CL = lens_of(19, {**{s: 4 for s in range(19)}, 5: 5, 17: 6, 2: 7, 18: 7})
_EXTREME_SEQ = ([0, 2, (18, 57), (16, 6), 1, 3, 5, 8, 10, 11, 14, 15, (18, 138), (18, 45), 13, 4, 0, 0, 6, (17, 5), 7, (17, 6), 12, (17, 10), 15, 9]
                + LADDER + [(18, 14)])


def rows_ops(rng, h, w, literals, lengths=(), dists=()):
    """ops of h rows of 1 + w bytes: a filter byte (0 .. 4, from literals), some literals, then matches of the given lengths at the
    given distances with literals between them.  No match crosses a row's end, so every filter byte is one the ops name."""
    literals = list(literals)
    filters = [v for v in literals if v <= 4]
    ops = []
    for r in range(h):
        made = r * (1 + w)                       # bytes these ops have produced: no distance reaches before them
        ops.append(filters[int(rng.integers(len(filters)))])
        left = w
        while left:
            ln = lengths[int(rng.integers(len(lengths)))] if lengths else 0
            near = [d for d in dists if d <= made]
            if ln and ln <= left and near and w - left >= 4 and rng.integers(3):
                ops.append((ln, near[int(rng.integers(len(near)))]))
                left -= ln
            else:
                ops.append(literals[int(rng.integers(len(literals)))])
                left -= 1
            made = (r + 1) * (1 + w) - left
    return ops


def _frame_of(h, w, ops, prefix=b""):
    raw = bytes(run_ops(ops, bytearray(prefix)))
    assert len(raw) == h * (1 + w) and all(raw[r] <= 4 for r in range(0, len(raw), 1 + w))
    return raw


# dyn_repeats, block A (rows 0 .. 4): literals 0 .. 15 and 164 .. 255, lengths 3 and 4, distances 1 .. 4.  Its sequence: a 16 of
# repeat 6 chained; an 18 of 138 zeros (inside the literal lengths: see below); a 16 straight after an 18 and one straight after a 17,
# which repeat zero; a 16 that starts at slot 258 -- the last literal/length slot -- and ends, as the last item, exactly at HLIT + HDIST.
_REPEATS_A_LIT = [8] * 16 + [0] * 148 + [8] * 88 + [7] * 4 + [4, 2, 2]
_REPEATS_A_DIST = [2, 2, 2, 2]
_REPEATS_A_SEQ = [8, (16, 6), (16, 6), (16, 3), (18, 138), (16, 3), (17, 3), (16, 4), 8] + [(16, 6)] * 14 + [(16, 3), 7, (16, 3), 4, 2, (16, 5)]
# block B (rows 5 .. 8): all 256 literals, no match.  An 18 that starts at slot 257 and runs across HLIT = 286 into the distance
# lengths, then a 17 that ends exactly at HLIT + HDIST = 316.  (No valid block has an 18 of 138 zeros ACROSS the boundary: slot 256,
# the end-of-block code, is never zero, and only 29 + 30 slots follow it.)
_REPEATS_B_LIT = [8] * 255 + [9, 9] + [0] * 29
_REPEATS_B_SEQ = [8] + [(16, 6)] * 42 + [8, 8, 9, 9, (18, 56), (17, 3)]


def dyn_repeats():
    """9 x 31 gray, the frame size of damaged_cases().  -> (file, raw, records, zlib stream)"""
    rng = np.random.default_rng(20263)
    ops_a = rows_ops(rng, 5, 31, list(range(16)) + list(range(164, 256)), (3, 4), (1, 2, 3, 4))
    ops_b = rows_ops(rng, 4, 31, range(256))
    raw = _frame_of(9, 31, ops_a + ops_b)
    assert expand_seq(_REPEATS_A_SEQ) == _REPEATS_A_LIT + _REPEATS_A_DIST and is_complete(_REPEATS_A_LIT) and is_complete(_REPEATS_A_DIST)
    assert expand_seq(_REPEATS_B_SEQ) == _REPEATS_B_LIT + [0] * 30 and is_complete(_REPEATS_B_LIT)
    bw, rec_a = dynamic_block(ops_a, _REPEATS_A_LIT, _REPEATS_A_DIST, length_seq=_REPEATS_A_SEQ, final=False)
    bw, rec_b = dynamic_block(ops_b, _REPEATS_B_LIT, [0] * 30, length_seq=_REPEATS_B_SEQ, bw=bw)
    stream = zlib_wrap(bw.done(), raw)
    return assemble(9, 31, 0, stream), raw, [rec_a, rec_b], stream


def dyn_single_distance():
    """2 x 300 gray.  Row 0 in a block whose one distance code is symbol 0 (distance 1), with lengths 258 and 41; row 1 in a block
    whose one distance code is symbol 6 (distances 9 .. 12, two extra bits)."""
    ops_a = [0, 201, (258, 1), (41, 1)]
    ops_b = [1] + list(range(10, 22)) + [(258, 9), (12, 10), (11, 11), (7, 12)]
    raw = _frame_of(2, 300, ops_a + ops_b)
    bw, rec_a = dynamic_block(ops_a, flat_lens(286, [0, 201, 256, 285, 273]), [1], final=False)
    bw, rec_b = dynamic_block(ops_b, flat_lens(286, [1] + list(range(10, 22)) + [256, 285, 265, 261]), [0] * 6 + [1], bw=bw)
    stream = zlib_wrap(bw.done(), raw)
    return assemble(2, 300, 0, stream), raw, [rec_a, rec_b], stream


def _literal_frame(seed, h=5, w=7):
    rng = np.random.default_rng(seed)
    ops = rows_ops(rng, h, w, range(256))
    return ops, _frame_of(h, w, ops)


def dyn_no_distance(dist_lens=(0,)):
    """5 x 7 gray, literals only, HLIT 257 and HDIST 1: the one distance length is 0 (no distance code) or 1 (one, unused)."""
    ops, raw = _literal_frame(20264 + dist_lens[0])
    bw, rec = dynamic_block(ops, flat_lens(257, range(257)), list(dist_lens))
    return assemble(5, 7, 0, zlib_wrap(bw.done(), raw)), raw, [rec]


def dyn_lone_eob():
    """5 x 7 gray: a non-final block whose only code is end-of-block at length 1, then the block that holds the frame."""
    ops, raw = _literal_frame(20266)
    bw, rec_a = dynamic_block([], lens_of(257, {256: 1}), [0], final=False)
    bw, rec_b = dynamic_block(ops, flat_lens(257, range(257)), [0], bw=bw)
    return assemble(5, 7, 0, zlib_wrap(bw.done(), raw)), raw, [rec_a, rec_b]


def dyn_len_284_31():
    """1 x 522 gray: length 258 as symbol 284 with extra bits 31, and as symbol 285, in one block."""
    ops = [1, 10, 20, 30, ("len", 284, 31, 2, 0), 10, ("len", 285, 0, 3, 0), 20, 30]

    def blocks(ops):
        bw, rec = dynamic_block(ops, flat_lens(286, [1, 10, 20, 30, 256, 284, 285]), [2, 2, 2, 2])
        return bw, [rec]
    return _one_row(ops, blocks)


def dyn_dist_32768(rng):
    """hand_far_matches_png with the matches in a dynamic block: 131 x 255 gray, a stored block of 33 000 bytes, then distance symbol 29
    with extra bits 8191 (32 768, the whole window) and 8181, and symbol 28 with 8191 (24 576)."""
    prefix = bytearray(rng.integers(0, 256, 33000, dtype=np.uint8).tobytes())
    for r in range(0, 33000, 256):
        prefix[r] = int(rng.integers(0, 5))      # the filter bytes of rows 0 .. 128; the first match copies row 1's into row 129's
    prefix[33280 - 32758] = 2                    # the byte the second match copies into row 130's filter byte
    ops = [("len", 285, 0, 29, 8191), ("len", 285, 0, 29, 8181), ("len", 257, 0, 28, 8191)]
    ops += [7] * (131 * 256 - 33000 - 258 - 258 - 3)
    raw = _frame_of(131, 255, ops, prefix)
    bw = stored_block(prefix, final=False)
    bw, rec = dynamic_block(ops, flat_lens(286, [7, 256, 257, 285]), [0] * 28 + [1, 1], bw=bw)
    return assemble(131, 255, 0, b"\x78\x01" + bw.done() + struct.pack(">I", zlib.adler32(raw))), raw, [rec]


def dyn_fixed_dyn_fixed():
    """9 x 31 gray in blocks fixed, dynamic, fixed, dynamic (other tables: literal codes of 1, 10 and 11 bits, three distance codes),
    stored (empty, begun off a byte boundary), fixed."""
    rng = np.random.default_rng(20267)
    parts = [rows_ops(rng, 2, 31, range(256), (3, 9, 20), (1, 5, 31)), rows_ops(rng, 2, 31, range(256)),
             rows_ops(rng, 2, 31, range(256), (4, 17), (2, 32)), rows_ops(rng, 1, 31, range(256), (3, 5), (1, 7, 30)),
             rows_ops(rng, 2, 31, range(256), (3, 10), (3, 33))]
    raw = _frame_of(9, 31, sum(parts, []))
    other = lens_of(260, {**{s: 10 if s < 130 else 11 for s in range(1, 256)}, 0: 1, 256: 3, 257: 3, 259: 4})
    other_dist = lens_of(10, {0: 1, 5: 2, 9: 2})                 # distances 1, 7 .. 8 and 25 .. 32
    assert is_complete(other) and is_complete(other_dist)
    bw = fixed_block(parts[0], final=False)
    bw, rec_a = dynamic_block(parts[1], flat_lens(257, range(257)), [0], final=False, bw=bw)
    bw = fixed_block(parts[2], final=False, bw=bw)
    bw, rec_b = dynamic_block(parts[3], other, other_dist, final=False, bw=bw)
    rec_b["stored_at"] = bw.at()
    bw = stored_block(b"", final=False, bw=bw)
    bw = fixed_block(parts[4], bw=bw)
    return assemble(9, 31, 0, zlib_wrap(bw.done(), raw)), raw, [rec_a, rec_b]


# dyn_header_on_window_edge: where the device's first refill of its 4 KiB input window falls.  The kernel asks for input whenever its
# buffer holds fewer than 32 bits, at the points where it begins to read something (the block header, the counts, an HCLEN field, an
# item of the length sequence, a symbol); the refill comes at the first such point more than WINDOW_BITS - 32 bits into the stream.
# Each variant puts one thing at WINDOW_BITS - 31 exactly -- so the refill is there, and the thing before it is not yet past the
# mark -- or across WINDOW_BITS itself, the window's last bit.
_EDGE_SEQ = [8] + [(16, 6)] * 42 + [8, 8, 9, 9, (18, 11), (18, 11), (18, 11), (18, 12), (18, 14)]
WINDOW_EDGE_VARIANTS = {"hclen": ("hclen_at", 4, WINDOW_BITS - 31),             # the refill at HCLEN field 4; field 14 lies across WINDOW_BITS
                        "extra": ("item_at", 50, WINDOW_BITS - 31),             # the refill at an 18, with its 7 extra bits still to come
                        "extra_across": ("extra_at", 50, WINDOW_BITS - 3),      # the 7 extra bits of an 18 lie across WINDOW_BITS
                        "literal": ("op_at", 0, WINDOW_BITS - 31),              # the refill at the first literal code
                        "literal_across": ("op_at", 0, WINDOW_BITS - 4)}        # the first literal code (8 or 9 bits) lies across WINDOW_BITS


def dyn_header_on_window_edge(variant):
    """17 x 255 gray: two fixed blocks of literals and nothing else (a stored block would re-seek the window), about 4 090 bytes of
    them, then a dynamic block.  The number of literals in the fixed blocks, and how many of them take 9 bits, put the dynamic block
    where the variant wants it."""
    key, index, want = WINDOW_EDGE_VARIANTS[variant]
    lit, dist = flat_lens(286, range(257)), [0] * 30
    assert expand_seq(_EDGE_SEQ) == lit + dist
    probe = dynamic_block([0], lit, dist, length_seq=_EDGE_SEQ)[1]
    start = want - 16 - probe[key][index]        # the bit of the deflate data at which the dynamic block has to begin
    count, nine = divmod(start - 2 * 10, 8)      # two fixed blocks (3 header bits and 7 end-of-block bits each) of `count` literals,
                                                 # `nine` of them of 9 bits and the rest of 8
    rng = np.random.default_rng(20268)
    raw = bytearray(rng.integers(0, 144, 17 * 256, dtype=np.uint8).tobytes())
    for r in range(0, len(raw), 256):
        raw[r] = int(rng.integers(0, 5))
    for k in range(nine):
        raw[1 + k] = 200 + k
    raw = bytes(raw)
    bw = fixed_block(list(raw[:2000]), final=False)
    bw = fixed_block(list(raw[2000:count]), final=False, bw=bw)
    bw, rec = dynamic_block(list(raw[count:]), lit, dist, length_seq=_EDGE_SEQ, bw=bw)
    assert rec[key][index] + 16 == want
    return assemble(17, 255, 0, zlib_wrap(bw.done(), raw)), raw, [rec]


# ---------------------------------------------------------------- the cases the CPU and the GPU tests share
SHAPES = ((1, 1), (1, 9), (9, 1), (3, 5), (63, 7), (64, 7), (65, 7), (130, 3))     # the band edges of the unfilter: 63, 64, 65, 130 rows
COLOR_TYPES = (0, 2, 3, 4, 6)


def _pixels(rng, h, w, color_type):
    shape = (h, w) if CHANNELS[color_type] == 1 else (h, w, CHANNELS[color_type])
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _palette(rng, entries=256):
    return rng.integers(0, 256, (entries, 3), dtype=np.uint8)


def noise_plus_repeats(rng):
    """200 x 200 gray: noise rows and copies of rows up to 160 rows (32 160 bytes) back, so a compressor finds matches at every distance."""
    px = rng.integers(0, 256, (200, 200), dtype=np.uint8)
    for r in range(200):
        back = (1, 3, 40, 100, 160)[r % 5]
        if r >= back and r % 2:
            px[r] = px[r - back]
    return px


_ACCEPTED = None


def accepted_cases():
    """name -> file bytes of every case a decoder must decode on the device; built once."""
    global _ACCEPTED
    if _ACCEPTED is not None:
        return _ACCEPTED
    rng = np.random.default_rng(20260)
    c = {}
    for k, (h, w) in enumerate(SHAPES):
        for j in range(2):
            ct = COLOR_TYPES[(2 * k + j) % 5]
            c["shape_%dx%d_type%d" % (h, w, ct)] = write_png(_pixels(rng, h, w, ct), ct, "random", palette=_palette(rng) if ct == 3 else None,
                                                             rng=rng)[0]
    big = noise_plus_repeats(rng)
    c["noise_repeats_wbits15"] = write_png(big, 0, "random", dict(level=9, wbits=15, mem_level=9), rng=rng)[0]
    c["noise_repeats_wbits9"] = write_png(big, 0, "random", dict(level=9, wbits=9, mem_level=9), rng=rng)[0]
    for ct in COLOR_TYPES:
        c["type%d" % ct] = write_png(_pixels(rng, 5, 7, ct), ct, "random", palette=_palette(rng) if ct == 3 else None, rng=rng)[0]
    c["palette_trns"] = write_png(_pixels(rng, 5, 7, 3), 3, "random", palette=_palette(rng), trns=bytes(range(0, 250, 10)), rng=rng)[0]
    c["gray_trns"] = write_png(_pixels(rng, 5, 7, 0), 0, "random", trns=b"\x00\x07", rng=rng)[0]
    c["palette_short"] = write_png(_pixels(rng, 5, 7, 3), 3, "random", palette=_palette(rng, 100), rng=rng)[0]     # indices 100 .. 255: (0, 0, 0)
    for f in range(5):
        c["filter%d_rgb" % f] = write_png(_pixels(rng, 9, 11, 2), 2, f)[0]
        c["filter%d_graya" % f] = write_png(_pixels(rng, 67, 5, 4), 4, f)[0]
    c["filter_random_rgba"] = write_png(_pixels(rng, 70, 6, 6), 6, "random", rng=rng)[0]
    c["constant_paeth"] = write_png(np.full((66, 9, 3), 173, dtype=np.uint8), 2, 4)[0]
    c["constant_avg"] = write_png(np.full((5, 9), 255, dtype=np.uint8), 0, 3)[0]
    smooth = (np.add.outer(np.arange(17), np.arange(13))[:, :, None] * np.array([3, 5, 7, 0]) + rng.integers(0, 3, (17, 13, 4))).astype(np.uint8)
    for form in DEFLATE_FORMS:
        c["form_" + form] = write_png(smooth, 6, "random", form, rng=rng)[0]
    for split in SPLIT_PATTERNS:
        c["split_" + split] = write_png(_pixels(rng, 6, 9, 0), 0, "random", "stored" if split == "stored_len" else "default", split, rng=rng)[0]
    mid = write_png(smooth, 6, 1, "fixed")                               # cuts inside code words: every byte boundary of a fixed block
    c["split_code_words"] = assemble(17, 13, 6, mid[2], list(range(2, len(mid[2]), 3)))
    c["hand_fixed"] = hand_fixed_png()[0]
    c["hand_stored"] = hand_stored_png(rng)[0]
    c["hand_far_matches"] = hand_far_matches_png(rng)[0]
    c.update(dynamic_cases())
    _ACCEPTED = c
    return c


_RECORDS = {}


def dynamic_cases():
    """name -> file bytes of the hand-made dynamic-Huffman cases; case_records() and case_raw() keep what dynamic_block wrote and the
    frame's raw bytes.  Their own generators: the cases above stay byte for byte what they were."""
    made = {"dyn_long_codes": dyn_long_codes(), "dyn_single_distance": dyn_single_distance(), "dyn_no_distance": dyn_no_distance(),
            "dyn_lone_eob": dyn_lone_eob(), "dyn_repeats": dyn_repeats(), "dyn_counts_extremes_257_1": dyn_no_distance((1,)),
            "dyn_counts_extremes_286_30": dyn_long_codes(30, _EXTREME_CL, _EXTREME_SEQ), "dyn_len_284_31": dyn_len_284_31(),
            "dyn_dist_32768": dyn_dist_32768(np.random.default_rng(20269)), "dyn_fixed_dyn_fixed": dyn_fixed_dyn_fixed()}
    for variant in WINDOW_EDGE_VARIANTS:
        made["dyn_header_on_window_edge_" + variant] = dyn_header_on_window_edge(variant)
    c = {}
    for name, (data, raw, records, *_) in made.items():
        c[name] = data
        _RECORDS[name] = (records, raw)
    for name, (h, w) in (("dyn_long_codes", (1, 880)), ("dyn_single_distance", (2, 300))):      # cut into IDAT chunks at every byte
        stream = made[name][3]
        c[name + "_split_every_byte"] = assemble(h, w, 0, stream, split_points(stream, "every_byte"))
        _RECORDS[name + "_split_every_byte"] = _RECORDS[name]
    return c


def case_records(name):
    accepted_cases()
    return _RECORDS[name][0]


def case_raw(name):
    accepted_cases()
    return _RECORDS[name][1]


_DAMAGED = None


def damaged_cases():
    """name -> file bytes of every damaged (or merely odd) case: what each means is PIL's to say."""
    global _DAMAGED
    if _DAMAGED is not None:
        return _DAMAGED
    rng = np.random.default_rng(20261)
    h, w = 9, 31
    px = rng.integers(0, 256, (h, w), dtype=np.uint8)
    raw = filter_rows(px, 1, [int(v) for v in rng.integers(0, 5, h)])
    c = {}
    c["block_type_3"] = assemble(h, w, 0, b"\x78\x9c" + b"\x07" + raw[:40] + struct.pack(">I", zlib.adler32(raw)))
    stored = bytearray(deflate(raw, level=0))
    stored[5] ^= 0x10
    c["len_nlen"] = assemble(h, w, 0, bytes(stored))
    c["distance_before_start"] = assemble(h, w, 0, zlib_wrap(fixed_block([0, 1, (3, 3)] + [2] * 300).done(), raw))
    for form in ("default", "stored"):
        z = deflate(raw, **DEFLATE_FORMS[form])
        for cut in range(1, 13):
            c["truncated_%s_%d" % (form, cut)] = assemble(h, w, 0, z[:len(z) - cut])
    z = deflate(raw)
    for k in range(1, 5):
        bad = bytearray(z)
        bad[-k] ^= 0x40
        c["adler_byte_%d" % k] = assemble(h, w, 0, bytes(bad))
    c["filter_5"] = assemble(h, w, 0, deflate(filter_rows(px, 1, [0, 1, 2, 5, 4, 3, 2, 1, 0])))
    c["filter_255_last_row"] = assemble(h, w, 0, deflate(filter_rows(px, 1, [0] * 8 + [255])))
    c["short_raw"] = assemble(h, w, 0, deflate(raw[:-1]))
    c["short_raw_stored"] = assemble(h, w, 0, deflate(raw[:-7], level=0))
    c["long_raw"] = assemble(h, w, 0, deflate(raw + bytes(rng.integers(0, 256, 700, dtype=np.uint8))))
    c["long_raw_stored"] = assemble(h, w, 0, deflate(raw + b"tail" * 9, level=0))
    c["garbage_after_stream"] = assemble(h, w, 0, z + b"garbage after the stream")
    c["idat_crc"] = assemble(h, w, 0, z, idat_crc_xor=0x00010000)
    c.update(damaged_dynamic_cases(h, w, raw))
    _DAMAGED = c
    return c


DAMAGED_DYNAMIC = []                             # the names damaged_dynamic_cases() adds: each one a corrupt deflate stream


def damaged_dynamic_cases(h, w, raw):
    """One stream per detection rule of the dynamic-block path (and of the symbols of a fixed block) on the h x w gray frame `raw`.
    Header damage sits in the first block, symbol damage after the first five bytes of the frame: far before the last raw byte, so a
    decoder that stops at the last row still meets it."""
    c = {}

    def add(name, bw):
        c[name] = assemble(h, w, 0, zlib_wrap((bw[0] if isinstance(bw, tuple) else bw).done(), raw))

    lits = list(raw)
    flat, head = flat_lens(257, range(257)), list(raw[:5])
    with_lengths = flat_lens(286, list(range(256)) + [256, 257, 258, 285])
    for field in (30, 31):
        add("hlit_field_%d" % field, dynamic_block(lits, flat + [0] * field, [0], raw_header=(field, None, None)))
        add("hdist_field_%d" % field, dynamic_block(lits, flat, [0] * (field + 1), raw_header=(None, field, None)))
    add("cl_oversubscribed", dynamic_block(lits, flat, [0], cl_lens=lens_of(19, {0: 1, 8: 1, 9: 1})))
    add("cl_incomplete", dynamic_block(lits, flat, [0], cl_lens=lens_of(19, {0: 2, 8: 2, 9: 2})))
    add("cl_single", dynamic_block([], [8] * 257, [8], cl_lens=lens_of(19, {8: 1})))
    add("lit_oversubscribed", dynamic_block(lits, [8] * 257, [0]))
    add("lit_incomplete", dynamic_block(head[:2], lens_of(257, {raw[0]: 2, raw[1]: 2, 256: 2}), [0]))
    add("lit_single_length_2", dynamic_block([], lens_of(257, {256: 2}), [0]))
    add("lit_no_eob", dynamic_block(lits, [8] * 256 + [0], [0]))
    add("dist_oversubscribed", dynamic_block(lits, flat, [1, 1, 1]))
    add("dist_incomplete", dynamic_block(lits, flat, [2, 2, 2]))
    add("dist_single_length_2", dynamic_block(lits, flat, [2]))
    add("repeat_16_first", dynamic_block(lits, flat, [0], length_seq=[(16, 3)] + flat[3:] + [0]))
    add("repeat_16_past_total", dynamic_block(lits, flat, [0] * 5, length_seq=flat + [0, 0, 0, (16, 3)]))
    add("repeat_17_past_total", dynamic_block(lits, flat, [0] * 5, length_seq=flat + [0, 0, 0, (17, 3)]))
    add("repeat_18_past_total", dynamic_block(lits, flat, [0] * 30, length_seq=flat + [0] * 20 + [(18, 11)]))
    add("repeat_18_from_literals", dynamic_block(lits, flat, [0], length_seq=flat[:200] + [(18, 138)]))
    add("single_distance_unused_1", dynamic_block(head + [("len", 257, 0, None, 0), ("bits", 1, 1)] + lits[8:], with_lengths, [1]))
    add("lone_eob_unused_1", dynamic_block([("bits", 1, 1)], lens_of(257, {256: 1}), [0], final=False))
    add("length_without_distance", dynamic_block(head + [("len", 257, 0, None, 0), ("bits", 0, 8)] + lits[8:], with_lengths, [0]))
    for symbol in (286, 287):
        add("fixed_length_%d" % symbol, fixed_block(head + [("len", symbol, 0, 0, 0)] + lits[8:]))
    for symbol in (30, 31):
        add("fixed_distance_%d" % symbol, fixed_block(head + [("len", 257, 0, symbol, 0)] + lits[8:]))
    add("dyn_distance_before_start", dynamic_block(head + [(3, 6)] + lits[8:], with_lengths, lens_of(5, {0: 1, 4: 1})))
    stream, (first, _) = dyn_repeats()[3], dyn_repeats()[2]
    last = 2 + first["op_at"][0] // 8 + 10       # the tenth byte of the first block's symbols
    assert last - 2 <= 80 and last < len(stream) - 4 - 100
    for cut in range(2, last + 1):               # stream[:2] is the zlib header alone; the Adler-32 is far behind every cut
        c["truncated_dyn_repeats_%d" % cut] = assemble(9, 31, 0, stream[:cut])
    DAMAGED_DYNAMIC[:] = sorted(c)
    return c


def refused_cases():
    """name -> (file bytes, a word of the reason png_read.parse_png must give)"""
    rng = np.random.default_rng(20262)
    px = rng.integers(0, 256, (5, 8), dtype=np.uint8)
    raw = filter_rows(px, 1, [0] * 5)
    z = deflate(raw)
    c = {"not_png": (b"\xff\xd8\xff\xe0 not a png", "signature"),
         "interlaced": (assemble(5, 8, 0, z, interlace=1), "interlac"),
         "apng": (assemble(5, 8, 0, z, extra=[(b"acTL", struct.pack(">II", 1, 0))]), "acTL"),
         "no_plte": (assemble(5, 8, 3, z), "PLTE"),
         "not_deflate": (assemble(5, 8, 0, bytes([0x79, 0x9c - 0]) + z[2:]), "deflate"),
         "fdict": (assemble(5, 8, 0, bytes([0x78, 0xbb]) + z[2:]), "FDICT"),
         "window": (assemble(5, 8, 0, bytes([0x88, 0x1c]) + z[2:]), "32 KiB")}
    for depth in (1, 2, 4, 16):
        c["depth_%d" % depth] = (assemble(5, 8, 0, z, depth=depth), "bit depth %d" % depth)
    return c
