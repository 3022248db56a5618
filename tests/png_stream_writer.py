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

    def done(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def _fixed_lit(bw, s):
    if s < 144:
        bw.code(0x30 + s, 8)
    elif s < 256:
        bw.code(0x190 + s - 144, 9)
    elif s < 280:
        bw.code(s - 256, 7)
    else:
        bw.code(0xC0 + s - 280, 8)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_block(ops, final=True, bw=None):
    """One fixed-Huffman block from ops: an int is a literal, (length, distance) a match.  -> (BitWriter, the bytes the ops produce given
    what came before is empty)."""
    bw = bw or BitWriter()
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    for op in ops:
        if isinstance(op, tuple):
            ln, d = op
            li = 28 if ln == 258 else max(i for i in range(28) if _LEN_BASE[i] <= ln)
            _fixed_lit(bw, 257 + li)
            bw.bits(ln - _LEN_BASE[li], _LEN_EXTRA[li])
            di = max(i for i in range(30) if _DIST_BASE[i] <= d)
            bw.code(di, 5)
            bw.bits(d - _DIST_BASE[di], _DIST_EXTRA[di])
        else:
            _fixed_lit(bw, op)
    _fixed_lit(bw, 256)
    return bw


def run_ops(ops, out=None):
    out = bytearray() if out is None else out
    for op in ops:
        if isinstance(op, tuple):
            for _ in range(op[0]):
                out.append(out[-op[1]])
        else:
            out.append(op)
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
    _ACCEPTED = c
    return c


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
    _DAMAGED = c
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
