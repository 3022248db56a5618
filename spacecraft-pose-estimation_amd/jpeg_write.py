"""Host side of the device JPEG encoder (csrc/jpeg_encode.hip), the counterpart of jpeg_read.py: everything of a baseline file
that is not entropy-coded data.  The kernels write the scan; this module states the bytes in front of it -- SOI, JFIF APP0, DQT,
SOF0, DHT, SOS in the order and form libjpeg's jcmarker.c emits them (what PIL's save writes with its defaults) -- the
quality-scaled quantisation tables of jcparam.c, and the standard Huffman tables of T.81 annex K.3 as one code / length word per
symbol for upload.
"""
import struct

import numpy as np

from .jpeg_read import MODES, ZIGZAG as _ZIGZAG

HUFF_WORDS = 4 * 256                              # the uploaded table: [DC lum, AC lum, DC chroma, AC chroma][symbol]
ZIGZAG = _ZIGZAG.tolist()                         # a list of ints: header() builds bytes from it

# T.81 annex K.1, natural order
STD_QUANT = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32,
)

# T.81 annex K.3: (number of codes of length 1 .. 16, symbols in code order)
_AC_TAIL = [(r << 4) | s for r in range(16) for s in range(1, 11)]
STD_HUFF = (
    ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
     (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36,
      51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
      83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
      134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179,
      180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
      225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
    ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
     (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21,
      98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
      73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130,
      131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169,
      170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
      216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
)
assert all(sum(b) == len(v) for b, v in STD_HUFF) and sorted(STD_HUFF[1][1]) == sorted(STD_HUFF[3][1]) == sorted([0, 0xF0] + _AC_TAIL)


def quant_tables(quality):
    """jcparam.c: jpeg_quality_scaling + jpeg_add_quant_table with force_baseline -> two tables of 64 in natural order"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality=%r (1 .. 100)" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [[min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in STD_QUANT]


def huff_codes(bits, vals):
    """T.81 annex C: -> {symbol: (code, length)}"""
    out, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[p]] = (code, length)
            code += 1
            p += 1
        code <<= 1
    return out


def huff_upload():
    """uint32 [4][256]: code | length << 16 per symbol, 0 for a symbol the table does not hold"""
    t = np.zeros((4, 256), dtype=np.uint32)
    for i, (bits, vals) in enumerate(STD_HUFF):
        for sym, (code, length) in huff_codes(bits, vals).items():
            t[i, sym] = code | (length << 16)
    return t


def _seg(marker, body):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def header(height, width, mode, quality, comment=None):
    """The bytes from SOI up to and including SOS.  comment: the body of one COM segment, placed where libjpeg's
    jpeg_write_marker puts it (after APP0, before the tables)."""
    if mode not in MODES:
        raise ValueError("mode=%r (gray, 444, 420)" % (mode,))
    if not (1 <= height <= 65535 and 1 <= width <= 65535):
        raise ValueError("frame %dx%d (HxW), each 1 .. 65535" % (height, width))
    nc = 1 if mode == "gray" else 3
    qt = quant_tables(quality)
    f = b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if comment is not None:
        f += _seg(0xFE, comment)
    for t in range(2 if nc == 3 else 1):
        f += _seg(0xDB, bytes([t]) + bytes(qt[t][n] for n in ZIGZAG))
    samp = [0x22 if mode == "420" else 0x11, 0x11, 0x11]
    f += _seg(0xC0, struct.pack(">BHHB", 8, height, width, nc) + b"".join(bytes([c + 1, samp[c], min(c, 1)]) for c in range(nc)))
    for t in range(2 if nc == 3 else 1):
        for cls in (0, 1):
            bits, vals = STD_HUFF[2 * t + cls]
            f += _seg(0xC4, bytes([(cls << 4) | t]) + bytes(bits) + bytes(vals))
    f += _seg(0xDA, bytes([nc]) + b"".join(bytes([c + 1, 0x11 * min(c, 1)]) for c in range(nc)) + b"\x00\x3f\x00")
    return f
