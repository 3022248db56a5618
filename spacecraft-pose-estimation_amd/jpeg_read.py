"""Host side of the device JPEG decoder (csrc/jpeg_decode.hip): the marker walk, the decode tables and the per-image descriptor.

parse_jpeg(data) walks the markers of a baseline JPEG file with NumPy / bytes only and returns a JpegHeader: the sizes, the
sampling, the quantisation tables in natural order, the Huffman tables as libjpeg's bits[17] / huffval[256], the restart interval,
the byte range of the entropy-coded data and the byte ranges of its restart segments.  Everything the device does not decode is
refused by name with UnsupportedJpeg -- never a wrong picture.  descriptor(header) packs what the kernels read into DESC_BYTES
bytes, pack_batch(headers, files) builds the three uploads of one scpose_jpeg_decode call.  sample_span / idct_window state which
samples and blocks of a frame scpose_jpeg_decode_crop needs for a window of it.

Layout of a descriptor (little endian; include/scpose.h repeats it):
    int32 [16]   file_off lo, file_off hi (offset of the file in the concatenated bytes), seg_row0 (first row of the image in the
                 segment table), nseg, nsub, restart interval in MCUs (the whole image when the file has none), 10 x 0
    uint16[3][64]  quantisation table of component c, natural order
    6 slots        component c's DC table (slot 2 c) and AC table (slot 2 c + 1), each
                   uint16[512] first-level table on the next 9 bits: code length << 8 | symbol, 0 = longer than 9 bits
                   int32 [18]  libjpeg's maxcode[l] (-1: no code of length l; [17] = 0xfffff)
                   int32 [18]  libjpeg's valoffset[l]
                   uint8 [256] huffval
A row of the segment table is int32[4]: first byte and end of the segment's raw bytes (relative to the file), index of its first
subsequence inside the image, 0.  One row more than segments closes the table: its third word is nsub.
"""
import numpy as np

SUBSEQ_BYTES = 128          # SCPOSE_JPEG_SUBSEQ_BYTES
LUT_BITS = 9
DESC_HEAD_BYTES = 64
DESC_QUANT_OFF = 64
DESC_TABLES_OFF = 448
SLOT_BYTES = 1024 + 72 + 72 + 256
DESC_BYTES = 9216           # SCPOSE_JPEG_DESC_BYTES
MODES = {"gray": 0, "444": 1, "420": 2}   # SCPOSE_JPEG_GRAY / _444 / _420

# jpeg_natural_order: natural index of the i-th coefficient in zig-zag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
    dtype=np.int32)


class JpegError(ValueError):
    """The file is not a JPEG stream this decoder can turn into the right picture (corrupt, truncated, not converged)."""


class UnsupportedJpeg(JpegError):
    """A well-formed JPEG outside the decoded subset; the message names the reason."""


class JpegHeader:
    """What parse_jpeg found.  width, height, ncomp, mode ('gray' | '444' | '420'), hmax, vmax, mcus_x, mcus_y, blocks_per_mcu,
    n_blocks; qt uint16 (4, 64) natural order and comp_q; dc_bits / ac_bits uint8 (4, 17), dc_huffval / ac_huffval uint8 (4, 256)
    and comp_dc / comp_ac; restart_interval (0: none); data_start, data_end: the entropy-coded bytes; seg_start, seg_end: int64
    arrays, the raw bytes of each restart segment (file offsets); seg_sub0: first subsequence of each segment, nsub in the last."""

    @property
    def geometry(self):
        return (self.height, self.width, self.mode)


def _u16(b, p):
    return (int(b[p]) << 8) | int(b[p + 1])


def huff_derived(bits, huffval):
    """libjpeg's jpeg_make_d_derived_tbl: (maxcode int32[18], valoffset int32[18], lut uint16[512]) of one table."""
    sizes = np.repeat(np.arange(17), bits[:17].astype(np.int64))      # huffsize, codes in order of length
    n = int(sizes.size)
    if n > 256:
        raise JpegError("bad Huffman table: %d symbols" % n)
    codes = np.zeros(n, dtype=np.int64)
    maxcode = np.full(18, -1, dtype=np.int32)
    valoffset = np.zeros(18, dtype=np.int32)
    code, p = 0, 0
    for l in range(1, 17):
        cnt = int(bits[l])
        if cnt:
            valoffset[l] = p - code
            codes[p:p + cnt] = code + np.arange(cnt)
            p += cnt
            code += cnt
            maxcode[l] = code - 1
            if code > (1 << l):
                raise JpegError("bad Huffman table: code lengths overflow")
        code <<= 1
    maxcode[17] = 0xFFFFF
    lut = np.zeros(1 << LUT_BITS, dtype=np.uint16)
    for i in range(n):
        l = int(sizes[i])
        if l > LUT_BITS:
            break
        first = int(codes[i]) << (LUT_BITS - l)
        lut[first:first + (1 << (LUT_BITS - l))] = (l << 8) | int(huffval[i])
    return maxcode, valoffset, lut


def parse_jpeg(data):
    """bytes / bytearray / uint8 array of one file -> JpegHeader; raises UnsupportedJpeg (reason in the message) or JpegError."""
    b = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    n = int(b.size)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        raise UnsupportedJpeg("not a JPEG file (no SOI marker)")
    h = JpegHeader()
    h.qt = np.zeros((4, 64), dtype=np.uint16)
    h.dc_bits = np.zeros((4, 17), dtype=np.uint8); h.ac_bits = np.zeros((4, 17), dtype=np.uint8)
    h.dc_huffval = np.zeros((4, 256), dtype=np.uint8); h.ac_huffval = np.zeros((4, 256), dtype=np.uint8)
    have_q, have_dc, have_ac = [False] * 4, [False] * 4, [False] * 4
    h.restart_interval = 0
    adobe, jfif, frame = None, False, None
    pos = 2
    past = "a segment length that runs past the file"
    while True:
        while pos < n and b[pos] != 0xFF:          # garbage between segments: libjpeg resynchronises the same way
            pos += 1
        while pos + 1 < n and b[pos + 1] == 0xFF:  # fill bytes
            pos += 1
        if pos + 2 > n:
            raise UnsupportedJpeg(past + " (no SOS marker)")
        m = int(b[pos + 1])
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise UnsupportedJpeg("EOI before any scan")
        if pos + 2 > n:
            raise UnsupportedJpeg(past)
        ln = _u16(b, pos)
        if ln < 2 or pos + ln > n:
            raise UnsupportedJpeg(past)
        seg, end = pos + 2, pos + ln
        if m == 0xC0 or m == 0xC1 or m == 0xC2 or (0xC3 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC)):
            if m == 0xC1:
                raise UnsupportedJpeg("SOF1 (extended sequential) is not decoded")
            if m == 0xC2:
                raise UnsupportedJpeg("SOF2 (progressive) is not decoded")
            if m != 0xC0:
                raise UnsupportedJpeg("SOF%d (%s) is not decoded" % (m - 0xC0, "arithmetic coding" if m >= 0xC9 else "lossless or differential"))
            if frame is not None:
                raise UnsupportedJpeg("more than one frame header")
            if end - seg < 6:
                raise UnsupportedJpeg(past)
            prec, hh, ww, nf = int(b[seg]), _u16(b, seg + 1), _u16(b, seg + 3), int(b[seg + 5])
            if prec != 8:
                raise UnsupportedJpeg("%d-bit samples are not decoded" % prec)
            if nf not in (1, 3):
                raise UnsupportedJpeg("%d components are not decoded (1 or 3)" % nf)
            if hh < 1 or ww < 1:
                raise UnsupportedJpeg("a frame of %d x %d (a DNL-defined height is not decoded)" % (ww, hh))
            if end - seg < 6 + 3 * nf:
                raise UnsupportedJpeg(past)
            frame = [(int(b[seg + 6 + 3 * c]), int(b[seg + 7 + 3 * c]) >> 4, int(b[seg + 7 + 3 * c]) & 15, int(b[seg + 8 + 3 * c]))
                     for c in range(nf)]
            h.height, h.width, h.ncomp = hh, ww, nf
        elif m == 0xCC:
            raise UnsupportedJpeg("arithmetic coding (DAC marker) is not decoded")
        elif m == 0xC4:
            p = seg
            while p < end:
                if p + 17 > end:
                    raise UnsupportedJpeg(past)
                tc, th = int(b[p]) >> 4, int(b[p]) & 15
                bits = np.zeros(17, dtype=np.uint8); bits[1:] = b[p + 1:p + 17]
                cnt = int(bits.sum())
                if tc > 1 or th > 3 or cnt > 256 or p + 17 + cnt > end:
                    raise JpegError("bad Huffman table definition")
                tgt_b, tgt_v, tgt_h = (h.dc_bits, h.dc_huffval, have_dc) if tc == 0 else (h.ac_bits, h.ac_huffval, have_ac)
                tgt_b[th] = bits; tgt_v[th] = 0; tgt_v[th, :cnt] = b[p + 17:p + 17 + cnt]; tgt_h[th] = True
                p += 17 + cnt
        elif m == 0xDB:
            p = seg
            while p < end:
                pq, tq = int(b[p]) >> 4, int(b[p]) & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or p + 1 + size > end:
                    raise JpegError("bad quantisation table definition")
                vals = (b[p + 1:p + 1 + size].astype(np.uint16).reshape(64, 2) @ np.array([256, 1], dtype=np.uint16)) if pq \
                    else b[p + 1:p + 65].astype(np.uint16)
                h.qt[tq, ZIGZAG] = vals
                have_q[tq] = True
                p += 1 + size
        elif m == 0xDD:
            if ln != 4:
                raise JpegError("bad DRI segment")
            h.restart_interval = _u16(b, seg)
        elif m == 0xEE:
            if ln >= 14 and bytes(b[seg:seg + 5]) == b"Adobe":
                adobe = int(b[seg + 11])
        elif m == 0xE0:
            if ln >= 7 and bytes(b[seg:seg + 5]) == b"JFIF\0":
                jfif = True
        elif m == 0xDA:
            if frame is None:
                raise UnsupportedJpeg("SOS before a frame header")
            ns = int(b[seg])
            if ns != h.ncomp:
                raise UnsupportedJpeg("a non-interleaved scan (%d of %d components) is not decoded" % (ns, h.ncomp))
            if end - seg < 1 + 2 * ns + 3:
                raise UnsupportedJpeg(past)
            h.comp_dc, h.comp_ac = [], []
            for c in range(ns):
                if int(b[seg + 1 + 2 * c]) != frame[c][0]:
                    raise UnsupportedJpeg("scan components out of frame order")
                h.comp_dc.append(int(b[seg + 2 + 2 * c]) >> 4); h.comp_ac.append(int(b[seg + 2 + 2 * c]) & 15)
            ss, se, ahal = int(b[seg + 1 + 2 * ns]), int(b[seg + 2 + 2 * ns]), int(b[seg + 3 + 2 * ns])
            if ss != 0 or se != 63 or ahal != 0:
                raise UnsupportedJpeg("spectral selection / successive approximation in a sequential scan")
            pos = end
            break
        pos = end
    # ---- the frame
    h.comp_q = [f[3] for f in frame]
    samp = [(f[1], f[2]) for f in frame]
    if h.ncomp == 1:
        h.mode, h.hmax, h.vmax = "gray", 1, 1                     # one component: the MCU is one block whatever the factors say
    else:
        if adobe is not None and adobe != 1:
            raise UnsupportedJpeg("Adobe marker with transform %d for three components (not YCbCr)" % adobe)
        if adobe is None and not jfif and [f[0] for f in frame] == [0x52, 0x47, 0x42]:
            raise UnsupportedJpeg("three components named R, G, B (not YCbCr)")
        if samp == [(1, 1)] * 3:
            h.mode, h.hmax, h.vmax = "444", 1, 1
        elif samp == [(2, 2), (1, 1), (1, 1)]:
            h.mode, h.hmax, h.vmax = "420", 2, 2
        else:
            name = {((2, 1), (1, 1), (1, 1)): "4:2:2", ((1, 2), (1, 1), (1, 1)): "4:4:0", ((4, 1), (1, 1), (1, 1)): "4:1:1"}.get(tuple(samp), "this")
            raise UnsupportedJpeg("%s sampling (%s) is not decoded" % (name, ",".join("%dx%d" % s for s in samp)))
    for c in range(h.ncomp):
        if h.comp_q[c] > 3 or not have_q[h.comp_q[c]]:
            raise UnsupportedJpeg("a missing table: quantisation table %d" % h.comp_q[c])
        if h.comp_dc[c] > 3 or not have_dc[h.comp_dc[c]]:
            raise UnsupportedJpeg("a missing table: DC Huffman table %d" % h.comp_dc[c])
        if h.comp_ac[c] > 3 or not have_ac[h.comp_ac[c]]:
            raise UnsupportedJpeg("a missing table: AC Huffman table %d" % h.comp_ac[c])
    h.mcus_x = (h.width + 8 * h.hmax - 1) // (8 * h.hmax)
    h.mcus_y = (h.height + 8 * h.vmax - 1) // (8 * h.vmax)
    h.blocks_per_mcu = 1 if h.ncomp == 1 else h.hmax * h.vmax + 2
    h.n_mcus = h.mcus_x * h.mcus_y
    h.n_blocks = h.n_mcus * h.blocks_per_mcu
    # ---- the entropy-coded data: up to the first marker that is not RSTn; segments start after each RSTn
    h.data_start = pos
    body = b[pos:]
    mk = np.flatnonzero((body[:-1] == 0xFF) & (body[1:] != 0)) if body.size > 1 else np.zeros(0, dtype=np.int64)
    if body.size and body[-1] == 0xFF:
        mk = np.append(mk, body.size - 1)                         # an FF the file ends on: nothing follows it
    kinds = body[np.minimum(mk + 1, body.size - 1)] if mk.size else np.zeros(0, dtype=np.uint8)
    is_rst = (kinds >= 0xD0) & (kinds <= 0xD7) & (mk + 1 < body.size)
    stop = np.flatnonzero(~is_rst)
    if stop.size:
        k = int(stop[0])
        h.data_end = pos + int(mk[k])
        q = h.data_end
        while q + 1 < n and b[q + 1] == 0xFF:
            q += 1
        if q + 1 < n and b[q + 1] != 0xD9:
            raise UnsupportedJpeg("more than one scan (marker 0x%02X after the first)" % int(b[q + 1]))
        mk, is_rst = mk[:k], is_rst[:k]
    else:
        h.data_end = n                                            # no EOI: the stream runs to the end of the file
    rst = mk[is_rst] + pos
    h.seg_start = np.concatenate([[h.data_start], rst + 2]).astype(np.int64)
    h.seg_end = np.concatenate([rst, [h.data_end]]).astype(np.int64)
    ri = h.restart_interval if h.restart_interval > 0 else h.n_mcus
    want = (h.n_mcus + ri - 1) // ri
    if h.seg_start.size != want:
        raise JpegError("corrupt stream: %d restart segments for %d MCUs at interval %d" % (h.seg_start.size, h.n_mcus, h.restart_interval))
    h.mcus_per_segment = ri
    subs = np.maximum((h.seg_end - h.seg_start + SUBSEQ_BYTES - 1) // SUBSEQ_BYTES, 1)
    h.seg_sub0 = np.concatenate([[0], np.cumsum(subs)]).astype(np.int64)
    h.nsub = int(h.seg_sub0[-1])
    return h


def sample_span(p0, length, full, half):
    """(lo, hi), inclusive: the samples of one axis of a component's plane that the pixels [p0, p0 + length) of that axis read;
    hi < lo when there are none.  half False -- luma, and chroma at 4:4:4: the pixel's own sample.  half True -- chroma at 4:2:0:
    libjpeg's fancy h2v2 upsampling takes sample p >> 1 and its neighbour on one side or the other, never one outside the plane of
    ceil(full / 2) samples, so one sample more on each side, clamped at the plane's edge.  csrc/jpeg_decode.hip: sample_span."""
    if length <= 0:
        return 0, -1
    if not half:
        return p0, p0 + length - 1
    return max((p0 >> 1) - 1, 0), min(((p0 + length - 1) >> 1) + 1, (full + 1) // 2 - 1)


def idct_window(h, roi):
    """Per component of JpegHeader h the blocks (bx0, bx1, by0, by1), inclusive and in the component's own plane, whose inverse
    DCT scpose_jpeg_decode_crop runs for the window roi = [x0, y0, w, h] of the frame: those that hold a sample of sample_span.
    None for a component (every component) when the window is empty."""
    x0, y0, rw, rh = (int(v) for v in roi)
    out = []
    for c in range(h.ncomp):
        half = c > 0 and h.mode == "420"
        sx, sy = sample_span(x0, rw, h.width, half), sample_span(y0, rh, h.height, half)
        out.append(None if sx[1] < sx[0] or sy[1] < sy[0] else (sx[0] >> 3, sx[1] >> 3, sy[0] >> 3, sy[1] >> 3))
    return out


def descriptor(h, file_off=0, seg_row0=0):
    """The DESC_BYTES bytes of one image (uint8 array)."""
    d = np.zeros(DESC_BYTES, dtype=np.uint8)
    head = d[:DESC_HEAD_BYTES].view(np.int32)
    d[:8].view(np.int64)[0] = int(file_off)
    head[2], head[3], head[4], head[5] = seg_row0, h.seg_start.size, h.nsub, h.mcus_per_segment
    q = d[DESC_QUANT_OFF:DESC_TABLES_OFF].view(np.uint16).reshape(3, 64)
    for c in range(h.ncomp):
        q[c] = h.qt[h.comp_q[c]]
        for kind, (bits, vals, sel) in enumerate(((h.dc_bits, h.dc_huffval, h.comp_dc), (h.ac_bits, h.ac_huffval, h.comp_ac))):
            o = DESC_TABLES_OFF + (2 * c + kind) * SLOT_BYTES
            maxcode, valoffset, lut = huff_derived(bits[sel[c]], vals[sel[c]])
            d[o:o + 1024].view(np.uint16)[:] = lut
            d[o + 1024:o + 1096].view(np.int32)[:] = maxcode
            d[o + 1096:o + 1168].view(np.int32)[:] = valoffset
            d[o + 1168:o + 1424] = vals[sel[c]]
    return d


def segment_rows(h):
    """int32 (nseg + 1, 4): [start, end, first subsequence, 0] relative to the file; the closing row carries nsub."""
    rows = np.zeros((h.seg_start.size + 1, 4), dtype=np.int32)
    rows[:-1, 0], rows[:-1, 1] = h.seg_start, h.seg_end
    rows[:, 2] = h.seg_sub0
    return rows


def pack_batch(headers, files):
    """Images of one geometry -> (desc uint8 (N, DESC_BYTES), segs int32 (R, 4), data uint8 (B,), max_subs): the three uploads of
    one scpose_jpeg_decode call.  Each file starts on a 16-byte boundary of `data`."""
    descs, rows, chunks, off, row0, max_subs = [], [], [], 0, 0, 1
    for h, f in zip(headers, files):
        raw = np.frombuffer(f, dtype=np.uint8) if not isinstance(f, np.ndarray) else f
        descs.append(descriptor(h, off, row0))
        r = segment_rows(h)
        rows.append(r); row0 += r.shape[0]
        pad = (-raw.size) % 16
        chunks.append(raw)
        if pad:
            chunks.append(np.zeros(pad, dtype=np.uint8))
        off += raw.size + pad
        max_subs = max(max_subs, h.nsub)
    return np.stack(descs), np.concatenate(rows), np.concatenate(chunks), max_subs
