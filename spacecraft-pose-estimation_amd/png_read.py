"""Host side of the device PNG decoder (csrc/png_decode.hip): the chunk walk and the per-image descriptor.

parse_png(data) walks the chunks of a PNG file with bytes / zlib.crc32 only and returns a PngHeader: the sizes, the colour type, the
palette zero-padded to 256 x 3 bytes and the byte spans of the IDAT payloads.  Everything the device does not decode is refused by
name with UnsupportedPng -- never a wrong picture.  A bad CRC of IHDR, PLTE or an IDAT is not a refusal: the header says so
(crc_ok False) and the file goes to the host decoder, which raises.  pack_batch(headers, files) joins the IDAT payloads of each image
into one contiguous zlib stream and builds the descriptors: chunk boundaries never reach the device.

Layout of a descriptor (little endian; include/scpose.h repeats it), DESC_BYTES bytes:
    int64        offset of the image's zlib stream in the concatenated bytes (a multiple of 16)
    int64        length of the stream in bytes: the two header bytes, the deflate blocks, the Adler-32 and whatever follows
    int32 [4]    height, width, colour type, channels (bytes per pixel of a scan line)
    int32 [8]    0
    uint8 [256][3]  the palette, R G B, entries the file does not define are 0 (colour type 3 only)
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
DESC_HEAD_BYTES = 64
DESC_BYTES = 832            # SCPOSE_PNG_DESC_BYTES
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}     # colour type -> bytes per pixel at bit depth 8
CORRUPT, CHECKSUM, FILTER = 1, 2, 4           # SCPOSE_PNG_CORRUPT / _CHECKSUM / _FILTER


class PngError(ValueError):
    """The file is not a PNG stream that decodes to a picture (corrupt, truncated, bad checksum); carries the host decoder's message."""


class UnsupportedPng(ValueError):
    """A PNG outside the decoded subset, or not a PNG; the message names the reason."""


class PngHeader:
    """What parse_png found.  height, width, color_type, channels; palette uint8 (256, 3); idat: list of (start, end) byte spans of
    the IDAT payloads in file order; stream_bytes: their total; crc_ok: False when IHDR, PLTE or an IDAT fails its CRC."""

    @property
    def geometry(self):
        return (self.height, self.width, self.channels)


def parse_png(data):
    """bytes / bytearray / uint8 array of one file -> PngHeader; raises UnsupportedPng with the reason in the message."""
    b = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    n = len(b)
    if n < 8 or b[:8] != SIGNATURE:
        raise UnsupportedPng("not a PNG file (no PNG signature)")
    h = PngHeader()
    h.palette = np.zeros((256, 3), dtype=np.uint8)
    h.idat, h.crc_ok = [], True
    have_ihdr, have_plte = False, False
    pos = 8
    while pos + 8 <= n:
        ln, kind = struct.unpack(">I4s", b[pos:pos + 8])
        body, end = pos + 8, pos + 8 + ln
        if end + 4 > n:
            if kind == b"IDAT" and have_ihdr:
                h.crc_ok = False             # a file cut inside its image data: the host decoder says what that means
                break
            raise UnsupportedPng("a chunk length that runs past the file (%s)" % kind.decode("latin-1"))
        if not have_ihdr and kind != b"IHDR":
            raise UnsupportedPng("not a PNG file (no IHDR chunk first)")
        if kind in (b"IHDR", b"PLTE", b"IDAT") and zlib.crc32(b[pos + 4:end]) != struct.unpack(">I", b[end:end + 4])[0]:
            h.crc_ok = False
        if kind == b"IHDR":
            if ln != 13:
                raise UnsupportedPng("an IHDR chunk of %d bytes" % ln)
            h.width, h.height, depth, h.color_type, comp, filt, interlace = struct.unpack(">IIBBBBB", b[body:end])
            if h.color_type not in CHANNELS:
                raise UnsupportedPng("colour type %d is not a PNG colour type" % h.color_type)
            if depth != 8:
                raise UnsupportedPng("bit depth %d is not decoded (8 only)" % depth)
            if interlace != 0:
                raise UnsupportedPng("Adam7 interlacing is not decoded")
            if comp != 0 or filt != 0:
                raise UnsupportedPng("compression method %d / filter method %d is not PNG's" % (comp, filt))
            if h.width < 1 or h.height < 1 or h.width > 65535 or h.height > 65535:
                raise UnsupportedPng("a frame of %d x %d (each side 1 .. 65535)" % (h.width, h.height))
            h.channels = CHANNELS[h.color_type]
            have_ihdr = True
        elif kind == b"acTL":
            raise UnsupportedPng("an acTL chunk (APNG) is not decoded")
        elif kind == b"PLTE":
            if ln % 3 or ln > 768:
                raise UnsupportedPng("a PLTE chunk of %d bytes" % ln)
            h.palette[:ln // 3] = np.frombuffer(b, dtype=np.uint8, count=ln, offset=body).reshape(-1, 3)
            have_plte = True
        elif kind == b"IDAT":
            h.idat.append((body, end))
        elif kind == b"IEND":
            break
        pos = end + 4
    if not have_ihdr:
        raise UnsupportedPng("not a PNG file (no IHDR chunk first)")
    if h.color_type == 3 and not have_plte:
        raise UnsupportedPng("a missing PLTE chunk for colour type 3")
    h.stream_bytes = sum(e - s for s, e in h.idat)
    head = b"".join(b[s:e] for s, e in h.idat if e > s)[:2] if h.stream_bytes >= 2 else b""
    if len(head) < 2:
        raise UnsupportedPng("no zlib header: %d bytes of image data" % h.stream_bytes)
    cmf, flg = head[0], head[1]
    if cmf & 15 != 8:
        raise UnsupportedPng("a zlib header that is not deflate (method %d)" % (cmf & 15))
    if cmf >> 4 > 7:
        raise UnsupportedPng("a zlib header that claims a window above 32 KiB")
    if flg & 32:
        raise UnsupportedPng("a zlib header with FDICT set (preset dictionary)")
    if ((cmf << 8) | flg) % 31:
        raise UnsupportedPng("a zlib header that fails its check bits")
    return h


def descriptor(h, stream_off, stream_len):
    """The DESC_BYTES bytes of one image (uint8 array)."""
    d = np.zeros(DESC_BYTES, dtype=np.uint8)
    d[:16].view(np.int64)[:] = (int(stream_off), int(stream_len))
    d[16:32].view(np.int32)[:] = (h.height, h.width, h.color_type, h.channels)
    d[DESC_HEAD_BYTES:] = h.palette.reshape(-1)
    return d


def pack_batch(headers, files):
    """Images of one geometry -> (desc uint8 (N, DESC_BYTES), data uint8 (B,)): the uploads of one scpose_png_decode call.  The IDAT
    payloads of an image are joined into one zlib stream, which starts on a 16-byte boundary of `data`."""
    descs, chunks, off = [], [], 0
    for h, f in zip(headers, files):
        raw = f.tobytes() if isinstance(f, np.ndarray) else bytes(f)
        stream = b"".join(raw[s:e] for s, e in h.idat)
        descs.append(descriptor(h, off, len(stream)))
        stream += b"\0" * ((-len(stream)) % 16)
        chunks.append(np.frombuffer(stream, dtype=np.uint8))
        off += len(stream)
    return np.stack(descs), np.concatenate(chunks)
