"""Which device decoder takes a compressed image file: the one rule the loader (dataset/JointsDataset._read_compressed) and the batch
driver (ops.decode_jpeg / decode_png / decode_crop) both ask.  Host only: bytes in, a header or a reason out.

A file is the JPEG decoder's when jpeg_read.parse_jpeg accepts it; else the PNG decoder's when png_read.parse_png accepts it and
every chunk it read passes its CRC; else the host decoder's, for the reason the refusing parser names.
"""
from .jpeg_read import UnsupportedJpeg, parse_jpeg
from .png_read import SIGNATURE, UnsupportedPng, parse_png

BAD_CRC = "a chunk fails its CRC"      # a PNG parse_png accepts, damaged: the host decoder says what that means
NO_DECODER = "no device decoder is enabled"


def is_png(raw):
    """Whether the file starts with the PNG signature: a refusal of such a file is the PNG side's (UnsupportedPng, PngError)."""
    return bytes(raw[:8]) == SIGNATURE


def sniff(raw, jpeg=True, png=False):
    """raw: the bytes of one file; jpeg, png: the device decoders on offer.  -> (kind, header, None) with kind "jpeg" | "png" and the
    parser's header, or (None, None, reason): the UnsupportedJpeg text; with png, the UnsupportedPng text when the file has the PNG
    signature (or the JPEG decoder is not on offer), or BAD_CRC.  A JpegError that is not UnsupportedJpeg (a broken table) passes through."""
    reason = NO_DECODER
    if jpeg:
        try:
            return "jpeg", parse_jpeg(raw), None
        except UnsupportedJpeg as e:
            reason = str(e)
    if png:
        try:
            head = parse_png(raw)
        except UnsupportedPng as e:
            return None, None, str(e) if not jpeg or is_png(raw) else reason
        if head.crc_ok:
            return "png", head, None
        reason = BAD_CRC
    return None, None, reason
