"""Makes tests/golden/zstd_frames.npz: Zstandard frames that the system's libzstd (through ctypes) makes of event-packet
flatbuffers, so that the GPU tests of the ZSTD reader need no libzstd.  Run from the repository root:

    python tests/golden/make_zstd_golden.py

raw_<events>: the size-prefixed EVTS flatbuffer of that many events (tests/aedat4_stream_writer.py).  frame_<events>_<level>_<c>:
one frame of it at that compression level, c = 1 with the content checksum flag.  version: libzstd's version number.
"""
import ctypes
import ctypes.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import aedat4_stream_writer as W  # noqa: E402

EVENTS = (0, 1, 12, 700, 9000)
LEVELS = (3, 19)
HW = (48, 64)
ZSTD_c_compressionLevel, ZSTD_c_checksumFlag = 100, 201


def load_libzstd():
    """libzstd through ctypes, or None."""
    for name in ("libzstd.so.1", ctypes.util.find_library("zstd")):
        if not name:
            continue
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        lib.ZSTD_compressBound.restype = ctypes.c_size_t
        lib.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        lib.ZSTD_createCCtx.restype = ctypes.c_void_p
        lib.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
        lib.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
        lib.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        lib.ZSTD_compress2.restype = ctypes.c_size_t
        lib.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        lib.ZSTD_decompress.restype = ctypes.c_size_t
        lib.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        lib.ZSTD_isError.restype = ctypes.c_uint
        lib.ZSTD_isError.argtypes = [ctypes.c_size_t]
        lib.ZSTD_versionNumber.restype = ctypes.c_uint
        return lib
    return None


def compress(lib, data, level=3, checksum=False):
    data = bytes(data)
    cctx = lib.ZSTD_createCCtx()
    try:
        for key, value in ((ZSTD_c_compressionLevel, level), (ZSTD_c_checksumFlag, int(checksum))):
            if lib.ZSTD_isError(lib.ZSTD_CCtx_setParameter(cctx, key, value)):
                raise RuntimeError("ZSTD_CCtx_setParameter(%d, %d) failed" % (key, value))
        cap = lib.ZSTD_compressBound(len(data))
        dst = ctypes.create_string_buffer(cap)
        n = lib.ZSTD_compress2(cctx, dst, cap, data, len(data))
        if lib.ZSTD_isError(n):
            raise RuntimeError("ZSTD_compress2 failed")
        return dst.raw[:n]
    finally:
        lib.ZSTD_freeCCtx(cctx)


def decompress(lib, frame, capacity):
    """-> the decoded bytes, None when libzstd refuses the frame."""
    frame = bytes(frame)
    dst = ctypes.create_string_buffer(max(capacity, 1))
    n = lib.ZSTD_decompress(dst, capacity, frame, len(frame))
    return None if lib.ZSTD_isError(n) else dst.raw[:n]


def main():
    lib = load_libzstd()
    if lib is None:
        raise SystemExit("libzstd does not load")
    out = {"version": np.int64(lib.ZSTD_versionNumber())}
    for n in EVENTS:
        raw = W.evts_payload(*W.random_events(n, HW, seed=100 + n, step=12))
        out["raw_%d" % n] = np.frombuffer(raw, dtype=np.uint8)
        for level in LEVELS:
            for c in (0, 1):
                frame = compress(lib, raw, level, bool(c))
                assert decompress(lib, frame, len(raw)) == raw
                out["frame_%d_%d_%d" % (n, level, c)] = np.frombuffer(frame, dtype=np.uint8)
    path = os.path.join(HERE, "zstd_frames.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
