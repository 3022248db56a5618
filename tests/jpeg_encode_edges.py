"""Frames that reach the paths of csrc/jpeg_encode.hip the fixtures of jpeg_encode_cases.py leave alone: more than one scan tile of
blocks, more than 256 tiles of raw bytes, 0xFF bytes and stream ends on the seams of the stuffing and write passes, a colour
lattice whose DC values state every component value exactly, and sweeps of sizes and qualities.  Every named case is
(frames, quality, mode); the CPU tests (test_jpeg_encode.py) prove from PIL's bytes that a case has the property it is named
for, the GPU tests (test_gpu_jpeg_encode_edges.py) hold the device to the same bytes."""
import functools

import numpy as np

import jpeg_encode_cases as C
import jpeg_encode_restated as R

SCAN_TILE = 4096                # blocks per workgroup of the bit-count scan (scan_device.h: kScanTile)
RAW_TILE = 4096                 # unstuffed bytes per workgroup of the stuffing passes (jpeg_encode.hip: kTileBytes)
COUNT_STEP = 256                # raw tiles per step of scan_tile_counts


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def raw_scan(file_bytes):
    """the entropy-coded bytes between the SOS segment and EOI, FF 00 unstuffed"""
    b = bytes(file_bytes)
    assert b[:2] == b"\xff\xd8" and b[-2:] == b"\xff\xd9"
    p = 2
    while True:
        assert b[p] == 0xFF and b[p + 1] not in (0x00, 0xFF, 0xD8, 0xD9), p
        marker, p = b[p + 1], p + 2 + int.from_bytes(b[p + 2:p + 4], "big")
        if marker == 0xDA:
            break
    body = b[p:-2]
    assert body.count(b"\xff") == body.count(b"\xff\x00")          # no restart markers: every FF is a stuffed data byte
    return body.replace(b"\xff\x00", b"\xff")


def blocks_of(h, w, mode):
    cdiv = lambda a, b: -(-a // b)
    return cdiv(h, 16) * cdiv(w, 16) * 6 if mode == "420" else cdiv(h, 8) * cdiv(w, 8) * (1 if mode == "gray" else 3)


# ---- more than one scan tile: [noise, constant, gradient] per mode, so the totals of one launch differ widely
MULTI_TILE_QUALITY = 95
MULTI_TILE_SIZES = {"gray": (520, 512), "444": (304, 304), "420": (423, 419)}     # 4160, 4332, 4374 blocks; 423 x 419: 27 x 27 MCUs


@functools.lru_cache(maxsize=None)
def multi_tile(mode):
    h, w = MULTI_TILE_SIZES[mode]
    return np.stack([C.content(name, h, w) for name in ("noise", "constant", "gradient")]), MULTI_TILE_QUALITY, mode


# ---- more than 256 tiles of raw bytes: the second step of scan_tile_counts and its int64 carry
def many_raw_tiles():
    return noise(560, 512, 560512)[None], 100, "444"


# ---- stream edges: noise at quality 100; the seeds were found with PIL, test_jpeg_encode.py proves each from PIL's bytes again
EDGE_QUALITY = 100
EDGES = {                       # name: ((H, W), mode, seed, property)
    "last_ff_444": ((40, 48), "444", 1, "last_ff"),
    "last_ff_420": ((40, 48), "420", 0, "last_ff"),
    "last_ff_gray": ((40, 48), "gray", 6, "last_ff"),
    "ff_ends_tile": ((40, 48), "444", 14, "ff_at_4095"),
    "ff_begins_tile": ((40, 48), "444", 203, "ff_at_4096"),
    "length_16n": ((40, 48), "444", 13, "length_16n"),
    "one_tile_a": ((40, 73), "gray", 21, "one_tile"),
    "one_tile_b": ((40, 73), "gray", 33, "one_tile"),
    "one_tile_c": ((40, 73), "gray", 55, "one_tile"),
}
EDGE_PROPERTIES = {
    "last_ff": lambda raw: raw[-1] == 0xFF,                        # FF 00 directly before EOI
    "ff_at_4095": lambda raw: len(raw) > RAW_TILE and raw[RAW_TILE - 1] == 0xFF,       # its 00 is the next tile's first byte
    "ff_at_4096": lambda raw: len(raw) > RAW_TILE + 1 and raw[RAW_TILE] == 0xFF,
    "length_16n": lambda raw: len(raw) % 16 == 0 and len(raw) % RAW_TILE != 0,         # the EOI thread holds 16 bytes
    "one_tile": lambda raw: len(raw) == RAW_TILE,
}
EDGE_BATCH = ("last_ff_444", "ff_ends_tile", "ff_begins_tile", "length_16n")            # the 40 x 48 4:4:4 frames, one launch


def edge(name):
    (h, w), mode, seed, _ = EDGES[name]
    return noise(h, w, seed)[None], EDGE_QUALITY, mode


def edge_batch():
    return np.concatenate([edge(name)[0] for name in EDGE_BATCH]), EDGE_QUALITY, "444"


# ---- colour lattice: one constant cell per colour; at quality 100 the DC value of a constant block is 8 (v - 128)
LEVELS = (0, 1, 2, 64, 127, 128, 129, 200, 253, 254, 255)
LATTICE_CELLS = (32, 42)        # rows, columns of cells


def lattice_colours():
    grid = np.array([(r, g, b) for r in LEVELS for g in LEVELS for b in LEVELS], dtype=np.uint8)
    pad = np.random.default_rng(1331).integers(0, 256, (LATTICE_CELLS[0] * LATTICE_CELLS[1] - len(grid), 3), dtype=np.uint8)
    return np.concatenate([grid, pad])


@functools.lru_cache(maxsize=None)
def lattice(mode):
    cell = 16 if mode == "420" else 8
    cells = lattice_colours().reshape(LATTICE_CELLS + (3,))
    return np.repeat(np.repeat(cells, cell, axis=0), cell, axis=1)[None].copy(), 100, mode


def lattice_dc(blocks, mode):
    """(blocks, 64) in scan order -> (cells, components) DC values; the four Y blocks of a 4:2:0 cell must agree"""
    dc = np.asarray(blocks)[:, 0]
    if mode == "gray":
        return dc.reshape(-1, 1)
    if mode == "444":
        return dc.reshape(-1, 3)
    mcu = dc.reshape(-1, 6)
    assert (mcu[:, :4] == mcu[:, :1]).all()
    return mcu[:, 3:]


def jccolor(rgb):
    """jccolor.c's rgb_ycc_convert from its FIX() constants, without the tables of the restatement: (..., 3) -> Y, Cb, Cr"""
    fix = lambda x: int(x * 65536 + 0.5)
    r, g, b = (np.asarray(rgb)[..., i].astype(np.int64) for i in range(3))
    half, offset = 1 << 15, 128 << 16
    y = (fix(0.29900) * r + fix(0.58700) * g + fix(0.11400) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.50000) * b + offset + half - 1) >> 16
    cr = (fix(0.50000) * r - fix(0.41869) * g - fix(0.08131) * b + offset + half - 1) >> 16
    return np.stack([y, cb, cr], axis=-1)


# ---- sweeps: every size around the block and MCU edges at quality 90, every quality on one frame
SWEEP_EDGES = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33)
SWEEP_SIZES = tuple((h, w) for h in SWEEP_EDGES for w in SWEEP_EDGES)
SWEEP_QUALITY = 90
QUALITY_SWEEP = tuple(range(1, 101))
QUALITY_SWEEP_SIZE = (16, 24)


def size_case(h, w, mode):
    return C.content("noise", h, w)[None], SWEEP_QUALITY, mode


def quality_case(q, mode):
    return C.content("noise", *QUALITY_SWEEP_SIZE)[None], q, mode


# ---- references, computed once per process and shared by the tests of a module
_refs = {}


def pil_files(key, case):
    """PIL's files of the case's frames; key names the case"""
    if ("pil", key) not in _refs:
        frames, q, mode = case
        _refs["pil", key] = [C.pil_bytes(f, q, mode) for f in frames]
    return _refs["pil", key]


def restated_files(key, case):
    if ("restated", key) not in _refs:
        frames, q, mode = case
        _refs["restated", key] = [R.encode(f, q, mode) for f in frames]
    return _refs["restated", key]
