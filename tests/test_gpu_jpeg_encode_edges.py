"""csrc/jpeg_encode.hip on the cases of tests/jpeg_encode_edges.py, each proven by tests/test_jpeg_encode.py to have its property:
more than one scan tile of blocks, more than 256 tiles of raw bytes, 0xFF bytes and stream ends on the seams of the stuffing and
write passes, the colour lattice, the sweeps of sizes and qualities; through the C ABI the SCPOSE_JPEG_ENC_TABLES status and a
capacity that ends exactly on a stream.  ops.encode_jpeg equals PIL and the NumPy restatement byte for byte everywhere."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import jpeg_encode_cases as C
import jpeg_encode_edges as E
import jpeg_encode_restated as R
import jpeg_decode_restated as D

pytestmark = pytest.mark.gpu


def _encode(gpu_ops, case):
    frames, q, mode = case
    got = gpu_ops.encode_jpeg(torch.from_numpy(frames).cuda(), quality=q, subsampling=mode)
    assert len(got) == len(frames)
    return got


def _check(gpu_ops, key, case):
    got = _encode(gpu_ops, case)
    for i, (g, p, r) in enumerate(zip(got, E.pil_files(key, case), E.restated_files(key, case))):
        assert len(g) == len(p), (key, i, len(g), len(p))
        assert g == p, (key, i, "PIL", next(k for k in range(len(p)) if g[k] != p[k]))
        assert g == r, (key, i, "restatement")
    return got


@pytest.mark.parametrize("mode", C.MODES)
def test_multi_tile_batches_and_two_runs(gpu_ops, mode):
    case = E.multi_tile(mode)
    a = _check(gpu_ops, ("multi", mode), case)
    assert _encode(gpu_ops, case) == a                             # the atomicOr emit does not depend on the order of the tiles


def test_multi_tile_420_round_trip_through_the_device_decoder(gpu_ops):
    case = E.multi_tile("420")
    files = _encode(gpu_ops, case)
    back, info = gpu_ops.decode_jpeg(files)
    assert not info["fallback"]
    got = back.cpu().numpy()
    for i, p in enumerate(E.pil_files(("multi", "420"), case)):
        assert np.array_equal(got[i], D.pil_decode(p)), i


def test_more_than_256_raw_tiles_then_a_small_frame(gpu_ops):
    _check(gpu_ops, "many_raw_tiles", E.many_raw_tiles())
    _check(gpu_ops, ("size", 9, 17, "444"), E.size_case(9, 17, "444"))      # another size in a call of its own, the workspace reused


@pytest.mark.parametrize("name", sorted(E.EDGES))
def test_stream_edges_one_frame_per_call(gpu_ops, name):
    _check(gpu_ops, name, E.edge(name))


def test_stream_edges_packed_in_one_batch(gpu_ops):
    got = _encode(gpu_ops, E.edge_batch())
    assert got == [E.pil_files(n, E.edge(n))[0] for n in E.EDGE_BATCH]
    assert got == [E.restated_files(n, E.edge(n))[0] for n in E.EDGE_BATCH]


@pytest.mark.parametrize("mode", C.MODES)
def test_colour_lattice(gpu_ops, mode):
    _check(gpu_ops, ("lattice", mode), E.lattice(mode))


@pytest.mark.parametrize("mode", C.MODES)
def test_size_sweep(gpu_ops, mode):
    for h, w in E.SWEEP_SIZES:
        _check(gpu_ops, ("size", h, w, mode), E.size_case(h, w, mode))


@pytest.mark.parametrize("mode", C.MODES)
def test_quality_sweep(gpu_ops, mode):
    for q in E.QUALITY_SWEEP:
        _check(gpu_ops, ("quality", q, mode), E.quality_case(q, mode))


# ---- the C ABI
GUARD = 4096


def _raw_call(gpu_ops, frames, quality, mode, huff, capacity):
    """scpose_jpeg_encode with the caller's tables and capacity; out is pre-filled with 0xA5 and carries a guard behind `capacity`
    -> (status, offsets, out as a host array, header)"""
    nat = gpu_ops.nat
    jw = importlib.import_module("spacecraft-pose-estimation_amd.jpeg_write")
    lib = nat.lib()
    n, h, w = frames.shape[:3]
    head = jw.header(h, w, mode, quality)
    ws = ctypes.c_size_t()
    assert lib.scpose_jpeg_encode_workspace_bytes(n, h, w, jw.MODES[mode], ctypes.byref(ws)) == 0
    d = torch.from_numpy(frames).cuda()
    d_huff = torch.from_numpy(np.ascontiguousarray(huff, dtype=np.uint32).view(np.int32)).cuda()
    assert d_huff.shape == (4, 256)
    d_head = torch.frombuffer(bytearray(head), dtype=torch.uint8).cuda()
    work = torch.empty(ws.value, dtype=torch.uint8, device="cuda")
    out = torch.full((capacity + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")      # the guard lies inside the allocation
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.scpose_jpeg_encode(p(d), n, h, w, jw.MODES[mode], quality, p(d_huff), p(d_head), len(head), p(out), capacity, p(offsets),
                                p(status), p(work), ws.value, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.scpose_last_error()
    torch.cuda.synchronize()
    return status.tolist(), offsets.tolist(), out.cpu().numpy(), head


def test_all_zero_tables_give_the_tables_status_to_the_image_without_bits(gpu_ops):
    nat = gpu_ops.nat
    frames = np.stack([np.full((16, 16, 3), 128, dtype=np.uint8), C.content("noise", 16, 16)])
    capacity = 2 * (1024 + 432 * 4 + 2)
    status, off, host, head = _raw_call(gpu_ops, frames, 75, "gray", np.zeros((4, 256), dtype=np.uint32), capacity)
    # mid-grey: every coefficient is zero and every code word has no bits, so the image's total is 0 bits
    assert status == [nat.JPEG_ENC_TABLES, 0]
    assert off[0] == 0 and off[1] == len(head) + 2 and off[2] > off[1] + len(head) + 2         # monotone; the noise has value bits
    assert off[2] <= capacity
    assert (host[:off[1]] == 0xA5).all()                           # nothing of the refused image is written
    assert host[off[1]:off[1] + len(head)].tobytes() == head and host[off[2] - 2:off[2]].tobytes() == b"\xff\xd9"
    assert (host[off[2]:] == 0xA5).all()


def test_tables_of_31_bit_words_give_the_tables_status_and_write_nothing(gpu_ops):
    nat = gpu_ops.nat
    frames = C.content("noise", 16, 16)[None]
    huff = np.full((4, 256), (31 << 16) | 0x5A5A, dtype=np.uint32)
    blocks = np.asarray(R.scan_blocks(frames[0], 100, "gray")[0])
    assert len(blocks) == 4 and 31 * (1 + np.count_nonzero(blocks[:, 1:])) > 4 * 1728       # the code words alone pass the bound
    capacity = 1024 + 432 * 4 + 2
    status, off, host, head = _raw_call(gpu_ops, frames, 100, "gray", huff, capacity)
    assert status == [nat.JPEG_ENC_TABLES]
    assert off == [0, len(head) + 2]
    assert (host == 0xA5).all()


def test_capacity_that_ends_exactly_on_the_second_stream(gpu_ops):
    nat = gpu_ops.nat
    jw = importlib.import_module("spacecraft-pose-estimation_amd.jpeg_write")
    frames, q, mode = E.edge_batch()
    want = [E.pil_files(n, E.edge(n))[0] for n in E.EDGE_BATCH]
    capacity = len(want[0]) + len(want[1])
    status, off, host, _ = _raw_call(gpu_ops, frames, q, mode, jw.huff_upload(), capacity)
    assert status == [0, 0, nat.JPEG_ENC_CAPACITY, nat.JPEG_ENC_CAPACITY]
    assert off == [0] + np.cumsum([len(x) for x in want]).tolist()
    assert host[:off[1]].tobytes() == want[0] and host[off[1]:off[2]].tobytes() == want[1]
    assert off[2] == capacity and (host[off[2]:] == 0xA5).all()    # neither a stream that does not fit nor the guard
