"""The built library exports the event writers' entry points, and reports their argument errors before anything is launched
(no device, no compute calls here)."""
import ctypes
import os

import pytest

NAMES = ("scpose_events_text_tiling", "scpose_events_text_workspace_bytes", "scpose_events_text_measure", "scpose_events_text_emit",
         "scpose_events_aedat2_pack")


@pytest.fixture(scope="module")
def nat(scpose):
    from importlib import import_module
    n = import_module("spacecraft-pose-estimation_amd._native")
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return n


def test_library_exports_the_writer_symbols(nat):
    handle = ctypes.CDLL(nat.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), name
        assert name in nat.SYMBOLS
    assert nat.lib().scpose_abi_version() == 7            # additive: the number does not move
    assert (nat.TEXT_CAPACITY, nat.AEDAT2_RANGE, nat.AEDAT2_TIME) == (1, 1, 2)


def test_wrappers_exist(nat):
    from importlib import import_module
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    ew = import_module("spacecraft-pose-estimation_amd.event_write")
    assert callable(ops.format_events_text) and callable(ops.pack_events_aedat2)
    assert callable(ew.write_events_text) and callable(ew.write_events_aedat2)
    tile, scan = ops.events_text_tiling()
    assert tile >= 64 and scan % tile == 0 and scan <= 1 << 19


def test_argument_errors_without_a_device(nat):
    lib = nat.lib()
    err = lambda: lib.scpose_last_error()
    b = ctypes.c_size_t()
    assert lib.scpose_events_text_workspace_bytes(0, ctypes.byref(b)) == 0 and b.value >= 8
    small = b.value
    assert lib.scpose_events_text_workspace_bytes(100000, ctypes.byref(b)) == 0 and b.value > small
    need = b.value
    assert lib.scpose_events_text_workspace_bytes(-1, ctypes.byref(b)) == -1 and b"n=-1" in err()
    assert lib.scpose_events_text_workspace_bytes(5, None) == -1 and b"null" in err()
    assert lib.scpose_events_text_tiling(None, None) == -1 and b"null" in err()

    # 16-byte aligned stand-ins for device pointers: every call below fails before it would touch them
    P = 4096
    # measure
    assert lib.scpose_events_text_measure(P, P, P, P, -1, P, P, need, None) == -1 and b"n=-1" in err()
    assert lib.scpose_events_text_measure(None, P, P, P, 100000, P, P, need, None) == -1 and b"null" in err()
    assert lib.scpose_events_text_measure(P, P, P, None, 100000, P, P, need, None) == -1 and b"null" in err()
    assert lib.scpose_events_text_measure(P, P, P, P, 100000, None, P, need, None) == -1 and b"null" in err()
    assert lib.scpose_events_text_measure(P, P, P, P, 100000, P, P, need - 1, None) == -1 and b"workspace" in err()
    assert lib.scpose_events_text_measure(P, P, P, P, 100000, P, None, need, None) == -1 and b"workspace" in err()
    # emit
    for sep in (0, ord("\t"), ord(";"), ord("\n"), 256 + ord(",")):
        assert lib.scpose_events_text_emit(P, P, P, P, 100000, sep, 0, P, 1 << 20, P, P, need, None) == -1 and b"separator" in err(), sep
    assert lib.scpose_events_text_emit(P, P, P, P, -5, ord(" "), 0, P, 1 << 20, P, P, need, None) == -1 and b"n=-5" in err()
    assert lib.scpose_events_text_emit(P, None, P, P, 100000, ord(","), 0, P, 1 << 20, P, P, need, None) == -1 and b"null" in err()
    assert lib.scpose_events_text_emit(P, P, P, P, 100000, ord(","), 0, None, 1 << 20, P, P, need, None) == -1 and b"null" in err()
    assert lib.scpose_events_text_emit(P, P, P, P, 100000, ord(","), 0, P, -1, P, P, need, None) == -1 and b"capacity" in err()
    assert lib.scpose_events_text_emit(P, P, P, P, 100000, ord(","), 1, P, 1 << 20, P, P, small, None) == -1 and b"workspace" in err()
    assert lib.scpose_events_text_emit(P, P, P, P, 100000, ord(","), 1, P + 8, 1 << 20, P, P, need, None) == -1 and b"aligned" in err()
    # pack
    # h 1 .. 1024; w up to 1280, the widest of the reference's sizes (1 .. 1024 would refuse its own 1280 x 720)
    for h, w in ((0, 640), (480, 0), (1025, 640), (480, 1281), (-1, 5), (1280, 720)):
        assert lib.scpose_events_aedat2_pack(P, P, P, P, 10, h, w, P, P, None) == -1 and b"not supported" in err(), (h, w)
    assert lib.scpose_events_aedat2_pack(P, P, P, P, -1, 480, 640, P, P, None) == -1 and b"n=-1" in err()
    assert lib.scpose_events_aedat2_pack(P, P, None, P, 10, 480, 640, P, P, None) == -1 and b"null" in err()
    assert lib.scpose_events_aedat2_pack(P, P, P, P, 10, 480, 640, None, P, None) == -1 and b"null" in err()
    assert lib.scpose_events_aedat2_pack(P, P, P, P, 10, 480, 640, P, None, None) == -1 and b"null" in err()
    assert lib.scpose_events_aedat2_pack(None, None, None, None, 0, 480, 640, None, None, None) == -1 and b"null" in err()
