"""The workspace and state sizes the event entry points report, against numbers recorded from the library of commit 6801876
(before the four hand-written layouts became one carving function each): a layout that moves shows up here, without a GPU.
The numbers are data, not a formula: (arguments, bytes)."""
import ctypes
import os

import pytest

RECORDED = {
    "scpose_events_area_bounds_workspace_bytes": (          # n_events, area_count, area_dimension, h, w
        ((0, 2, 8, 480, 640), 512), ((1, 2, 8, 480, 640), 2816), ((2, 2, 8, 480, 640), 2816), ((4096, 3, 1, 24, 40), 263680),
        ((4097, 100, 16, 720, 1280), 184064), ((1000, 50, 640, 480, 640), 41984), ((3000000, 1000, 8, 480, 640), 204753920),
        ((200000000, 2, 4, 1080, 1920), 26450196480), ((2000000000, 1000000, 8, 480, 640), 104501954304)),
    "scpose_events_csv_workspace_bytes": (                  # n_bytes
        ((0,), 768), ((1,), 768), ((4096,), 768), ((4097,), 768), ((262144,), 1024), ((50000000,), 146944),
        ((6000000000,), 17578752)),
    "scpose_events_text_workspace_bytes": (                 # n rows
        ((0,), 256), ((1,), 768), ((256,), 768), ((257,), 768), ((65536,), 3328), ((65836,), 3840), ((3000000,), 141312),
        ((5000000000,), 234375424)),
    "scpose_dvs_workspace_bytes": (                         # h, w, n_frames, max_iters
        ((5, 37, 0, 1024), 25344), ((5, 37, 1, 1024), 25344), ((24, 40, 6, 1024), 123648), ((16, 16, 2, 1024), 33536),
        ((64, 64, 63, 32), 17408), ((240, 256, 2, 1024), 7866880), ((720, 1280, 63, 1024), 117994496),
        ((1080, 1920, 500, 256), 66377728), ((1, 1, 1, 4096), 33536)),
    "scpose_dvs_state_bytes": (                             # h, w: the state is visible through DvsEmulator.state()
        ((1, 1), 1792), ((5, 37), 4864), ((8, 8), 1792), ((24, 40), 23296), ((240, 256), 1474816), ((720, 1280), 22118656)),
}


@pytest.fixture(scope="module")
def nat(scpose):
    from importlib import import_module
    n = import_module("spacecraft-pose-estimation_amd._native")
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return n


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_sizes_equal_the_recorded_ones(nat, name):
    fn = getattr(nat.lib(), name)
    b = ctypes.c_size_t()
    for args, expected in RECORDED[name]:
        assert fn(*args, ctypes.byref(b)) == 0, (name, args)
        assert b.value == expected, "%s%r: %d bytes, recorded %d" % (name, args, b.value, expected)
