"""COUNT and AREA_COUNT exposure of the event renderer, without a device: the restatement against the reference's recorded
frames, stems and frame-times files; the suffix-minimum form against the serial loop; --dvs_exposure parsing and the
rejections of the host layer and of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import event_exposure_restated as X
import event_render_restated as ER

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "event_exposure_reference.npz")
EMPTY_CASES = {"count_all", "area_none", "area_n1", "area_n2", "count_n2"}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def er(scpose):
    from importlib import import_module
    return import_module("spacecraft-pose-estimation_amd.event_render")


def restated_case(g, c):
    """(frames (F, H, W), stems, frame-times text) of fixture case c from the serial restatement."""
    ev = g[c + "_events"]; hw = (int(g[c + "_hw"][0]), int(g[c + "_hw"][1])); fs = int(g[c + "_fs"])
    tok = [str(s) for s in g[c + "_exposure"]]
    t, x, y = ev[:, 0], ev[:, 1], ev[:, 2]
    mode = tok[0].lower()
    if mode == "duration":
        frames, names = ER.render(t, x, y, None, hw, interval=float(tok[1]), fs=fs)
        return frames[..., 0], names, X.frame_times_text(str(g["dvs_vid"]), X.duration_times(t, float(tok[1])))
    if mode == "count":
        bounds = X.serial_count_bounds(len(t), int(float(tok[1])))
    else:
        bounds = X.serial_area_bounds(x, y, hw, int(tok[1]), int(tok[2]))
    frames, stems, times = X.render_bounds(t, x, y, bounds, hw, fs)
    return frames, stems, X.frame_times_text(str(g["dvs_vid"]), times)


def test_serial_restatement_equals_reference(golden):
    for c in golden["cases"]:
        frames, stems, text = restated_case(golden, str(c))
        assert stems == list(golden[c + "_names"]), c
        assert np.array_equal(frames, golden[c + "_frames"]), c
        assert text == str(golden[c + "_frame_times"]), c


def test_fixture_guards(golden):
    """The M = 2 case has stem collisions (the later file wins); every case not meant to be empty writes frames."""
    names = list(golden["area_collide_names"])
    assert len(set(names)) < len(names)
    for c in golden["cases"]:
        assert (len(golden[c + "_names"]) == 0) == (str(c) in EMPTY_CASES), c


def _seeded(seed, n, hw, D, margin_areas=1, hot=0.0):
    rng = np.random.default_rng(seed)
    nw, nh = X.area_grid(hw, D)
    x = rng.integers(-margin_areas * D, nw * D, n); y = rng.integers(-margin_areas * D, nh * D, n)
    if hot:
        sel = rng.random(n) < hot
        x[sel] = rng.integers(0, 4, sel.sum()); y[sel] = 3
    return x, y


@pytest.mark.parametrize("seed,n,hw,M,D,hot", [
    (0, 20000, (48, 64), 2, 8, 0.0), (1, 20000, (48, 64), 40, 16, 0.0), (2, 30000, (24, 32), 7, 7, 0.1),
    (3, 8000, (12, 16), 3, 1, 0.0), (4, 8000, (12, 16), 2, 1, 0.3), (5, 50000, (48, 64), 300, 32, 0.1),
    (6, 5000, (20, 20), 5000, 4, 0.0), (7, 3, (8, 8), 2, 8, 0.0)])
def test_suffix_min_equals_serial(seed, n, hw, M, D, hot):
    x, y = _seeded(seed, n, hw, D, hot=hot)
    serial = X.serial_area_bounds(x, y, hw, M, D)
    assert X.area_bounds_suffix_min(x, y, hw, M, D) == serial
    if M < 100 and n > 100:
        assert len(serial) > 0


def test_count_bounds():
    assert X.serial_count_bounds(10, 3) == [(0, 3), (3, 6)]          # 9 < n - 1 = 9 fails: the third frame is not written
    assert X.serial_count_bounds(11, 3) == [(0, 3), (3, 6), (6, 9)]
    assert X.serial_count_bounds(1, 1) == [] and X.serial_count_bounds(2, 1) == []
    for n, N in ((10, 3), (11, 3), (5000, 137), (2, 1), (3, 1), (0, 4)):
        assert len(X.serial_count_bounds(n, N)) == (max(n - 2, 0) // N)


def test_parse_dvs_exposure(er):
    assert er.parse_dvs_exposure(["duration", "0.01"]) == ("duration", 0.01, None)
    assert er.parse_dvs_exposure(["DURATION", "10000"]) == ("duration", 10000.0, None)
    assert er.parse_dvs_exposure(["Count", "137.7"]) == ("count", 137.7, None)
    assert er.parse_dvs_exposure(["area_COUNT", "500", "64"]) == ("area_count", 500, 64)
    for bad in ([], ["frames", "3"], ["duration"], ["duration", "1", "2"], ["count", "5", "5"], ["area_count", "500"],
                ["area_count", "500", "64", "1"], ["area_count", "500.5", "64"], ["area_count", "500", "6.4"],
                ["count", "many"]):
        with pytest.raises(ValueError):
            er.parse_dvs_exposure(bad)
    assert er.exposure_kwargs(*er.parse_dvs_exposure(["count", "137.7"])) == {"exposure": "count", "event_count": 137}
    assert er.exposure_kwargs(*er.parse_dvs_exposure(["area_count", "40", "16"])) == {
        "exposure": "area_count", "area_count": 40, "area_dimension": 16}
    assert er.exposure_kwargs(*er.parse_dvs_exposure(["duration", "2500.3"])) == {"exposure": "duration", "interval": 2500.3}
    for bad in (["count", "0.9"], ["count", "0"], ["count", "-3"], ["area_count", "1", "8"], ["area_count", "0", "8"],
                ["area_count", "5", "0"], ["area_count", "5", "-2"]):
        with pytest.raises(ValueError):
            er.exposure_kwargs(*er.parse_dvs_exposure(bad))


def test_frame_times_file_contract(er):
    assert er.frame_times_path("/o", "dvs-video.avi") == os.path.join("/o", "dvs-video-frame_times.txt")
    assert er.frame_times_path("o", "x-frame_times.txt") == os.path.join("o", "x-frame_times.txt")
    assert er.frame_times_text("v.avi", [np.float64(12.5), 3.0]) == X.frame_times_text("v.avi", [12.5, 3.0])


def test_restatement_rejects(golden):
    with pytest.raises(ValueError):
        X.serial_count_bounds(100, 0)
    for M, D in ((1, 8), (0, 8), (2, 0)):
        with pytest.raises(ValueError):
            X.serial_area_bounds(np.zeros(10, np.int64), np.zeros(10, np.int64), (16, 24), M, D)
        with pytest.raises(ValueError):
            X.area_bounds_suffix_min(np.zeros(10, np.int64), np.zeros(10, np.int64), (16, 24), M, D)
    # 16 x 24, D = 8: nw = 4, nh = 3 -> x in [-32, 32), y in [-24, 24)
    for bx, by in ((32, 0), (-33, 0), (0, 24), (0, -25)):
        x = np.zeros(50, np.int64); y = np.zeros(50, np.int64); x[20] = bx; y[20] = by
        with pytest.raises(IndexError):
            X.serial_area_bounds(x, y, (16, 24), 2, 8)
        with pytest.raises(IndexError):
            X.area_bounds_suffix_min(x, y, (16, 24), 2, 8)
    x = np.zeros(50, np.int64); x[20] = 31; x[21] = -32
    y = np.zeros(50, np.int64); y[22] = 23; y[23] = -24
    X.serial_area_bounds(x, y, (16, 24), 2, 8)                        # the edges of the grid are valid


def test_abi_rejects_without_a_device(scpose):
    from importlib import import_module
    nat = import_module("spacecraft-pose-estimation_amd._native")
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.lib()
    ws = ctypes.c_size_t(); f = ctypes.c_int64()
    assert lib.scpose_events_count_frames(10, 3, ctypes.byref(f)) == 0 and f.value == 2
    assert lib.scpose_events_count_frames(1, 3, ctypes.byref(f)) == 0 and f.value == 0
    assert lib.scpose_events_count_frames(10, 0, ctypes.byref(f)) == -1 and b"count" in lib.scpose_last_error()
    assert lib.scpose_events_count_bounds(10, 0, 0, None, None) == -1
    assert lib.scpose_events_count_bounds(10, 3, 3, None, None) == -1                    # only 2 frames
    assert lib.scpose_events_count_bounds(10, 3, 0, None, None) == 0
    assert lib.scpose_events_area_bounds_workspace_bytes(1000, 40, 16, 48, 64, ctypes.byref(ws)) == 0 and ws.value > 0
    assert lib.scpose_events_area_bounds_workspace_bytes(1000, 1, 16, 48, 64, ctypes.byref(ws)) == -1
    assert b"area_count" in lib.scpose_last_error()
    assert lib.scpose_events_area_bounds_workspace_bytes(1000, 2, 0, 48, 64, ctypes.byref(ws)) == -1
    assert b"area_dimension" in lib.scpose_last_error()
    assert lib.scpose_events_area_bounds_workspace_bytes(2 ** 31, 2, 8, 48, 64, ctypes.byref(ws)) == -1
    assert lib.scpose_events_area_bounds_workspace_bytes(2 ** 31 - 1, 2, 8, 48, 64, ctypes.byref(ws)) == 0
    assert lib.scpose_events_area_bounds_workspace_bytes(1000, 2, 8, 0, 64, ctypes.byref(ws)) == -1
    for M, D in ((1, 8), (2, 0)):
        assert lib.scpose_events_area_bounds(None, None, 1000, M, D, 48, 64, None, 10000, None, None, 0, None) == -1
    assert lib.scpose_events_area_bounds(None, None, 2 ** 31, 2, 8, 48, 64, None, 2 ** 31, None, None, 0, None) == -1
    assert lib.scpose_events_area_bounds(None, None, 1000, 2, 8, 48, 64, None, 997, None, None, 0, None) == -1
    assert b"capacity" in lib.scpose_last_error()
    assert lib.scpose_events_bounds_midpoints(None, None, 0, None, None) == 0
    assert lib.scpose_events_bounds_midpoints(None, None, 3, None, None) == -1
