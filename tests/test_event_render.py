"""Event renderer without a GPU: the NumPy restatement and the host-side schedule against frames the reference's own
EventRenderer wrote (tests/golden/event_render_reference.npz, recorded by tests/golden/make_event_render_golden.py), the
undistortion arithmetic against a float64 bilinear evaluation, the CSV reader, and the argument checks of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import event_render_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "event_render_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def er(scpose):
    from importlib import import_module
    return import_module("spacecraft-pose-estimation_amd.event_render")


def _case(g, c):
    ev = g[c + "_events"]
    return ev, (int(g[c + "_hw"][0]), int(g[c + "_hw"][1])), int(g[c + "_fs"]), float(g[c + "_interval"])


def test_golden_holds_the_cases(golden):
    assert set(golden["cases"]) >= {"seeded", "boundary", "empty", "fractional"}
    assert list(golden["seeded_names"]) == ["1015000", "1025000", "1035000", "1045000", "1055000"]
    assert golden["seeded_frames"].shape == (5, 48, 64, 3) and set(np.unique(golden["seeded_frames"])) == {127, 191, 255}


def test_restatement_equals_reference_bit_for_bit(golden):
    for c in golden["cases"]:
        ev, hw, fs, interval = _case(golden, c)
        frames, names = R.render(ev[:, 0], ev[:, 1], ev[:, 2], ev[:, 3], hw, interval, fs, fold_polarity=True)
        assert names == list(golden[c + "_names"]), c
        assert frames.shape == golden[c + "_frames"].shape, c
        assert np.array_equal(frames, golden[c + "_frames"]), c


def test_signed_polarity_equals_reference(golden, er):
    ev = golden["signed_events"]
    hw = tuple(int(v) for v in golden["signed_hw"]); fs = int(golden["signed_fs"])
    c = R.counts(ev[:, 1], ev[:, 2], ev[:, 3], hw, fold_polarity=False)
    assert np.abs(c).max() > fs                                   # the clip is exercised
    assert np.array_equal(np.clip(c, -fs, fs), golden["signed_counts"])
    assert np.array_equal(R.gray(c, fs), golden["signed_gray"])
    assert np.array_equal(er.gray_table(fs)[np.clip(c, -fs, fs) + fs], golden["signed_gray"])
    assert list(er.gray_table(2)) == [0, 63, 127, 191, 255]


def test_frame_schedule_equals_reference(golden, er):
    """The package's schedule from three stamps == the reference's loop: names, number of frames, and the slices the start
    times select (dropped last event, boundary events in both neighbouring frames)."""
    for c in golden["cases"]:
        ev, hw, fs, interval = _case(golden, c)
        t = ev[:, 0]
        starts, names = er.frame_schedule(t[0], t[-2], t[-1], interval)
        assert names == list(golden[c + "_names"]) and len(starts) == len(names) + 1, c
        sched = R.schedule(t, interval)
        for k, (b, e, name) in enumerate(sched):
            assert b == np.searchsorted(t, starts[k], "left") and e == np.searchsorted(t, starts[k + 1], "right") and e < len(t) - 1
        assert er.frame_schedule(t[0], t[-2], t[-1], interval, max_frames=2)[1] == names[:2]
    # boundary events are counted twice: the slices of neighbouring frames overlap exactly by the events on the boundary
    ev, hw, fs, interval = _case(golden, "boundary")
    t = ev[:, 0]
    sched = R.schedule(t, interval)
    overlaps = [sched[k][1] - sched[k + 1][0] for k in range(len(sched) - 1)]
    on_boundary = [int((t == t[0] + interval * (k + 1)).sum()) for k in range(len(sched) - 1)]
    assert overlaps == on_boundary and min(on_boundary) >= 2
    # an empty frame in the middle is still written
    ev, hw, fs, interval = _case(golden, "empty")
    sched = R.schedule(ev[:, 0], interval)
    assert any(b == e for b, e, _ in sched[1:-1])
    # repeated addition is not t0 + k * interval
    ev, hw, fs, interval = _case(golden, "fraclong")
    starts, _ = er.frame_schedule(ev[0, 0], ev[-2, 0], ev[-1, 0], interval)
    assert (starts != ev[0, 0] + np.arange(len(starts)) * (1 / (1 / interval))).any()


def test_frame_schedule_rejects(er):
    with pytest.raises(ValueError):
        er.frame_schedule(0, 2 ** 53, 2 ** 53 + 5, 10000.0)
    with pytest.raises(ValueError):
        er.frame_schedule(0, 10, 20, 0.0)
    with pytest.raises(ValueError):
        er.frame_schedule(5, 3, 20, 1.0)
    assert er.frame_schedule(100, 100, 100, 10.0)[1] == []


def _speedplus_camera(h, w):
    from importlib import import_module
    syn = import_module("spacecraft-pose-estimation_amd.synthetic")
    K = syn.SPEEDPLUS_K.copy()
    K[0] *= w / 1920.0; K[1] *= h / 1200.0
    return K, syn.SPEEDPLUS_DIST.copy()


def test_undistort_identity_and_integer_map(scpose):
    rng = np.random.default_rng(0)
    img = rng.choice(np.array([127, 191, 255], np.uint8), (48, 64))
    K, _ = _speedplus_camera(48, 64)
    assert np.array_equal(R.undistort(img, K, np.zeros(5)), img)
    rgb = np.repeat(img[..., None], 3, 2)
    assert np.array_equal(R.undistort(rgb, K, np.zeros(5)), rgb)


def test_undistort_within_derived_bound_of_float64_bilinear(scpose):
    """Holds the ARITHMETIC of the undistortion (5-bit coordinate grid, 15-bit weights, final rounding), not cv2 parity:
    cv2 is unobtainable here, so cv2.undistort stays unpinned like rows a12 / f1.  Reference: float64 bilinear
    (scipy.ndimage.map_coordinates, order 1, cval 0) at the float64 map.  Per-pixel bound, derived, no pixel excluded:
    (Dx + Dy) / 64 + 4 * 255 * 2^-15 + 0.5 gray levels; Dx / Dy = the largest horizontal / vertical neighbour difference
    inside the 3 x 3 source neighbourhood of the sampled position (3 x 3 because rounding may move a position across a
    cell edge; the border counts as 0); 1/64 px is the coordinate rounding of the 1/32-px grid, the second term the rounding
    of the four weights, 0.5 the final rounding."""
    from scipy.ndimage import map_coordinates
    rng = np.random.default_rng(1)
    for h, w in ((48, 64), (120, 160)):
        K, dist = _speedplus_camera(h, w)
        img = rng.choice(np.array([127, 191, 255], np.uint8), (h, w), p=[0.9, 0.07, 0.03])
        mx, my = R.undistort_map((h, w), K, dist)
        assert np.abs(mx - np.arange(w)[None, :]).max() > 0.5                 # the map really moves pixels
        got = R.undistort(img, K, dist).astype(np.float64)
        # cval = 0 outside AND linear blending towards it at the border: pad by one pixel of zeros, sample the padded image
        pad = np.zeros((h + 4, w + 4)); pad[2:-2, 2:-2] = img
        ref = map_coordinates(pad, [np.clip(my, -2, h + 1) + 2, np.clip(mx, -2, w + 1) + 2], order=1, mode="constant", cval=0.0)
        # 3 x 3 pixels around the pixel nearest to the sampled position, in the padded image (offset 2; positions further than
        # one pixel outside the frame sample zeros on both sides and have an all-zero neighbourhood, so clipping them is exact)
        cy = np.clip(np.rint(my), -1, h).astype(np.int64) + 2; cx = np.clip(np.rint(mx), -1, w).astype(np.int64) + 2
        dxm = np.abs(np.diff(pad, axis=1)); dym = np.abs(np.diff(pad, axis=0))      # dxm[r, c] = |pad[r, c + 1] - pad[r, c]|
        Dx = np.zeros((h, w)); Dy = np.zeros((h, w))
        for o in (-1, 0, 1):                # the three rows (columns) of the neighbourhood ...
            for q in (-1, 0):               # ... and the two neighbour pairs inside each
                Dx = np.maximum(Dx, dxm[cy + o, cx + q])
                Dy = np.maximum(Dy, dym[cy + q, cx + o])
        bound = (Dx + Dy) / 64.0 + 4 * 255 * 2.0 ** -15 + 0.5
        err = np.abs(got - ref)
        print("undistort %dx%d: max err %.4f, max err/bound %.4f" % (h, w, err.max(), (err / bound).max()))
        assert (err <= bound).all()


def test_read_events_csv(tmp_path, er):
    rows = [(1000500, 3, 7, 1), (2000999, 10, 2, 0), (3999999, 5, 5, 1)]
    comma = tmp_path / "a.csv"
    comma.write_text("# t,x,y,p\n" + "".join("%d,%d,%d,%d\n" % r for r in rows))
    space = tmp_path / "b.csv"
    space.write_text("".join("%d %d  %d %d\n" % r for r in rows))
    for path, ws in ((comma, False), (space, True)):
        t, x, y, p = er.read_events_csv(str(path), delim_whitespace=ws)
        assert all(a.dtype == np.int64 for a in (t, x, y, p))
        assert t.tolist() == [1000500, 2000999, 3999999] and x.tolist() == [3, 10, 5] and y.tolist() == [7, 2, 5] and p.tolist() == [1, 0, 1]
    t, x, y, p = er.read_events_csv(str(comma), swap_xy=True)
    assert x.tolist() == [7, 2, 5] and y.tolist() == [3, 10, 5]
    assert er.read_events_csv(str(comma), microseconds_timestamp=True)[0].tolist() == [1, 2, 3]          # truncated, not rounded
    assert er.read_events_csv(str(comma), milliseconds_timestamp=True)[0].tolist() == [1000, 2000, 3999]
    frac = tmp_path / "c.csv"
    frac.write_text("10.9,1,2,1\n20.2,3,4,0\n")
    assert er.read_events_csv(str(frac))[0].tolist() == [10, 20]


def test_abi_events_without_a_device(scpose):
    from importlib import import_module
    nat = import_module("spacecraft-pose-estimation_amd._native")
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.lib()
    for name in ("scpose_events_frame_bounds", "scpose_events_render", "scpose_events_workspace_bytes"):
        assert hasattr(lib, name) and name in nat.SYMBOLS
    assert lib.scpose_abi_version() == 7
    ws = ctypes.c_size_t()
    assert lib.scpose_events_workspace_bytes(256, 480, 640, ctypes.byref(ws)) == 0 and ws.value == 256 * 480 * 640
    assert lib.scpose_events_workspace_bytes(1, 480, 50000, ctypes.byref(ws)) == -1 and b"not supported" in lib.scpose_last_error()
    assert lib.scpose_events_workspace_bytes(1, 480, 640, None) == -1
    # empty cases: no-ops, pointers may be null
    assert lib.scpose_events_frame_bounds(None, 0, None, 0, None, None) == 0
    assert lib.scpose_events_frame_bounds(None, 100, None, 0, None, None) == 0
    assert lib.scpose_events_render(None, None, None, 0, None, 0, 480, 640, 2, 1, None, None, None, None, None, None, 0, None) == 0
    # argument errors
    assert lib.scpose_events_frame_bounds(None, 100, None, 4, None, None) == -1 and b"null" in lib.scpose_last_error()
    assert lib.scpose_events_render(None, None, None, 0, None, 4, 480, 640, 2, 1, None, None, None, None, None, None, 0, None) == -1
    assert b"null" in lib.scpose_last_error()
    assert lib.scpose_events_render(None, None, None, 0, None, 0, 480, 640, 0, 1, None, None, None, None, None, None, 0, None) == -1
    assert b"full_scale" in lib.scpose_last_error()
    assert lib.scpose_events_render(None, None, None, 0, None, 4, 8192, 8192, 2, 1, None, None, None, None, None, None, 0, None) == -1
    assert b"not supported" in lib.scpose_last_error()
    assert lib.scpose_events_render(None, None, None, 3, None, 0, 480, 640, 2, 0, None, None, None, None, None, None, 0, None) == -1
    assert b"p_itemsize" in lib.scpose_last_error()
    one = ctypes.c_double(1.0)
    assert lib.scpose_events_render(None, None, None, 0, None, 0, 480, 640, 2, 1, None, ctypes.byref(one), None, None, None, None, 0, None) == -1
    assert b"together" in lib.scpose_last_error()
