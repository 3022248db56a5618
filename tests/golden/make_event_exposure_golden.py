#!/usr/bin/env python3
"""Generates tests/golden/event_exposure_reference.npz by IMPORTING THE REFERENCE's event renderer in the build container
(it never ships; the reference tree does not exist where the GPU tests run).

Same stand-ins as make_event_render_golden.py (numba.jit -> identity, cv2.cvtColor -> 3-channel repeat, cv2.imwrite -> a
recorder of (file name, array), empty tkinter / engineering_notation / tqdm / v2ecore.emulator).  Every case runs what
v2e/e2v.py runs for its --dvs_exposure tokens:
    mode, value, dim = v2e_check_dvs_exposure_args(args)                 (v2ecore/v2e_args.py)
    EventRenderer(output_path=tmp, dvs_vid='dvs-video.avi', preview=False, full_scale_count=fs, exposure_mode=mode,
                  exposure_value=value, area_dimension=dim, avi_frame_rate=30)
        .render_events_to_frames(events, height=h, width=w, output_to_images=True)
and records, in write order, every frame and file name the renderer "wrote", plus its frame-times file (read after cleanup(),
before the temporary directory goes).  The three channels of every frame are asserted equal and one is stored.

Only data is written (arrays and strings): no reference source text.  Re-run: python tests/golden/make_event_exposure_golden.py
"""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_event_render_golden import REF, _install_stand_ins  # noqa: E402

OUT = os.path.join(HERE, "event_exposure_reference.npz")
DVS_VID = "dvs-video.avi"


def main():
    written = []
    _install_stand_ins(written)
    sys.path.insert(0, REF)
    from v2ecore import renderer as R
    from v2ecore.v2e_args import v2e_check_dvs_exposure_args

    class _Video:
        def write(self, frame): pass
        def release(self): pass
    R.video_writer = lambda *a, **k: _Video()

    def reference(ev, h, w, fs, tokens):
        del written[:]
        mode, value, dim = v2e_check_dvs_exposure_args(argparse.Namespace(dvs_exposure=list(tokens)))
        with tempfile.TemporaryDirectory() as tmp:
            r = R.EventRenderer(output_path=tmp, dvs_vid=DVS_VID, preview=False, full_scale_count=fs, exposure_mode=mode,
                                exposure_value=value, area_dimension=dim, avi_frame_rate=30)
            r.render_events_to_frames(ev.copy(), height=h, width=w, output_to_images=True)
            r.cleanup()
            with open(os.path.join(tmp, "dvs-video-frame_times.txt")) as f:
                times = f.read()
        names = [n[:-4] for n, _ in written]
        frames = np.stack([f for _, f in written]) if written else np.zeros((0, h, w, 3), np.uint8)
        assert frames.dtype == np.uint8 and frames.shape[1:] == (h, w, 3)
        assert (frames[..., 0] == frames[..., 1]).all() and (frames[..., 0] == frames[..., 2]).all()
        return frames[..., 0].copy(), names, times

    out, cases = {}, []

    def stream(seed, n, t0, span, x_range, y_range):
        rng = np.random.default_rng(seed)
        t = np.sort(rng.integers(t0, t0 + span, n)); t[0] = t0
        x = rng.integers(x_range[0], x_range[1], n); y = rng.integers(y_range[0], y_range[1], n)
        p = rng.integers(0, 2, n)
        return np.stack([t, x, y, p], 1).astype(np.int64)

    def add(name, ev, h, w, tokens, fs=2, empty=False):
        frames, names, times = reference(ev, h, w, fs, tokens)
        assert (len(names) == 0) == empty, (name, len(names))
        out[name + "_events"] = ev
        out[name + "_hw"] = np.array([h, w], np.int64)
        out[name + "_fs"] = np.int64(fs)
        out[name + "_exposure"] = np.array(tokens, dtype="U16")
        out[name + "_frames"] = frames
        out[name + "_names"] = np.array(names, dtype="U32")
        out[name + "_frame_times"] = np.array(times)
        cases.append(name)
        print("%-14s %-28s %6d events -> %5d frames, %5d distinct stems %s" % (
            name, " ".join(tokens), len(ev), len(names), len(set(names)), names[:2]))
        return names

    # COUNT
    add("count_frac", stream(10, 3000, 1000000, 40000, (-4, 44), (-4, 36)), 32, 40, ["count", "137.7"])
    add("count_one", stream(11, 300, 5000, 3000, (0, 24), (0, 16)), 16, 24, ["COUNT", "1"])
    add("count_all", stream(12, 500, 0, 9000, (0, 24), (0, 16)), 16, 24, ["count", "499"], empty=True)
    # AREA_COUNT: D divides W and H (events in [W, nw * D) count toward their area, are not drawn)
    add("area_div", stream(13, 8000, 2000000, 80000, (0, 70), (0, 52)), 48, 64, ["area_count", "40", "16"])
    # D divides neither H nor W
    add("area_nodiv", stream(14, 6000, 300000, 50000, (0, 56), (0, 40)), 40, 50, ["area_count", "7", "7"])
    # the right / bottom strip [W, nw * D) x [H, nh * D) only: 30 x 50, D = 16 -> areas up to x 63, y 31
    ev = stream(15, 5000, 0, 60000, (0, 64), (0, 32))
    add("area_edge", ev, 30, 50, ["Area_Count", "40", "16"])
    # negative coordinates: numpy's wraparound, x in [-nw * D, 0), y in [-nh * D, 0)
    add("area_negative", stream(16, 6000, 7000000, 30000, (-56, 48), (-40, 32)), 32, 48, ["area_count", "12", "8"])
    # a hot pixel: 10 % of the events on (17, 9)
    ev = stream(17, 20000, 100000, 200000, (-3, 67), (-3, 51))
    hot = np.random.default_rng(18).random(len(ev)) < 0.1
    ev[hot, 1] = 17; ev[hot, 2] = 9
    add("area_hot", ev, 48, 64, ["area_count", "300", "32"])
    # M = 2 with stem collisions: dense stamps (several events per tick)
    names = add("area_collide", stream(19, 6000, 400000, 2000, (0, 24), (0, 16)), 16, 24, ["area_count", "2", "8"])
    assert len(set(names)) < len(names), "no stem collision"
    # no area ever reaches M: 2000 events over 63 areas, M = 100
    add("area_none", stream(20, 2000, 0, 20000, (0, 64), (0, 48)), 48, 64, ["area_count", "100", "8"], empty=True)
    add("area_n1", stream(21, 1, 50, 1, (0, 24), (0, 16)), 16, 24, ["area_count", "2", "8"], empty=True)
    ev = stream(22, 2, 50, 10, (0, 8), (0, 8)); ev[:, 1:3] = [3, 4]
    add("area_n2", ev, 16, 24, ["area_count", "2", "8"], empty=True)
    add("count_n2", stream(23, 2, 50, 10, (0, 24), (0, 16)), 16, 24, ["count", "1"], empty=True)
    # one DURATION case through the same CLI path, for the frame-times text
    add("duration_cli", stream(24, 5000, 123456, 26000, (-3, 51), (-3, 35)), 32, 48, ["duration", "2500.3"])
    out["cases"] = np.array(cases, dtype="U16")
    out["dvs_vid"] = np.array(DVS_VID)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
