#!/usr/bin/env python3
"""Generates tests/golden/event_render_reference.npz by IMPORTING THE REFERENCE's event renderer in the build container
(it never ships; the reference tree does not exist where the GPU tests run).

v2e/v2ecore/renderer.py is imported as-is under stand-ins for what the image lacks: `numba.jit / njit` become identity
decorators, `cv2.cvtColor(gray, COLOR_GRAY2BGR)` a 3-channel repeat, `cv2.imwrite` a recorder of (file name, array);
tkinter, engineering_notation, tqdm and v2ecore.emulator (torch / h5py side of the DVS emulator, unused by the renderer)
are empty stand-ins.  Each case feeds a seeded stream to
    EventRenderer(full_scale_count=fs, exposure_mode=DURATION, exposure_value=interval, output_path=..., dvs_vid='x.avi')
        .render_events_to_frames(events, height, width, output_to_images=True)
exactly as v2e/e2v.py does (int64 [t, x, y, p] rows) and records the frames and names it "wrote".  The signed-polarity
case calls the renderer's accumulate_event_frame on one frame's events with polarities -1 / +1 and applies its gray
formula, because render_events_to_frames itself overwrites the polarity column with 1.

Only data is written (arrays and strings): no reference source text.  Re-run: python tests/golden/make_event_render_golden.py
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SCPOSE_REFERENCE_V2E", "/root/reference/v2e")
OUT = os.path.join(HERE, "event_render_reference.npz")


def _install_stand_ins(recorder):
    def _decorator(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda fn: fn
    numba = types.ModuleType("numba"); numba.jit = _decorator; numba.njit = _decorator
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_GRAY2BGR = 8
    cv2.cvtColor = lambda img, code: np.repeat(np.asarray(img)[..., None], 3, axis=2)
    cv2.imwrite = lambda path, img: recorder.append((os.path.basename(path), np.array(img))) or True
    cv2.destroyAllWindows = lambda: None
    tk = types.ModuleType("tkinter"); fd = types.ModuleType("tkinter.filedialog"); tk.filedialog = fd
    eng = types.ModuleType("engineering_notation"); eng.EngNumber = lambda v, *a, **k: v
    tqdm = types.ModuleType("tqdm"); tqdm.tqdm = lambda it, *a, **k: it
    emu = types.ModuleType("v2ecore.emulator"); emu.EventEmulator = type("EventEmulator", (), {})
    for name, mod in (("numba", numba), ("cv2", cv2), ("tkinter", tk), ("tkinter.filedialog", fd),
                      ("engineering_notation", eng), ("tqdm", tqdm), ("v2ecore.emulator", emu)):
        sys.modules[name] = mod


def main():
    written = []
    _install_stand_ins(written)
    sys.path.insert(0, REF)
    from v2ecore import renderer as R

    class _Video:                       # the renderer writes every frame to its AVI writer first; nothing is kept of it
        def write(self, frame): pass
        def release(self): pass
    R.video_writer = lambda *a, **k: _Video()

    def reference_frames(ev, h, w, fs, interval):
        del written[:]
        with tempfile.TemporaryDirectory() as tmp:
            r = R.EventRenderer(full_scale_count=fs, output_path=tmp, dvs_vid="x.avi", preview=False,
                                exposure_mode=R.ExposureMode.DURATION, exposure_value=interval)
            r.render_events_to_frames(ev.copy(), height=h, width=w, output_to_images=True)
            r.cleanup()
        names = [n[:-4] for n, _ in written]
        frames = np.stack([f for _, f in written]) if written else np.zeros((0, h, w, 3), np.uint8)
        assert frames.dtype == np.uint8 and frames.shape[1:] == (h, w, 3)
        return frames, names

    out = {}
    cases = []

    def stream(seed, n, t0, span, h, w, margin=6):
        rng = np.random.default_rng(seed)
        t = np.sort(rng.integers(t0, t0 + span, n)); t[0] = t0
        x = rng.integers(-margin, w + margin, n); y = rng.integers(-margin, h + margin, n)
        p = rng.integers(0, 2, n)
        return np.stack([t, x, y, p], 1).astype(np.int64)

    def add(name, ev, h, w, fs, interval):
        frames, names = reference_frames(ev, h, w, fs, interval)
        out[name + "_events"] = ev
        out[name + "_hw"] = np.array([h, w], np.int64)
        out[name + "_fs"] = np.int64(fs)
        out[name + "_interval"] = np.float64(interval)
        out[name + "_frames"] = frames
        out[name + "_names"] = np.array(names, dtype="U32")
        cases.append(name)
        print("%-10s %6d events -> %d frames %s values %s" % (name, len(ev), len(names), names[:2], np.unique(frames)))

    # (a) the seeded stream: 20 000 events, t0 = 1 000 000, 55 000 ticks, coordinates partly outside 64 x 48
    add("seeded", stream(0, 20000, 1000000, 55000, 48, 64), 48, 64, 2, 10000.0)
    # (b) several events exactly on frame boundaries (t0 + k * 10000): counted in both neighbouring frames
    ev = stream(1, 6000, 500000, 45000, 40, 56)
    for k, idx in enumerate(range(100, 5900, 290)):
        ev[idx, 0] = 500000 + 10000 * (1 + k % 4)
    ev = ev[np.argsort(ev[:, 0], kind="stable")]
    add("boundary", ev, 40, 56, 2, 10000.0)
    # (c) an empty frame in the middle: no event in [t0 + 20000, t0 + 30000]
    ev = stream(2, 5000, 200000, 52000, 32, 48)
    ev = ev[(ev[:, 0] < 219990) | (ev[:, 0] > 230010)]
    add("empty", ev, 32, 48, 2, 10000.0)
    # (d) int64 stamps with a non-integer interval: repeated addition differs from t0 + k * interval
    add("fractional", stream(3, 8000, 123456789, 60000, 48, 64), 48, 64, 2, 2500.3)
    # a long run of the same, so that the accumulated rounding shows up in the names / boundaries
    add("fraclong", stream(4, 4000, 987654321, 700000, 16, 24), 16, 24, 2, 1000.1)
    out["cases"] = np.array(cases, dtype="U16")

    # (e) signed polarity, full_scale_count = 3: accumulate_event_frame on one frame's events with polarities -1 / +1
    rng = np.random.default_rng(5)
    n, h, w, fs = 3000, 24, 32, 3
    ev = np.stack([np.sort(rng.integers(0, 10000, n)), rng.integers(-3, w + 3, n), rng.integers(-3, h + 3, n),
                   rng.choice([-1, 1], n)], 1).astype(np.int64)
    ev[:400, 1:3] = [5, 7]; ev[:400, 3] = np.where(np.arange(400) % 3 == 0, -1, 1)       # a hot pixel of both polarities
    r = R.EventRenderer(full_scale_count=fs, exposure_mode=R.ExposureMode.DURATION, exposure_value=10000.0)
    r.width, r.height = w, h
    r.accumulate_event_frame(ev, np.asarray([(0, v) for v in (h, w)], dtype=np.int64))
    img = (r.currentFrame + r.full_scale_count) / float(r.full_scale_count * 2)          # normalize_frame's formula
    out["signed_events"] = ev
    out["signed_hw"] = np.array([h, w], np.int64)
    out["signed_fs"] = np.int64(fs)
    out["signed_counts"] = r.currentFrame.astype(np.int64)
    out["signed_gray"] = (img * 255).astype(np.uint8)
    print("signed     counts %s gray %s" % (np.unique(out["signed_counts"]), np.unique(out["signed_gray"])))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
