#!/usr/bin/env python3
"""Generates tests/golden/dvs_emulator_reference.npz by IMPORTING THE REFERENCE's DVS emulator (it never ships; the reference
tree does not exist where the GPU tests run).

v2e/v2ecore/emulator.py is imported as-is with device="cpu", under empty stand-ins for what it imports without using here:
cv2, h5py, v2ecore.v2e_utils (checkAddSuffix) and the two output writers.  Every case of tests/dvs_emulator_restated.py:
make_cases (40 x 24 and 37 x 5) is fed frame by frame to EventEmulator.generate_events with sigma_thres = 0,
shot_noise_rate_hz = 0 and leak_jitter_fraction = 0; after the first frame the per-pixel thresholds and the noise-rate array of
the case replace the ones _init made (these are inputs of the device emulator, not drawn inside it).  Stored per case: the
inputs, the parameters, the returned rows with every equal-stamp group sorted by (polarity, y, x) -- the reference shuffles
them -- the number of rows per frame, and the state after the last frame.

Only data is written: no reference source text.  Re-run: python tests/golden/make_dvs_emulator_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SCPOSE_REFERENCE_V2E", "/root/reference/v2e")
OUT = os.path.join(HERE, "dvs_emulator_reference.npz")
sys.path.insert(0, os.path.dirname(HERE))


def _install_stand_ins():
    cv2 = types.ModuleType("cv2")
    h5py = types.ModuleType("h5py")
    utils = types.ModuleType("v2ecore.v2e_utils"); utils.checkAddSuffix = lambda path, suffix: path
    out = types.ModuleType("v2ecore.output")
    a2 = types.ModuleType("v2ecore.output.aedat2_output"); a2.AEDat2Output = type("AEDat2Output", (), {})
    tx = types.ModuleType("v2ecore.output.ae_text_output"); tx.DVSTextOutput = type("DVSTextOutput", (), {})
    for name, mod in (("cv2", cv2), ("h5py", h5py), ("v2ecore.v2e_utils", utils), ("v2ecore.output", out),
                      ("v2ecore.output.aedat2_output", a2), ("v2ecore.output.ae_text_output", tx)):
        sys.modules[name] = mod


def main():
    _install_stand_ins()
    sys.path.insert(0, REF)
    from v2ecore.emulator import EventEmulator
    import dvs_emulator_restated as R

    out = {}
    names = []
    for h, w in ((24, 40), (5, 37)):
        for cname, case in R.make_cases(h, w).items():
            name = "%s_%dx%d" % (cname, w, h)
            emu = EventEmulator(pos_thres=float(np.mean(case["pos_thres"])), neg_thres=float(np.mean(case["neg_thres"])),
                                sigma_thres=0, cutoff_hz=case.get("cutoff_hz", 0), leak_rate_hz=case.get("leak_rate_hz", 0),
                                refractory_period_s=case.get("refractory_period_s", 0), shot_noise_rate_hz=0,
                                leak_jitter_fraction=0, noise_rate_cov_decades=0, seed=7, device="cpu")
            rows, per_frame = [], []
            for k, (frame, t) in enumerate(zip(case["frames"], case["t"])):
                ev = emu.generate_events(frame, float(t))
                if k == 0:
                    for key, attr in (("pos_thres", "pos_thres"), ("neg_thres", "neg_thres"), ("noise_rate_array", "noise_rate_array")):
                        if key in case and np.ndim(case[key]) == 2:
                            setattr(emu, attr, torch.from_numpy(np.asarray(case[key], np.float32)))
                        elif key in case and key != "noise_rate_array":
                            setattr(emu, attr, float(case[key]))
                    continue
                per_frame.append(0 if ev is None else len(ev))
                if ev is not None:
                    assert ev.dtype == np.float32 and ev.shape[1] == 4
                    rows.append(ev)
            rows = R.canonical(np.concatenate(rows) if rows else np.zeros((0, 4), np.float32))
            out[name + "_frames"] = case["frames"]
            out[name + "_t"] = np.asarray(case["t"], np.float64)
            for key in R.PARAM_KEYS:
                if key in case:
                    out[name + "_" + key] = np.asarray(case[key], np.float32 if np.ndim(case[key]) == 2 else np.float64)
            out[name + "_rows"] = rows
            out[name + "_per_frame"] = np.asarray(per_frame, np.int64)
            out[name + "_base"] = emu.base_log_frame.numpy().astype(np.float32)
            out[name + "_lp0"] = emu.lp_log_frame0.numpy().astype(np.float32)
            out[name + "_lp1"] = emu.lp_log_frame1.numpy().astype(np.float32)
            if case.get("refractory_period_s", 0) > 0:
                out[name + "_tmem"] = emu.timestamp_mem.numpy().astype(np.float32)
            names.append(name)
            print("%-20s %6d rows, per frame %s" % (name, len(rows), per_frame))
    out["cases"] = np.array(names, dtype="U32")
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
