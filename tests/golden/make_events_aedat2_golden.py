#!/usr/bin/env python3
"""Generates tests/golden/events_aedat2_reference.npz from the reference's AEDAT-2.0 writer (run by hand, not by the tests).

v2e/v2ecore/output/aedat2_output.py is imported as-is under stand-ins for the two modules it imports without needing them here:
engineering_notation (EngNumber, used in a log line) and v2ecore.v2e_utils (v2e_quit).  For each of the five sizes the class
takes, about 50 seeded float32 rows [t_s, x, y, p (-1 / +1)] go to AEDat2Output.appendEvents in two calls.  The first three
rows have the flipped y 141, so their records start with '#' and the class drops them; the first row of the second call has the
flipped y 140, starts with '#' too and is kept, because only the first write to a file is looked at.  Stored per size: the rows,
the length of the first call, and the file's bytes after the header (its length is file.tell() right after construction).

    SCPOSE_REFERENCE_V2E=<checkout>/v2e python tests/golden/make_events_aedat2_golden.py
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((346, 260), (692, 520), (1280, 720), (640, 480), (240, 180))      # (width, height)
N_ROWS, FIRST_CALL = 50, 21


def reference_class():
    ref = os.environ.get("SCPOSE_REFERENCE_V2E")
    if not ref or not os.path.isdir(ref):
        sys.exit("set SCPOSE_REFERENCE_V2E to the v2e directory of a checkout of the reference")
    eng = types.ModuleType("engineering_notation"); eng.EngNumber = lambda v: v
    pkg = types.ModuleType("v2ecore"); pkg.__path__ = [os.path.join(ref, "v2ecore")]
    utils = types.ModuleType("v2ecore.v2e_utils"); utils.v2e_quit = sys.exit
    for name, mod in (("engineering_notation", eng), ("v2ecore", pkg), ("v2ecore.v2e_utils", utils)):
        sys.modules[name] = mod
    from v2ecore.output.aedat2_output import AEDat2Output
    return AEDat2Output


def rows_for(w, h, seed):
    rng = np.random.default_rng(seed)
    r = np.empty((N_ROWS, 4), np.float32)
    r[:, 0] = np.sort(rng.uniform(0.001, 30.0, N_ROWS)).astype(np.float32)
    r[:, 1] = rng.integers(0, w, N_ROWS)
    r[:, 2] = rng.integers(0, h, N_ROWS)
    r[:, 3] = rng.integers(0, 2, N_ROWS) * 2 - 1
    r[:3, 2] = h - 1 - 141
    r[3, 2] = h - 1 - 139                      # the first record that stays
    r[FIRST_CALL, 2] = h - 1 - 140
    r[0, 1], r[1, 1] = 0, w - 1                # both ends of the flipped x
    r[4, 2], r[5, 2] = 0, h - 1                # both ends of the flipped y (flipped y above 511 wraps at 1280 x 720)
    return r


def main():
    cls = reference_class()
    out = {}
    for k, (w, h) in enumerate(SIZES):
        rows = rows_for(w, h, 100 + k)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "g.aedat")
            o = cls(path, output_width=w, output_height=h)
            header = o.file.tell()
            o.appendEvents(rows[:FIRST_CALL])
            o.appendEvents(rows[FIRST_CALL:])
            o.close()
            body = np.fromfile(path, dtype=np.uint8)[header:]
        assert len(body) == 8 * (N_ROWS - 3), len(body)
        tag = "%dx%d" % (w, h)
        out[tag + "_rows"] = rows
        out[tag + "_first_call"] = np.int64(FIRST_CALL)
        out[tag + "_body"] = body
    np.savez_compressed(os.path.join(HERE, "events_aedat2_reference.npz"), **out)
    print("wrote events_aedat2_reference.npz: %s" % ", ".join("%dx%d" % s for s in SIZES))


if __name__ == "__main__":
    main()
