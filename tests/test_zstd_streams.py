"""The Zstandard test writer (zstd_stream_writer.py) and the restated decoder (zstd_restated.py) pinned to each other and to a
third party, libzstd, before either judges the device decoder (csrc/events_aedat4_zstd.hip).  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_zstd_golden as G  # noqa: E402
import zstd_cases as C  # noqa: E402
import zstd_restated as R  # noqa: E402
import zstd_stream_writer as Z  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "zstd_frames.npz"))
LIBZSTD = G.load_libzstd()
# libzstd decodes a payload of several frames only through its streaming calls; these two are checked by the restatement alone
SEVERAL_FRAMES = ("two_frames", "skippable_first")


def test_xxh64_twice():
    for probe in (b"", b"a", b"a" * 20, bytes(range(256)) * 3 + b"xyz", b"q" * 32, b"q" * 39):
        assert Z.xxh64(probe) == R.xxh64(probe)
    assert R.xxh64(b"") == 0xEF46DB3751D8E999 and R.xxh64(b"abc") == 0x44BC2CF5AD770999          # the published test vectors


@pytest.mark.parametrize("name", sorted(C.valid()))
def test_writer_frames_decode_to_their_plan(name):
    payload, planned = C.valid()[name]
    assert R.measure(payload) == (len(planned), 0)
    assert R.decode(payload) == (planned, 0)


@pytest.mark.parametrize("name", sorted(set(C.valid()) - set(SEVERAL_FRAMES)))
def test_writer_frames_decode_with_libzstd(name):
    if LIBZSTD is None:
        pytest.skip("libzstd does not load through ctypes: the writer is checked by the restated decoder alone")
    payload, planned = C.valid()[name]
    assert G.decompress(LIBZSTD, payload, len(planned) + 64) == planned


@pytest.mark.parametrize("name", sorted(k for k in GOLDEN.files if k.startswith("frame_")))
def test_golden_frames_decode_with_the_restatement(name):
    raw = GOLDEN["raw_" + name.split("_")[1]].tobytes()
    assert R.decode(GOLDEN[name].tobytes()) == (raw, 0)


@pytest.mark.parametrize("name", sorted(C.refused()))
def test_restatement_refuses(name):
    payload, with_verify, without = C.refused()[name]
    assert R.decode(payload, True) == (b"", with_verify)
    got, status = R.decode(payload, False)
    assert status == without and (got != b"") == (without == 0 and name == "wrong_checksum")


def test_golden_is_small_and_covers_both_literal_kinds():
    assert os.path.getsize(os.path.join(HERE, "golden", "zstd_frames.npz")) < 256 * 1024
    big = GOLDEN["frame_9000_3_0"].tobytes()
    assert big[:4] == b"\x28\xb5\x2f\xfd" and len(GOLDEN["raw_9000"]) > 1 << 17                     # more than one block


def test_greedy_plan_round_trip():
    data = GOLDEN["raw_700"].tobytes()
    payload, planned = Z.frame(Z.greedy_plan(data, block=4096, lit="huffman", streams=4, ll="fse", of="fse", ml="fse", of_log=7),
                               checksum=True)
    assert planned == data and R.decode(payload) == (data, 0)
