"""The device JPEG decoder without a device: the restatement (tests/jpeg_decode_restated.py) against PIL bit for bit, the
relaxation schedule against the sequential decode, and the refusals of jpeg_read.parse_jpeg."""
import io
from importlib import import_module

import numpy as np
import pytest

import jpeg_decode_restated as R

J = R.J
SIZES = ((8, 8), (16, 16), (13, 17), (1, 1), (48, 40), (67, 130))       # (height, width): 17x13, 40x48 and 130x67 as width x height
MODES = ("gray", "444", "420")
# (quality, extra arguments of Image.save)
VARIANTS = ((30, {}), (75, {}), (95, {}), (100, {}), (75, dict(optimize=True)), (95, dict(restart_marker_blocks=1)),
            (75, dict(restart_marker_blocks=2)), (100, dict(optimize=True, restart_marker_blocks=2)))
KINDS = ("noise", "const", "gradient")
_worst = {"rounds": 0}


def check(data):
    ref = R.pil_decode(data)
    st = R.Stream(data)
    coef, states = R.decode_sequential(st)
    assert np.array_equal(R.render(st, coef), ref)
    assert np.array_equal(R.render(st, coef, rgb=False), ref[:, :, ::-1])
    entries, rounds, converged = R.relax(st)
    assert converged and entries == states                             # the schedule's fixed point is the sequential decode
    assert 1 <= rounds <= R.DEFAULT_MAX_ROUNDS, rounds
    _worst["rounds"] = max(_worst["rounds"], rounds)
    return st, rounds


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_restatement_equals_pil_and_schedule_equals_sequential(mode, size):
    h, w = size
    for quality, kw in VARIANTS:
        for kind in KINDS:
            check(R.fixture(mode, h, w, quality, kind, **kw))
    print("largest number of rounds so far: %d (default max_rounds %d)" % (_worst["rounds"], R.DEFAULT_MAX_ROUNDS))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("quality", (95, 100))
def test_noise_fixtures_hold_byte_stuffing_and_several_subsequences(mode, quality):
    data = R.fixture(mode, 67, 130, quality, "noise")
    h = J.parse_jpeg(data)
    body = data[h.data_start:h.data_end]
    assert b"\xff\x00" in body                                         # byte stuffing is exercised
    assert h.seg_start.size == 1 and len(body) > 4 * R.S               # one entropy segment longer than 4 subsequences
    st, rounds = check(data)
    assert st.segs[0].m > 4 and rounds > 1


def test_a_stuffed_zero_at_a_subsequence_boundary_starts_one_byte_later():
    """searched over seeds so that the case cannot go vacuous: a file whose raw byte i * S is the 00 of an FF 00 pair"""
    for seed in range(400):
        data = R.fixture("gray", 48, 40, 100, "noise", seed=seed)
        h = J.parse_jpeg(data)
        body = np.frombuffer(data[h.data_start:h.data_end], dtype=np.uint8)
        at = np.arange(R.S, body.size, R.S)
        if np.any((body[at] == 0) & (body[at - 1] == 0xFF)):
            check(data)
            return
    pytest.fail("no fixture with a stuffed zero on a subsequence boundary in 400 seeds")


def test_header_fields():
    data = R.fixture("420", 13, 17, 75, "noise", restart_marker_blocks=1)
    h = J.parse_jpeg(data)
    assert (h.height, h.width, h.ncomp, h.mode, h.hmax, h.vmax) == (13, 17, 3, "420", 2, 2)
    assert (h.mcus_x, h.mcus_y, h.blocks_per_mcu, h.n_blocks) == (2, 1, 6, 12)
    assert h.restart_interval == 1 and h.seg_start.size == 2 and h.seg_sub0[-1] == h.nsub
    assert data[h.seg_end[0]:h.seg_end[0] + 2] == b"\xff\xd0" and data[h.data_end:h.data_end + 2] == b"\xff\xd9"
    assert h.qt.shape == (4, 64) and h.qt[0, 0] > 0 and h.dc_bits.shape == (4, 17) and h.ac_huffval.shape == (4, 256)
    d = J.descriptor(h, file_off=(1 << 33) + 16, seg_row0=5)
    assert d.size == J.DESC_BYTES == 9216 and d[:8].view(np.int64)[0] == (1 << 33) + 16
    assert d[8:24].view(np.int32).tolist() == [5, 2, h.nsub, 1]
    desc, rows, blob, max_subs = J.pack_batch([h, h], [data, data])
    assert desc.shape == (2, J.DESC_BYTES) and rows.shape == (6, 4) and blob.size % 16 == 0 and max_subs == h.nsub
    assert rows[2, 2] == h.nsub and desc[1, 8:12].view(np.int32)[0] == 3


def _pil(arr, mode, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_refusals_name_the_reason():
    rgb = R.content("noise", 16, 16, 3)
    with pytest.raises(J.UnsupportedJpeg, match="progressive"):
        J.parse_jpeg(_pil(rgb, "RGB", progressive=True))
    with pytest.raises(J.UnsupportedJpeg, match="4:2:2"):
        J.parse_jpeg(_pil(rgb, "RGB", subsampling=1))
    cmyk = np.concatenate([rgb, rgb[:, :, :1]], axis=2)
    with pytest.raises(J.UnsupportedJpeg, match="4 components"):
        J.parse_jpeg(_pil(cmyk, "CMYK"))
    good = _pil(rgb, "RGB")
    h = J.parse_jpeg(good)
    with pytest.raises(J.UnsupportedJpeg, match="runs past the file"):
        J.parse_jpeg(good[:h.data_start - 5])                          # cut inside the SOS segment
    with pytest.raises(J.UnsupportedJpeg, match="runs past the file"):
        J.parse_jpeg(good[:30])                                        # cut inside a table segment
    with pytest.raises(J.UnsupportedJpeg, match="not a JPEG"):
        J.parse_jpeg(b"\x89PNG\r\n\x1a\n" + bytes(32))
    assert issubclass(J.UnsupportedJpeg, J.JpegError)


def test_truncated_entropy_data_is_corrupt_in_the_restatement():
    data = R.fixture("gray", 48, 40, 95, "noise")
    h = J.parse_jpeg(data)
    cut = data[:h.data_start + (h.data_end - h.data_start) // 2] + b"\xff\xd9"
    with pytest.raises(J.JpegError):
        R.decode(cut)
