"""ops.decode_png / csrc/png_decode.hip: kernels == restatement == PIL by equality on every accepted case, and on every damaged case
PIL's pixels or PngError exactly where PIL raises, with the restatement's status word."""
import io
from importlib import import_module

import numpy as np
import pytest
import torch
from PIL import Image

import png_decode_restated as R
import png_stream_writer as W

pytestmark = pytest.mark.gpu
pr = R.pr
_REF = {}


def reference(name, data):
    """(PIL's RGB pixels or None when PIL raises, the restatement's pixels, its status) -- computed once per case"""
    if name not in _REF:
        try:
            with Image.open(io.BytesIO(data)) as im:
                pil = np.array(im.convert("RGB"))
        except OSError:
            pil = None
        px, status, _ = R.decode(data)
        _REF[name] = (pil, px, status)
    return _REF[name]


def device_status(gpu_ops, data, rgb=True):
    dev = torch.device("cuda", torch.cuda.current_device())
    frames, status = gpu_ops._png_decode_group([pr.parse_png(data)], [data], rgb, dev)
    return frames[0].cpu().numpy(), status[0]


def geometry_groups(cases):
    groups = {}
    for name, data in cases.items():
        hd = pr.parse_png(data)
        groups.setdefault((hd.height, hd.width), []).append(name)
    return groups


@pytest.mark.parametrize("rgb", [True, False])
def test_every_accepted_case_equals_the_restatement_and_pil(gpu_ops, rgb):
    """all cases, grouped by frame size into calls that mix colour types, deflate forms and split patterns"""
    cases = W.accepted_cases()
    seen = 0
    for (h, w), names in geometry_groups(cases).items():
        got, info = gpu_ops.decode_png([cases[k] for k in names], rgb=rgb, fallback=False)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(names), h, w, 3) and got.is_cuda
        assert info["fallback"] == {} and info["device"] == [True] * len(names)
        got = got.cpu().numpy()
        for i, k in enumerate(names):
            pil, px, status = reference(k, cases[k])
            assert status == 0 and np.array_equal(px, pil), k
            assert np.array_equal(got[i], pil if rgb else pil[:, :, ::-1]), k
            seen += 1
    assert seen == len(cases)


def test_one_call_mixes_every_channel_count(gpu_ops):
    cases = W.accepted_cases()
    names = ["type0", "type2", "type3", "type4", "type6", "palette_trns", "gray_trns", "palette_short"]
    assert len({pr.parse_png(cases[k]).geometry for k in names}) == 4
    got, info = gpu_ops.decode_png([cases[k] for k in names], fallback=False)
    assert info["fallback"] == {}
    for i, k in enumerate(names):
        assert np.array_equal(got[i].cpu().numpy(), reference(k, cases[k])[0]), k


def test_six_frame_sizes_in_one_call(gpu_ops):
    """frames of different sizes share a call only through decode_crop: the identity warp into a crop that holds the whole frame"""
    cases = W.accepted_cases()
    names = ["shape_1x1_type0", "shape_1x9_type3", "shape_9x1_type6", "shape_3x5_type2", "shape_63x7_type4", "shape_65x7_type3", "hand_fixed",
             "dyn_long_codes", "dyn_single_distance", "dyn_lone_eob"]
    names = [k for k in names if k in cases]
    assert len({pr.parse_png(cases[k]).geometry for k in names}) >= 6
    trans = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (len(names), 1, 1))
    got, info = gpu_ops.decode_crop([cases[k] for k in names], trans, (16, 70), fallback=False, png=True)
    assert info["fallback"] == {} and info["png"] == list(range(len(names))) and info["rounds"] == [0] * len(names)
    for i, k in enumerate(names):
        pil = reference(k, cases[k])[0]
        want = np.zeros((70, 16, 3), dtype=np.uint8)
        hh, ww = min(70, pil.shape[0]), min(16, pil.shape[1])
        want[:hh, :ww] = pil[:hh, :ww]
        assert np.array_equal(got[i].cpu().numpy(), want), k


def test_whatever_the_workspace_held(gpu_ops):
    cases = W.accepted_cases()
    names = [k for k in cases if k.startswith("form_")]
    files = [cases[k] for k in names]
    dev = torch.cuda.current_device()
    first, _ = gpu_ops.decode_png(files, fallback=False)                  # sizes the cached workspace
    got = []
    for fill in (0x00, 0xFF):
        gpu_ops._IMAGE_WORKSPACE[dev].fill_(fill)
        got.append(gpu_ops.decode_png(files, fallback=False)[0])
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], first)
    assert np.array_equal(first[0].cpu().numpy(), reference(names[0], files[0])[0])


@pytest.mark.parametrize("name", sorted(W.damaged_cases()))
def test_damaged_files_are_the_host_decoders(gpu_ops, name):
    data = W.damaged_cases()[name]
    pil, px, status = reference(name, data)
    hd = pr.parse_png(data)
    if hd.crc_ok:
        device_status(gpu_ops, data)                                      # sizes the cached workspace
        for fill in (0x00, 0xFF, 0x03):                                   # whatever the workspace held: all-bad and all-good "filter bytes"
            gpu_ops._IMAGE_WORKSPACE[torch.cuda.current_device()].fill_(fill)
            frame, got_status = device_status(gpu_ops, data)
            assert got_status == status, (name, fill, got_status, status)
            if status == 0:
                assert np.array_equal(frame, pil)
    assert (status != 0) == (pil is None)
    if pil is None:
        with pytest.raises(pr.PngError):
            gpu_ops.decode_png([data])
        with pytest.raises(pr.PngError):
            gpu_ops.decode_png([data], fallback=False)
    else:
        got, info = gpu_ops.decode_png([data])
        assert np.array_equal(got[0].cpu().numpy(), pil)
        assert info["device"] == [hd.crc_ok] and (sorted(info["fallback"]) == ([] if hd.crc_ok else [0]))


def test_a_damaged_file_beside_good_ones(gpu_ops):
    good, bad = W.damaged_cases()["long_raw"], W.damaged_cases()["adler_byte_2"]
    crc = W.damaged_cases()["idat_crc"]
    got, info = gpu_ops.decode_png([good, crc, good])
    want = reference("long_raw", good)[0]
    assert info["device"] == [True, False, True] and "CRC" in info["fallback"][1]
    assert all(np.array_equal(got[i].cpu().numpy(), w) for i, w in enumerate((want, reference("idat_crc", crc)[0], want)))
    with pytest.raises(pr.PngError, match="file 1"):
        gpu_ops.decode_png([good, bad, good])
    gpu_ops._IMAGE_WORKSPACE[torch.cuda.current_device()].fill_(0xFF)       # the message names what the stream is, not what the workspace held
    with pytest.raises(pr.PngError, match=r"device status 1 \(corrupt deflate stream\)"):
        gpu_ops.decode_png([good, W.damaged_cases()["block_type_3"]], fallback=False)
    with pytest.raises(pr.PngError, match="CRC"):
        gpu_ops.decode_png([good, crc], fallback=False)


def test_refused_files_go_to_pil_or_raise_by_name(gpu_ops):
    word = W.refused_cases()["interlaced"][1]
    data = W.assemble(1, 1, 0, W.deflate(b"\x00\x9c"), interlace=1)        # 1 x 1: one Adam7 pass, the data of the plain file
    good = W.accepted_cases()["type0"]
    with pytest.raises(pr.UnsupportedPng, match=word):
        gpu_ops.decode_png([data], fallback=False)
    with Image.open(io.BytesIO(data)) as im:
        pil = np.array(im.convert("RGB"))
    got, info = gpu_ops.decode_png([data])
    assert info["device"] == [False] and word in info["fallback"][0] and np.array_equal(got[0].cpu().numpy(), pil)
    with pytest.raises(ValueError, match="different sizes"):
        gpu_ops.decode_png([data, good])
    with pytest.raises(ValueError, match="no files"):
        gpu_ops.decode_png([])
