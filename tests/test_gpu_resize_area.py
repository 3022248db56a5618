"""ops.resize_area (csrc/resize_area.hip) against the NumPy restatement, bit for bit: resized channels, gray with the channels both ways,
one-channel frames, host and device inputs, a source that starts off a 16-byte boundary, the rejections, and the result as the
emulator's input."""
import numpy as np
import pytest
import torch

import resize_area_restated as R

pytestmark = pytest.mark.gpu
_resized = {}


def resized(name):
    """The restatement's resized channels of the case's frames, computed once."""
    if name not in _resized:
        out_hw = next(c for c in R.CASES if c[0] == name)[2]
        _resized[name] = R.resize_area(R.frames_for(name), out_hw)
        _resized[name].setflags(write=False)
    return _resized[name]


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d values differ, first at %s: %d, expected %d" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c[0])
def test_device_equals_restatement(gpu_ops, case):
    name, _, out_hw, c = case
    fr = torch.from_numpy(R.frames_for(name)).cuda()
    want = resized(name)
    if c == 1:                                                        # (F, H, W): resized, `gray` ignored
        same(gpu_ops.resize_area(fr, out_hw, gray=True), want, name)
        same(gpu_ops.resize_area(fr, out_hw, gray=False), want, name + " gray=False")
        return
    same(gpu_ops.resize_area(fr, out_hw, gray=False), want, name + " channels")
    same(gpu_ops.resize_area(fr, out_hw, gray=False, channels="bgr"), want, name + " channels, bgr")
    for order in ("rgb", "bgr"):
        same(gpu_ops.resize_area(fr, out_hw, gray=True, channels=order), R.gray(want, order), "%s gray %s" % (name, order))
    if name == "box_2x4_ties":                                        # the constructed ties: 10.5 -> 10 and 11.5 -> 12
        assert gpu_ops.resize_area(fr, out_hw, gray=False)[0, 0, :, 0].tolist() == [10, 12]
    if name == "gray_only":
        same(gpu_ops.resize_area(fr, out_hw, gray=False), R.frames_for(name), "the input's own size copies")


def test_host_input_and_a_source_off_the_16_byte_boundary(gpu_ops):
    name, (H, W), out_hw, _ = R.CASES[0]
    fr = R.frames_for(name)
    want = R.gray(resized(name))
    same(gpu_ops.resize_area(fr, out_hw), want, "host array")         # gray=True, channels="rgb" by default
    dev = torch.from_numpy(fr).cuda()
    tail = dev[1:]                                                    # starts H * W * 3 = 429 bytes into the allocation
    assert tail.is_contiguous() and tail.data_ptr() % 16 != 0
    same(gpu_ops.resize_area(tail, out_hw), want[1:], "frames 1 ..")
    head = dev[:2]                                                    # the last 16-byte window of the batch ends outside it
    same(gpu_ops.resize_area(head, out_hw), want[:2], "frames .. 2")
    flat = torch.zeros(5 + fr.size, dtype=torch.uint8, device="cuda")
    flat[5:] = dev.flatten()
    same(gpu_ops.resize_area(flat[5:].view(fr.shape), out_hw), want, "5 bytes off")


def test_output_is_the_emulators_input(gpu_ops):
    name, _, (h, w), _ = R.CASES[0]
    out = gpu_ops.resize_area(R.frames_for(name), (h, w))
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and tuple(out.shape) == (R.F, h, w)
    emu = gpu_ops.dvs_emulator(h, w, pos_thres=0.15, neg_thres=0.15)
    cols = emu.emulate(out, np.arange(R.F) / 100.0)
    assert cols[0].numel() > 0 and int(cols[1].max()) < w and int(cols[2].max()) < h


def test_rejections(gpu_ops):
    fr = R.frames_for("fractional_both")
    for bad, what in ((fr.astype(np.float32), "uint8"), (fr[0, :, :, 0], "shape"), (fr[..., :2], "shape"),
                      (np.concatenate([fr, fr[..., :1]], axis=3), "shape")):
        with pytest.raises(ValueError, match=what):
            gpu_ops.resize_area(bad, (4, 5))
    for out_hw in ((12, 5), (4, 14), (0, 5)):
        with pytest.raises(ValueError, match="13 x 11"):
            gpu_ops.resize_area(fr, out_hw)
    with pytest.raises(ValueError, match="channels"):
        gpu_ops.resize_area(fr, (4, 5), channels="gbr")
