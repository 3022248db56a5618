"""v2e/v2e.py from image files of another size than the sensor to event text and event frames in one pass: the resize on the device
against the restatement's gray frames, the rendering against e2v.py on the text file of the same run, --device_decode, several
batches, and the count modes.

Scene: 8 RGB frames of 22 x 26, a bright 6 x 6 square moving 2 px per frame over a dim textured background, saved as PNG, BMP and
baseline JPEG in turn; the sensor is 10 x 12."""
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
from PIL import Image

import dvs_emulator_restated as D
import event_render_restated as ER
import resize_area_restated as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (10, 12)
FLAGS = ["--dvs_text", "ev", "--input_frame_rate", "100", "--pos_thres", ".15", "--neg_thres", ".15", "--sigma_thres", "0"]
SIZE = ["--output_width", "12", "--output_height", "10"]
EXTRA = ["--overwrite", "--avi_frame_rate", "10"]


def cli_module(name):
    sys.path.insert(0, os.path.join(ROOT, "v2e"))
    try:
        return import_module(name)
    finally:
        sys.path.pop(0)


def tree(folder):
    """{relative path: bytes} of everything under folder"""
    out = {}
    for base, _, files in os.walk(folder):
        for n in files:
            with open(os.path.join(base, n), "rb") as f:
                out[os.path.relpath(os.path.join(base, n), folder)] = f.read()
    return out


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The files, and the restatement's gray sensor frames of what PIL decodes from them -- as BMP files in a second folder."""
    root = tmp_path_factory.mktemp("v2e_frames")
    src = root / "frames"; src.mkdir()
    rng = np.random.default_rng(5)
    bg = rng.integers(20, 60, size=(22, 26, 3), dtype=np.uint8)
    decoded = []
    for k in range(8):
        f = bg.copy()
        f[8:14, 2 + 2 * k:8 + 2 * k] = (250, 240, 230)
        path = src / ("%03d.%s" % (k, ("png", "bmp", "jpg")[k % 3]))
        Image.fromarray(f).save(path, **({"quality": 90} if k % 3 == 2 else {}))
        decoded.append(np.array(Image.open(path).convert("RGB")))
    gray = R.gray(R.resize_area(np.stack(decoded), HW))
    ref = root / "gray"; ref.mkdir()
    for k, g in enumerate(gray):
        Image.fromarray(g).save(ref / ("%03d.bmp" % k))
    # the scene is worth testing: enough events, and at least three 20 ms frames
    cols = D.columns(D.RestatedEmulator(0.15, 0.15).emulate(gray, np.arange(8) / 100.0))
    names = ER.render(cols[0], cols[1], cols[2], cols[3], HW, interval=20000.0, fs=2, fold_polarity=True)[1]
    assert len(cols[0]) >= 200 and len(names) >= 3, (len(cols[0]), names)
    return {"root": root, "src": src, "gray": ref, "columns": cols}


def run_v2e(folder, out, *flags, max_batch_frames=None):
    v2e = cli_module("v2e")
    assert v2e.main(["--input", str(folder), "--output_folder", str(out), *FLAGS, *flags], max_batch_frames=max_batch_frames) == 0
    return tree(out)


def run_e2v(events, out, *exposure):
    cli_module("e2v").main(["--events_file", str(events), "--delim_whitespace", "--output_folder", str(out), "--output_width", "12",
                            "--output_height", "10", "--dvs_exposure", *exposure])
    return tree(out)


@pytest.fixture(scope="module")
def main_run(gpu_ops, scene):
    """The run of the issue, through the command line itself"""
    out = scene["root"] / "out"
    cmd = [sys.executable, os.path.join(ROOT, "v2e", "v2e.py"), "--input", str(scene["src"]), "--output_folder", str(out), *SIZE,
           "--dvs_exposure", "duration", "0.02", *FLAGS, *EXTRA]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "no AVI is written" in r.stderr
    return tree(out)


def test_events_equal_the_run_on_the_restated_gray_frames(gpu_ops, scene, main_run):
    plain = run_v2e(scene["gray"], scene["root"] / "plain")
    assert set(plain) == {"ev.txt"} and main_run["ev.txt"] == plain["ev.txt"]
    t, x, y, p = (c.cpu().numpy() for c in gpu_ops.parse_events_csv(main_run["ev.txt"], delim_whitespace=True))
    for got, want in zip((t, x, y, p), scene["columns"]):
        assert np.array_equal(got, want)


def test_event_frames_equal_e2v_on_the_text_of_the_same_run(gpu_ops, scene, main_run):
    chain = run_e2v(scene["root"] / "out" / "ev.txt", scene["root"] / "chain", "duration", "20000")
    frames = {k: v for k, v in main_run.items() if k != "ev.txt"}
    assert "dvs-video-frame_times.txt" in frames and sum(k.startswith("event-frames" + os.sep) for k in frames) >= 3
    assert frames == chain


def test_device_decode_gives_the_same_bytes(gpu_ops, scene, main_run):
    got = run_v2e(scene["src"], scene["root"] / "dd", *SIZE, "--dvs_exposure", "duration", "0.02", "--device_decode", *EXTRA)
    assert got == main_run
    # without a resize the device's frames are reduced to gray by the same kernel
    own = run_v2e(scene["gray"], scene["root"] / "dd_own", "--device_decode")
    assert own["ev.txt"] == main_run["ev.txt"]


@pytest.mark.parametrize("decode", ([], ["--device_decode"]), ids=("host", "device"))
def test_batches_of_two_frames_give_the_same_bytes(gpu_ops, scene, main_run, decode):
    got = run_v2e(scene["src"], scene["root"] / ("b2" + "".join(decode)), *SIZE, "--dvs_exposure", "duration", "0.02", *decode, *EXTRA,
                  max_batch_frames=2)
    assert got == main_run


@pytest.mark.parametrize("exposure", (("count", "150"), ("area_count", "40", "4")), ids=lambda e: e[0])
def test_count_modes_equal_the_e2v_chain(gpu_ops, scene, main_run, exposure):
    out = scene["root"] / ("v_" + exposure[0])
    got = run_v2e(scene["src"], out, *SIZE, "--dvs_exposure", *exposure)
    chain = run_e2v(out / "ev.txt", scene["root"] / ("c_" + exposure[0]), *exposure)
    assert got["ev.txt"] == main_run["ev.txt"]
    frames = {k: v for k, v in got.items() if k != "ev.txt"}
    assert len(frames) >= 3 and frames == chain


def test_skip_video_output_and_the_sensor_size_for_aedat2(gpu_ops, scene, main_run, tmp_path):
    got = run_v2e(scene["src"], tmp_path / "skip", *SIZE, "--dvs_exposure", "duration", "0.02", "--skip_video_output")
    assert set(got) == {"ev.txt"} and got["ev.txt"] == main_run["ev.txt"]
    with pytest.raises(SystemExit, match="events_aedat2"):             # 12 x 10 is none of the AEDAT-2.0 sensors: judged at the output size
        run_v2e(scene["src"], tmp_path / "aedat", *SIZE, "--events_aedat2", "ev")
