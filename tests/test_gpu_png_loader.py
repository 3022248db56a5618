"""DATASET.DEVICE_DECODE_PNG through validate(): files -> key points with the PNG frames decoded on the device (ops.decode_crop,
png=True) must give the rows, the .mat and the image order of the flag-off run, bit for bit -- whatever the workers, the engine batch,
COLOR_RGB and DEVICE_DECODE -- on a scene of gray, RGB, palette and RGBA PNGs, an interlaced PNG, a baseline JPEG and a BMP."""
import json
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

import jpeg_decode_restated as J
import png_stream_writer as W
from device_decode_scene import P, ROOT, scene_config, scene_dataset
from oracle import hrnet_ref as R

pytestmark = pytest.mark.gpu
SIZE = (120, 160)
KINDS = ("png_gray", "png_rgb", "png_palette", "png_rgba", "png_interlaced", "jpeg", "bmp")


def adam7(px):
    """the filtered scan lines (filter 0) of the seven passes of an RGB frame"""
    out = bytearray()
    for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = px[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            for row in sub:
                out += b"\x00" + row.tobytes()
    return bytes(out)


def write_scene(root):
    from PIL import Image
    os.makedirs(os.path.join(root, "frames")); os.makedirs(os.path.join(root, "data"))
    rng = np.random.default_rng(77)
    images, anns = [], []
    for i, kind in enumerate(KINDS):
        rgb = J.content("noise", SIZE[0], SIZE[1], 3, seed=60 + i)
        name = "f%02d.%s" % (i, {"jpeg": "jpg", "bmp": "bmp"}.get(kind, "png"))
        path = os.path.join(root, "frames", name)
        if kind == "png_gray":
            data = W.write_png(rgb[:, :, 0], 0, "random", rng=rng)[0]
        elif kind == "png_rgb":
            data = W.write_png(rgb, 2, "random", "best", "thirds", rng=rng)[0]
        elif kind == "png_palette":
            data = W.write_png(rgb[:, :, 1], 3, "random", palette=rng.integers(0, 256, (256, 3), dtype=np.uint8), rng=rng)[0]
        elif kind == "png_rgba":
            data = W.write_png(np.concatenate([rgb, rgb[:, :, :1]], axis=2), 6, "random", "fixed", rng=rng)[0]
        elif kind == "png_interlaced":
            data = W.assemble(SIZE[0], SIZE[1], 2, W.deflate(adam7(rgb)), interlace=1)
        elif kind == "jpeg":
            data = J.encode(rgb, "420", 90)
        else:
            Image.fromarray(rgb, "RGB").save(path, "BMP")
            data = None
        if data is not None:
            with open(path, "wb") as fh:
                fh.write(data)
        images.append({"id": i + 1, "file_name": name, "width": SIZE[1], "height": SIZE[0]})
        anns.append({"image_id": i + 1, "bbox": [10.0 + 3 * i, 8.0, 90.0, 70.0 + i], "keypoints": [2.0] * 33, "id": i, "category_id": 1})
    with open(os.path.join(root, "data", "real_test.json"), "w") as fh:
        json.dump({"images": images, "annotations": anns}, fh)


@pytest.fixture(scope="module")
def scene(gpu_ops, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("device_decode_png"))
    write_scene(root)
    models = import_module(P + ".models")
    net = models.pose_hrnet.get_pose_net(scene_config(root), is_train=False)
    net.load_state_dict(R.make_state_dict(R.w32_cfg(11, 64), seed=31), strict=False)
    return {"root": root, "net": net.cuda().eval(), "runs": {}}


class Seen:
    """the data set as validate() sees it, keeping what evaluate() is handed"""

    def __init__(self, ds):
        self.ds, self.flip_pairs = ds, ds.flip_pairs
        self.device_decode, self.device_decode_png = ds.device_decode, ds.device_decode_png

    def __len__(self):
        return len(self.ds)

    def evaluate(self, c, preds, output_dir, name, boxes, image_path, *a, **k):
        self.preds, self.image_path = preds.copy(), list(image_path)
        return self.ds.evaluate(c, preds, output_dir, name, boxes, image_path, *a, **k)


def run(scene, rgb, jpeg, png, workers, engine_batch):
    """one validate() over the scene -> (all_preds, the preds of pred_test.mat, image_path); cached: the reference run is shared"""
    key = (rgb, jpeg, png, workers, engine_batch)
    if key not in scene["runs"]:
        from scipy.io import loadmat
        fn = import_module(P + ".core.function"); par = import_module(P + ".parallel")
        cfg = scene_config(scene["root"], ["DATASET.COLOR_RGB", str(rgb), "DATASET.DEVICE_DECODE_PNG", str(png)])
        ds = scene_dataset(cfg, jpeg)
        assert ds.device_decode_png is png and ds.device_decode is jpeg        # the key is an override every CLI takes
        out = os.path.join(scene["root"], "out_%d_%d_%d_%d_%d" % key)
        os.makedirs(out, exist_ok=True)
        seen = Seen(ds)
        loader = par.valid_loader(ds, 0, len(ds), 1, 4, workers, True)
        fn.validate(cfg, loader, seen, scene["net"], None, out, "", pred_file_name="pred_test", log_metrics=False, engine_batch=engine_batch)
        scene["runs"][key] = (seen.preds, loadmat(os.path.join(out, "pred_test.mat"))["preds"], seen.image_path)
    return scene["runs"][key]


def test_the_scene_is_what_it_says(scene):
    pr = import_module(P + ".png_read")
    frames = os.path.join(scene["root"], "frames")
    heads = {}
    for i, kind in enumerate(KINDS[:4]):
        heads[kind] = pr.parse_png(open(os.path.join(frames, "f%02d.png" % i), "rb").read())
    assert [heads[k].color_type for k in KINDS[:4]] == [0, 2, 3, 6] and len(heads["png_rgb"].idat) == 3
    with pytest.raises(pr.UnsupportedPng, match="interlac"):
        pr.parse_png(open(os.path.join(frames, "f04.png"), "rb").read())
    from PIL import Image
    assert np.array_equal(np.array(Image.open(os.path.join(frames, "f04.png")).convert("RGB")), J.content("noise", SIZE[0], SIZE[1], 3, seed=64))


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("rgb", [True, False])
def test_validate_rows_do_not_depend_on_where_the_pngs_are_decoded(scene, rgb, workers):
    want = run(scene, rgb, False, False, 0, 0)
    assert want[0].shape == (len(KINDS), 11, 3) and np.array_equal(want[0], want[1]) and len(want[2]) == len(KINDS)
    for jpeg in (False, True):
        for engine_batch in (0, 8):
            got = run(scene, rgb, jpeg, True, workers, engine_batch)
            assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (jpeg, engine_batch)
            assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]) and got[2] == want[2], (jpeg, engine_batch)
    other = run(scene, not rgb, False, False, 0, 0)
    assert not np.array_equal(other[0], want[0])                          # the channel order reaches the key points: the flag must follow it


@pytest.mark.parametrize("jpeg", [False, True])
def test_the_device_decodes_the_pngs(scene, gpu_ops, monkeypatch, jpeg):
    """not the fallback in disguise: the four PNGs arrive as files and are decoded on the device, the interlaced one neither"""
    fn = import_module(P + ".core.function")
    calls = []
    real = gpu_ops.decode_crop

    def spy(files, *a, **k):
        crops, info = real(files, *a, **k)
        calls.append((len(files), k.get("png"), list(info["png"]), dict(info["fallback"]), list(info["rounds"])))
        return crops, info
    monkeypatch.setattr(fn.ops, "decode_crop", spy)
    scene["runs"].pop((True, jpeg, True, 0, 8), None)
    run(scene, True, jpeg, True, 0, 8)
    # loader batches of 4: [gray, rgb, palette, rgba] and [interlaced, jpeg, bmp]
    assert calls[0] == (4, True, [0, 1, 2, 3], {}, [0, 0, 0, 0])
    if jpeg:                                # the JPEG travels compressed as well; the interlaced PNG and the BMP are windows
        assert len(calls) == 2 and calls[1][0] == 1 and calls[1][2] == [] and not calls[1][3] and calls[1][4][0] >= 1
    else:
        assert len(calls) == 1
    # handed to decode_crop as a file all the same, the interlaced PNG is a fallback row
    frames = os.path.join(scene["root"], "frames")
    files = [open(os.path.join(frames, "f%02d.png" % i), "rb").read() for i in (3, 4)]
    trans = np.tile(np.array([[0.5, 0.0, 0.0], [0.0, 0.5, 0.0]]), (2, 1, 1))
    _, info = real(files, trans, (64, 64), png=True)
    assert info["png"] == [0] and list(info["fallback"]) == [1] and "interlac" in info["fallback"][1]


def test_refusals(scene):
    ds = scene_dataset(scene_config(scene["root"], ["DATASET.DEVICE_DECODE_PNG", "True"]), False)
    ds.numpy_transform = lambda a: a
    with pytest.raises(ValueError, match="cannot be combined with numpy_transform"):
        ds[0]
    ds.numpy_transform = None
    ds.device_crop = False
    with pytest.raises(ValueError, match="needs device_crop"):
        ds[0]
    r = subprocess.run([sys.executable, os.path.join("tools", "test.py"), "--device_decode_png", "--host_crop", "--cfg",
                        os.path.join(ROOT, "landmark_regression", "experiments", "bench", "w32_256.yaml")],
                       cwd=os.path.join(ROOT, "landmark_regression"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--device_decode_png cannot be combined with --host_crop" in r.stderr, r.stderr[-500:]
