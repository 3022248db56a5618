"""dataset.device_decode through validate(): files -> key points with the frames decoded on the device (ops.decode_crop) must give
the rows, the .mat and the image order of the run that decodes them in the loader, bit for bit -- whatever the workers, the
engine batch and COLOR_RGB -- on a scene that holds all three baseline modes, a progressive JPEG and a PNG."""
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

from device_decode_scene import P, ROOT, scene_config, scene_dataset, write_scene
from oracle import hrnet_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(gpu_ops, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("device_decode"))
    write_scene(root)
    models = import_module(P + ".models")
    net = models.pose_hrnet.get_pose_net(scene_config(root), is_train=False)
    net.load_state_dict(R.make_state_dict(R.w32_cfg(11, 64), seed=31), strict=False)
    return {"root": root, "net": net.cuda().eval(), "runs": {}}


class Seen:
    """the data set as validate() sees it, keeping what evaluate() is handed (the data set itself travels to the loader's workers)"""

    def __init__(self, ds):
        self.ds, self.flip_pairs = ds, ds.flip_pairs

    def __len__(self):
        return len(self.ds)

    def evaluate(self, c, preds, output_dir, name, boxes, image_path, *a, **k):
        self.preds, self.image_path = preds.copy(), list(image_path)
        return self.ds.evaluate(c, preds, output_dir, name, boxes, image_path, *a, **k)


def run(scene, rgb, device_decode, workers, engine_batch):
    """one validate() over the scene -> (all_preds, the preds of pred_test.mat, image_path); cached: the reference run is shared"""
    key = (rgb, device_decode, workers, engine_batch)
    if key not in scene["runs"]:
        from scipy.io import loadmat
        fn = import_module(P + ".core.function"); par = import_module(P + ".parallel")
        cfg = scene_config(scene["root"], ["DATASET.COLOR_RGB", str(rgb)])
        assert bool(cfg.DATASET.COLOR_RGB) is rgb
        ds = scene_dataset(cfg, device_decode)
        out = os.path.join(scene["root"], "out_%d_%d_%d_%d" % key)
        os.makedirs(out, exist_ok=True)
        seen = Seen(ds)
        loader = par.valid_loader(ds, 0, len(ds), 1, 4, workers, True)
        fn.validate(cfg, loader, seen, scene["net"], None, out, "", pred_file_name="pred_test", log_metrics=False, engine_batch=engine_batch)
        scene["runs"][key] = (seen.preds, loadmat(os.path.join(out, "pred_test.mat"))["preds"], seen.image_path)
    return scene["runs"][key]


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("rgb", [True, False])
def test_validate_rows_do_not_depend_on_where_the_frames_are_decoded(scene, rgb, workers):
    want = run(scene, rgb, False, 0, 0)
    assert want[0].shape == (10, 11, 3) and np.array_equal(want[0], want[1]) and len(want[2]) == 10
    for device_decode in (True, False):
        for engine_batch in (0, 8):
            got = run(scene, rgb, device_decode, workers, engine_batch)
            assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (device_decode, engine_batch)
            assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]) and got[2] == want[2], (device_decode, engine_batch)
    other = run(scene, not rgb, False, 0, 0)
    assert not np.array_equal(other[0], want[0])                          # the channel order reaches the key points: the flag must follow it


def test_the_device_decodes_what_it_can(scene, gpu_ops, monkeypatch):
    """the run above is not the fallback in disguise: of each loader batch only the progressive JPEG and the PNG arrive as windows"""
    fn = import_module(P + ".core.function")
    calls = []
    real = gpu_ops.decode_crop

    def spy(files, *a, **k):
        crops, info = real(files, *a, **k)
        calls.append((len(files), dict(info["fallback"]), min(info["rounds"])))
        return crops, info
    monkeypatch.setattr(fn.ops, "decode_crop", spy)
    scene["runs"].pop((True, True, 0, 8), None)
    run(scene, True, True, 0, 8)
    assert [c[0] for c in calls] == [3, 3, 2] and all(not c[1] and c[2] >= 1 for c in calls)


def test_numpy_transform_is_refused(scene):
    ds = scene_dataset(scene_config(scene["root"]), True)
    ds.numpy_transform = lambda a: a
    with pytest.raises(ValueError, match="numpy_transform"):
        ds[0]


def test_cli_refuses_device_decode_with_host_crop(scene):
    r = subprocess.run([sys.executable, os.path.join("tools", "test.py"), "--device_decode", "--host_crop", "--cfg",
                        os.path.join(ROOT, "landmark_regression", "experiments", "bench", "w32_256.yaml")],
                       cwd=os.path.join(ROOT, "landmark_regression"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--device_decode cannot be combined with --host_crop" in r.stderr, r.stderr[-500:]


def test_ensemble_loop_and_its_cli_take_the_config_key(scene, tmp_path):
    """validate_cv() over two members with the frames decoded on the device equals the run that decodes them in the loader; and
    tools/test_cv_ensemble.py, which has no flag of its own, reaches the same path through DATASET.DEVICE_DECODE True."""
    from scipy.io import loadmat
    fn = import_module(P + ".core.function"); par = import_module(P + ".parallel"); models = import_module(P + ".models")
    cfg = scene_config(scene["root"])
    other = models.pose_hrnet.get_pose_net(cfg, is_train=False)
    other.load_state_dict(R.make_state_dict(R.w32_cfg(11, 64), seed=32), strict=False)
    nets = [scene["net"], other.cuda().eval()]
    got = {}
    for flag in (False, True):
        ds = scene_dataset(scene_config(scene["root"], ["DATASET.DEVICE_DECODE", str(flag)]), None)
        assert ds.device_decode is flag
        seen = Seen(ds)
        fn.validate_cv(cfg, par.valid_loader(ds, 0, len(ds), 1, 4, 0, True), seen, nets, None, "", "", "pred_real", log_metrics=False, engine_batch=8)
        got[flag] = seen.preds
    assert np.array_equal(got[True].view(np.int32), got[False].view(np.int32)) and got[True].any()
    files = []
    for k, net in enumerate(nets):
        files.append(str(tmp_path / ("member%d.pth" % k)))
        torch.save(net.state_dict(), files[-1])
    r = subprocess.run([sys.executable, os.path.join("tools", "test_cv_ensemble.py"), "--cfg",
                        os.path.join(ROOT, "landmark_regression", "experiments", "bench", "w32_256.yaml"), "DATA_DIR", os.path.join(scene["root"], "frames"),
                        "DATASET.ROOT", os.path.join(scene["root"], "data"), "DATASET.TEST_SET", "test", "MODEL.NUM_JOINTS", "11", "MODEL.IMAGE_SIZE", "[64, 64]",
                        "MODEL.HEATMAP_SIZE", "[16, 16]", "OUTPUT_DIR", str(tmp_path / "o"), "LOG_DIR", str(tmp_path / "l"), "TEST.BATCH_SIZE_PER_GPU", "4",
                        "TEST.MODEL_FILE", files[0], "TEST.MODEL_FILE2", files[1], "DATASET.DEVICE_DECODE", "True"],
                       cwd=os.path.join(ROOT, "landmark_regression"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "decoded on the device" in r.stdout + r.stderr
    preds = loadmat(tmp_path / "o" / "EventsDataset" / "pose_hrnet" / "w32_256" / "pred_real.mat")["preds"]
    assert np.array_equal(preds, got[False])

