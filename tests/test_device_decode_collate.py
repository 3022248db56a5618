"""dataset.device_decode on the host: __getitem__ hands out the compressed file for a baseline JPEG and the usual window for any
other file; the collate -> unpack round trip of such a batch is exact and costs two tensors when no row fell back."""
import pickle
from importlib import import_module

import pytest
import torch

from device_decode_scene import P, same, scene_config, scene_dataset, write_scene


def test_items_collate_and_pickle(tmp_path):
    import scpose  # noqa: F401
    par = import_module(P + ".parallel")
    write_scene(str(tmp_path))
    cfg = scene_config(str(tmp_path))
    ds, off = scene_dataset(cfg, True), scene_dataset(cfg, False)
    items, plain_items = [ds[i] for i in range(10)], [off[i] for i in range(10)]
    for i, (a, b) in enumerate(zip(items, plain_items)):
        assert same(a[1:], b[1:]), i                                      # targets, weights and every meta field: those of device_crop
        if i in (3, 7):
            assert a[0].dim() == 3 and torch.equal(a[0], b[0])           # a refused file: the window, as without the flag
        else:
            with open(a[3]["image"], "rb") as fh:
                assert a[0].dim() == 1 and a[0].dtype == torch.uint8 and bytes(a[0].numpy()) == fh.read()
    # rows 0, 1, 2: files only -> two tensors across the process boundary; rows 2 .. 7 hold both refused files -> three
    clean, mixed = items[:3], items[2:8]
    frames = ds.collate_device_crop(clean)[0]
    assert set(frames) == {"files", "file_offsets", "file_rows"} and frames["file_rows"].tolist() == [0, 1, 2]
    packed = ds.collate_device_crop_packed(clean)
    assert sum(torch.is_tensor(v) for v in packed.values()) == 2 and same(ds.collate_device_crop(clean), ds.unpack_device_crop_batch(packed))
    plain = ds.collate_device_crop(mixed)
    frames = plain[0]
    assert frames["file_rows"].tolist() == [0, 2, 3, 4] and frames["window_rows"].tolist() == [1, 5]
    offs = frames["file_offsets"].tolist()
    for k, row in enumerate(frames["file_rows"].tolist()):
        assert torch.equal(frames["files"][offs[k]:offs[k + 1]], mixed[row][0])
    assert same({k: frames[k] for k in ("flat", "offsets", "hw")}, off.collate_device_crop([plain_items[3], plain_items[7]])[0])
    packed = ds.collate_device_crop_packed(mixed)
    assert sum(torch.is_tensor(v) for v in packed.values()) == 3 and same(plain, ds.unpack_device_crop_batch(packed))
    # a batch of refused files only is an ordinary device_crop batch
    assert same(ds.collate_device_crop([items[3], items[7]]), off.collate_device_crop([plain_items[3], plain_items[7]]))
    # the loader the CLIs build: worker processes, packed batches, loader order
    got = list(par.valid_loader(ds, 0, len(ds), 1, 4, 2, True))
    assert len(got) == 3 and all(same(ds.collate_device_crop(items[4 * k:4 * k + 4]), b) for k, b in enumerate(got))
    back = pickle.loads(pickle.dumps(ds))
    assert back.device_decode and back.device_crop and same(back[4], items[4]) and same(back[7], items[7])


def test_flag_needs_device_crop_and_no_numpy_transform(tmp_path):
    import scpose  # noqa: F401
    write_scene(str(tmp_path), n=2)
    # the override every CLI takes (tools/test_cv_ensemble.py has no flag of its own) sets the attribute; it is off by default
    assert scene_dataset(scene_config(str(tmp_path), ["DATASET.DEVICE_DECODE", "True"]), None).device_decode is True
    assert scene_dataset(scene_config(str(tmp_path)), None).device_decode is False
    ds = scene_dataset(scene_config(str(tmp_path)), True)
    ds.numpy_transform = lambda a: a
    with pytest.raises(ValueError, match="numpy_transform"):
        ds[0]
    ds.numpy_transform = None; ds.device_crop = False
    with pytest.raises(ValueError, match="device_crop"):
        ds[0]
