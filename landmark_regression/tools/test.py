#!/usr/bin/env python3
"""Drop-in for the reference's landmark_regression/tools/test.py (:35-130), on the MI355X HIP path.

    cd landmark_regression
    python tools/test.py --cfg experiments/events/events-config.yaml KEY VAL ...

Same arguments (--cfg, --modelDir, --logDir, --dataDir, --prevModelDir, trailing yacs KEY VAL
overrides), same inputs (<DATASET.ROOT>/<TEST_SET>.json COCO dict, images under DATA_DIR,
TEST.MODEL_FILE state_dict) and same output
(<OUTPUT_DIR>/<DATASET>/<MODEL.NAME>/<cfg basename>/pred_test.mat with 'preds' N x J x 3), so
evaluate_pipeline.py:69-79 can spawn it unchanged.  Multi-GPU: launch with
`python -m torch.distributed.run --nproc-per-node N tools/test.py ...` (one process per GPU,
frames sharded, results all-gathered) instead of cfg.GPUS + DataParallel (:98).
"""
import argparse
import os
import pprint
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.utils.data  # noqa: E402

import scpose  # noqa: E402,F401  (alias of ./spacecraft-pose-estimation_amd)
from importlib import import_module  # noqa: E402

_P = "spacecraft-pose-estimation_amd"
config_mod = import_module(_P + ".config")
models = import_module(_P + ".models")
dataset = import_module(_P + ".dataset")
parallel = import_module(_P + ".parallel")
from_utils = import_module(_P + ".utils.utils")
transforms = import_module(_P + ".utils.transforms")
JointsMSELoss = import_module(_P + ".core.loss").JointsMSELoss
validate = import_module(_P + ".core.function").validate
cfg, update_config = config_mod.cfg, config_mod.update_config


def parse_args():
    parser = argparse.ArgumentParser(description="Train keypoints network")
    parser.add_argument("--cfg", help="experiment configure file name", required=True, type=str)
    parser.add_argument("opts", help="Modify config options using the command-line", default=None, nargs=argparse.REMAINDER)
    parser.add_argument("--modelDir", help="model directory", type=str, default="")
    parser.add_argument("--logDir", help="log directory", type=str, default="")
    parser.add_argument("--dataDir", help="data directory", type=str, default="")
    parser.add_argument("--prevModelDir", help="prev Model directory", type=str, default="")
    parser.add_argument("--device_crop", action="store_true", default=True,
                        help="(extension, the default) warp the crops on the GPU (scpose_crop_warp): the loader only decodes the frames")
    parser.add_argument("--host_crop", dest="device_crop", action="store_false",
                        help="(extension) warp and normalise the crops in the data loader, as the reference does")
    parser.add_argument("--device_decode", action="store_true",
                        help="(extension) decode baseline JPEG frames on the GPU, straight into the crops (ops.decode_crop): the loader only reads "
                             "the files; any other file is decoded by the loader as usual.  Same pred .mat, bit for bit; not with --host_crop.  "
                             "The same as the override DATASET.DEVICE_DECODE True, which tools/test_cv_ensemble.py takes as well")
    parser.add_argument("--device_decode_png", action="store_true",
                        help="(extension) decode PNG frames (8-bit, not interlaced) on the GPU, straight into the crops (ops.decode_crop, png=True): "
                             "the loader only reads the files; any other file is decoded by the loader as usual.  Same pred .mat, bit for bit; "
                             "with or without --device_decode, not with --host_crop.  The same as the override DATASET.DEVICE_DECODE_PNG True")
    parser.add_argument("--no_auto_workers", action="store_true",
                        help="(extension) keep cfg.WORKERS = 0 as 'decode in this process'.  By default a data set of 512 frames or more is decoded by "
                             "min(32, cores / 4) worker processes even when the YAML says WORKERS: 0 (the reference's events-config.yaml does): same "
                             "output, 10-35x the frames/s; smaller sets are not worth the workers' start-up")
    parser.add_argument("--engine_batch", type=int, default=256,
                        help="(extension) frames per engine launch: the loop coalesces the loader's batches (TEST.BATCH_SIZE_PER_GPU, 16 in the "
                             "reference's YAML) into engine batches of this size -- a frame's result does not depend on its batch, bit for bit, so "
                             "the pred .mat is the same; 0 = one launch per loader batch.  Ignored with --log_metrics (loss / PCK are per loader batch)")
    parser.add_argument("--log_metrics", action="store_true",
                        help="(extension) compute the loss / PCK the reference logs per batch; they need the heat-maps, so the forward "
                             "then writes them instead of handing key points out of its last kernel (same pred .mat, bit for bit)")
    args = parser.parse_args()
    if args.device_decode and not args.device_crop:
        parser.error("--device_decode cannot be combined with --host_crop: the device decodes a frame straight into its crop")
    if args.device_decode_png and not args.device_crop:
        parser.error("--device_decode_png cannot be combined with --host_crop: the device decodes a frame straight into its crop")
    return args


def main():
    args = parse_args()
    update_config(cfg, args)
    logger, final_output_dir, tb_log_dir = from_utils.create_logger(cfg, args.cfg, "valid")
    logger.info(pprint.pformat(args))
    logger.info(cfg)

    ws, rank, local = parallel.world()
    if not torch.cuda.is_available():
        raise SystemExit("tools/test.py: no ROCm device visible; the HIP path has no CPU fallback")
    torch.cuda.set_device(local if ws > 1 else int(cfg.GPUS[0]))

    model = getattr(models, cfg.MODEL.NAME).get_pose_net(cfg, is_train=False)
    if cfg.TEST.MODEL_FILE:
        logger.info("=> loading model from {}".format(cfg.TEST.MODEL_FILE))
        model.load_state_dict(torch.load(cfg.TEST.MODEL_FILE, map_location="cpu"), strict=False)
    else:
        model_state_file = os.path.join(final_output_dir, "final_state.pth")
        logger.info("=> loading model from {}".format(model_state_file))
        model.load_state_dict(torch.load(model_state_file, map_location="cpu"))
    model = model.cuda().eval()

    criterion = JointsMSELoss(use_target_weight=cfg.LOSS.USE_TARGET_WEIGHT).cuda()
    normalize = transforms.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
    valid_dataset = getattr(dataset, cfg.DATASET.DATASET)(
        cfg, cfg.DATASET.ROOT, cfg.DATA_DIR, cfg.DATASET.TEST_SET, False,
        transforms.Compose([transforms.ToTensor(), normalize]))
    lo, hi = parallel.shard_range(len(valid_dataset), rank, ws)
    valid_dataset.device_crop = bool(args.device_crop)
    valid_dataset.device_decode = bool(args.device_decode or cfg.DATASET.DEVICE_DECODE)      # the flag, or the config key every CLI takes
    valid_dataset.device_decode_png = bool(args.device_decode_png or cfg.DATASET.DEVICE_DECODE_PNG)
    valid_dataset.want_target = bool(args.log_metrics)     # gaussian targets feed the logged loss / PCK only
    workers = parallel.auto_workers(hi - lo, cfg.WORKERS, keep=args.no_auto_workers)
    if workers != int(cfg.WORKERS):
        logger.info("=> WORKERS: 0 and %d frames: decoding with %d worker processes (--no_auto_workers keeps it in this process)" % (hi - lo, workers))
    # (workers come from a clean fork server, never from this process: it has initialised HIP)
    valid_loader = parallel.valid_loader(valid_dataset, lo, hi, ws, cfg.TEST.BATCH_SIZE_PER_GPU * len(cfg.GPUS), workers, args.device_crop)
    validate(cfg, valid_loader, valid_dataset, model, criterion, final_output_dir, tb_log_dir, pred_file_name="pred_test",
             log_metrics=bool(args.log_metrics), engine_batch=args.engine_batch)


if __name__ == "__main__":
    main()
