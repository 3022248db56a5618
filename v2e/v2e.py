#!/usr/bin/env python3
"""v2e: DVS events from intensity frames, the emulator core of the reference's v2e/v2e.py on the MI355X HIP path.

    python v2e/v2e.py --input DIR --input_frame_rate 100 --dvs_params clean --output_folder OUT --dvs_text events [--events_aedat2 events]

reads the image files of DIR in name order (PIL; grayscale as is, RGB reduced with OpenCV's 8-bit BGR2GRAY weights
(4899 R + 9617 G + 1868 B + 8192) >> 14, which is what the reference's cv2.imread + cvtColor gives), stamps frame k with
k / input_frame_rate seconds, runs the emulator on the device (csrc/dvs_emulator.hip through ops.dvs_emulator) and writes
<output_folder>/<dvs_text>.txt: '#' header lines, then one event per line, `t x y p` separated by single spaces, t in integer
microseconds (the reference's h5 rule uint32(float32(t_s) * 1e6)), p = 1 for ON and 0 for OFF.  That is the grammar both
ops.parse_events_csv(..., delim_whitespace=True) and the reference's e2v.py reader (pandas, comment='#') take.  Two deviations
from the reference's DVSTextOutput, which writes float seconds and the constant polarity 1: integer microseconds survive the
readers' cast to int64, and the real polarity is written.  The text is formatted on the device and streamed to the file
(event_write.write_events_text); write_text below states the same bytes in Python.  --events_aedat2 NAME adds
<output_folder>/<NAME>.aedat, the AEDAT-2.0 file the reference's AEDat2Output writes for jAER (same records, a header without
date and user lines), for the reference's five sensor sizes; e2v.py --aedat_layout v2e reads such a file back (all sizes but
1280x720, whose address word cannot be inverted).

Only the emulator core and these two writers exist here.  SloMo interpolation, video input / output, the h5 writer, the
reference's --dvs_aedat2 and --ddd_output, shot noise and leak jitter do not: their arguments are refused by name, not ignored.
--disable_slomo is accepted (it asks for what happens anyway).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REFUSED = {
    "SloMo interpolation is not part of this emulator (frames are used at --input_frame_rate as they are)":
        ("--slomo_model", "--timestamp_resolution", "--auto_timestamp_resolution", "--batch_size", "--vid_orig", "--vid_slomo",
         "--slomo_stats_plot", "--input_slowmotion_factor"),
    "video files are neither read nor written here (give a directory of image files with --input)":
        ("--start_time", "--stop_time", "--dvs_vid", "--dvs_vid_full_scale", "--dvs_exposure", "--avi_frame_rate", "--crop",
         "--synthetic_input", "--skip_video_output"),
    "the h5 writer is not part of this emulator (use --dvs_text)":
        ("--dvs_h5", "--ddd_output"),
    "the AEDAT-2.0 file is written by --events_aedat2 NAME here":
        ("--dvs_aedat2",),
    "the DVS model state display is not part of this emulator":
        ("--show_dvs_model_state", "--no_preview"),
}


def v2e_args(parser):
    parser.add_argument("--input", "-i", type=str, required=True, help="directory of grayscale or RGB image files, used in name order")
    parser.add_argument("--input_frame_rate", type=float, required=True, help="frames per second of the image sequence")
    parser.add_argument("--pos_thres", type=float, default=0.2, help="ON threshold in log intensity")
    parser.add_argument("--neg_thres", type=float, default=0.2, help="OFF threshold in log intensity")
    parser.add_argument("--sigma_thres", type=float, default=0.03, help="1-sigma per-pixel threshold variation")
    parser.add_argument("--cutoff_hz", type=float, default=0.0, help="photoreceptor low-pass cutoff in Hz (0: off)")
    parser.add_argument("--leak_rate_hz", type=float, default=0.0, help="leak event rate per pixel in Hz (0: off)")
    parser.add_argument("--refractory_period_s", type=float, default=0.0, help="refractory period in seconds (0: off)")
    parser.add_argument("--shot_noise_rate_hz", type=float, default=0.0, help="must be 0: shot noise is not modelled")
    parser.add_argument("--leak_jitter_fraction", type=float, default=0.0, help="must be 0: leak jitter is not modelled")
    parser.add_argument("--noise_rate_cov_decades", type=float, default=0.1, help="spread of the per-pixel leak rates in decades")
    parser.add_argument("--dvs_params", type=str, default=None, help="'clean' overrides the DVS model arguments with the clean set")
    parser.add_argument("--dvs_emulator_seed", type=int, default=0, help="seed of the per-pixel threshold / leak-rate draw (0: unseeded)")
    parser.add_argument("--max_iters", type=int, default=1024, help="most events of one polarity one pixel may emit in one frame")
    parser.add_argument("--disable_slomo", action="store_true", default=False, help="accepted: SloMo never runs here")
    parser.add_argument("--output_folder", "-o", type=str, default=".", help="where the event text file goes")
    parser.add_argument("--dvs_text", type=str, required=True, help="name of the event text file ('.txt' is added when missing)")
    parser.add_argument("--events_aedat2", type=str, default=None,
                        help="name of an AEDAT-2.0 file for jAER ('.aedat' is added when the name has no extension); frames of "
                             "346x260, 692x520, 1280x720, 640x480 or 240x180 only")
    return parser


def refuse_unsupported(argv):
    """Exits with a message when argv names an argument of the reference's v2e.py that has no meaning here."""
    for tok in argv:
        name = tok.split("=", 1)[0]
        for why, names in REFUSED.items():
            if name in names:
                sys.exit("v2e: %s is not supported: %s" % (name, why))


def bgr2gray_u8(rgb):
    """OpenCV's 8-bit RGB -> gray: (4899 R + 9617 G + 1868 B + 8192) >> 14."""
    import numpy as np
    a = rgb.astype(np.int64)
    return ((a[..., 0] * 4899 + a[..., 1] * 9617 + a[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def read_frames(folder):
    """uint8 (F, H, W) of the image files of `folder` in name order."""
    import numpy as np
    from PIL import Image
    names = sorted(n for n in os.listdir(folder) if "." in n and os.path.isfile(os.path.join(folder, n)))
    if not names:
        sys.exit("v2e: no image file in %s" % folder)
    frames = []
    for n in names:
        img = Image.open(os.path.join(folder, n))
        if img.mode in ("1", "P"):
            img = img.convert("RGB")
        if img.mode == "L":
            g = np.asarray(img, dtype=np.uint8)
        elif img.mode in ("RGB", "RGBA"):
            g = bgr2gray_u8(np.asarray(img.convert("RGB"), dtype=np.uint8))
        else:
            sys.exit("v2e: %s has mode %s; only 8-bit grayscale and RGB images are read" % (n, img.mode))
        if frames and g.shape != frames[0].shape:
            sys.exit("v2e: %s is %s, the first frame %s" % (n, g.shape, frames[0].shape))
        frames.append(g)
    return np.stack(frames)


def model_params(args):
    """The emulator's keyword arguments from the command line; --dvs_params clean replaces the model arguments."""
    import scpose  # noqa: F401
    from importlib import import_module
    de = import_module("spacecraft-pose-estimation_amd.dvs_emulator")
    p = dict(pos_thres=args.pos_thres, neg_thres=args.neg_thres, sigma_thres=args.sigma_thres, cutoff_hz=args.cutoff_hz,
             leak_rate_hz=args.leak_rate_hz, leak_jitter_fraction=args.leak_jitter_fraction,
             noise_rate_cov_decades=args.noise_rate_cov_decades, shot_noise_rate_hz=args.shot_noise_rate_hz,
             refractory_period_s=args.refractory_period_s)
    if args.dvs_params is not None:
        p.update(de.dvs_params(args.dvs_params))
    return p


TEXT_HEADER = "#!events.txt\n# DVS events from the device emulator\n# format: time (integer microseconds), x, y, polarity (0=off, 1=on)\n"


def write_text(path, t, x, y, p):
    """The event text file stated in Python, from host columns: the bytes event_write.write_events_text(path, ..., sep=" ",
    header=TEXT_HEADER) makes on the device.  main() does not come through here; tests compare the two."""
    with open(path, "w") as f:
        f.write(TEXT_HEADER)
        for row in zip(t.tolist(), x.tolist(), y.tolist(), p.tolist()):
            f.write("%d %d %d %d\n" % row)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    refuse_unsupported(argv)
    args = v2e_args(argparse.ArgumentParser(description="DVS events from intensity frames, on the device.")).parse_args(argv)
    if args.input_frame_rate <= 0:
        sys.exit("v2e: --input_frame_rate must be > 0")
    if not os.path.isdir(args.input):
        sys.exit("v2e: --input must be a directory of image files (video files are not read)")
    import numpy as np
    import scpose  # noqa: F401
    from importlib import import_module
    de = import_module("spacecraft-pose-estimation_amd.dvs_emulator")
    ew = import_module("spacecraft-pose-estimation_amd.event_write")
    p = model_params(args)
    frames = read_frames(args.input)
    f, h, w = frames.shape
    if args.events_aedat2 is not None:
        try:
            ew.check_aedat2_size((h, w))
        except ValueError as e:
            sys.exit("v2e: --events_aedat2: %s" % e)
    de.validate(h, w, cutoff_hz=p["cutoff_hz"], leak_rate_hz=p["leak_rate_hz"], refractory_period_s=p["refractory_period_s"],
                shot_noise_rate_hz=p["shot_noise_rate_hz"], leak_jitter_fraction=p["leak_jitter_fraction"], max_iters=args.max_iters)
    pos, neg, noise = de.draw_pixel_arrays(h, w, p["pos_thres"], p["neg_thres"], p["sigma_thres"], p["noise_rate_cov_decades"],
                                           p["leak_rate_hz"], args.dvs_emulator_seed)
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    emu = ops.dvs_emulator(h, w, pos_thres=pos, neg_thres=neg, cutoff_hz=p["cutoff_hz"], leak_rate_hz=p["leak_rate_hz"],
                           noise_rate_array=noise, refractory_period_s=p["refractory_period_s"], max_iters=args.max_iters)
    t, x, y, pol, _ = emu.emulate(frames, np.arange(f, dtype=np.float64) / args.input_frame_rate)
    os.makedirs(args.output_folder, exist_ok=True)
    name = args.dvs_text if args.dvs_text.endswith(".txt") else args.dvs_text + ".txt"
    path = os.path.join(args.output_folder, name)
    ew.write_events_text(path, t, x, y, pol, sep=" ", header=TEXT_HEADER.encode())
    print("v2e: %d frames of %d x %d -> %d events (%d ON) in %s" % (f, w, h, int(t.numel()), int(pol.sum().item()), path))
    if args.events_aedat2 is not None:
        name = args.events_aedat2 if os.path.splitext(args.events_aedat2)[1] else args.events_aedat2 + ".aedat"
        path = os.path.join(args.output_folder, name)
        print("v2e: %d AEDAT-2.0 records in %s" % (ew.write_events_aedat2(path, t, x, y, pol, (h, w)), path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
