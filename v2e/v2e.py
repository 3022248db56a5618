#!/usr/bin/env python3
"""v2e: DVS events from intensity frames, the emulator core of the reference's v2e/v2e.py on the MI355X HIP path.

    python v2e/v2e.py --input DIR --input_frame_rate 100 --dvs_params clean --output_folder OUT --dvs_text events [--events_aedat2 events]
                      [--events_aedat4 events] [--output_width W --output_height H] [--dvs_exposure duration 0.2] [--device_decode]

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
1280x720, whose address word cannot be inverted).  --events_aedat4 NAME adds <output_folder>/<NAME>.aedat4, the AEDAT-4.0 file
that DV and dv-processing open (event_write.write_events_aedat4: LZ4 packets of 10 000 events made on the device, a file data
table), at any sensor size, 1280x720 included; e2v.py, aedat_to_csv.py and events_convert.py read it back.

Frames of another size than the sensor: --output_width W --output_height H (both or neither) resizes every frame on the device
before the emulator sees it (csrc/resize_area.hip through ops.resize_area: cv2.resize's INTER_AREA on the three channels, then the
gray rule above, in the reference's order), and the emulator, the AEDAT-2.0 writer and the renderer work at H x W.  Frames smaller
than the sensor on either axis are refused.  --device_decode hands the files' bytes to the device decoders (ops.decode_jpeg /
ops.decode_png, chosen per file by image_read.sniff; what neither takes -- BMP, progressive JPEG -- is decoded by PIL and uploaded),
so the pixels go from the compressed bytes to the event columns without coming back to the host.  Frames run through in batches of
at most 256 MiB of decoded pixels: decode -> resize -> emulate, the emulator's state carried from batch to batch.

--dvs_exposure MODE ... (duration T | count N | area_count M D, parsed by event_render.parse_dvs_exposure as in e2v.py) renders the
whole event stream after the last frame into <output_folder>/event-frames/<stem>.bmp and <output_folder>/dvs-video-frame_times.txt
(the reference's default --dvs_vid stem; --dvs_vid itself stays refused), through the function e2v.py writes its frames with:
the result is what e2v.py --delim_whitespace --dvs_exposure ... gives on the text file of the same run.  T is in SECONDS here, as
in the reference's v2e (T * 1e6 ticks of the microsecond stream); e2v.py takes ticks.  Two deviations from the reference's v2e
renderer: the reference feeds its renderer one packet of events per input frame and so drops the last event of every packet, while
the whole stream is rendered once here; and the reference formats the stems from seconds, so that most frames of a run overwrite
each other, while the stems here are e2v.py's, formatted from microseconds.  --skip_video_output turns the rendering off;
--avi_frame_rate is accepted and no AVI is written; --overwrite is accepted and does nothing, the output is always overwritten.

SloMo interpolation, video input / output, the h5 writer, the reference's --dvs_aedat2 and --ddd_output, shot noise and leak jitter
do not exist here: their arguments are refused by name, not ignored.  --disable_slomo is accepted (it asks for what happens anyway).
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
        ("--start_time", "--stop_time", "--dvs_vid", "--dvs_vid_full_scale", "--crop", "--synthetic_input"),
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
    parser.add_argument("--events_aedat4", type=str, default=None,
                        help="name of an AEDAT-4.0 file for DV ('.aedat4' is added when the name has no extension); any frame size")
    parser.add_argument("--output_width", type=int, default=None, help="sensor width; frames of another size are area-resized on the device")
    parser.add_argument("--output_height", type=int, default=None, help="sensor height (give both or neither)")
    parser.add_argument("--dvs_exposure", nargs="+", type=str, default=None,
                        help="render event frames after the last frame: duration T (seconds), count N, or area_count M D")
    parser.add_argument("--avi_frame_rate", type=int, default=None, help="accepted: no AVI is written")
    parser.add_argument("--skip_video_output", action="store_true", default=False, help="accepted: turns the --dvs_exposure output off")
    parser.add_argument("--overwrite", action="store_true", default=False, help="accepted: the output is always overwritten")
    parser.add_argument("--device_decode", action="store_true", default=False,
                        help="decode JPEG and PNG files on the device instead of with PIL on the host")
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


def frame_names(folder):
    """The image files of `folder` in name order; exits when there is none"""
    names = sorted(n for n in os.listdir(folder) if "." in n and os.path.isfile(os.path.join(folder, n)))
    if not names:
        sys.exit("v2e: no image file in %s" % folder)
    return names


def read_frames(folder, names=None, rgb=False):
    """uint8 (F, H, W) gray frames of the image files of `folder` in name order (names: these files only); rgb: (F, H, W, 3) instead,
    a grayscale file repeated into the three channels -- what the resize takes, which reduces to gray after it."""
    import numpy as np
    from PIL import Image
    names = frame_names(folder) if names is None else names
    frames = []
    for n in names:
        img = Image.open(os.path.join(folder, n))
        if img.mode in ("1", "P"):
            img = img.convert("RGB")
        if img.mode == "L":
            g = np.asarray(img, dtype=np.uint8)
            g = np.repeat(g[..., None], 3, axis=2) if rgb else g
        elif img.mode in ("RGB", "RGBA"):
            g = np.asarray(img.convert("RGB"), dtype=np.uint8)
            g = g if rgb else bgr2gray_u8(g)
        else:
            sys.exit("v2e: %s has mode %s; only 8-bit grayscale and RGB images are read" % (n, img.mode))
        if frames and g.shape != frames[0].shape:
            sys.exit("v2e: %s is %s, the first frame %s" % (n, g.shape, frames[0].shape))
        frames.append(g)
    return np.stack(frames)


def decode_frames_device(paths, device=None):
    """(N, H, W, 3) uint8 RGB frames on the device from image files: each file goes to the device decoder image_read.sniff names
    (ops.decode_jpeg, ops.decode_png); a file neither takes is decoded by PIL inside those calls (fallback=True)."""
    import torch
    from importlib import import_module
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    image_read = import_module("spacecraft-pose-estimation_amd.image_read")
    blobs = []
    for p in paths:
        with open(p, "rb") as f:
            blobs.append(f.read())
    groups = {"jpeg": [], "png": []}
    for i, b in enumerate(blobs):
        kind = image_read.sniff(b, jpeg=True, png=True)[0]
        groups[kind or ("png" if image_read.is_png(b) else "jpeg")].append(i)
    parts = [(idx, (ops.decode_jpeg if kind == "jpeg" else ops.decode_png)([blobs[i] for i in idx], rgb=True, device=device, fallback=True)[0])
             for kind, idx in groups.items() if idx]
    if len(parts) == 1:
        return parts[0][1]
    if len({tuple(fr.shape[1:]) for _, fr in parts}) != 1:
        raise ValueError("the frames have different sizes %s" % sorted({tuple(fr.shape[1:3]) for _, fr in parts}))
    out = torch.empty((len(blobs),) + tuple(parts[0][1].shape[1:]), dtype=torch.uint8, device=parts[0][1].device)
    for idx, fr in parts:
        out.index_copy_(0, torch.tensor(idx, dtype=torch.int64, device=out.device), fr)
    return out


BATCH_BYTES = 256 << 20          # decoded pixels of one batch, at most


def batch_ranges(n_frames, frame_bytes, max_batch_frames=None):
    """[(k0, k1)] that cover the frames in order: as many frames as BATCH_BYTES of decoded pixels hold (and max_batch_frames allows),
    never none"""
    per = max(1, BATCH_BYTES // max(1, frame_bytes))
    if max_batch_frames is not None:
        per = max(1, min(per, int(max_batch_frames)))
    return [(k0, min(k0 + per, n_frames)) for k0 in range(0, n_frames, per)]


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


DVS_VID = "dvs-video.avi"          # the reference's default --dvs_vid: names the frame-times file
TEXT_HEADER = "#!events.txt\n# DVS events from the device emulator\n# format: time (integer microseconds), x, y, polarity (0=off, 1=on)\n"


def write_text(path, t, x, y, p):
    """The event text file stated in Python, from host columns: the bytes event_write.write_events_text(path, ..., sep=" ",
    header=TEXT_HEADER) makes on the device.  main() does not come through here; tests compare the two."""
    with open(path, "w") as f:
        f.write(TEXT_HEADER)
        for row in zip(t.tolist(), x.tolist(), y.tolist(), p.tolist()):
            f.write("%d %d %d %d\n" % row)


def main(argv=None, max_batch_frames=None):
    """max_batch_frames: fewer frames per batch than BATCH_BYTES allows (tests force several batches on a short sequence)"""
    argv = list(sys.argv[1:] if argv is None else argv)
    refuse_unsupported(argv)
    args = v2e_args(argparse.ArgumentParser(description="DVS events from intensity frames, on the device.")).parse_args(argv)
    if args.input_frame_rate <= 0:
        sys.exit("v2e: --input_frame_rate must be > 0")
    if not os.path.isdir(args.input):
        sys.exit("v2e: --input must be a directory of image files (video files are not read)")
    if (args.output_width is None) != (args.output_height is None):
        sys.exit("v2e: give --output_width and --output_height together, or neither (the frames' own size)")
    if args.output_width is not None and (args.output_width < 1 or args.output_height < 1):
        sys.exit("v2e: --output_width and --output_height must be >= 1")
    import scpose  # noqa: F401
    from importlib import import_module
    er = import_module("spacecraft-pose-estimation_amd.event_render")
    exposure = None
    if args.dvs_exposure is not None:
        try:
            mode, value, dim = er.parse_dvs_exposure(args.dvs_exposure)
            exposure = er.exposure_kwargs(mode, value * 1e6 if mode == "duration" else value, dim)    # duration: seconds -> ticks
        except ValueError as e:
            sys.exit("v2e: --dvs_exposure: %s" % e)
    p = model_params(args)
    names = frame_names(args.input)
    from PIL import Image
    with Image.open(os.path.join(args.input, names[0])) as first:
        src_w, src_h = first.size
    h, w = (src_h, src_w) if args.output_width is None else (args.output_height, args.output_width)
    if h > src_h or w > src_w:
        sys.exit("v2e: the frames are %d x %d (W x H), smaller than the sensor of %d x %d on an axis: frames are only ever shrunk"
                 % (src_w, src_h, w, h))
    resize = (h, w) != (src_h, src_w)
    import numpy as np
    de = import_module("spacecraft-pose-estimation_amd.dvs_emulator")
    ew = import_module("spacecraft-pose-estimation_amd.event_write")
    f = len(names)
    if args.events_aedat2 is not None:
        try:
            ew.check_aedat2_size((h, w))
        except ValueError as e:
            sys.exit("v2e: --events_aedat2: %s" % e)
    de.validate(h, w, cutoff_hz=p["cutoff_hz"], leak_rate_hz=p["leak_rate_hz"], refractory_period_s=p["refractory_period_s"],
                shot_noise_rate_hz=p["shot_noise_rate_hz"], leak_jitter_fraction=p["leak_jitter_fraction"], max_iters=args.max_iters)
    pos, neg, noise = de.draw_pixel_arrays(h, w, p["pos_thres"], p["neg_thres"], p["sigma_thres"], p["noise_rate_cov_decades"],
                                           p["leak_rate_hz"], args.dvs_emulator_seed)
    import torch
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    emu = ops.dvs_emulator(h, w, pos_thres=pos, neg_thres=neg, cutoff_hz=p["cutoff_hz"], leak_rate_hz=p["leak_rate_hz"],
                           noise_rate_array=noise, refractory_period_s=p["refractory_period_s"], max_iters=args.max_iters)
    stamps = np.arange(f, dtype=np.float64) / args.input_frame_rate
    rgb = args.device_decode or resize                           # decoded pixels per frame: three channels, or gray read by PIL
    cols = []
    for k0, k1 in batch_ranges(f, src_h * src_w * (3 if rgb else 1), max_batch_frames):
        if args.device_decode:
            try:
                frames = decode_frames_device([os.path.join(args.input, n) for n in names[k0:k1]])
            except ValueError as e:
                sys.exit("v2e: %s .. %s: %s" % (names[k0], names[k1 - 1], e))
        else:
            frames = read_frames(args.input, names[k0:k1], rgb=resize)
        if tuple(frames.shape[1:3]) != (src_h, src_w):
            sys.exit("v2e: %s .. %s are %d x %d (W x H), the first frame %d x %d" % (names[k0], names[k1 - 1], frames.shape[2], frames.shape[1],
                                                                                 src_w, src_h))
        if rgb:
            frames = ops.resize_area(frames, (h, w), gray=True)  # the input's own size: gray only
        cols.append(emu.emulate(frames, stamps[k0:k1])[:4])
        del frames
    t, x, y, pol = (torch.cat([c[j] for c in cols]) for j in range(4))
    os.makedirs(args.output_folder, exist_ok=True)
    name = args.dvs_text if args.dvs_text.endswith(".txt") else args.dvs_text + ".txt"
    path = os.path.join(args.output_folder, name)
    ew.write_events_text(path, t, x, y, pol, sep=" ", header=TEXT_HEADER.encode())
    print("v2e: %d frames of %d x %d -> %d events (%d ON) in %s" % (f, w, h, int(t.numel()), int(pol.sum().item()), path))
    if args.events_aedat2 is not None:
        name = args.events_aedat2 if os.path.splitext(args.events_aedat2)[1] else args.events_aedat2 + ".aedat"
        path = os.path.join(args.output_folder, name)
        print("v2e: %d AEDAT-2.0 records in %s" % (ew.write_events_aedat2(path, t, x, y, pol, (h, w)), path))
    if args.events_aedat4 is not None:
        name = args.events_aedat4 if os.path.splitext(args.events_aedat4)[1] else args.events_aedat4 + ".aedat4"
        path = os.path.join(args.output_folder, name)
        print("v2e: %d AEDAT-4.0 packets in %s" % (ew.write_events_aedat4(path, t, x, y, pol, (h, w)), path))
    if args.avi_frame_rate is not None:
        print("v2e: no AVI is written (--avi_frame_rate %d): there is no video encoder here" % args.avi_frame_rate, file=sys.stderr)
    if exposure is not None and not args.skip_video_output:
        stems = er.write_event_frames(args.output_folder, DVS_VID, t, x, y, (h, w), full_scale=2, **exposure)
        print("v2e: %d event frames (%s) in %s" % (len(stems), " ".join(args.dvs_exposure), os.path.join(args.output_folder, "event-frames")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
