#!/usr/bin/env python3
"""e2v: event frames from a DVS events CSV, the reference's v2e/e2v.py on the MI355X HIP path.

Same arguments and defaults as the reference script.  Every frame the reference's renderer writes lands in
    <output_folder>/event-frames/<t>.bmp        t = '{:.0f}' of the frame time; a later frame with the same stem overwrites
                                                an earlier one, as the reference's imwrite does (frames are written in order)
    <output_folder>/<dvs_vid stem>-frame_times.txt
with all three exposure modes of --dvs_exposure: duration T, count N, area_count M D (event_render.parse_dvs_exposure).  The
CSV parser, the histogram, the gray mapping and the frame ends of the count modes run on the device (csrc/events_csv.hip,
csrc/events.hip, csrc/events_exposure.hip); --host_csv (an extension) reads the file with the pandas reader instead, which is
also the fallback for text outside the device parser's grammar.  An --events_file that ends in .aedat / .aedat2 (or starts with
'#!AER-DAT') is read as AEDAT-2.0 on the device instead (csrc/events_aedat2_read.hip, an extension): the sensor size is
--output_height x --output_width, --aedat_layout picks jAER's DAVIS address word or the one v2e.py --events_aedat2 writes,
--aedat_no_flip_x / --aedat_no_flip_y keep an axis as stored, the two time-stamp flags divide as for a CSV, and the flags that
describe text (--delim_whitespace, --swap_xy, --host_csv) are refused.  An --events_file that ends in .aedat4 (or starts with
'#!AER-DAT4.0') is a DV recording, decompressed and unpacked on the device (csrc/events_aedat4_read.hip): the frame size is the
sensor size the file states unless --output_width and --output_height are both given, and the text flags, the time-stamp
flags and the --aedat_* flags are refused.  An --events_file that ends in .aedat3 (or starts with '#!AER-DAT3.', whatever its
name) is an AEDAT-3.1 recording of a DAVIS or DVS128 camera: its polarity packets are unpacked on the device
(csrc/events_aedat3_read.hip), the frame size is that of the camera the file names unless --output_width and --output_height are
both given, and the same flags are refused.  No undistortion, as in e2v.py.  The AVI video is not written
(there is no video encoder here); --no_preview and --avi_frame_rate are accepted and ignored."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def e2v_args(parser):
    """The arguments of e2v.py.  --aedat_layout, --output_width and --output_height default to None here, so that main() can tell
    whether they were given (an AEDAT-4.0 input states its own layout and size); main() fills in the documented defaults, 'davis',
    1280 and 720, for every other input.  A caller that parses with this helper alone has to do the same."""
    parser.add_argument("--events_file", type=str, help="events CSV, one event per line: t, x, y, p (no header, '#' comments)")
    parser.add_argument("--delim_whitespace", action="store_true", default=False,
                        help="the CSV columns are separated by whitespace, not commas")
    parser.add_argument("--swap_xy", action="store_true", default=False, help="the second CSV column is y and the third x")
    parser.add_argument("--microseconds_timestamp", action="store_true", default=False,
                        help="divide the time stamps by 1e6 (int64, truncated) before rendering")
    parser.add_argument("--milliseconds_timestamp", action="store_true", default=False,
                        help="divide the time stamps by 1e3 (int64, truncated) before rendering")
    parser.add_argument("--host_csv", action="store_true", default=False,
                        help="read the CSV with the pandas reader on the host instead of the device parser")
    parser.add_argument("--aedat_layout", choices=("davis", "v2e"), default=None,
                        help="address word of an AEDAT-2.0 --events_file: jAER's DAVIS word (the default), or the word v2e.py "
                             "--events_aedat2 writes")
    parser.add_argument("--aedat_no_flip_x", action="store_true", default=False,
                        help="AEDAT-2.0 input: keep x as stored instead of undoing the writers' flip")
    parser.add_argument("--aedat_no_flip_y", action="store_true", default=False,
                        help="AEDAT-2.0 input: keep y as stored instead of undoing the writers' flip")
    parser.add_argument("--avi_frame_rate", type=int, default=30, help="accepted and ignored: no AVI is written")
    parser.add_argument("--dvs_vid", type=str, default="dvs-video.avi",
                        help="name the frame-times file is derived from (<stem>-frame_times.txt); no AVI is written")
    parser.add_argument("--dvs_vid_full_scale", type=int, default=2,
                        help="events per pixel that map to full white")
    parser.add_argument("--no_preview", action="store_true", default=False, help="accepted and ignored: there is no preview")
    parser.add_argument("--dvs_exposure", nargs="+", type=str, default=["duration", "0.01"],
                        help="Mode to finish DVS frame event integration: duration T (ticks of the time column), "
                             "count N (N events per frame), area_count M D (the frame ends when any D x D pixel area "
                             "has received M events)")
    parser.add_argument("--output_folder", type=str, default=".", help="where event-frames/ and the frame-times file go")
    parser.add_argument("--output_width", type=int, default=None,
                        help="frame width in pixels (default 1280; for an AEDAT-4.0 or AEDAT-3.1 input, the sensor width the file states or names)")
    parser.add_argument("--output_height", type=int, default=None,
                        help="frame height in pixels (default 720; for an AEDAT-4.0 or AEDAT-3.1 input, the sensor height the file states or names)")
    return parser


# event_read.EVENT_FORMATS, restated so that the sniffing works before the package is imported (tests/test_events_aedat3.py holds
# the two tables equal): (key, name suffixes, first bytes), tested in this order
EVENT_FORMATS = (("aedat4", (".aedat4",), b"#!AER-DAT4.0\r\n"),
                 ("aedat3", (".aedat3",), b"#!AER-DAT3."),
                 ("aedat2", (".aedat", ".aedat2"), b"#!AER-DAT"))


def _sniff(path, suffixes, magic):
    if path is None:
        return False
    if path.lower().endswith(suffixes):
        return True
    try:
        with open(path, "rb") as f:
            return f.read(len(magic)) == magic
    except OSError:
        return False


def events_format(path):
    """event_read.events_format, without importing the package: 'aedat4', 'aedat3', 'aedat2' or None (text, no path)."""
    return next((key for key, suffixes, magic in EVENT_FORMATS if _sniff(path, suffixes, magic)), None)


def is_aedat3(path):
    """event_read.is_aedat3_path, without the package."""
    return _sniff(path, *EVENT_FORMATS[1][1:])


def main(argv=None):
    args = e2v_args(argparse.ArgumentParser(description="Event frames from an events CSV, on the device.")).parse_args(argv)
    fmt = events_format(args.events_file)
    aedat4, aedat3, aedat = fmt == "aedat4", fmt == "aedat3", fmt is not None
    version = "AEDAT-4.0" if aedat4 else "AEDAT-3.1"
    if aedat4 or aedat3:
        for flag in ("delim_whitespace", "swap_xy", "host_csv", "microseconds_timestamp", "milliseconds_timestamp", "aedat_layout",
                     "aedat_no_flip_x", "aedat_no_flip_y"):
            if getattr(args, flag):
                sys.exit("e2v: --%s cannot be used with the %s input %s: the file states its own layout, and its time "
                         "stamps are microseconds" % (flag, version, args.events_file))
        if (args.output_width is None) != (args.output_height is None):
            sys.exit("e2v: give --output_width and --output_height together, or neither (the %s file states its sensor%s)"
                     % (version, " size" if aedat4 else ", and a known camera's size is taken from its name"))
    else:
        args.output_width = 1280 if args.output_width is None else args.output_width
        args.output_height = 720 if args.output_height is None else args.output_height
    args.aedat_layout = args.aedat_layout or "davis"
    if aedat and not (aedat4 or aedat3):
        for flag in ("delim_whitespace", "swap_xy", "host_csv"):
            if getattr(args, flag):
                sys.exit("e2v: --%s describes a text file and cannot be used with the AEDAT-2.0 input %s" % (flag, args.events_file))
    import torch
    import scpose  # noqa: F401
    from importlib import import_module
    er = import_module("spacecraft-pose-estimation_amd.event_render")
    mode, value, dim = er.parse_dvs_exposure(args.dvs_exposure)
    kw = er.exposure_kwargs(mode, value, dim)
    print("e2v: the AVI video (%s) is not written: no video encoder is available; frames go to %s" %
          (args.dvs_vid, os.path.join(args.output_folder, "event-frames")), file=sys.stderr)
    out_dir = os.path.join(args.output_folder, "event-frames")
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    h, w = args.output_height, args.output_width
    try:
        if aedat4 or aedat3:
            rd = import_module("spacecraft-pose-estimation_amd.event_read")
            t, x, y, _, info = rd.read_events_file(args.events_file, hw=None if h is None else (h, w), device=dev)
            h, w = info["hw"]
            if info["n_backward"] > 0:
                raise ValueError("the event stream must be sorted by time")
        else:
            t, x, y = er.read_events_device(args.events_file, dev, host_csv=args.host_csv, hw=(h, w), aedat_layout=args.aedat_layout,
                                            aedat_flip_x=not args.aedat_no_flip_x, aedat_flip_y=not args.aedat_no_flip_y,
                                            delim_whitespace=args.delim_whitespace, swap_xy=args.swap_xy,
                                            microseconds_timestamp=args.microseconds_timestamp,
                                            milliseconds_timestamp=args.milliseconds_timestamp)
    except ValueError as e:
        if not aedat:
            raise
        sys.exit("e2v: %s" % e)
    names = er.write_event_frames(args.output_folder, args.dvs_vid, t, x, y, (h, w), full_scale=args.dvs_vid_full_scale, **kw)
    print("e2v: %d frames (%s)" % (len(names), " ".join(args.dvs_exposure)))


if __name__ == "__main__":
    main()
