#!/usr/bin/env python3
"""events_convert: an event text / CSV / AEDAT-2.0 file into another event file, on the device.

    python v2e/events_convert.py --events_file IN [--delim_whitespace] [--swap_xy] --output OUT [--width W --height H]
                                 [--aedat_layout {davis,v2e}] [--aedat4_compression {lz4,none}]

IN is read by ops.parse_events_csv (csrc/events_csv.hip; --delim_whitespace and --swap_xy are e2v.py's flags of the same
names) and the four columns go straight to one of the device writers (event_write), chosen by OUT's extension, without a host
copy of the columns:
    .csv     `t,x,y,p` lines without a header: what the reference's aedat_to_csv.py writes (to_csv(index=False, header=False))
             and convert_aedats.py reads
    .txt     `t x y p` lines without a header: the --delim_whitespace grammar
    .aedat   AEDAT-2.0 for jAER; needs --width and --height, one of 346x260, 692x520, 1280x720, 640x480, 240x180, and time
             stamps in microseconds
    .aedat4  AEDAT-4.0 for DV and dv-processing (event_write.write_events_aedat4, csrc/events_aedat4_write.hip): any sensor
             size up to 32767 x 32767; needs --width and --height unless IN is an .aedat4 or .aedat3 file, which states its
             sensor size; time stamps in microseconds, written as given; --aedat4_compression picks LZ4 packets (the default,
             what DV writes) or raw ones
The text forms write x before y whatever --swap_xy says: the flag describes IN.

An IN that ends in .aedat / .aedat2 is an AEDAT-2.0 file and is read by event_read.read_events_aedat2
(csrc/events_aedat2_read.hip): it needs --width and --height, the sensor size, and --aedat_layout names its address word (jAER's
DAVIS word, the default, or the word this tool and v2e.py --events_aedat2 write); the two text flags are refused.  An IN that
ends in .aedat4 (or starts with the AEDAT-4.0 version line) is a DV recording and is read by event_read.read_events_aedat4
(csrc/events_aedat4_read.hip): the sensor size comes from the file unless --width and --height say otherwise, and the text flags
and --aedat_layout are refused.  An IN that ends in .aedat3 (or starts with '#!AER-DAT3.', whatever its name) is an AEDAT-3.1
recording and is read by event_read.read_events_aedat3 (csrc/events_aedat3_read.hip) under the same rules: the sensor size is
that of the camera the file names unless --width and --height say otherwise.  With a .csv or
.txt OUT this is the device counterpart of the reference's aedat_to_csv.py for AEDAT-2.0 files.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FORMATS = (".csv", ".txt", ".aedat", ".aedat4")


def convert_args(parser):
    """The arguments of events_convert.py.  --aedat_layout defaults to None here so that main() can refuse it for an AEDAT-4.0
    input; main() fills in the documented default, 'davis', for every other input.  A caller that parses with this helper alone
    has to do the same."""
    parser.add_argument("--events_file", type=str, required=True, help="event text file: t, x, y, p per line, '#' comments")
    parser.add_argument("--delim_whitespace", action="store_true", default=False, help="fields are separated by blanks, not commas")
    parser.add_argument("--swap_xy", action="store_true", default=False, help="the second column of the input is y, the third x")
    parser.add_argument("--output", type=str, required=True, help="file to write; the extension picks the format: %s" % ", ".join(FORMATS))
    parser.add_argument("--width", type=int, default=None, help="sensor width in pixels (.aedat / .aedat4 input or output only)")
    parser.add_argument("--height", type=int, default=None, help="sensor height in pixels (.aedat / .aedat4 input or output only)")
    parser.add_argument("--aedat_layout", choices=("davis", "v2e"), default=None,
                        help="address word of an .aedat input: jAER's DAVIS word (the default), or the word the .aedat output here has")
    parser.add_argument("--aedat4_compression", choices=("lz4", "none"), default="lz4",
                        help="packets of an .aedat4 output: LZ4 frames (the default, what DV writes) or raw flatbuffers")
    return parser


def main(argv=None):
    args = convert_args(argparse.ArgumentParser(description="Convert an event text file on the device.")).parse_args(argv)
    ext = os.path.splitext(args.output)[1].lower()
    if ext not in FORMATS:
        sys.exit("events_convert: --output %s: the extension must be one of %s" % (args.output, ", ".join(FORMATS)))
    if ext == ".aedat" and (args.width is None or args.height is None):
        sys.exit("events_convert: an .aedat output needs --width and --height")
    import scpose  # noqa: F401
    from importlib import import_module
    er = import_module("spacecraft-pose-estimation_amd.event_read")
    fmt = er.events_format(args.events_file)
    aedat4_in, aedat3_in = fmt == "aedat4", fmt == "aedat3"
    version = "AEDAT-4.0" if aedat4_in else "AEDAT-3.1"
    if (aedat4_in or aedat3_in) and (args.delim_whitespace or args.swap_xy or args.aedat_layout):
        sys.exit("events_convert: --delim_whitespace, --swap_xy and --aedat_layout cannot be used with the %s input %s"
                 % (version, args.events_file))
    if (aedat4_in or aedat3_in) and (args.width is None) != (args.height is None):
        sys.exit("events_convert: give --width and --height together, or neither (the %s file states its sensor%s)"
                 % (version, " size" if aedat4_in else ", and a known camera's size is taken from its name"))
    args.aedat_layout = args.aedat_layout or "davis"
    aedat_in = fmt == "aedat2" and args.events_file.lower().endswith((".aedat", ".aedat2"))     # by its name alone, as ever
    if aedat_in and (args.width is None or args.height is None):
        sys.exit("events_convert: an .aedat input needs --width and --height, the sensor size")
    if aedat_in and (args.delim_whitespace or args.swap_xy):
        sys.exit("events_convert: --delim_whitespace and --swap_xy describe a text file and cannot be used with the AEDAT-2.0 "
                 "input %s" % args.events_file)
    if ext == ".aedat4" and not (aedat4_in or aedat3_in) and (args.width is None or args.height is None):
        sys.exit("events_convert: an .aedat4 output needs --width and --height, the sensor size, unless the input states it")
    if not os.path.isfile(args.events_file):
        sys.exit("events_convert: --events_file %s is not a file" % args.events_file)
    ew = import_module("spacecraft-pose-estimation_amd.event_write")
    if ext == ".aedat":
        try:
            ew.check_aedat2_size((args.height, args.width))
        except ValueError as e:
            sys.exit("events_convert: %s" % e)
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    if aedat4_in or aedat3_in or aedat_in:
        hw = None if args.width is None else (args.height, args.width)
        try:
            t, x, y, p, info = er.read_events_file(args.events_file, hw, **({"layout": args.aedat_layout} if aedat_in else {}))
        except ValueError as e:
            sys.exit("events_convert: %s" % e)
        item = "%s=%d" if aedat_in else "%s=%s"
        print("events_convert: %s: %s" % (args.events_file, ", ".join(item % kv for kv in sorted(info.items()))))
    else:
        t, x, y, p = ops.parse_events_csv(args.events_file, delim_whitespace=args.delim_whitespace, swap_xy=args.swap_xy)
    if ext == ".aedat":
        try:
            n = ew.write_events_aedat2(args.output, t, x, y, p, (args.height, args.width))
        except ValueError as e:
            sys.exit("events_convert: %s" % e)
        print("events_convert: %d events -> %d AEDAT-2.0 records in %s" % (int(t.numel()), n, args.output))
    elif ext == ".aedat4":
        hw = (args.height, args.width) if args.width is not None else info["hw"]
        try:
            n = ew.write_events_aedat4(args.output, t, x, y, p, hw, compression=args.aedat4_compression)
        except ValueError as e:
            sys.exit("events_convert: %s" % e)
        print("events_convert: %d events -> %d AEDAT-4.0 packets (%s) in %s" % (int(t.numel()), n, args.aedat4_compression, args.output))
    else:
        n = ew.write_events_text(args.output, t, x, y, p, sep="," if ext == ".csv" else " ")
        print("events_convert: %d events -> %d bytes in %s" % (int(t.numel()), n, args.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
