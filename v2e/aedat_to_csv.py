#!/usr/bin/env python3
"""The reference's v2e/aedat_to_csv.py on the MI355X HIP path: an AEDAT-4.0 recording (DVXplorer / DV) -> events.csv.

    python v2e/aedat_to_csv.py --events_file REC.aedat4 --output_file OUT.csv

Same name and arguments as the reference script, and the same bytes: one `t,x,y,p` line per event of the file's event streams in
file order, no header line, t in microseconds counted from the first event -- what the reference's pandas
`to_csv(index=False, header=False)` writes.  Nothing loops over events on the host: the file is uploaded once, its LZ4 packets
are decompressed and unpacked on the device (event_read.read_events_aedat4, csrc/events_aedat4_read.hip) and the text is
formatted there too (ops.format_events_text).  ZSTD recordings are decoded on the device too (csrc/events_aedat4_zstd.hip).

An --events_file that ends in .aedat3 (or starts with '#!AER-DAT3.', whatever its name) is an AEDAT-3.1 recording of a DAVIS or
DVS128 camera: the valid events of its polarity packets are unpacked on the device (event_read.read_events_aedat3,
csrc/events_aedat3_read.hip) into the same text.  --width and --height (an extension) give the sensor size in place of the one the
file states or names."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    p = argparse.ArgumentParser(description="Convert an AEDAT-4.0 file to CSV, on the device.")
    p.add_argument("--events_file", type=str, required=True, help="path to the input .aedat4 file, or an AEDAT-3.1 one")
    p.add_argument("--output_file", type=str, required=True, help="path to the output CSV file")
    p.add_argument("--width", type=int, default=None, help="sensor width in pixels, in place of the file's")
    p.add_argument("--height", type=int, default=None, help="sensor height in pixels, in place of the file's")
    args = p.parse_args(argv)
    if (args.width is None) != (args.height is None):
        sys.exit("aedat_to_csv: give --width and --height together, or neither")
    if not os.path.isfile(args.events_file):
        sys.exit("aedat_to_csv: --events_file %s is not a file" % args.events_file)
    import scpose  # noqa: F401
    from importlib import import_module
    er = import_module("spacecraft-pose-estimation_amd.event_read")
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    try:
        # a file that is neither a 4.0 nor a 3.1 recording is handed to the 4.0 reader, which refuses it by its first bytes
        read = er.read_events_file if er.events_format(args.events_file) in ("aedat4", "aedat3") else er.read_events_aedat4
        t, x, y, pol, info = read(args.events_file, hw=None if args.width is None else (args.height, args.width))
    except ValueError as e:
        sys.exit("aedat_to_csv: %s" % e)
    text = ops.format_events_text(t, x, y, pol, sep=",")
    with open(args.output_file, "wb") as f:
        f.write(text.cpu().numpy().tobytes())
    print("aedat_to_csv: %d events of %d packets (%d x %d) -> %d bytes in %s" % (
        info["n_events"], info["n_packets"], info["hw"][1], info["hw"][0], int(text.numel()), args.output_file))
    return 0


if __name__ == "__main__":
    sys.exit(main())
