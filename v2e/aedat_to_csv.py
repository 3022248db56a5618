#!/usr/bin/env python3
"""The reference's v2e/aedat_to_csv.py on the MI355X HIP path: an AEDAT-4.0 recording (DVXplorer / DV) -> events.csv.

    python v2e/aedat_to_csv.py --events_file REC.aedat4 --output_file OUT.csv

Same name and arguments as the reference script, and the same bytes: one `t,x,y,p` line per event of the file's event streams in
file order, no header line, t in microseconds counted from the first event -- what the reference's pandas
`to_csv(index=False, header=False)` writes.  Nothing loops over events on the host: the file is uploaded once, its LZ4 packets
are decompressed and unpacked on the device (event_read.read_events_aedat4, csrc/events_aedat4_read.hip) and the text is
formatted there too (ops.format_events_text).  ZSTD recordings are refused by name."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    p = argparse.ArgumentParser(description="Convert an AEDAT-4.0 file to CSV, on the device.")
    p.add_argument("--events_file", type=str, required=True, help="path to the input .aedat4 file")
    p.add_argument("--output_file", type=str, required=True, help="path to the output CSV file")
    args = p.parse_args(argv)
    if not os.path.isfile(args.events_file):
        sys.exit("aedat_to_csv: --events_file %s is not a file" % args.events_file)
    import scpose  # noqa: F401
    from importlib import import_module
    er = import_module("spacecraft-pose-estimation_amd.event_read")
    ops = import_module("spacecraft-pose-estimation_amd.ops")
    try:
        t, x, y, pol, info = er.read_events_aedat4(args.events_file)
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
