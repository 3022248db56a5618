#!/usr/bin/env python3
"""Stage 0 of the reference's event pipeline (v2e/convert_aedats.py) on the MI355X HIP path.

Same four arguments and the same directory contract as the reference script: for every scene directory under --scenes_dir
that holds events.csv (t, x, y, p per line), or an AEDAT-2.0 file events.aedat and no events.csv, it writes
    <scene>/event-frames-distorted/<t>.bmp   the events of each 10 000-tick window as a gray frame (e2v.py --dvs_exposure
                                             duration 10000 --dvs_vid_full_scale 2)
    <scene>/event-frames/<t>.bmp             the same frame after cv2.undistort with the calibration file's camera
as 24-bit BMP files; evaluate_pipeline.py then runs on the result unchanged.  The CSV text is parsed on the device
(csrc/events_csv.hip), and histogram, gray mapping and undistortion run there too (csrc/events.hip); a process that already
holds the file's bytes or the events can skip the files altogether with ops.parse_events_csv and ops.render_events, whose
output ops.crop_warp accepts as is.

Extensions (optional): --no_distorted skips event-frames-distorted/; the CSV flags of e2v.py (--delim_whitespace, --swap_xy,
--microseconds_timestamp, --milliseconds_timestamp); --host_csv reads events.csv with the pandas reader, which is also what a
file outside the device parser's grammar (an exponent, a quoted field, ...) falls back to by itself; a scene's events.aedat
is decoded on the device (csrc/events_aedat2_read.hip) with --image_height x --image_width as the sensor size and --aedat_layout
as the address word, and events.csv wins when both exist; a scene with neither but exactly one *.aedat4 file (an AEDAT-4.0
recording) is rendered from that file, decompressed and unpacked on the device (csrc/events_aedat4_read.hip); failing that, a scene with exactly one AEDAT-3.1
recording (a *.aedat or *.aedat3 file that starts with '#!AER-DAT3.', events.aedat included) is rendered from its polarity packets
(csrc/events_aedat3_read.hip) with --image_height x --image_width as the sensor size.  Not reproduced: the AVI video and
frame-times file e2v.py also writes, AEDAT-3.0, and the frame, IMU and special events of an AEDAT-3.1 recording."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Frames from event files.")
    p.add_argument("--scenes_dir", required=True, type=str, help="directory with one sub-directory per scene, each holding events.csv")
    p.add_argument("--calibration_file_path", required=True, type=str, help="Path to the calibration file")
    p.add_argument("--image_width", type=int, default=640, help="Image width")
    p.add_argument("--image_height", type=int, default=480, help="Image height")
    p.add_argument("--no_distorted", action="store_true", help="do not write event-frames-distorted/")
    p.add_argument("--delim_whitespace", action="store_true", help="events.csv is separated by whitespace instead of commas")
    p.add_argument("--swap_xy", action="store_true", help="the second column of events.csv is y")
    p.add_argument("--microseconds_timestamp", action="store_true", help="divide the time stamps by 1e6 as e2v.py does")
    p.add_argument("--milliseconds_timestamp", action="store_true", help="divide the time stamps by 1e3 as e2v.py does")
    p.add_argument("--host_csv", action="store_true", help="read events.csv with the pandas reader on the host instead of the device parser")
    p.add_argument("--aedat_layout", choices=("davis", "v2e"), default="davis",
                   help="address word of a scene's events.aedat: jAER's DAVIS word, or the word v2e.py --events_aedat2 writes")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import scpose  # noqa: F401
    from importlib import import_module
    er = import_module("spacecraft-pose-estimation_amd.event_render")
    with open(args.calibration_file_path, "r") as f:
        calib = json.load(f)
    K = np.array(calib["intrinsics"]["camera_matrix"], dtype=np.float64)
    dist = np.array(calib["intrinsics"]["distortion_coefficients"], dtype=np.float64).reshape(-1)[:5]
    for scene in sorted(os.listdir(args.scenes_dir)):
        full = os.path.join(args.scenes_dir, scene)
        if os.path.isdir(full) and (os.path.exists(os.path.join(full, "events.csv")) or
                                    os.path.exists(os.path.join(full, "events.aedat")) or er.scene_aedat4(full) is not None or
                                    er.scene_aedat3(full) is not None):
            names = er.render_scene(full, (args.image_height, args.image_width), K=K, dist=dist,
                                    write_distorted=not args.no_distorted, delim_whitespace=args.delim_whitespace,
                                    swap_xy=args.swap_xy, microseconds_timestamp=args.microseconds_timestamp,
                                    milliseconds_timestamp=args.milliseconds_timestamp, host_csv=args.host_csv,
                                    aedat_layout=args.aedat_layout)
            print("%s: %d frames" % (scene, len(names)))


if __name__ == "__main__":
    main()
