"""Event stream -> event frames: the host side of stage 0 of the reference's event pipeline.

The reference's entry script first runs v2e/convert_aedats.py: `e2v.py --dvs_exposure duration 10000 --dvs_vid_full_scale 2`
on every scene's events.csv (t, x, y, p per line) histograms the events of each 10 000-tick window into a frame
(v2e/v2ecore/renderer.py: render_events_to_frames), writes event-frames-distorted/<t>.bmp, and cv2.undistort turns every frame
into event-frames/<t>.bmp.  Here the CSV text is parsed (csrc/events_csv.hip, ops.parse_events_csv) and the histogram, the gray
mapping and the undistortion are computed (csrc/events.hip, ops.render_events) by HIP kernels; this module holds what stays on
the host: the frame schedule (a handful of float64 additions), the pandas reader the device parser falls back to for text
outside its grammar (read_events_csv, also the oracle of the device parser), and the scene driver that the CLI
v2e/convert_aedats.py calls."""
import os

import numpy as np

MAX_EXACT_TICK = 2 ** 53      # int64 ticks are compared as float64 (as the reference's searchsorted does): exact below 2^53


def gray_table(full_scale):
    """uint8 (2 * fs + 1,): the gray value of the clipped count c = -fs ... fs, the reference's
    (img * 255).astype(np.uint8) with img = (c + fs) / float(2 * fs) (renderer.py: normalize_frame), float64, truncated.
    fs = 2: 0, 63, 127, 191, 255."""
    fs = int(full_scale)
    if fs < 1:
        raise ValueError("full_scale must be >= 1 (got %d)" % fs)
    c = np.arange(-fs, fs + 1, dtype=np.float64)
    return (((c + fs) / float(fs * 2)) * 255).astype(np.uint8)


def frame_schedule(t_first, t_before_last, t_last, interval, max_frames=None):
    """The frames the reference's renderer writes for a time-sorted stream (DURATION mode), from three of its stamps:
    t_first = t[0], t_before_last = t[n - 2], t_last = t[n - 1].  Returns (starts float64 (F + 1,), names list of F str).

    Frame k takes the events [searchsorted(t, starts[k], 'left'), searchsorted(t, starts[k + 1], 'right')): an event exactly on
    a boundary is in both neighbouring frames.  starts[0] = t[0] and starts[k + 1] = starts[k] + interval by REPEATED float64
    addition (not t0 + k * interval: they differ for non-integer intervals); the interval itself is 1 / (1 / interval) as the
    renderer derives it from its frame rate.  As soon as a frame's end reaches n - 1 the renderer clamps it there and stops
    without writing: the last event of a stream is never drawn and the last, partial frame never written.  A frame is
    therefore written exactly while t[n - 2] > starts[k + 1].  Its name is '{:.0f}'.format(starts[k + 1] + interval / 2): the
    start time is advanced before the mid-time is taken."""
    interval = float(interval)
    if not interval > 0.0:
        raise ValueError("interval must be positive (got %r)" % interval)
    if max(abs(int(t_first)), abs(int(t_last))) >= MAX_EXACT_TICK:
        raise ValueError("time stamps beyond 2^53 ticks cannot be compared exactly as float64")
    if not int(t_first) <= int(t_before_last) <= int(t_last):
        raise ValueError("the event stream must be sorted by time")
    step = 1.0 / (1.0 / interval)
    start = np.float64(np.int64(t_first))
    starts, names = [start], []
    while max_frames is None or len(names) < max_frames:
        nxt = start + step
        if not np.int64(t_before_last) > nxt:
            break
        start = nxt
        starts.append(start)
        names.append("{:.0f}".format(start + step / 2))
        if len(names) > 50000000:
            raise ValueError("more than 5e7 frames: interval %r is too small for this stream" % interval)
    return np.asarray(starts, dtype=np.float64), names


def read_events_csv(path, delim_whitespace=False, swap_xy=False, microseconds_timestamp=False, milliseconds_timestamp=False):
    """events.csv -> (t, x, y, p) int64 arrays the way v2e/e2v.py reads it: no header, '#' comments, columns t, x, y, p
    (t, y, x, p with swap_xy), everything cast to int64 (fractions truncated), and under the two time-stamp flags the
    in-place division of the int64 stamps by 1e6 / 1e3, which truncates toward zero again."""
    import pandas as pd
    names = ["t", "y", "x", "p"] if swap_xy else ["t", "x", "y", "p"]
    df = pd.read_csv(path, header=None, comment="#", sep=r"\s+" if delim_whitespace else ",", names=names)
    ev = df[["t", "x", "y", "p"]].values.astype(np.int64)
    if microseconds_timestamp:
        ev[:, 0] = ev[:, 0] / 1000000.0
    elif milliseconds_timestamp:
        ev[:, 0] = ev[:, 0] / 1000.0
    return ev[:, 0].copy(), ev[:, 1].copy(), ev[:, 2].copy(), ev[:, 3].copy()


def read_events_device(path, device=None, host_csv=False, hw=None, aedat_layout="davis", aedat_flip_x=True, aedat_flip_y=True,
                       **csv_flags):
    """events.csv -> (t int64, x int32, y int32) device tensors, the stream ops.render_events takes.  The file's bytes are
    uploaded in one piece and parsed on the device (ops.parse_events_csv); text outside that parser's grammar
    (ops.UnsupportedCsv) and host_csv=True go through read_events_csv and one upload per column, as every file did before:
    the columns are the same either way.

    A path that ends in .aedat / .aedat2, or a file whose first bytes are '#!AER-DAT', is an AEDAT-2.0 file and goes through
    event_read.read_events_aedat2 instead: hw = (height, width) of the sensor is then required, aedat_layout is 'davis' or
    'v2e', aedat_flip_x / aedat_flip_y undo the writers' flips, and the two time-stamp flags become the decoder's divisor.  The
    flags that describe text (delim_whitespace, swap_xy, host_csv) are refused by name, and a stream with backward time steps
    raises ValueError("the event stream must be sorted by time").

    A path that ends in .aedat4, or a file whose first 14 bytes are the AEDAT-4.0 version line, is looked at first and goes
    through event_read.read_events_aedat4 (rebased time stamps in microseconds): hw defaults to the size the file states, and
    every flag that describes text or a time-stamp unit is refused by name.  A path that ends in .aedat3, or a file that starts
    with '#!AER-DAT3.', is an AEDAT-3.1 recording and is looked at before the AEDAT-2.0 test (it usually carries the .aedat name):
    event_read.read_events_aedat3 with the same rules, hw defaulting to the size of the camera the file names."""
    import torch
    from . import event_read, ops
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    fmt = event_read.events_format(path)
    kw = {}
    if fmt in ("aedat4", "aedat3"):
        for name, on in [("host_csv", host_csv)] + sorted(csv_flags.items()):
            if on:
                raise ValueError("%s describes a text file and cannot be used with the %s input %s"
                                 % (name, {"aedat4": "AEDAT-4.0", "aedat3": "AEDAT-3.1"}[fmt], path))
    elif fmt == "aedat2":
        for name, on in (("host_csv", host_csv), ("delim_whitespace", csv_flags.get("delim_whitespace")),
                         ("swap_xy", csv_flags.get("swap_xy"))):
            if on:
                raise ValueError("%s describes a text file and cannot be used with the AEDAT-2.0 input %s" % (name, path))
        if hw is None:
            raise ValueError("an AEDAT-2.0 input needs the sensor size hw = (height, width)")
        div = 1000000.0 if csv_flags.get("microseconds_timestamp") else (1000.0 if csv_flags.get("milliseconds_timestamp") else 0.0)
        kw = dict(layout=aedat_layout, flip_x=aedat_flip_x, flip_y=aedat_flip_y, t_divisor=div)
    if fmt is not None:
        t, x, y, _, info = event_read.read_events_file(path, hw, dev, **kw)
        if info["n_backward"] > 0:
            raise ValueError("the event stream must be sorted by time")
        return t, x, y
    if not host_csv:
        try:
            t, x, y, _ = ops.parse_events_csv(path, device=dev, **csv_flags)
            return t, x, y
        except ops.UnsupportedCsv:
            pass
    t, x, y, _ = read_events_csv(path, **csv_flags)
    return (torch.from_numpy(t).to(dev), torch.from_numpy(x.astype(np.int32)).to(dev),
            torch.from_numpy(y.astype(np.int32)).to(dev))


def write_bmp(path, frame):
    """HxWx3 uint8 -> 24-bit BMP.  The three channels of an event frame are equal, so channel order is not an issue."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(frame), "RGB").save(path, format="BMP")


EXPOSURE_MODES = ("duration", "count", "area_count")


def parse_dvs_exposure(dvs_exposure):
    """e2v.py's --dvs_exposure tokens -> (mode, value, area_dimension), checked as v2ecore/v2e_args.py:
    v2e_check_dvs_exposure_args does: the mode name is case-insensitive; duration and count take exactly one number (float()),
    area_count exactly two (int(), so '500.5' is an error); area_dimension is None outside area_count.  ValueError otherwise."""
    if not dvs_exposure:
        raise ValueError("--dvs_exposure needs a mode: duration, count or area_count")
    mode = str(dvs_exposure[0]).lower()
    if mode not in EXPOSURE_MODES:
        raise ValueError("unknown exposure mode %r: duration, count or area_count" % (dvs_exposure[0],))
    if mode == "area_count" and len(dvs_exposure) != 3:
        raise ValueError("area_count needs three parameters: 'area_count M D'; the frame ends when any D x D area has "
                         "received M events")
    if mode != "area_count" and len(dvs_exposure) != 2:
        raise ValueError("duration or count needs two parameters, e.g. 'duration 10000' or 'count 3000'")
    if mode != "area_count":
        try:
            return mode, float(dvs_exposure[1]), None
        except (TypeError, ValueError):
            raise ValueError("%s takes one number (got %r)" % (mode, dvs_exposure[1]))
    try:
        return mode, int(dvs_exposure[1]), int(dvs_exposure[2])
    except (TypeError, ValueError):
        raise ValueError("area_count must be M D: M the event count, D the area dimension in pixels (integers)")


def exposure_kwargs(mode, value, area_dimension=None):
    """ops.render_events keyword arguments of a parsed --dvs_exposure, with the arguments the reference would loop on forever
    (count N < 1 after truncation, area_count M < 2) and D < 1 rejected."""
    if mode == "duration":
        return {"exposure": "duration", "interval": float(value)}
    if mode == "count":
        if int(value) < 1:
            raise ValueError("count exposure needs at least 1 event per frame (got %r)" % (value,))
        return {"exposure": "count", "event_count": int(value)}
    if mode == "area_count":
        if int(value) < 2:
            raise ValueError("area_count exposure needs M >= 2 events per area (got %r)" % (value,))
        if area_dimension is None or int(area_dimension) < 1:
            raise ValueError("area_count exposure needs an area dimension D >= 1 (got %r)" % (area_dimension,))
        return {"exposure": "area_count", "area_count": int(value), "area_dimension": int(area_dimension)}
    raise ValueError("unknown exposure mode %r" % (mode,))


def frame_times_path(output_folder, dvs_vid):
    """checkAddSuffix(join(output_folder, dvs_vid), '-frame_times.txt') of the reference's renderer."""
    fn = os.path.join(output_folder, dvs_vid)
    suffix = "-frame_times.txt"
    return fn if fn.endswith(suffix) else os.path.splitext(fn)[0] + suffix


def frame_times_text(dvs_vid, times):
    """The reference's frame-times file: a two-line header, then '{k}\\t{t:10.6f}' per written frame."""
    return "# frame times for {}\n# frame# time(s)\n".format(dvs_vid) + "".join(
        "{}\t{:10.6f}\n".format(k, float(tk)) for k, tk in enumerate(times))


def write_event_frames(output_folder, dvs_vid, t, x, y, hw, full_scale=2, chunk=256, **exposure):
    """The output of e2v.py, which v2e.py --dvs_exposure writes too: the time-sorted device columns t, x, y rendered by
    ops.render_events (polarity folded, frame times wanted) with the exposure keywords of exposure_kwargs, every frame as
    <output_folder>/event-frames/<stem>.bmp in frame order -- a repeated stem keeps the later frame -- and the frame-times file of
    dvs_vid.  An empty stream writes the times file's header alone.  -> the stems."""
    from . import ops
    h, w = hw
    out_dir = os.path.join(output_folder, "event-frames")
    os.makedirs(out_dir, exist_ok=True)
    times, names = [], []
    if len(t) > 0:
        frames, names = ops.render_events(t, x, y, None, (h, w), full_scale=full_scale, fold_polarity=True, want_times=True, **exposure)
        times = frames["times"]
        img = frames["flat"].view(-1, h, w, 3)
        for k0 in range(0, len(names), chunk):            # in frame order: a repeated stem keeps the later frame
            host = img[k0:k0 + chunk].cpu().numpy()
            for i, name in enumerate(names[k0:k0 + chunk]):
                write_bmp(os.path.join(out_dir, name + ".bmp"), host[i])
    with open(frame_times_path(output_folder, dvs_vid), "w") as f:
        f.write(frame_times_text(dvs_vid, times))
    return names


def scene_aedat4(scene_dir):
    """The scene's one *.aedat4 file, None when it has none or several."""
    found = sorted(f for f in os.listdir(scene_dir) if f.lower().endswith(".aedat4"))
    return os.path.join(scene_dir, found[0]) if len(found) == 1 else None


def scene_aedat3(scene_dir):
    """The scene's one AEDAT-3.1 recording among its *.aedat and *.aedat3 files, None when it has none or several."""
    from . import event_read
    found = sorted(f for f in os.listdir(scene_dir) if f.lower().endswith((".aedat", ".aedat3")))
    found = [f for f in found if event_read.is_aedat3_path(os.path.join(scene_dir, f))]
    return os.path.join(scene_dir, found[0]) if len(found) == 1 else None


def render_scene(scene_dir, hw, K=None, dist=None, interval=10000.0, full_scale=2, write_distorted=True, device=None,
                 chunk_frames=256, exposure=None, host_csv=False, aedat_layout="davis", **csv_flags):
    """scene_dir/events.csv -> scene_dir/event-frames/<t>.bmp (undistorted when K / dist are given) and, with
    write_distorted, scene_dir/event-frames-distorted/<t>.bmp: the directory contract of the reference's convert_aedats.py.
    The file is uploaded once, parsed and rendered on the device (read_events_device, ops.render_events); frames come back
    chunk_frames at a time.  host_csv: read the file with the pandas reader instead (the device parser's fallback).
    exposure: None (DURATION over `interval`) or ops.render_events keyword arguments (exposure_kwargs) that replace it.
    A scene that holds events.aedat (AEDAT-2.0, address layout aedat_layout, sensor size hw) and no events.csv is rendered from
    that file; when both exist, events.csv wins.  A scene with neither, but exactly one *.aedat4 file (an AEDAT-4.0 recording), is
    rendered from that file; failing that, exactly one AEDAT-3.1 recording (*.aedat or *.aedat3 that starts with '#!AER-DAT3.'),
    with hw as the sensor size.  Returns the list of frame names."""
    import torch
    from . import ops
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    src = os.path.join(scene_dir, "events.csv")
    if not os.path.exists(src) and os.path.exists(os.path.join(scene_dir, "events.aedat")):
        src = os.path.join(scene_dir, "events.aedat")
    elif not os.path.exists(src) and scene_aedat4(scene_dir) is not None:
        src = scene_aedat4(scene_dir)
    elif not os.path.exists(src) and scene_aedat3(scene_dir) is not None:
        src = scene_aedat3(scene_dir)
    t, x, y = read_events_device(src, dev, host_csv=host_csv, hw=hw, aedat_layout=aedat_layout, **csv_flags)
    out_dir = os.path.join(scene_dir, "event-frames"); dis_dir = os.path.join(scene_dir, "event-frames-distorted")
    os.makedirs(out_dir, exist_ok=True)
    if write_distorted:
        os.makedirs(dis_dir, exist_ok=True)
    mode = dict(exposure) if exposure is not None else {"interval": interval}
    frames, names = ops.render_events(t, x, y, None, hw, full_scale=full_scale, fold_polarity=True, K=K, dist=dist,
                                      want_distorted=write_distorted, **mode)
    h, w = int(hw[0]), int(hw[1])
    und = frames["flat"].view(-1, h, w, 3)
    for k0 in range(0, len(names), chunk_frames):
        host = und[k0:k0 + chunk_frames].cpu().numpy()
        hdis = frames["distorted"][k0:k0 + chunk_frames].cpu().numpy() if write_distorted else None
        for i, name in enumerate(names[k0:k0 + chunk_frames]):
            write_bmp(os.path.join(out_dir, name + ".bmp"), host[i])
            if write_distorted:
                write_bmp(os.path.join(dis_dir, name + ".bmp"), hdis[i])
    return names
