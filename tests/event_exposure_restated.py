"""NumPy restatement of the COUNT and AREA_COUNT exposure modes of the event renderer (test infrastructure; the product is
csrc/events_exposure.hip + ops.render_events).

Written from the reference's lines (v2e/v2ecore/renderer.py: render_events_to_frames, compute_area_counts), independently of
the package.  serial_* is the reference loop restated literally: a frame starts at `start`, the area counters start at zero,
the first event whose area reaches M ends it, the triggering event opens the next frame; a frame is written while its end is
< n - 1.  area_bounds_suffix_min is the form the device computes: g[j] = index of the M-th occurrence of area(j) counting j as
the first, the frame starting at s ends at min_{i >= s} g[i].  The histogram and gray value are event_render_restated's."""
import numpy as np

import event_render_restated as ER


def area_grid(hw, D):
    h, w = hw
    return 1 + w // D, 1 + h // D


def area_index(x, y, hw, D):
    """(ax, ay) int64 after Python / NumPy wraparound, as area_counts[x // D, y // D] resolves them; IndexError off the grid."""
    nw, nh = area_grid(hw, D)
    ax = np.asarray(x, np.int64) // D
    ay = np.asarray(y, np.int64) // D
    if ((ax < -nw) | (ax >= nw) | (ay < -nh) | (ay >= nh)).any():
        raise IndexError("event coordinate off the %d x %d area grid" % (nw, nh))
    return np.where(ax < 0, ax + nw, ax), np.where(ay < 0, ay + nh, ay)


def stem(t, b, e):
    return "{:.0f}".format((np.int64(t[b]) + np.int64(t[e])) / 2)


def frame_time(t, b, e):
    return (np.int64(t[b]) + np.int64(t[e])) / 2


def serial_count_bounds(n, N):
    """[(begin, end)] of COUNT N (N = int(float(arg)))."""
    if N < 1:
        raise ValueError("COUNT needs N >= 1")
    out, start = [], 0
    if n < 2:
        return out
    while True:
        end = start + N
        if end >= n - 1:
            return out
        out.append((start, end))
        start = end


def serial_area_bounds(x, y, hw, M, D):
    """[(begin, end)] of AREA_COUNT M D: the reference's loop, counters reset on every trigger."""
    if M < 2 or D < 1:
        raise ValueError("AREA_COUNT needs M >= 2 and D >= 1")
    n = len(x)
    if n < 2:
        if n == 1:
            area_index(x, y, hw, D)
        return []
    ax, ay = area_index(x, y, hw, D)
    nw, nh = area_grid(hw, D)
    ax = ax.tolist(); ay = ay.tolist()
    out, start = [], 0
    while True:
        counts = [[0] * nh for _ in range(nw)]
        end = n - 1
        for i in range(start, n):
            c = counts[ax[i]][ay[i]] + 1
            counts[ax[i]][ay[i]] = c
            if c >= M:
                end = i
                break
        if end >= n - 1:
            return out
        out.append((start, end))
        start = end


def area_bounds_suffix_min(x, y, hw, M, D):
    """The same bounds from g and its suffix minimum (stable sort by area, gather, reversed minimum.accumulate)."""
    if M < 2 or D < 1:
        raise ValueError("AREA_COUNT needs M >= 2 and D >= 1")
    n = len(x)
    if n < 2:
        if n == 1:
            area_index(x, y, hw, D)
        return []
    ax, ay = area_index(x, y, hw, D)
    nw, nh = area_grid(hw, D)
    key = ax * nh + ay
    order = np.argsort(key, kind="stable")
    sk = key[order]
    g = np.full(n, n - 1, np.int64)
    q = np.arange(n - (M - 1)) if n > M - 1 else np.zeros(0, np.int64)
    same = sk[q + M - 1] == sk[q]
    g[order[q[same]]] = np.minimum(order[q[same] + M - 1], n - 1)
    nxt = np.minimum.accumulate(g[::-1])[::-1]
    out, s = [], 0
    while nxt[s] < n - 1:
        out.append((s, int(nxt[s])))
        s = int(nxt[s])
    return out


def render_bounds(t, x, y, bounds, hw, fs=2):
    """(frames uint8 (F, H, W) -- one channel, the three are equal --, stems, frame times) of the given bounds."""
    frames = np.zeros((len(bounds), hw[0], hw[1]), np.uint8)
    for k, (b, e) in enumerate(bounds):
        frames[k] = ER.gray(ER.counts(x[b:e], y[b:e], None, hw), fs)
    return frames, [stem(t, b, e) for b, e in bounds], [frame_time(t, b, e) for b, e in bounds]


def frame_times_text(dvs_vid, times):
    """The renderer's frame-times file for these frame times."""
    return "# frame times for {}\n# frame# time(s)\n".format(dvs_vid) + "".join(
        "{}\t{:10.6f}\n".format(k, tk) for k, tk in enumerate(times))


def duration_times(t, interval):
    """The frame times of DURATION mode (the value each stem is formatted from): starts[k + 1] + interval / 2."""
    step = 1 / (1 / interval)
    sched = ER.schedule(t, interval)
    start = t[0]
    out = []
    for _ in sched:
        start = start + step
        out.append(start + step / 2)
    return out
