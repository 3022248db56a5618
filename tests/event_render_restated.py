"""NumPy restatement of the event renderer (test infrastructure; the product is csrc/events.hip + event_render.py).

Written from the reference's lines, independently of the package: the schedule is the renderer's own loop over the whole stamp
column (v2e/v2ecore/renderer.py: render_events_to_frames, DURATION mode), the histogram np.add.at with the bounds test of
v2ecore/v2e_utils.py: hist2d_numba_seq, the gray value renderer.py's normalize_frame followed by (img * 255).astype(uint8).
undistort() restates what cv2.undistort(img, K, dist) does for a uint8 image with the fixed-point bilinear tap this project
already uses for cv2.warpAffine (utils/transforms.py: warp_affine_bilinear); cv2 is not available, so that half holds the
arithmetic, not cv2 parity."""
import numpy as np


def schedule(t, interval):
    """[(begin, end, name)] of the frames the reference writes for the time-sorted stamps t."""
    t = np.asarray(t)
    n = len(t)
    if n == 0:
        return []
    step = 1 / (1 / interval)                   # frame_rate_hz = 1 / exposure_value; frameIntevalS = 1 / frame_rate_hz
    start = t[0]
    nxt = start + step
    out = []
    while True:
        b = np.searchsorted(t, start, side="left")
        e = np.searchsorted(t, nxt, side="right")
        if e >= n - 1:
            return out                           # the remaining events are accumulated but the frame is never written
        start = start + step
        nxt = start + step
        out.append((int(b), int(e), "{:.0f}".format(start + step / 2)))


def counts(x, y, p, hw, fold_polarity=True):
    """int64 (H, W): ON minus OFF counts (every event +1 with fold_polarity); row = y, column = x; outside events dropped."""
    h, w = hw
    x = np.asarray(x, np.int64); y = np.asarray(y, np.int64)
    ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    val = np.ones(len(x), np.int64) if fold_polarity else np.where(np.asarray(p) == 1, 1, -1).astype(np.int64)
    c = np.zeros((h, w), np.int64)
    np.add.at(c, (y[ok], x[ok]), val[ok])
    return c


def gray(c, fs):
    img = (np.clip(c, -fs, fs).astype(np.float64) + fs) / float(fs * 2)
    return (img * 255).astype(np.uint8)


def render(t, x, y, p, hw, interval=10000.0, fs=2, fold_polarity=True):
    """(frames uint8 (F, H, W, 3), names)"""
    sched = schedule(t, interval)
    frames = np.zeros((len(sched), hw[0], hw[1], 3), np.uint8)
    for k, (b, e, _) in enumerate(sched):
        frames[k] = gray(counts(x[b:e], y[b:e], None if p is None else p[b:e], hw, fold_polarity), fs)[..., None]
    return frames, [s[2] for s in sched]


def undistort_map(hw, K, dist):
    """float64 (map_x, map_y): for every output pixel the source position, through the forward distortion model with new
    camera matrix = K.  The order of operations is the kernel's."""
    h, w = hw
    K = np.asarray(K, np.float64).reshape(3, 3); d = np.asarray(dist, np.float64).reshape(5)
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    k1, k2, p1, p2, k3 = d
    u = np.arange(w, dtype=np.float64)[None, :]; v = np.arange(h, dtype=np.float64)[:, None]
    xn = (u - cx) / fx + 0 * v; yn = (v - cy) / fy + 0 * u
    r2 = xn * xn + yn * yn
    cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = xn * cd + p1 * 2 * xn * yn + p2 * (r2 + 2 * xn * xn)
    yd = yn * cd + p1 * (r2 + 2 * yn * yn) + p2 * 2 * xn * yn
    return fx * xd + cx, fy * yd + cy


def fixed_coords(m):
    """1/32-px coordinate of a float64 map: round half to even, saturated to int32; pixel saturated to int16; 5-bit fraction."""
    X = np.clip(np.rint(m * 32.0), -2147483648.0, 2147483647.0).astype(np.int64)
    return np.clip(X >> 5, -32768, 32767), X & 31


def undistort(img, K, dist):
    """cv2.undistort(img, K, dist) for uint8 HxW or HxWxC: fixed-point bilinear, constant border 0."""
    src = img if img.ndim == 3 else img[..., None]
    h, w = src.shape[:2]
    mx, my = undistort_map((h, w), K, dist)
    sx, a = fixed_coords(mx); sy, b = fixed_coords(my)
    a = a[..., None]; b = b[..., None]

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64) * ok[..., None]
    acc = (tap(sy, sx) * ((32 - a) * (32 - b) * 32) + tap(sy, sx + 1) * (a * (32 - b) * 32) +
           tap(sy + 1, sx) * ((32 - a) * b * 32) + tap(sy + 1, sx + 1) * (a * b * 32))
    out = np.clip((acc + 16384) >> 15, 0, 255).astype(np.uint8)
    return out if img.ndim == 3 else out[..., 0]
