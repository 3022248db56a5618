"""The area resize of csrc/resize_area.hip stated a second time in NumPy, and the exact area mean it approximates.

tables / resize_area follow OpenCV 4.x's INTER_AREA for shrinking (computeResizeAreaTab, ResizeArea_, ResizeAreaFast_) as the project
documents it; written from memory of resize.cpp, not checked against cv2.  Nothing here imports the product: the product's table
builder is compared against tables() by the tests, never used to define it.

CASES lists the shapes both test files run: (name, (H, W), (h, w), channels)."""
import sys

import numpy as np

CASES = (
    ("fractional_both", (11, 13), (4, 5), 3),
    ("box_2x2", (6, 8), (3, 4), 3),
    ("box_3x3", (6, 9), (2, 3), 3),
    ("box_2x4_ties", (4, 8), (2, 2), 3),           # added: the only listed box whose products can end in .5 (see frames_for)
    ("whole_y_fractional_x", (12, 10), (4, 7), 3),
    ("gray_only", (5, 7), (5, 7), 3),
    ("one_pixel", (48, 64), (1, 1), 3),
    ("long_row", (3, 2051), (1, 640), 3),
    ("one_channel", (9, 70), (9, 33), 1),
    ("row_strips", (45, 20), (19, 7), 3),          # added: three strips of eight output rows, boundary rows shared inside and across them
    ("two_passes", (2, 5000), (1, 300), 3),        # added: a strip's source segment longer than one 4080-byte pass of the kernel
)
F = 3


def frames_for(name):
    """Three distinct random uint8 frames of the case.  box_2x4_ties: the channel-0 boxes of frame 0 are set so that their sums are
    8 k + 4 with k even (0, 0) and k odd (0, 1): float32(s) * 0.125 is exactly k + 0.5, and round-half-to-even decides."""
    _, (H, W), _, c = next(x for x in CASES if x[0] == name)
    rng = np.random.default_rng(sum(name.encode()) * 7919 + H * 131 + W)
    fr = rng.integers(0, 256, size=(F, H, W, c) if c == 3 else (F, H, W), dtype=np.uint8)
    if name == "box_2x4_ties":
        fr[0, 0:2, 0:4, 0] = np.array([[10, 10, 10, 10], [10, 10, 10, 14]])      # 84 = 8 * 10 + 4 -> 10.5 -> 10
        fr[0, 0:2, 4:8, 0] = np.array([[11, 11, 11, 11], [11, 11, 11, 15]])      # 92 = 8 * 11 + 4 -> 11.5 -> 12
    return fr


def tables(size_in, size_out):
    """Per output index d of one axis: the source indices it sums and their float32 weights, in order.
    -> (ofs int32 [size_out + 1], idx int32 [K], w float32 [K])"""
    scale = float(size_in) / float(size_out)
    ofs, idx, w = [0], [], []
    for d in range(size_out):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, size_in - f1)
        s1 = int(np.ceil(f1))
        s2 = min(int(np.floor(f2)), size_in)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            idx.append(s1 - 1); w.append(np.float32((s1 - f1) / cell))
        for s in range(s1, s2):
            idx.append(s); w.append(np.float32(1.0 / cell))
        if f2 - s2 > 1e-3:
            idx.append(s2); w.append(np.float32(min(min(f2 - s2, 1.0), cell) / cell))
        ofs.append(len(idx))
    return np.array(ofs, np.int32), np.array(idx, np.int32), np.array(w, np.float32)


def _whole(size_in, size_out):
    scale = float(size_in) / float(size_out)
    return abs(scale - round(scale)) < sys.float_info.epsilon


def _round_u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def resize_area(frames, out_hw):
    """uint8 (F, H, W, C) or (F, H, W) -> the same rank at out_hw: per channel, float32 in the stated order, or the box rules."""
    fr = np.asarray(frames)
    one = fr.ndim == 3
    x = fr[..., None] if one else fr
    n, H, W, c = x.shape
    h, w = out_hw
    assert h <= H and w <= W
    if (h, w) == (H, W):
        out = x.copy()
    elif _whole(W, w) and _whole(H, h):
        cx, cy = W // w, H // h
        s = x.astype(np.int64).reshape(n, h, cy, w, cx, c).sum(axis=(2, 4))
        if cx == 2 and cy == 2:
            out = ((s + 2) >> 2).astype(np.uint8)
        else:
            inv = np.float32(np.float32(1.0) / np.float32(cx * cy))
            prod = s.astype(np.float32) * inv
            assert prod.dtype == np.float32
            out = _round_u8(prod)
    else:
        xo, xi, xw = tables(W, w)
        yo, yi, yw = tables(H, h)
        xf = x.astype(np.float32)
        hor = np.zeros((n, H, w, c), np.float32)
        for d in range(w):
            acc = np.zeros((n, H, c), np.float32)
            for e in range(xo[d], xo[d + 1]):
                acc = acc + xf[:, :, xi[e], :] * xw[e]
            hor[:, :, d, :] = acc
        ver = np.zeros((n, h, w, c), np.float32)
        for d in range(h):
            acc = None
            for e in range(yo[d], yo[d + 1]):
                term = yw[e] * hor[:, yi[e]]
                acc = term if acc is None else acc + term
            ver[:, d] = acc
        assert hor.dtype == np.float32 and ver.dtype == np.float32
        out = _round_u8(ver)
    return out[..., 0] if one else out


def gray(frames, channels="rgb"):
    """OpenCV's 8-bit gray of (.., 3) uint8: (4899 R + 9617 G + 1868 B + 8192) >> 14"""
    a = np.asarray(frames).astype(np.int64)
    r, b = (0, 2) if channels == "rgb" else (2, 0)
    return ((4899 * a[..., r] + 9617 * a[..., 1] + 1868 * a[..., b] + 8192) >> 14).astype(np.uint8)


def _axis_mean(a, axis, size_out):
    """float64 mean of the piecewise-constant signal along `axis` over [d s, (d + 1) s) clipped to the axis, by its integral"""
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    scale = n / size_out
    cum = np.concatenate([np.zeros(a.shape[:-1] + (1,)), np.cumsum(a, axis=-1)], axis=-1)     # integral up to each whole position

    def integral(t):
        i = min(int(np.floor(t)), n - 1)
        return cum[..., i] + (t - i) * a[..., i]
    out = np.empty(a.shape[:-1] + (size_out,))
    for d in range(size_out):
        lo, hi = d * scale, min((d + 1) * scale, float(n))
        out[..., d] = (integral(hi) - integral(lo)) / (hi - lo)
    return np.moveaxis(out, -1, axis)


def exact_mean(frames, out_hw):
    """float64: the true area average of every output pixel, per channel"""
    a = np.asarray(frames).astype(np.float64)
    return _axis_mean(_axis_mean(a, 2, out_hw[1]), 1, out_hw[0])
