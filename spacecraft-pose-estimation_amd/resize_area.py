"""Host side of the device area resize (csrc/resize_area.hip through ops.resize_area): the per-axis tables of cv2.resize's INTER_AREA
for shrinking, and their packing into the records the kernel applies.  NumPy only.

The rule is written from OpenCV 4.x's resize.cpp (computeResizeAreaTab, ResizeArea_, ResizeAreaFast_) from memory; cv2 is not
installed where this was built, so agreement with cv2 itself is unverified.  tests/resize_area_restated.py states the same rule a
second time and is what the kernel is held to.

Per axis, scale = size_in / size_out as a double.  When both scales are whole numbers within DBL_EPSILON the box rule applies: the
integer sum s of the box, (s + 2) >> 2 for 2 x 2, else float32(s) * float32(1.0f / area), rounded half to even.  Every other pair of
scales takes the weighted rule with the tables below.  An axis that grows is refused: cv2 takes another branch there.
"""
import math
import sys

import numpy as np

REC_WORDS = 5            # int32 words per record: first, count, bits of the first / inner / last weight
WEIGHTED, BOX = 0, 1


def tables(size_in, size_out):
    """computeResizeAreaTab for one axis -> (ofs int32 [size_out + 1], idx int32 [K], w float32 [K]): output index d sums the source
    indices idx[ofs[d]:ofs[d + 1]] with the weights w[...], in that order.  Weights are computed in double and stored as float32."""
    size_in, size_out = int(size_in), int(size_out)
    if not 1 <= size_out <= size_in:
        raise ValueError("resize_area: %d -> %d: the output must be 1 .. the input size" % (size_in, size_out))
    scale = size_in / size_out
    ofs, idx, w = [0], [], []
    for d in range(size_out):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, size_in - f1)
        s2 = min(int(math.floor(f2)), size_in)
        s1 = min(int(math.ceil(f1)), s2)
        if s1 - f1 > 1e-3:
            idx.append(s1 - 1)
            w.append((s1 - f1) / cell)
        for s in range(s1, s2):
            idx.append(s)
            w.append(1.0 / cell)
        if f2 - s2 > 1e-3:
            idx.append(s2)
            w.append(min(min(f2 - s2, 1.0), cell) / cell)
        ofs.append(len(idx))
    idx = np.asarray(idx, dtype=np.int32)
    if len(idx) and (idx.min() < 0 or idx.max() >= size_in):
        raise ValueError("resize_area: %d -> %d: a tap outside the axis" % (size_in, size_out))
    return np.asarray(ofs, dtype=np.int32), idx, np.asarray(w, dtype=np.float64).astype(np.float32)


def whole_ratio(size_in, size_out):
    """The whole number c when size_in / size_out equals it within DBL_EPSILON, else None."""
    scale = size_in / size_out
    c = int(round(scale))
    return c if abs(scale - c) < sys.float_info.epsilon else None


def pack(ofs, idx, w):
    """tables() -> int32 [size_out, REC_WORDS] records.  Lossless: the taps of an output index are consecutive source indices and its
    inner taps share one weight, which is checked here (unpack() returns the tables)."""
    n = len(ofs) - 1
    rec = np.zeros((n, REC_WORDS), dtype=np.int32)
    wf = rec[:, 2:].view(np.float32)
    for d in range(n):
        a, b = int(ofs[d]), int(ofs[d + 1])
        if b <= a or not np.array_equal(idx[a:b], np.arange(idx[a], idx[a] + b - a)):
            raise ValueError("resize_area: output index %d has no taps or taps that are not consecutive" % d)
        inner = w[a + 1:b - 1]
        if len(inner) and not (inner.view(np.uint32) == inner.view(np.uint32)[0]).all():
            raise ValueError("resize_area: output index %d: the inner taps do not share one weight" % d)
        rec[d, :2] = (idx[a], b - a)
        wf[d] = (w[a], inner[0] if len(inner) else 0.0, w[b - 1])
    return rec


def unpack(rec):
    """records -> the (ofs, idx, w) they stand for"""
    ofs, idx, w = [0], [], []
    wf = np.ascontiguousarray(rec[:, 2:]).view(np.float32)
    for d in range(len(rec)):
        first, count = int(rec[d, 0]), int(rec[d, 1])
        idx += list(range(first, first + count))
        w += [wf[d, 0] if k == 0 else (wf[d, 2] if k == count - 1 else wf[d, 1]) for k in range(count)]
        ofs.append(len(idx))
    return np.asarray(ofs, np.int32), np.asarray(idx, np.int32), np.asarray(w, np.float32)


def box_records(size_in, c):
    """The records of the box rule: output index d sums the c source indices from d * c; the weights are not read."""
    rec = np.zeros((size_in // c, REC_WORDS), dtype=np.int32)
    rec[:, 0] = np.arange(size_in // c, dtype=np.int32) * c
    rec[:, 1] = c
    return rec


def check_sizes(in_hw, out_hw, who="resize_area"):
    """ValueError when the output is empty or an axis would grow; names both sizes"""
    (H, W), (h, w) = (int(v) for v in in_hw), (int(v) for v in out_hw)
    if h < 1 or w < 1 or h > H or w > W:
        raise ValueError("%s: frames of %d x %d (W x H) cannot be resized to %d x %d: the area rule only shrinks, every output axis must be "
                         "1 .. the input's" % (who, W, H, w, h))
    return H, W, h, w


def plan(in_hw, out_hw):
    """-> (rule, xrec, yrec): what scpose_resize_area_u8 takes for frames of in_hw = (H, W) resized to out_hw = (h, w)"""
    H, W, h, w = check_sizes(in_hw, out_hw)
    cx, cy = whole_ratio(W, w), whole_ratio(H, h)
    if cx is not None and cy is not None:
        if cx * cy > 1 << 23:
            raise ValueError("resize_area: a box of %d x %d pixels overflows the integer sum (at most 2^23 pixels)" % (cx, cy))
        return BOX, box_records(W, cx), box_records(H, cy)
    return WEIGHTED, pack(*tables(W, w)), pack(*tables(H, h))
