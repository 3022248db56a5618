"""pose_export.draw_overlay's drawing restated on an array: the outline of ImageDraw.rectangle(width=2), then the discs of
ImageDraw.ellipse over an 11 x 11 box, clipped to the frame.  Tests pin it to PIL."""
import numpy as np

# ImageDraw.ellipse([c - 5, c - 5, c + 5, c + 5], fill=...): one string per row
DISC = ("...#####...", "..#######..", ".#########.", "###########", "###########", "###########", "###########", "###########",
        ".#########.", "..#######..", "...#####...")
GREEN, BLUE = (0, 255, 0), (0, 0, 255)


def draw(frame, bbox, points):
    """frame (H, W, 3) uint8, changed in place; bbox (x, y, w, h) ints with w, h >= 0; points (J, 2) floats"""
    hh, ww = frame.shape[:2]
    x0, y0, w, h = (int(v) for v in bbox)
    x1, y1 = x0 + w, y0 + h
    for y in range(max(y0, 0), min(y1, hh - 1) + 1):
        for x in range(max(x0, 0), min(x1, ww - 1) + 1):
            if x < x0 + 2 or x > x1 - 2 or y < y0 + 2 or y > y1 - 2:
                frame[y, x] = GREEN
    for px, py in np.asarray(points, dtype=np.float64).reshape(-1, 2):
        if not (np.isfinite(px) and np.isfinite(py)):
            continue
        cx, cy = int(px), int(py)                      # truncation toward zero
        for r, row in enumerate(DISC):
            for c, ch in enumerate(row):
                x, y = cx - 5 + c, cy - 5 + r
                if ch == "#" and 0 <= x < ww and 0 <= y < hh:
                    frame[y, x] = BLUE
    return frame


def pil_draw(frame, bbox, points):
    from PIL import Image, ImageDraw
    img = Image.fromarray(frame)
    d = ImageDraw.Draw(img)
    x, y, w, h = [int(v) for v in bbox]
    d.rectangle([x, y, x + w, y + h], outline=GREEN, width=2)
    for px, py in np.asarray(points, dtype=np.float64).reshape(-1, 2):
        if np.isfinite(px) and np.isfinite(py):
            d.ellipse([int(px) - 5, int(py) - 5, int(px) + 5, int(py) + 5], fill=BLUE)
    return np.array(img)


def pil_points(points):
    """the points ImageDraw.ellipse accepts: for coordinates of 1e300 its argument parser raises (this Pillow: SystemError), so
    a point that large is held to the restatement alone"""
    return [(px, py) for px, py in points if not (np.isfinite(px) and np.isfinite(py)) or max(abs(px), abs(py)) < 2.0 ** 62]


def _scatter(h, w, count, seed):
    """count points over the frame and a margin of 8 pixels around it: discs inside, cut by every edge, and wholly outside"""
    rng = np.random.default_rng(seed)
    return [(float(x), float(y)) for x, y in zip(rng.uniform(-8, w + 8, count), rng.uniform(-8, h + 8, count))]


H, W = 48, 64
# name: (bbox, points); the frame is H x W unless FRAME_SIZES says otherwise
CASES = {
    "inside": ((10, 8, 30, 20), [(32.2, 24.9)]),
    "left": ((-5, 10, 20, 20), []),
    "right": ((50, 10, 20, 20), []),
    "top": ((10, -6, 20, 20), []),
    "bottom": ((10, 40, 20, 20), []),
    "outside": ((100, 100, 10, 10), []),
    "negative": ((-30, -30, 31, 32), []),
    "thin": ((20, 20, 1, 2), []),                      # the thinnest box PIL draws as an outline (below: lines)
    "corners": ((0, 0, 63, 47), [(0.0, 0.0), (63.9, 0.2), (0.7, 47.0), (63.0, 47.5), (-3.0, -3.0), (66.0, 50.0)]),
    "overlap": ((5, 5, 10, 10), [(30.0, 20.0), (34.5, 23.5), (12.0, 12.0)]),
    "nonfinite": ((8, 8, 8, 8), [(float("nan"), 10.0), (10.0, float("inf")), (float("-inf"), float("nan")), (40.0, 30.0)]),
    "minus_half": ((1, 1, 5, 5), [(-0.5, 20.0), (20.0, -0.5), (-0.99, -0.99)]),
    # around the kernel's |p| < 1e9 test and the int32 conversion behind it: none of the six draws, the last point does.
    # ImageDraw.ellipse raises for the last two of the six (pil_points): those are held to the restatement alone
    "guards": ((8, 8, 8, 8), [(999999999.0, 5.0), (1e9, 5.0), (-1e9, 5.0), (2147483648.0, 5.0), (1e300, -1e300), (5.0, 1.7e308),
                              (40.0, 30.0)]),
    # a tall frame: H > W, the rows of the rectangle take fewer threads than its columns
    "tall_inside": ((6, 20, 25, 60), _scatter(96, 40, 16, 1)),
    "tall_crossing": ((22, 70, 30, 40), _scatter(96, 40, 17, 2)),      # over the right and the bottom edge
    # 4 (W + H) = 3280 threads: thirteen workgroups for the rectangle, eight and more for the discs
    "large_inside": ((100, 50, 300, 200), _scatter(300, 520, 16, 3)),
    "large_crossing": ((-40, -25, 200, 120), _scatter(300, 520, 20, 4)),     # over the left and the top edge
}
FRAME_SIZES = {"tall_inside": (96, 40), "tall_crossing": (96, 40), "large_inside": (300, 520), "large_crossing": (300, 520)}     # (H, W)
DRAWN = ("inside", "corners", "overlap", "nonfinite", "guards", "tall_inside", "tall_crossing", "large_inside", "large_crossing")


def size_of(case):
    return FRAME_SIZES.get(case, (H, W))


def base_frame(h=H, w=W):
    return np.random.default_rng(7).integers(0, 256, (h, w, 3), dtype=np.uint8)
