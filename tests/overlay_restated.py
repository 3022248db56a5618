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


H, W = 48, 64
# (bbox, points) of one 64 x 48 frame each
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
}


def base_frame():
    return np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
