"""Frames and PIL references shared by the encoder's CPU and GPU tests."""
import io

import numpy as np
from PIL import Image

MODES = ("gray", "444", "420")
QUALITIES = (1, 30, 75, 95, 100)
SIZES = ((1, 1), (8, 8), (16, 16), (9, 17), (47, 33), (67, 130))          # (H, W); 17 x 9 pads both edges, odd chroma size
PIL_SUBSAMPLING = {"444": 0, "420": 2}


def content(name, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "constant":
        return np.broadcast_to(np.array([77, 130, 200], dtype=np.uint8), (h, w, 3)).copy()
    if name == "gradient":
        return np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 3) % 256], axis=2).astype(np.uint8)
    if name == "noise":
        return np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if name == "blocks":            # 8 x 8 blocks alternating 0 and 255: DC differences of size 11 at quality 100
        return np.repeat((((xx // 8 + yy // 8) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if name == "checker":           # one-pixel checkerboard: AC size 10 at quality 100
        return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if name == "cosine":            # only coefficient (7, 7) survives: a run of 62 zeros, three ZRL symbols, no EOB
        v = 128 + 12 * np.cos((2 * (xx % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (yy % 8) + 1) * 7 * np.pi / 16)
        return np.repeat(np.rint(v).astype(np.uint8)[:, :, None], 3, axis=2)
    raise KeyError(name)


def cases():
    """(content, (h, w), quality) of every frame; every mode codes every one of them"""
    out = [(c, s, q) for s in SIZES for q in QUALITIES for c in ("constant", "gradient", "noise")]
    out += [("blocks", (47, 33), q) for q in QUALITIES]
    out += [("checker", s, 100) for s in ((9, 17), (47, 33))]
    out += [("cosine", s, 100) for s in ((16, 16), (47, 33))]
    return out


def pil_bytes(rgb, quality, mode, comment=None):
    im = Image.fromarray(rgb)
    kw = {} if comment is None else {"comment": comment}
    b = io.BytesIO()
    if mode == "gray":
        im.convert("L").save(b, "JPEG", quality=quality, **kw)
    else:
        im.save(b, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[mode], **kw)
    return b.getvalue()
