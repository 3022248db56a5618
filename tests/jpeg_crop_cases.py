"""Shared by the tests of ops.decode_crop / scpose_jpeg_decode_crop: PIL-written frames in the three sampling modes and the
affines (frame -> crop, as get_affine_transform returns them) of the cases the crop tail must get right."""
import functools

import numpy as np

import jpeg_decode_restated as R

MODES = ("gray", "444", "420")
SIZES = ((67, 130), (40, 48))            # (height, width)
CROP_WH = (32, 24)


@functools.lru_cache(None)
def frame(mode, size, seed=0, **kw):
    """(bytes PIL wrote, the RGB frame PIL decodes from them)"""
    data = R.fixture(mode, size[0], size[1], 90, "noise", seed=seed, **kw)
    return data, R.pil_decode(data)


def affines(size):
    """{name: 2 x 3 float64}: crop pixel u = a * x + t.  The crop covers CROP_WH / a frame pixels from -t / a on."""
    h, w = size

    def m(a, x0, y0):                    # crop (0, 0) lies at frame (x0, y0)
        return np.array([[a, 0.0, -a * x0], [0.0, a, -a * y0]], dtype=np.float64)
    return {"scale_1_fractional": m(1.0, 10.3, 7.6), "down_3": m(1.0 / 3.0, -5.2, -8.7), "up_2.5": m(2.5, 8.2, 3.3),
            "half_outside": m(1.0, -16.4, -11.5), "outside": m(1.0, w + 50.5, h + 50.25)}


# One call that crosses kRoiChunk (csrc/crop_tail.h: 128 windows travel in the arguments of one launch of the crop tail)
CHUNK_N = 130
CHUNK_SIZE, CHUNK_WH = (16, 16), (8, 6)


def chunk_affines(n=CHUNK_N):
    """(n, 2, 3): in turn a half-pixel shift from the near corner, a 2x zoom across the top or bottom edge (taps leave the frame), a
    crop wholly outside and the identity from the far corner, each from another origin, so that every image whose crop meets the
    frame has a window of its own.  Rows 127, 128 and 129 -- the last of the first launch, the two of the second -- are the
    identity, the half-pixel shift and the zoom."""
    out = []
    for i in range(n):
        ox, oy = (i // 4) % 7, (i // 4) // 7
        a, x0, y0 = ((1.0, ox + 0.5, oy + 0.5), (2.0, 9.25 + ox, (-2.25, -1.25, 13.25, 14.25, 15.25)[oy]), (1.0, 66.5 + ox, 66.25 + oy),
                     (1.0, 8.0 - ox, 10.0 - oy))[i % 4]
        out.append([[a, 0.0, -a * x0], [0.0, a, -a * y0]])
    return np.array(out, dtype=np.float64)


def check_chunk_call(ops, files, frames, **kw):
    """decode_crop of CHUNK_N files in one call equals crop_warp of the PIL frames row by row, in both channel orders; -> info"""
    import torch
    trans = chunk_affines(len(files))
    windows = [tuple(ops.warp_window(t, CHUNK_WH, f.shape[:2])) for t, f in zip(trans, frames)]
    inside = [w for i, w in enumerate(windows) if i % 4 != 2]
    assert len(set(inside)) == len(inside) and all(w[2] > 0 and w[3] > 0 for w in inside)
    assert all(w[1] == 0 or w[1] + w[3] == 16 for w in windows[1::4])                    # the zoom reaches the frame's first or last row
    for rgb in (True, False):
        got, info = ops.decode_crop(files, trans, CHUNK_WH, rgb=rgb, fallback=False, **kw)
        want = ops.crop_warp([np.ascontiguousarray(f if rgb else f[:, :, ::-1]) for f in frames], trans, CHUNK_WH)
        assert tuple(got.shape) == (len(files), CHUNK_WH[1], CHUNK_WH[0], 3)
        bad = [i for i in range(len(files)) if not np.array_equal(got[i].cpu().numpy(), want[i].cpu().numpy())]
        assert not bad, bad
        edge = [got[i] for i in (0, 127, 128, 129)]
        assert all(bool(r.any()) for r in edge) and all(not torch.equal(edge[a], edge[b]) for a in range(4) for b in range(a))
        assert not bool(got[2::4].any())                                                  # the crops wholly outside
    return info
