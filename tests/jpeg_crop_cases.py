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
