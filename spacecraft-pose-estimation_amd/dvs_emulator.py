"""Host side of the DVS emulator (csrc/dvs_emulator.hip; the reference's v2e/v2ecore/emulator.py): the lin-log table, the
parameter checks, the 'clean' parameter set and the helper that draws the per-pixel quantities the reference draws once.
NumPy and torch-CPU only: nothing here touches the device (ops.dvs_emulator does)."""
import math

import numpy as np

MAX_ITERS_LIMIT = 4096


def lin_log_table():
    """float32 [256]: the reference's lin_log (emulator_utils.py) on 0 ... 255 -- x * ln(20) / 20 up to 20, ln(x) above, in
    float64, rounded to 8 decimals, then float32.  The kernel looks intensities up here; no device log is on the path."""
    x = np.arange(256, dtype=np.float64)
    f = (1.0 / 20) * math.log(20)
    with np.errstate(divide="ignore"):
        y = np.where(x <= 20, x * f, np.log(x))
    return (np.round(y * 1e8) / 1e8).astype(np.float32)


# set_dvs_params('clean') of the reference: no filter, no leak, no noise, thresholds 0.2 +- 0.02
CLEAN = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.02, cutoff_hz=0.0, leak_rate_hz=0.0, leak_jitter_fraction=0.0,
             noise_rate_cov_decades=0.0, shot_noise_rate_hz=0.0, refractory_period_s=0.0)


def dvs_params(model):
    """The named parameter set of the reference's set_dvs_params.  Only 'clean' exists here: 'noisy' turns on shot noise and
    leak jitter, whose per-frame random streams this emulator does not have."""
    if model == "clean":
        return dict(CLEAN)
    if model == "noisy":
        raise ValueError("dvs_params 'noisy' needs shot noise and leak jitter, which the device emulator does not model; "
                         "use 'clean' or give the parameters one by one")
    raise ValueError("dvs_params %r not known: use 'clean'" % (model,))


def draw_pixel_arrays(h, w, pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, noise_rate_cov_decades=0.1, leak_rate_hz=0.0, seed=0):
    """The per-pixel arrays EventEmulator._init draws once, on the CPU with torch's generator and in _init's order:
    pos_thres ~ normal(pos_thres, sigma_thres) clamped at 0.01, neg_thres likewise (both only when sigma_thres > 0, else the
    scalars come back), and with leak_rate_hz > 0 noise_rate_array = exp(ln 10 * noise_rate_cov_decades * randn).
    Returns (pos, neg, noise_rate_array or None); seed != 0 seeds torch first, as the reference's constructor does."""
    import torch
    if sigma_thres < 0 or noise_rate_cov_decades < 0:
        raise ValueError("sigma_thres and noise_rate_cov_decades must be >= 0")
    if seed != 0:
        torch.manual_seed(seed)
    pos, neg, noise = float(pos_thres), float(neg_thres), None
    if sigma_thres > 0:
        pos = torch.clamp(torch.normal(pos, sigma_thres, size=(h, w), dtype=torch.float32), min=0.01).numpy()
        neg = torch.clamp(torch.normal(neg, sigma_thres, size=(h, w), dtype=torch.float32), min=0.01).numpy()
    if leak_rate_hz > 0:
        noise = torch.exp(math.log(10) * noise_rate_cov_decades * torch.randn((h, w), dtype=torch.float32)).numpy()
    return pos, neg, noise


def _threshold(name, v, h, w):
    a = np.asarray(v, dtype=np.float32)
    if a.ndim == 0:
        if not (np.isfinite(a) and a > 0):
            raise ValueError("dvs_emulator: %s must be a finite value > 0 (got %r)" % (name, v))
        return float(a), None
    if a.shape != (h, w):
        raise ValueError("dvs_emulator: %s must be a scalar or an array of shape (%d, %d) (got %s)" % (name, h, w, a.shape))
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError("dvs_emulator: every %s must be finite and > 0" % name)
    return 0.0, np.ascontiguousarray(a)


def validate(h, w, pos_thres=0.2, neg_thres=0.2, cutoff_hz=0.0, leak_rate_hz=0.0, noise_rate_array=None, refractory_period_s=0.0,
             shot_noise_rate_hz=0.0, leak_jitter_fraction=0.0, max_iters=1024):
    """Checks one parameter set and returns it in the form the device call takes: dict(h, w, pos, pos_map, neg, neg_map,
    noise_map, cutoff_hz, leak_rate_hz, refractory_period_s, max_iters) with scalars as Python floats and maps as float32
    (h, w) arrays or None.  Shot noise and a non-zero leak jitter are refused: both draw random numbers every frame."""
    h, w = int(h), int(w)
    if h < 1 or w < 1 or h * w > (1 << 24):
        raise ValueError("dvs_emulator: bad frame size %d x %d" % (w, h))
    if shot_noise_rate_hz != 0:
        raise ValueError("dvs_emulator: shot_noise_rate_hz != 0 is not supported: shot noise draws random numbers every frame, "
                         "a stream that cannot be pinned to the reference's")
    if leak_jitter_fraction != 0:
        raise ValueError("dvs_emulator: leak_jitter_fraction != 0 is not supported: the jitter draws random numbers every frame, "
                         "a stream that cannot be pinned to the reference's")
    for name, v in (("cutoff_hz", cutoff_hz), ("leak_rate_hz", leak_rate_hz), ("refractory_period_s", refractory_period_s)):
        if not (isinstance(v, (int, float, np.floating, np.integer)) and math.isfinite(v) and v >= 0):
            raise ValueError("dvs_emulator: %s must be a finite number >= 0 (got %r)" % (name, v))
    pos, pos_map = _threshold("pos_thres", pos_thres, h, w)
    neg, neg_map = _threshold("neg_thres", neg_thres, h, w)
    noise_map = None
    if noise_rate_array is not None:
        a = np.asarray(noise_rate_array, dtype=np.float32)
        if a.ndim == 0:
            a = np.full((h, w), a, np.float32)
        if a.shape != (h, w) or not np.isfinite(a).all():
            raise ValueError("dvs_emulator: noise_rate_array must be a finite scalar or (%d, %d) array" % (h, w))
        noise_map = np.ascontiguousarray(a)
    max_iters = int(max_iters)
    if not (1 <= max_iters <= MAX_ITERS_LIMIT) or 2 * h * w * max_iters >= (1 << 31):
        raise ValueError("dvs_emulator: max_iters must be in 1 ... %d with 2 * h * w * max_iters < 2^31 (got %d)"
                         % (MAX_ITERS_LIMIT, max_iters))
    return dict(h=h, w=w, pos=pos, pos_map=pos_map, neg=neg, neg_map=neg_map, noise_map=noise_map, cutoff_hz=float(cutoff_hz),
                leak_rate_hz=float(leak_rate_hz), refractory_period_s=float(refractory_period_s), max_iters=max_iters)


def check_times(t, t_prev=None):
    """float64 array of the stamps; raises the reference's ValueError when one is not later than its predecessor."""
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1))
    if not np.isfinite(t).all():
        raise ValueError("dvs_emulator: frame times must be finite")
    prev = t_prev
    for k, v in enumerate(t.tolist()):
        if prev is not None and v <= prev:
            raise ValueError("this frame time={} must be later than previous frame time={}".format(v, prev))
        prev = v
    return t
