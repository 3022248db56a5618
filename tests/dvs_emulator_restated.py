"""The DVS emulator core, restated with torch tensor expressions (CPU by default): what csrc/dvs_emulator.hip has to equal
bit for bit, and what tests/golden/dvs_emulator_reference.npz (recorded from the reference's EventEmulator) pins.

State after frame 0: base = lp0 = lp1 = lin_log(frame0), timestamp_mem = -refractory, t_prev = t0.  Every later frame:
  1. log_new = lin_log(frame)                       float64 formula, rounded to 1e-8, then float32: a 256-entry table
  2. cutoff > 0: eps = min(((frame + 20) / 275) * (dt / tau), 1); lp0' = (1 - eps) * lp0 + eps * log_new; lp1' = the OLD lp0
     else lp0' = lp1' = log_new
  3. leak > 0: base -= (dt * (leak * noise_rate)) * pos_thres
  4. diff = lp1' - base; ON / OFF = floor_divide(relu(+-diff), thres) as int32 (torch's fmod form); n = max over the frame
  5. ts_step = reciprocal(n) * dt in float32; stamps = linspace(t_prev + ts_step, t_frame, n) in float32
  6. for i < n: pos = ON >= i + 1, neg = OFF >= i + 1; if refractory > ts_step both become
     ((cord ? ts[i] : 0) - timestamp_mem) > refractory, then timestamp_mem = ts[i] where either fired;
     rows: all ON pixels row-major, then all OFF pixels row-major, [ts[i], x, y, +-1]
  7. base += final_ON * pos_thres; base -= final_OFF * neg_thres

Scalars meet float32 tensors as float32 (a Python float next to a float32 tensor is rounded to float32 first), which is why
dt, dt / tau, the leak rate, scalar thresholds and the refractory period are all rounded before they are used.  The linspace is
written out: start for one step, else step = (end - start) / (n - 1) in float32 and element i = start + step * i for i < n // 2,
end - step * (n - 1 - i) otherwise, each with ONE rounding (evaluated in float64, where the product is exact).

The reference shuffles the rows of one sub-iteration (they share a stamp); this emits them unshuffled, and `canonical` sorts
each equal-stamp group of an (N, 4) array by (polarity ON first, y, x) -- the order the unshuffled form has already.
"""
import math

import numpy as np
import torch

F32 = torch.float32


def lin_log_table():
    """lin_log on 0 ... 255, the float32 values the reference computes through float64."""
    x = np.arange(256, dtype=np.float64)
    f = (1.0 / 20) * math.log(20)
    with np.errstate(divide="ignore"):
        y = np.where(x <= 20, x * f, np.log(x))
    return (np.round(y * 1e8) / 1e8).astype(np.float32)


def floor_divide_f32(a, b):
    """torch.div(a, b, rounding_mode='floor') on float32 tensors, written out (b != 0, finite operands)."""
    mod = torch.fmod(a, b)
    div = (a - mod) / b
    div = torch.where((mod != 0) & ((b < 0) != (mod < 0)), div - 1, div)
    fl = torch.floor(div)
    fl = torch.where(div - fl > 0.5, fl + 1, fl)
    return torch.where(div != 0, fl, torch.copysign(torch.zeros_like(div), a / b))


def linspace_f32(start, end, n):
    """float32 numpy array of n stamps (see the module docstring)."""
    start = np.float32(start); end = np.float32(end)
    if n == 0:
        return np.zeros(0, np.float32)
    if n == 1:
        return np.array([start], np.float32)
    step = np.float32((end - start) / np.float32(n - 1))
    i = np.arange(n, dtype=np.float64)
    lo = np.float64(start) + np.float64(step) * i
    hi = np.float64(end) - np.float64(step) * (n - 1 - i)
    return np.where(np.arange(n) < n // 2, lo, hi).astype(np.float32)


def canonical(rows):
    """Stable sort of every run of equal stamps by (ON before OFF, y, x); rows (N, 4) [ts, x, y, +-1]."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    out = rows.copy()
    n = len(rows)
    s = 0
    while s < n:
        e = s
        while e < n and rows[e, 0] == rows[s, 0]:
            e += 1
        g = rows[s:e]
        order = np.lexsort((g[:, 1], g[:, 2], -g[:, 3]))
        out[s:e] = g[order]
        s = e
    return out


def stamps_us(ts):
    """The reference's h5 rule: uint32(float32(ts) * 1e6), the product in float32, truncated."""
    return (np.asarray(ts, dtype=np.float32) * np.float32(1e6)).astype(np.uint32).astype(np.int64)


class RestatedEmulator:
    def __init__(self, pos_thres=0.2, neg_thres=0.2, cutoff_hz=0.0, leak_rate_hz=0.0, noise_rate_array=None,
                 refractory_period_s=0.0, device="cpu"):
        self.device = torch.device(device)
        self.pos_thres = self._param(pos_thres)
        self.neg_thres = self._param(neg_thres)
        self.cutoff_hz = float(cutoff_hz)
        self.leak_rate_hz = float(leak_rate_hz)
        self.noise_rate = self._param(1.0 if noise_rate_array is None else noise_rate_array)
        self.refractory = float(refractory_period_s)
        self.table = torch.from_numpy(lin_log_table()).to(self.device)
        self.base = None
        self.num_iters = []                    # one entry per frame after the first: for the tests

    def _param(self, v):
        return torch.as_tensor(np.asarray(v, dtype=np.float32)).to(self.device)      # 0-d or H x W float32

    def reset(self):
        self.base = None
        self.num_iters = []

    def state(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("base", "lp0", "lp1", "tmem")}

    def frame(self, frame_u8, t):
        """One frame; returns (ts float32, x int32, y int32, pol int8 in {+1, -1}) device tensors (None for frame 0)."""
        dev = self.device
        frame_u8 = torch.as_tensor(frame_u8).to(dev)
        t = float(t)
        log_new = self.table[frame_u8.long()]
        if self.base is None:
            self.base = log_new.clone(); self.lp0 = log_new.clone(); self.lp1 = log_new.clone()
            self.tmem = torch.zeros_like(log_new) - torch.tensor(self.refractory, dtype=F32, device=dev)
            self.t_prev = t
            return None
        if t <= self.t_prev:
            raise ValueError("this frame time=%r must be later than previous frame time=%r" % (t, self.t_prev))
        dt = t - self.t_prev
        sc = lambda v: torch.tensor(v, dtype=F32, device=dev)       # a Python float meeting a float32 tensor
        if self.cutoff_hz > 0:
            inten01 = (frame_u8.to(F32) + sc(20.0)) / sc(275.0)
            tau = 1 / (math.pi * 2 * self.cutoff_hz)
            eps = torch.clamp(inten01 * sc(dt / tau), max=1)
            old0 = self.lp0
            self.lp0 = (1 - eps) * old0 + eps * log_new
            self.lp1 = old0
        else:
            self.lp0 = log_new; self.lp1 = log_new
        if self.leak_rate_hz > 0:
            self.base = self.base - (sc(dt) * (sc(self.leak_rate_hz) * self.noise_rate)) * self.pos_thres
        diff = self.lp1 - self.base
        on = floor_divide_f32(torch.relu(diff), self.pos_thres.expand_as(diff)).to(torch.int32)
        off = floor_divide_f32(torch.relu(-diff), self.neg_thres.expand_as(diff)).to(torch.int32)
        n = int(torch.maximum(on.max(), off.max()))
        self.num_iters.append(n)
        fin_on = torch.zeros_like(on); fin_off = torch.zeros_like(off)
        out = []
        if n > 0:
            ts_step = np.float32(np.float32(1.0) / np.float32(n)) * np.float32(dt)
            ts = linspace_f32(np.float32(self.t_prev) + ts_step, np.float32(t), n)
            refr = np.float32(self.refractory)
            filt = bool(refr > ts_step)
            for i in range(n):
                pos = on >= i + 1; neg = off >= i + 1
                if filt:
                    tsi = sc(float(ts[i]))
                    pos_since = pos * tsi - self.tmem
                    neg_since = neg * tsi - self.tmem
                    pos = pos_since > sc(float(refr)); neg = neg_since > sc(float(refr))
                    self.tmem = torch.where(pos | neg, tsi, self.tmem)
                fin_on += pos; fin_off += neg
                py, px = pos.nonzero(as_tuple=True); ny, nx = neg.nonzero(as_tuple=True)
                k = int(py.numel()) + int(ny.numel())
                if k:
                    pol = torch.ones(k, dtype=torch.int8, device=dev); pol[py.numel():] = -1
                    out.append((torch.full((k,), float(ts[i]), dtype=F32, device=dev), torch.cat([px, nx]).to(torch.int32),
                                torch.cat([py, ny]).to(torch.int32), pol))
        self.base = self.base + fin_on * self.pos_thres
        self.base = self.base - fin_off * self.neg_thres
        self.t_prev = t
        if not out:
            z = lambda dt_: torch.zeros(0, dtype=dt_, device=dev)
            return z(F32), z(torch.int32), z(torch.int32), z(torch.int8)
        return tuple(torch.cat([o[j] for o in out]) for j in range(4))

    def emulate(self, frames, t):
        """All frames; returns the (N, 4) float32 rows [ts, x, y, +-1] in the unshuffled order (numpy)."""
        parts = []
        for k in range(len(frames)):
            r = self.frame(frames[k], t[k])
            if r is not None and r[0].numel():
                parts.append(torch.stack([r[0], r[1].to(F32), r[2].to(F32), r[3].to(F32)], 1).cpu().numpy())
        return np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


def columns(rows):
    """(t int64 us, x int32, y int32, p int8 ON = 1 / OFF = 0, t_s float32): the device's output columns of restated rows."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    return (stamps_us(rows[:, 0]), rows[:, 1].astype(np.int32), rows[:, 2].astype(np.int32),
            (rows[:, 3] > 0).astype(np.int8), rows[:, 0].copy())


# ------------------------------------------------------------------------------------------------ the shared test cases
def moving_frames(seed, f, h, w, steps=3):
    """f uint8 frames: a smooth gradient that moves, plus a few isolated pixels that step."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, 2)
    out = np.empty((f, h, w), np.uint8)
    for k in range(f):
        g = 90 + 70 * np.sin(2 * np.pi * (xx - 2.5 * k) / w + ph[0]) + 40 * np.cos(2 * np.pi * (yy + 1.5 * k) / h + ph[1])
        out[k] = np.clip(np.round(g), 0, 255).astype(np.uint8)
    for _ in range(steps):
        y, x, k = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(1, f))
        out[k:, y, x] = 255 - out[k:, y, x]
    return out


def make_cases(h, w, f=7):
    """name -> dict(frames, t, and the emulator's keyword arguments): the cases both the fixture and the device tests run."""
    rng = np.random.default_rng(1000 + h * w)
    t_even = 0.5 + 0.01 * np.arange(f)
    cases = {}
    cases["scalar"] = dict(frames=moving_frames(1, f, h, w), t=t_even, pos_thres=0.2, neg_thres=0.2)
    pos = np.clip(rng.normal(0.2, 0.05, (h, w)), 0.01, None).astype(np.float32)
    neg = np.clip(rng.normal(0.2, 0.05, (h, w)), 0.01, None).astype(np.float32)
    pos[h // 2, w // 3] = 0.01; neg[h // 3, w // 2] = 0.01                       # pixels at the clamp
    cases["perpixel"] = dict(frames=moving_frames(2, f, h, w), t=t_even, pos_thres=pos, neg_thres=neg)
    cases["cutoff"] = dict(frames=moving_frames(3, f, h, w), t=t_even, pos_thres=0.2, neg_thres=0.2, cutoff_hz=30.0)
    nra = np.exp(math.log(10) * 0.3 * rng.standard_normal((h, w))).astype(np.float32)
    cases["leak"] = dict(frames=moving_frames(4, f, h, w), t=0.25 + 0.4 * np.arange(f), pos_thres=pos, neg_thres=0.15,
                         leak_rate_hz=0.7, noise_rate_array=nra)
    # ts_step = dt / num_iters (about 20 here): the 10 ms refractory filter is active after the short steps, inactive after the long ones
    dts = np.array([0.004, 0.6, 0.01, 0.9, 0.002, 0.7, 0.02, 0.5, 0.04])[:f - 1]
    cases["refractory"] = dict(frames=moving_frames(5, f, h, w), t=1.0 + np.concatenate([[0.0], np.cumsum(dts)]),
                               pos_thres=0.2, neg_thres=0.18, refractory_period_s=0.01)
    fr = moving_frames(6, f, h, w)
    fr[2] = fr[1]; fr[5 % f] = fr[4 % f]
    cases["repeat"] = dict(frames=fr, t=t_even, pos_thres=0.2, neg_thres=0.2)
    fr = np.zeros((f, h, w), np.uint8)
    fr[3:, h // 2, w - 2] = 255
    cases["step"] = dict(frames=fr, t=t_even, pos_thres=0.2, neg_thres=0.2)
    cases["all"] = dict(frames=moving_frames(7, f, h, w), t=1.0 + np.concatenate([[0.0], np.cumsum(dts[::-1])]), pos_thres=pos,
                        neg_thres=neg, cutoff_hz=30.0, leak_rate_hz=0.7, noise_rate_array=nra, refractory_period_s=0.01)
    return cases


PARAM_KEYS = ("pos_thres", "neg_thres", "cutoff_hz", "leak_rate_hz", "noise_rate_array", "refractory_period_s")


def case_params(case):
    return {k: case[k] for k in PARAM_KEYS if k in case}
