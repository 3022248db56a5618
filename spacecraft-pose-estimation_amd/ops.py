"""Thin torch-facing wrappers over the C ABI (device memory, streams: plumbing only).

Every function here launches HIP kernels from libscpose_hip.so on the current torch
stream; tensors must live on a ROCm device.  Nothing falls back to eager PyTorch.
"""
import collections
import ctypes
from ctypes import c_int32, c_int64, c_void_p, c_char_p, c_size_t, c_double

import numpy as np
import torch

from . import _native as nat, image_read, jpeg_read as jr, png_read as pr

_TORCH_DT = {nat.DT_BF16: torch.bfloat16, nat.DT_F16: torch.float16}
_DT_OF = {"bf16": nat.DT_BF16, "f16": nat.DT_F16, "fp16": nat.DT_F16, "bfloat16": nat.DT_BF16,
          "float16": nat.DT_F16}


def dtype_code(dtype):
    if isinstance(dtype, int):
        return dtype
    return _DT_OF[str(dtype).replace("torch.", "")]


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise nat.NativeError("scpose ops need device tensors (got %s); there is no CPU path" % t.device)


def _query_bytes(name, *args):
    """The size query scpose_<name>(*args, &bytes) of the C ABI -> bytes."""
    b = c_size_t()
    nat.check(getattr(nat.lib(), "scpose_" + name)(*args, ctypes.byref(b)), name)
    return b.value


def _empty_event_columns(n, dev):
    """Uninitialised (t int64, x int32, y int32, p int8) columns of n rows on dev."""
    return tuple(torch.empty(n, dtype=dt, device=dev) for dt in (torch.int64, torch.int32, torch.int32, torch.int8))


# ------------------------------------------------------------------ layout
def to_blocked(x, dtype="bf16"):
    """float32 NCHW (C % 8 == 0) -> blocked [N][C/8][H][W][8] 16-bit tensor."""
    _need_cuda(x)
    dt = dtype_code(dtype)
    x = x.contiguous().float()
    n, c, h, w = x.shape
    out = torch.empty((n, c // 8, h, w, 8), dtype=_TORCH_DT[dt], device=x.device)
    nat.check(nat.lib().scpose_nchw_f32_to_blocked(_ptr(x), n, c, h, w, dt, _ptr(out), _stream()), "nchw_f32_to_blocked")
    return out


def from_blocked(xb):
    """blocked 16-bit tensor -> float32 NCHW."""
    _need_cuda(xb)
    n, cg, h, w, _ = xb.shape
    dt = nat.DT_BF16 if xb.dtype == torch.bfloat16 else nat.DT_F16
    out = torch.empty((n, cg * 8, h, w), dtype=torch.float32, device=xb.device)
    nat.check(nat.lib().scpose_blocked_to_nchw_f32(_ptr(xb), n, cg * 8, h, w, dt, _ptr(out), _stream()), "blocked_to_nchw_f32")
    return out


# ------------------------------------------------------------------ single conv layer
class Conv:
    """One (BN-folded) convolution on the MFMA kernel: y = [relu](conv(x) + b [+ res])."""

    def __init__(self, weight, bias=None, stride=1, dtype="bf16"):
        w = weight.detach().float().cpu().contiguous()
        self.cout, self.cin, self.ks, _ = w.shape
        self.stride = stride
        self.dt = dtype_code(dtype)
        b = bias.detach().float().cpu().contiguous() if bias is not None else None
        h = c_void_p()
        nat.check(nat.lib().scpose_conv_create(c_void_p(w.data_ptr()), c_void_p(b.data_ptr()) if b is not None else c_void_p(0),
                                               self.cout, self.cin, self.ks, stride, self.dt, ctypes.byref(h)), "conv_create")
        self._h = h

    def __call__(self, xb, residual=None, relu=False, out_nchw_f32=False):
        _need_cuda(xb, residual)
        n, cg, h, w, _ = xb.shape
        assert cg * 8 == self.cin, (cg * 8, self.cin)
        ho, wo = (h - 1) // self.stride + 1, (w - 1) // self.stride + 1
        if out_nchw_f32:
            out = torch.empty((n, self.cout, ho, wo), dtype=torch.float32, device=xb.device)
        else:
            out = torch.empty((n, self.cout // 8, ho, wo, 8), dtype=xb.dtype, device=xb.device)
        nat.check(nat.lib().scpose_conv_forward(self._h, _ptr(xb), n, h, w, _ptr(residual), int(relu), int(out_nchw_f32),
                                                _ptr(out), _stream()), "conv_forward")
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                nat.lib().scpose_conv_destroy(self._h)
                self._h = None
        except Exception:
            pass


class GatherConv:
    """One pose_resnet layer of csrc/conv_gather.hip: y = [relu](layer(x) + b [+ res]), blocked 16-bit in and out.
    deconv_kernel 4 / 3 / 2: ConvTranspose2d(stride 2), weight (cin, cout, k, k), out 2h x 2w; None: Conv2d 1x1 stride 2, weight
    (cout, cin, 1, 1), out ceil(h / 2) x ceil(w / 2)."""

    def __init__(self, weight, bias=None, deconv_kernel=None, dtype="bf16"):
        w = weight.detach().float().cpu().contiguous()
        self.deconv = deconv_kernel is not None
        self.cin, self.cout = (w.shape[0], w.shape[1]) if self.deconv else (w.shape[1], w.shape[0])
        b = bias.detach().float().cpu().contiguous() if bias is not None else None
        pb = c_void_p(b.data_ptr()) if b is not None else c_void_p(0)
        h = c_void_p()
        if self.deconv:
            nat.check(nat.lib().scpose_deconv_create(c_void_p(w.data_ptr()), pb, self.cin, self.cout, int(deconv_kernel), dtype_code(dtype),
                                                     ctypes.byref(h)), "deconv_create")
        else:
            nat.check(nat.lib().scpose_conv1x1s2_create(c_void_p(w.data_ptr()), pb, self.cout, self.cin, dtype_code(dtype), ctypes.byref(h)),
                      "conv1x1s2_create")
        self._h = h

    def __call__(self, xb, residual=None, relu=False):
        _need_cuda(xb, residual)
        n, cg, h, w, _ = xb.shape
        assert cg * 8 == self.cin, (cg * 8, self.cin)
        ho, wo = (2 * h, 2 * w) if self.deconv else ((h + 1) // 2, (w + 1) // 2)
        out = torch.empty((n, self.cout // 8, ho, wo, 8), dtype=xb.dtype, device=xb.device)
        nat.check(nat.lib().scpose_gather_forward(self._h, _ptr(xb), n, h, w, _ptr(residual), int(relu), _ptr(out), _stream()), "gather_forward")
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                nat.lib().scpose_gather_destroy(self._h)
                self._h = None
        except Exception:
            pass


def resnet_stem(x, weight, bias, dtype="bf16", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """relu(conv 7x7 s2 p3 (3 -> 64) + bias) -> max-pool 3x3 s2 p1 as one launch (csrc/resnet_stem.hip).  x: uint8 (N, H, W, 3), normalised
    with mean / std, or float32 (N, 3, H, W); weight (64, 3, 7, 7) and bias (64,) BN-folded.  Returns blocked 16-bit 64 x H/4 x W/4."""
    _need_cuda(x)
    x = x.contiguous()
    fmt, n, h, w = HrnetEngine._input_format(x, "resnet_stem")
    wt = weight.detach().float().cpu().contiguous(); b = bias.detach().float().cpu().contiguous()
    ms = torch.tensor(list(mean) + list(std), dtype=torch.float32)
    dt = dtype_code(dtype)
    out = torch.empty((n, 8, h // 4, w // 4, 8), dtype=_TORCH_DT[dt], device=x.device)
    nat.check(nat.lib().scpose_resnet_stem_forward(c_void_p(wt.data_ptr()), c_void_p(b.data_ptr()), c_void_p(ms.data_ptr()), _ptr(x), fmt,
                                                   n, h, w, dt, _ptr(out), _stream()), "resnet_stem_forward")
    return out


def fuse_sum(terms, shifts, out_hw):
    """relu(sum_t nearest_upsample(term_t, 2**shift_t)); terms blocked, out at (H, W)."""
    _need_cuda(*terms)
    h, w = out_hw
    n, cg = terms[0].shape[0], terms[0].shape[1]
    dt = nat.DT_BF16 if terms[0].dtype == torch.bfloat16 else nat.DT_F16
    out = torch.empty((n, cg, h, w, 8), dtype=terms[0].dtype, device=terms[0].device)
    tp = (c_void_p * len(terms))(*[t.data_ptr() for t in terms])
    sh = (c_int32 * len(terms))(*shifts)
    nat.check(nat.lib().scpose_fuse_sum(tp, sh, len(terms), n, cg * 8, h, w, dt, _ptr(out), _stream()), "fuse_sum")
    return out


# ------------------------------------------------------------------ decode
def decode(heatmaps, center, scale, post_process=True):
    """heatmaps (N,J,H,W) f32 device; center/scale (N,2) f32 device -> (N,J,3) [x_img,y_img,maxval]."""
    _need_cuda(heatmaps, center, scale)
    hm = heatmaps.contiguous().float()
    n, j, h, w = hm.shape
    c = center.contiguous().float()
    s = scale.contiguous().float()
    out = torch.empty((n, j, 3), dtype=torch.float32, device=hm.device)
    nat.check(nat.lib().scpose_decode(_ptr(hm), n, j, h, w, _ptr(c), _ptr(s), int(bool(post_process)), _ptr(out), _stream()), "decode")
    return out


def max_preds(heatmaps):
    _need_cuda(heatmaps)
    hm = heatmaps.contiguous().float()
    n, j, h, w = hm.shape
    coords = torch.empty((n, j, 2), dtype=torch.float32, device=hm.device)
    maxvals = torch.empty((n, j, 1), dtype=torch.float32, device=hm.device)
    nat.check(nat.lib().scpose_max_preds(_ptr(hm), n, j, h, w, _ptr(coords), _ptr(maxvals), _stream()), "max_preds")
    return coords, maxvals


def crop_warp(frames, trans, out_wh, swap_rb=False, device=None, roi=None, frame_hw=None):
    """Batched cv2.warpAffine(frame_i, trans_i, (W, H), INTER_LINEAR) on the device.
    frames: list of HxWx3 uint8 arrays/tensors (any sizes); trans: (N,2,3) forward affines as returned by
    get_affine_transform (frame -> crop).  Returns uint8 (N, H, W, 3) device crops.
    roi (N,4) [x0, y0, w, h] + frame_hw (N,2): frames[i] is only that WINDOW of a frame of size frame_hw[i] (warp_window below
    computes one that contains every tap); same crops bit for bit (scpose_crop_warp_roi).
    ValueError, before anything is launched, for a transform with a non-finite entry."""
    import numpy as np
    packed = isinstance(frames, dict)      # pack_frames(): one flat uint8 tensor + offsets + sizes (what the data-loader workers send)
    if not packed:
        frames = pack_frames(frames)
    n = int(frames["hw"].shape[0])
    _finite_affines("crop_warp", trans, n)
    dev = device or torch.device("cuda", torch.cuda.current_device())
    w, h = int(out_wh[0]), int(out_wh[1])
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    offs = frames["offsets"].tolist(); hw = [tuple(v) for v in frames["hw"].tolist()]
    buf = frames["flat"].to(dev, non_blocking=True)
    from .utils.transforms import invert_affine_cv
    minv = np.zeros((n, 6), dtype=np.float64)
    for i in range(n):
        minv[i] = invert_affine_cv(trans[i])            # the inverse map exactly as cv::warpAffine derives it
    offs_d = torch.tensor(offs, dtype=torch.int64, device=dev)
    minv_d = torch.from_numpy(minv).to(dev)
    if roi is not None:
        roi = np.asarray(roi, dtype=np.int32).reshape(n, 4); fhw = np.asarray(frame_hw, dtype=np.int32).reshape(n, 2)
        for i in range(n):
            if (int(roi[i, 3]), int(roi[i, 2])) != hw[i]:
                raise ValueError("crop_warp: window %d is %s but roi says %dx%d" % (i, hw[i], roi[i, 3], roi[i, 2]))
        fhw_d = torch.from_numpy(fhw).to(dev); roi_d = torch.from_numpy(roi).to(dev)      # (named: both must outlive the launch call)
        nat.check(nat.lib().scpose_crop_warp_roi(_ptr(buf), _ptr(offs_d), _ptr(fhw_d), _ptr(roi_d),
                                                 _ptr(minv_d), n, h, w, int(bool(swap_rb)), _ptr(out), _stream()), "crop_warp_roi")
        return out
    hw_d = torch.tensor(hw, dtype=torch.int32, device=dev)
    nat.check(nat.lib().scpose_crop_warp(_ptr(buf), _ptr(offs_d), _ptr(hw_d), _ptr(minv_d), n, h, w, int(bool(swap_rb)),
                                         _ptr(out), _stream()), "crop_warp")
    return out


def pack_frames(frames):
    """list of HxWx3 uint8 arrays / tensors (any sizes) -> {"flat": all bytes back to back, "offsets": int64 (n,), "hw": int32 (n, 2)}:
    the form scpose_crop_warp[_roi] takes.  The data-loader workers call it (dataset.collate_device_crop), so a batch crosses the
    process boundary as one tensor instead of one per frame."""
    import numpy as np
    flat, offs, hw, o = [], [], [], 0
    for f in frames:
        t = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("crop_warp: frames must be HxWx3 uint8")
        flat.append(t.reshape(-1)); offs.append(o); hw.append((t.shape[0], t.shape[1])); o += t.numel()
    return {"flat": torch.cat(flat) if flat else torch.zeros(0, dtype=torch.uint8), "offsets": torch.tensor(offs, dtype=torch.int64),
            "hw": torch.tensor(hw, dtype=torch.int32).reshape(-1, 2)}


def render_events(t, x, y, p, hw, interval=10000.0, full_scale=2, fold_polarity=True, K=None, dist=None, max_frames=None,
                  want_distorted=False, exposure="duration", event_count=None, area_count=None, area_dimension=None,
                  want_times=False):
    """Event stream -> event frames on the device: the reference's stage 0 (v2e/convert_aedats.py = e2v.py's renderer in DURATION
    mode + cv2.undistort) without a file.  t int64 ticks (time-sorted, not checked), x, y int32, p int8 / int32 (ON is p == 1;
    may be None with fold_polarity, which counts every event +1 as e2v.py does): device tensors of one length.  hw = (H, W).
    K (3x3) and dist [k1, k2, p1, p2, k3] (arrays or tensors) undistort every frame; both None: frames stay distorted.
    Returns (frames_dict, names): frames_dict in pack_frames() form with "flat" on the device -- F x H x W x 3 uint8 back to
    back, accepted as is by crop_warp -- plus "distorted" (F, H, W, 3) with want_distorted; names = the reference's file stems
    (event_render.frame_schedule).  Three stamps (t[0], t[n-2], t[n-1]) are read back for the schedule: one small sync.

    exposure selects how a frame ends, as e2v.py's --dvs_exposure does (event_render.parse_dvs_exposure):
      "duration"    every `interval` ticks (the default, above)
      "count"       every event_count events (int(float(event_count)) >= 1): frame k = [kN, (k+1)N) of the stream
      "area_count"  when any area_dimension x area_dimension area has received area_count events since the frame began
                    (csrc/events_exposure.hip); a coordinate off the area grid raises ValueError
    In both count modes the host reads back the frame count (area_count only) and one float64 per frame, the frame time
    (t[begin] + t[end]) / 2 the stem is formatted from; never the stream.  want_times: frames_dict["times"] = those frame
    times (float64 numpy, what the reference's frame-times file lists)."""
    from . import event_render as er
    mode = str(exposure).lower()
    if mode not in ("duration", "count", "area_count"):
        raise ValueError("render_events: exposure must be 'duration', 'count' or 'area_count' (got %r)" % (exposure,))
    n = _check_stream(t, x, y, p, fold_polarity, K, dist)
    t, x, y = t.contiguous(), x.contiguous(), y.contiguous()
    p = p.contiguous() if p is not None else None
    dev = t.device
    h, w = int(hw[0]), int(hw[1])
    lut = er.gray_table(full_scale)
    lib = nat.lib()
    times = None
    with torch.cuda.device(dev):
        if mode == "duration":
            if n >= 2:
                first, before_last, last = t[torch.tensor([0, n - 2, n - 1], device=dev)].tolist()
                starts, names = er.frame_schedule(first, before_last, last, interval, max_frames)
            else:
                starts, names = np.zeros(1), []
            f = len(names)
            starts_d = torch.from_numpy(starts).to(dev)
            bounds = torch.empty((f, 2), dtype=torch.int64, device=dev)
            nat.check(lib.scpose_events_frame_bounds(_ptr(t), n, _ptr(starts_d), f, _ptr(bounds), _stream()), "events_frame_bounds")
            if want_times:
                step = 1.0 / (1.0 / float(interval))
                times = np.asarray([starts[k + 1] + step / 2 for k in range(f)], dtype=np.float64)
        else:
            bounds = _counted_bounds(x, y, n, h, w, mode, event_count, area_count, area_dimension, max_frames)
            f = int(bounds.shape[0])
            mids = torch.empty(f, dtype=torch.float64, device=dev)
            nat.check(lib.scpose_events_bounds_midpoints(_ptr(t), _ptr(bounds), f, _ptr(mids), _stream()), "events_bounds_midpoints")
            times = mids.cpu().numpy()
            names = ["{:.0f}".format(v) for v in times.tolist()]
        ws = _query_bytes("events_workspace_bytes", f, h, w)
        frames = torch.empty((f, h, w, 3), dtype=torch.uint8, device=dev)
        out = {"flat": frames.view(-1), "offsets": torch.arange(f, dtype=torch.int64) * (h * w * 3),
               "hw": torch.tensor([[h, w]] * f, dtype=torch.int32).reshape(-1, 2)}
        distorted = torch.empty((f, h, w, 3), dtype=torch.uint8, device=dev) if want_distorted else None
        if want_distorted:
            out["distorted"] = distorted
        lut_d = torch.from_numpy(lut).to(dev)
        k_d = torch.as_tensor(np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64).reshape(3, 3)).to(dev) if K is not None else None
        d_d = torch.as_tensor(np.asarray(dist.cpu() if torch.is_tensor(dist) else dist, dtype=np.float64).reshape(5)).to(dev) if dist is not None else None
        work = torch.empty(ws if K is not None else 0, dtype=torch.uint8, device=dev)
        nat.check(lib.scpose_events_render(_ptr(x), _ptr(y), _ptr(p), p.element_size() if p is not None else 0, _ptr(bounds), f, h, w,
                                           int(full_scale), int(bool(fold_polarity)), _ptr(lut_d), _ptr(k_d), _ptr(d_d), _ptr(frames),
                                           _ptr(distorted), _ptr(work), work.numel(), _stream()), "events_render")
    if want_times:
        out["times"] = times
    return out, names


def _check_stream(t, x, y, p, fold_polarity, K, dist):
    if p is None and not fold_polarity:
        raise ValueError("render_events: fold_polarity=False needs the polarity column")
    _need_cuda(t, x, y, p)
    n = int(t.numel())
    if t.dtype != torch.int64 or x.dtype != torch.int32 or y.dtype != torch.int32 or x.numel() != n or y.numel() != n:
        raise ValueError("render_events: t must be int64, x and y int32, all of one length")
    if p is not None and (p.dtype not in (torch.int8, torch.int32) or p.numel() != n):
        raise ValueError("render_events: p must be int8 or int32 of the stream's length")
    if (K is None) != (dist is None):
        raise ValueError("render_events: give K and dist together, or neither")
    return n


def _counted_bounds(x, y, n, h, w, mode, event_count, area_count, area_dimension, max_frames):
    """The (F, 2) frame bounds of render_events' exposure = "count" / "area_count" (csrc/events_exposure.hip), on the current
    device; max_frames caps F."""
    lib = nat.lib()
    dev = x.device
    if mode == "count":
        if event_count is None:
            raise ValueError("render_events: exposure='count' needs event_count")
        N = int(float(event_count))
        if N < 1:
            raise ValueError("render_events: event_count must be >= 1 after truncation (got %r)" % (event_count,))
        fc = c_int64()
        nat.check(lib.scpose_events_count_frames(n, N, ctypes.byref(fc)), "events_count_frames")
        f = fc.value if max_frames is None else min(fc.value, int(max_frames))
        bounds = torch.empty((f, 2), dtype=torch.int64, device=dev)
        nat.check(lib.scpose_events_count_bounds(n, N, f, _ptr(bounds), _stream()), "events_count_bounds")
        return bounds
    if area_count is None or area_dimension is None:
        raise ValueError("render_events: exposure='area_count' needs area_count and area_dimension")
    M, D = int(area_count), int(area_dimension)
    if M < 2:
        raise ValueError("render_events: area_count must be >= 2 (got %d)" % M)
    if D < 1:
        raise ValueError("render_events: area_dimension must be >= 1 (got %d)" % D)
    ws = _query_bytes("events_area_bounds_workspace_bytes", n, M, D, h, w)
    cap = (n - 2) // (M - 1) if n >= 2 else 0
    bounds = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=dev)
    cs = torch.empty(2, dtype=torch.int64, device=dev)
    work = torch.empty(ws, dtype=torch.uint8, device=dev)
    nat.check(lib.scpose_events_area_bounds(_ptr(x), _ptr(y), n, M, D, h, w, _ptr(bounds), cap, _ptr(cs), _ptr(work), ws, _stream()),
              "events_area_bounds")
    f_all, status = cs.tolist()                            # the one small read-back: [F, status]
    del work
    if status == 1:
        raise ValueError("render_events: an event lies off the %d x %d area grid of area_dimension %d (x in [-%d, %d), "
                         "y in [-%d, %d))" % (1 + w // D, 1 + h // D, D, (1 + w // D) * D, (1 + w // D) * D,
                                              (1 + h // D) * D, (1 + h // D) * D))
    if status != 0:
        raise nat.NativeError("render_events: events_area_bounds status %d" % status)
    return bounds[:f_all if max_frames is None else min(f_all, int(max_frames))]


class UnsupportedCsv(ValueError):
    """parse_events_csv: the text is outside the grammar the device reader accepts (include/scpose.h:
    scpose_events_csv_parse).  The host reader, event_render.read_events_csv, takes the reference's whole grammar."""


def parse_events_csv(data, delim_whitespace=False, swap_xy=False, microseconds_timestamp=False, milliseconds_timestamp=False,
                     device=None):
    """events.csv text -> (t int64, x int32, y int32, p int8) device tensors, rows in file order: what
    event_render.read_events_csv gives (the reference's pandas.read_csv call of v2e/e2v.py), parsed on the device
    (csrc/events_csv.hip), in the dtypes render_events takes.  data: a uint8 device tensor holding the file's bytes, or bytes /
    bytearray / a path, uploaded in one piece to `device` (default: the current one).  The flags are e2v.py's.  One small
    read-back, [n_rows, status].  Raises UnsupportedCsv when the text is outside the accepted grammar (exponents, quotes, a wrong
    field count, a decimal column with more than 15 digits, ...: include/scpose.h lists it); the host reader is the fallback.
    Offsets are 64-bit, but files above 2^31 bytes have not been tested."""
    if torch.is_tensor(data):
        _need_cuda(data)
        if data.dtype != torch.uint8:
            raise ValueError("parse_events_csv: the bytes must be a uint8 tensor (got %s)" % data.dtype)
        buf = data.contiguous().view(-1)
    else:
        if isinstance(data, (bytes, bytearray, memoryview)):
            host = np.frombuffer(data, dtype=np.uint8)
        else:
            host = np.fromfile(data, dtype=np.uint8)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        buf = torch.from_numpy(host.copy() if not host.flags.writeable else host).to(dev)
    if buf.data_ptr() % 16:
        buf = buf.clone()
    dev = buf.device
    n = int(buf.numel())
    div = 1000000.0 if microseconds_timestamp else (1000.0 if milliseconds_timestamp else 0.0)
    cap = (n + 1) // 8                                          # the shortest row, '1,2,3,4' and a line end, takes 8 bytes
    lib = nat.lib()
    ws = _query_bytes("events_csv_workspace_bytes", n)
    with torch.cuda.device(dev):
        t, x, y, p = _empty_event_columns(cap, dev)
        cs = torch.empty(2, dtype=torch.int64, device=dev)
        work = torch.empty(ws, dtype=torch.uint8, device=dev)
        nat.check(lib.scpose_events_csv_parse(_ptr(buf), n, int(bool(delim_whitespace)), int(bool(swap_xy)), c_double(div), _ptr(t),
                                              _ptr(x), _ptr(y), _ptr(p), cap, _ptr(cs), _ptr(work), ws, _stream()),
                  "events_csv_parse")
        rows, status = cs.tolist()                              # the one small read-back
        if status == nat.CSV_UNSUPPORTED:
            raise UnsupportedCsv("parse_events_csv: the text is outside the grammar the device reader accepts")
        if status != 0:
            raise nat.NativeError("parse_events_csv: events_csv_parse status %d" % status)
        # the columns were sized for the shortest possible rows: give back right-sized ones
        return t[:rows].clone(), x[:rows].clone(), y[:rows].clone(), p[:rows].clone()


def events_text_tiling():
    """(rows per workgroup, rows per step of the offset scan) of the text formatter (csrc/events_write.hip)."""
    a, b = c_int32(), c_int32()
    nat.check(nat.lib().scpose_events_text_tiling(ctypes.byref(a), ctypes.byref(b)), "events_text_tiling")
    return a.value, b.value


def _event_columns(who, t, x, y, p):
    """The four columns as contiguous device tensors of the dtypes the kernels read; their device and row count."""
    _need_cuda(t, x, y, p)
    for name, c, dt in (("t", t, torch.int64), ("x", x, torch.int32), ("y", y, torch.int32), ("p", p, torch.int8)):
        if c.dtype != dt or c.dim() != 1:
            raise ValueError("%s: %s must be a 1-d %s tensor (got %s %s)" % (who, name, dt, c.dtype, tuple(c.shape)))
    n = int(t.numel())
    if not (x.numel() == n and y.numel() == n and p.numel() == n):
        raise ValueError("%s: the columns differ in length: %s" % (who, [int(c.numel()) for c in (t, x, y, p)]))
    if not (x.device == t.device and y.device == t.device and p.device == t.device):
        raise ValueError("%s: the columns live on different devices" % who)
    return t.contiguous(), x.contiguous(), y.contiguous(), p.contiguous(), t.device, n


def _sep_byte(sep):
    b = sep.encode() if isinstance(sep, str) else bytes(sep)
    if b not in (b" ", b","):
        raise ValueError("format_events_text: sep must be ' ' or ',' (got %r)" % (sep,))
    return b[0]


def format_events_text(t, x, y, p, sep=" ", swap_xy=False):
    """(t int64, x int32, y int32, p int8) device tensors -> a uint8 device tensor holding the rows as text, one
    `t SEP x SEP y SEP p` line per event with every value printed as "%d" (csrc/events_write.hip): the inverse of
    parse_events_csv, and byte for byte what `"%d %d %d %d\\n" % row` writes.  sep: ' ' or ','.  swap_xy: write y before x (the
    reader's flag).  The tensor has exactly the text's length; one small read-back, [n_bytes, status], sizes it."""
    sb = _sep_byte(sep)
    t, x, y, p, dev, n = _event_columns("format_events_text", t, x, y, p)
    lib = nat.lib()
    ws = _query_bytes("events_text_workspace_bytes", n)
    with torch.cuda.device(dev):
        work = torch.empty(ws, dtype=torch.uint8, device=dev)
        cs = torch.empty(2, dtype=torch.int64, device=dev)
        nat.check(lib.scpose_events_text_measure(_ptr(t), _ptr(x), _ptr(y), _ptr(p), n, _ptr(cs), _ptr(work), ws, _stream()),
                  "events_text_measure")
        n_bytes = int(cs.tolist()[0])                           # the one small read-back
        out = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        # capacity == n_bytes: the status word of emit cannot be set, and is not read back
        nat.check(lib.scpose_events_text_emit(_ptr(t), _ptr(x), _ptr(y), _ptr(p), n, sb, int(bool(swap_xy)), _ptr(out), n_bytes,
                                              _ptr(cs), _ptr(work), ws, _stream()), "events_text_emit")
    return out


def pack_events_aedat2(t, x, y, p, hw):
    """(t int64 microseconds, x int32, y int32, p int8 in {0, 1}) device tensors -> (uint8 device tensor of 8 * n bytes, lead):
    the AEDAT-2.0 records of the events for a sensor of hw = (height, width), two big-endian 32-bit words per event as the
    reference's AEDat2Output.appendEvents packs them (both axes flipped), and the number of leading records whose first byte is
    '#', which a writer drops at the start of a file (event_write.write_events_aedat2 does).  Raises ValueError when a
    coordinate or polarity is out of range or a time stamp is outside [0, 2^31).  One small read-back, [n, status, lead]."""
    h, w = int(hw[0]), int(hw[1])
    t, x, y, p, dev, n = _event_columns("pack_events_aedat2", t, x, y, p)
    lib = nat.lib()
    with torch.cuda.device(dev):
        out = torch.empty(8 * n, dtype=torch.uint8, device=dev)
        cs = torch.empty(3, dtype=torch.int64, device=dev)
        nat.check(lib.scpose_events_aedat2_pack(_ptr(t), _ptr(x), _ptr(y), _ptr(p), n, h, w, _ptr(out), _ptr(cs), _stream()),
                  "events_aedat2_pack")
        _, status, lead = cs.tolist()                           # the one small read-back
    if status & nat.AEDAT2_RANGE:
        raise ValueError("pack_events_aedat2: an event lies outside the %d x %d sensor, or a polarity is neither 0 nor 1" % (w, h))
    if status & nat.AEDAT2_TIME:
        raise ValueError("pack_events_aedat2: a time stamp is outside [0, 2^31) microseconds, which AEDAT-2.0 cannot hold")
    return out, int(lead)


AEDAT2_LAYOUTS = {"davis": nat.AEDAT2_LAYOUT_DAVIS, "v2e": nat.AEDAT2_LAYOUT_V2E}
AEDAT2_INFO = ("n_events", "n_other", "n_special", "n_wraps", "n_backward")


def _aedat2_layout(layout):
    try:
        return AEDAT2_LAYOUTS[str(layout).lower()]
    except KeyError:
        raise ValueError("unpack_events_aedat2: layout must be 'davis' or 'v2e' (got %r)" % (layout,))


def _unpack_events_aedat2_into(buf, n, hw, layout, flip_x, flip_y, unwrap, t_divisor, t, x, y, p, capacity):
    """One scpose_events_aedat2_unpack call on the current stream into caller-sized columns; returns count_status as a list
    (the one small read-back)."""
    h, w = int(hw[0]), int(hw[1])
    lib = nat.lib()
    ws = _query_bytes("events_aedat2_unpack_workspace_bytes", n)
    with torch.cuda.device(buf.device):
        cs = torch.empty(6, dtype=torch.int64, device=buf.device)
        work = torch.empty(ws, dtype=torch.uint8, device=buf.device)
        nat.check(lib.scpose_events_aedat2_unpack(_ptr(buf), n, h, w, _aedat2_layout(layout), int(bool(flip_x)), int(bool(flip_y)),
                                                  int(bool(unwrap)), c_double(float(t_divisor)), _ptr(t), _ptr(x), _ptr(y), _ptr(p),
                                                  int(capacity), _ptr(cs), _ptr(work), ws, _stream()), "events_aedat2_unpack")
        return cs.tolist()


def unpack_events_aedat2(records, hw, layout="davis", flip_x=True, flip_y=True, unwrap=True, t_divisor=0.0):
    """AEDAT-2.0 records -> (t int64, x int32, y int32, p int8, info): the kept events in file order, decoded on the device
    (csrc/events_aedat2_read.hip), in the dtypes render_events takes.  records: a uint8 device tensor of 8 * n bytes, the part
    of the file after its '#' header (event_read.read_events_aedat2 splits it off).  hw = (height, width) of the sensor.
    layout 'davis': jAER's DAVIS word, APS / IMU samples and special events dropped and counted; 'v2e': the records
    pack_events_aedat2 and the reference's AEDat2Output write.  flip_x / flip_y: undo the writers' flips (the default, so that
    unpack(pack(cols)) == cols).  unwrap: count full 32-bit roll-overs of the time stamp word into t; else t is the
    sign-extended word.  t_divisor: 0, 1e3 or 1e6, applied as parse_events_csv applies its time-stamp flags.
    info: the counters n_events, n_other, n_special, n_wraps, n_backward (include/scpose.h: scpose_events_aedat2_unpack).
    One small read-back, count_status.  Raises ValueError when a polarity event lies outside the sensor."""
    if not torch.is_tensor(records) or records.dtype != torch.uint8:
        raise ValueError("unpack_events_aedat2: the records must be a uint8 device tensor")
    _need_cuda(records)
    buf = records.contiguous().view(-1)
    if buf.numel() % 8:
        raise ValueError("unpack_events_aedat2: %d bytes are not a whole number of 8-byte records" % buf.numel())
    if buf.data_ptr() % 8:
        buf = buf.clone()
    n = int(buf.numel()) // 8
    dev = buf.device
    _aedat2_layout(layout)
    with torch.cuda.device(dev):
        t, x, y, p = _empty_event_columns(n, dev)
        cs = _unpack_events_aedat2_into(buf, n, hw, layout, flip_x, flip_y, unwrap, t_divisor, t, x, y, p, n)
    status = cs[1]
    if status & nat.AEDAT2_READ_RANGE:
        raise ValueError("unpack_events_aedat2: a polarity event lies outside the %d x %d sensor under the %s layout"
                         % (int(hw[1]), int(hw[0]), layout))
    if status != 0:
        raise nat.NativeError("unpack_events_aedat2: events_aedat2_unpack status %d" % status)
    info = dict(zip(AEDAT2_INFO, (int(cs[0]), int(cs[2]), int(cs[3]), int(cs[4]), int(cs[5]))))
    rows = info["n_events"]
    if rows == n:
        return t, x, y, p, info
    return t[:rows].clone(), x[:rows].clone(), y[:rows].clone(), p[:rows].clone(), info


AEDAT3_MAX_PACKET_EVENTS = (1 << 23) - 1


def unpack_events_aedat3(buf, packets, hw, rebase=True):
    """The polarity packets of an AEDAT-3.1 file -> (t int64, x int32, y int32, p int8, info), the valid events in file order,
    unpacked on the device (csrc/events_aedat3_read.hip), in the dtypes render_events takes.  buf: a uint8 device tensor, the whole
    file.  packets: (n, 3) int64, payload offset, eventNumber and eventTSOverflow of each polarity packet
    (event_read.parse_aedat3 finds them).  hw = (height, width) of the sensor.  rebase: t minus the first event's t.  One small
    read-back sizes the columns, a second brings the counters.  info: n_events, n_packets, t0, n_backward, n_out_of_range.  Raises
    ValueError for a negative time stamp, valid bits that contradict the packet's header and an event outside the sensor."""
    who = "unpack_events_aedat3"
    buf, pk, n = _packet_descriptors(who, buf, packets, 3)
    if n and (pk.min() < 0 or int(pk[:, 0].min()) < 28 or int(pk[:, 1].max()) > AEDAT3_MAX_PACKET_EVENTS or
              int((pk[:, 0] + 8 * pk[:, 1]).max()) > buf.numel()):
        if pk.min() >= 0 and int(pk[:, 1].max()) > AEDAT3_MAX_PACKET_EVENTS:
            raise ValueError("unpack_events_aedat3: a packet holds %d events: 2^23 or more in one packet are not read" % int(pk[:, 1].max()))
        raise ValueError(_NOT_INSIDE % (who, buf.numel()))
    if n and int(pk[:, 2].max()) > 0x7FFFFFFF:
        raise ValueError("unpack_events_aedat3: eventTSOverflow %d is not an int32" % int(pk[:, 2].max()))
    h, w = int(hw[0]), int(hw[1])
    lib = nat.lib()
    ws = _query_bytes("events_aedat3_workspace_bytes", n)
    with torch.cuda.device(buf.device):
        work = torch.empty(ws, dtype=torch.uint8, device=buf.device)
        cs = torch.empty(6, dtype=torch.int64, device=buf.device)
        pkd = torch.from_numpy(pk).to(buf.device)
        return _count_then_unpack(
            who, hw, _AEDAT3_STATUS, n, cs,
            lambda: nat.check(lib.scpose_events_aedat3_count(_ptr(buf), _ptr(pkd), n, _ptr(cs), _ptr(work), ws, _stream()),
                              "events_aedat3_count"),
            lambda t, x, y, p, rows: nat.check(
                lib.scpose_events_aedat3_unpack(_ptr(buf), _ptr(pkd), n, h, w, int(bool(rebase)), _ptr(t), _ptr(x), _ptr(y), _ptr(p),
                                                rows, _ptr(cs), _ptr(work), ws, _stream()), "events_aedat3_unpack"))


# ---- what the two packet readers (AEDAT-3.1, AEDAT-4.0) share on the host
_NOT_INSIDE = "%s: a packet does not lie inside the %d bytes of the file"


def _packet_descriptors(who, buf, packets, k):
    """The whole file and its packet descriptors, checked -> (the file as a flat uint8 device tensor, the descriptors as an
    (n, k) int64 NumPy array, n).  Whether each packet lies inside the file is the format's own expression, at the call site."""
    if not torch.is_tensor(buf) or buf.dtype != torch.uint8:
        raise ValueError("%s: the file must be a uint8 device tensor" % who)
    _need_cuda(buf)
    buf = buf.contiguous().view(-1)
    pk = np.ascontiguousarray(packets, dtype=np.int64).reshape(-1, k)
    return buf, pk, int(pk.shape[0])


def _count_then_unpack(who, hw, table, n, cs, count, unpack):
    """The tail of both readers, on the device of cs: count() leaves [n_events, status, t0, 0, 0, 0] in cs, a small read-back sizes
    the columns, unpack(t, x, y, p, rows) fills them and adds its counters to cs, a second read-back brings those.
    -> (t, x, y, p, info); a status bit raises what `table` says (_raise_status)."""
    count()
    rows, status, t0 = cs.tolist()[:3]                              # small read-back: the columns' size
    _raise_status(who, status, hw, table)
    t, x, y, p = _empty_event_columns(int(rows), cs.device)
    unpack(t, x, y, p, int(rows))
    got = cs.tolist()                                               # the counters
    _raise_status(who, got[1], hw, table)
    return t, x, y, p, {"n_events": int(rows), "n_packets": n, "t0": int(t0) if rows else 0, "n_backward": int(got[3]),
                        "n_out_of_range": int(got[4])}


def _raise_status(who, status, hw, table):
    """Raises for a status word of the event-file kernels: `table` is an ordered list of (bit, exception type, message); the first
    bit that is set decides, any other non-zero status is a NativeError.  A message may name %(who)s and the sensor's %(w)d, %(h)d."""
    for bit, exc, message in table:
        if status & bit:
            h, w = (None, None) if hw is None else (int(hw[0]), int(hw[1]))
            raise exc(message % {"who": who, "w": w, "h": h})
    if status != 0:
        raise nat.NativeError("%s: status %d" % (who, status))


_AEDAT3_STATUS = (
    (nat.AEDAT3_CORRUPT, ValueError, "%(who)s: a polarity event has a negative time stamp, or a packet descriptor is out of range "
                                     "(status CORRUPT)"),
    (nat.AEDAT3_VALID_MISMATCH, ValueError, "%(who)s: the valid bits of a packet's events do not add up to the eventValid its header "
                                            "states (status VALID_MISMATCH)"),
    (nat.AEDAT3_RANGE, ValueError, "%(who)s: an event lies outside the %(w)d x %(h)d sensor (status RANGE)"),
    (nat.AEDAT3_CAPACITY, nat.NativeError, "%(who)s: the columns are shorter than the events counted (status CAPACITY)"))
_AEDAT4_STATUS = (
    (nat.AEDAT4_CORRUPT, ValueError, "%(who)s: a packet is not a valid LZ4 frame (status CORRUPT: a bad magic, version or header "
                                     "checksum, an offset of 0 or before the output's start, an input overrun, a size that differs)"),
    (nat.AEDAT4_CHECKSUM, ValueError, "%(who)s: an LZ4 block or content checksum differs (status CHECKSUM)"),
    (nat.AEDAT4_FLATBUFFER, ValueError, "%(who)s: an event packet's flatbuffer is damaged (status FLATBUFFER)"),
    (nat.AEDAT4_RANGE, ValueError, "%(who)s: an event lies outside the %(w)d x %(h)d sensor (status RANGE)"))
_AEDAT4_ZSTD_STATUS = (
    (nat.AEDAT4_CORRUPT, ValueError, "%(who)s: a packet is not a valid Zstandard frame (status CORRUPT: a bad magic, a reserved bit, "
                                     "a dictionary, a damaged table or bitstream, an offset of 0, beyond the window or before the "
                                     "output's start, an input overrun, a size that differs)"),
    (nat.AEDAT4_CHECKSUM, ValueError, "%(who)s: a Zstandard content checksum differs (status CHECKSUM)")) + _AEDAT4_STATUS[2:]
_AEDAT4_WRITE_STATUS = (
    (nat.AEDAT4_WRITE_RANGE, ValueError, "%(who)s: an event lies outside the %(w)d x %(h)d sensor, or a polarity is neither 0 nor 1"),
    (nat.AEDAT4_WRITE_SIZE, ValueError, "%(who)s: a packet is larger than the reader takes (2^23 - 16 bytes: 524284 events)"))


def unpack_events_aedat4(buf, packets, compression, hw, rebase=True, verify=True):
    """The event packets of an AEDAT-4.0 file -> (t int64, x int32, y int32, p int8, info), events in file order, decompressed
    and unpacked on the device (csrc/events_aedat4_read.hip), in the dtypes render_events takes.  buf: a uint8 device tensor, the
    whole file.  packets: (n, 2) int64, payload offset and size of each EVENT packet (event_read.parse_aedat4 finds them).
    compression: the IOHeader's value, 0 NONE, 1 / 2 LZ4 or 3 / 4 ZSTD (csrc/events_aedat4_zstd.hip).  hw = (height, width) of the
    sensor.  rebase: t minus the first event's t.  verify: check the checksums the frames carry.  Two small read-backs size the staging buffer and the columns,
    a third brings the counters.  info: n_events, n_packets, t0, n_backward, n_out_of_range.  Raises ValueError for a damaged
    frame, a checksum that differs, a damaged flatbuffer and an event outside the sensor."""
    who = "unpack_events_aedat4"
    buf, pk, n = _packet_descriptors(who, buf, packets, 2)
    if compression not in (0, 1, 2, 3, 4):
        raise ValueError("unpack_events_aedat4: compression %r (0 NONE, 1 LZ4, 2 LZ4_HIGH, 3 ZSTD, 4 ZSTD_HIGH)" % (compression,))
    zstd = compression in (3, 4)
    stem = "events_aedat4_zstd_" if zstd else "events_aedat4_"              # the measure / decode pair and its workspace
    table = _AEDAT4_ZSTD_STATUS if zstd else _AEDAT4_STATUS
    if n and (pk.min() < 0 or int((pk[:, 0] + pk[:, 1]).max()) > buf.numel()):
        raise ValueError(_NOT_INSIDE % (who, buf.numel()))
    h, w = int(hw[0]), int(hw[1])
    lib = nat.lib()
    ws = _query_bytes(stem + "workspace_bytes", n)
    with torch.cuda.device(buf.device):
        work = torch.empty(ws, dtype=torch.uint8, device=buf.device)
        cs = torch.empty(6, dtype=torch.int64, device=buf.device)
        pkd = torch.from_numpy(pk).to(buf.device)
        src = buf
        if compression:
            nat.check(getattr(lib, "scpose_" + stem + "measure")(_ptr(buf), _ptr(pkd), n, _ptr(cs), _ptr(work), ws, _stream()),
                      stem + "measure")
            total, status = cs.tolist()[:2]                         # small read-back: the staging buffer's size
            _raise_status(who, status, hw, table)
            if total < 0 or total % 16 or total > n * (1 << 23):
                raise nat.NativeError("unpack_events_aedat4: %smeasure reports %d staging bytes for %d packets" % (stem, total, n))
            src = torch.empty(max(int(total), 16), dtype=torch.uint8, device=buf.device)
            nat.check(getattr(lib, "scpose_" + stem + "decode")(_ptr(buf), _ptr(pkd), n, _ptr(src), int(total), int(bool(verify)),
                                                                _ptr(work), ws, _stream()),
                      stem + "decode")
        return _count_then_unpack(
            who, hw, table, n, cs,
            lambda: nat.check(lib.scpose_events_aedat4_count(_ptr(src), _ptr(pkd), n, int(bool(compression)), _ptr(cs), _ptr(work), ws,
                                                             _stream()), "events_aedat4_count"),
            lambda t, x, y, p, rows: nat.check(
                lib.scpose_events_aedat4_unpack(_ptr(src), n, h, w, int(bool(rebase)), _ptr(t), _ptr(x), _ptr(y), _ptr(p), rows,
                                                _ptr(cs), _ptr(work), ws, _stream()), "events_aedat4_unpack"))


AEDAT4_COMPRESSIONS = {"none": nat.AEDAT4_NONE, "lz4": nat.AEDAT4_LZ4}
AEDAT4_TABLE = ("offset", "size", "n_events", "t_first", "t_last")


def _aedat4_compression(who, compression):
    try:
        return AEDAT4_COMPRESSIONS[compression]
    except (KeyError, TypeError):
        raise ValueError("%s: compression %r: the compressions are 'lz4' and 'none' (ZSTD and LZ4_HIGH are not written)"
                         % (who, compression))


def _packet_bounds(who, bounds, n, what):
    b = np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1)
    if b.size == 0 or b[0] != 0 or b[-1] != n or (np.diff(b) < 0).any():
        raise ValueError("%s: the packet boundaries must rise from 0 to the %d %s (got %d values, %s .. %s)"
                         % (who, n, what, b.size, b[0] if b.size else None, b[-1] if b.size else None))
    return b


def pack_events_aedat4(t, x, y, p, hw, packet_rows, compression="lz4", stream_id=0):
    """(t int64 microseconds, x int32, y int32, p int8 in {0, 1}) device tensors -> (uint8 device tensor, table): the event
    packets of an AEDAT-4.0 file for a sensor of hw = (height, width), `int32 streamID, int32 size, payload` one after the
    other (csrc/events_aedat4_write.hip).  packet_rows: n_packets + 1 row boundaries rising from 0 to n; packet k holds rows
    packet_rows[k] .. packet_rows[k + 1] - 1, an empty one is written as an empty packet.  compression: 'none' (a payload is the
    packet's size-prefixed EVTS flatbuffer) or 'lz4' (one LZ4 frame of it, compressed on the device).  table: int64 NumPy
    (n_packets, 5), per packet AEDAT4_TABLE: byte offset of its record in the tensor, payload size, events, first and last time
    stamp -- what the file data table needs.  Raises ValueError for an event outside the sensor, a polarity outside {0, 1} and
    a packet above the reader's limits; nothing has been stored then.  One read-back: [bytes, status] and the table."""
    who = "pack_events_aedat4"
    comp = _aedat4_compression(who, compression)
    h, w = int(hw[0]), int(hw[1])
    t, x, y, p, dev, n = _event_columns(who, t, x, y, p)
    bounds = _packet_bounds(who, packet_rows, n, "rows")
    npk = int(bounds.size) - 1
    lib = nat.lib()
    ws, cap = c_size_t(), c_size_t()
    nat.check(lib.scpose_events_aedat4_pack_sizes(n, npk, comp, ctypes.byref(ws), ctypes.byref(cap)), "events_aedat4_pack_sizes")
    with torch.cuda.device(dev):
        work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
        out = torch.empty(cap.value, dtype=torch.uint8, device=dev)
        res = torch.empty(2 + 5 * max(npk, 1), dtype=torch.int64, device=dev)      # [bytes, status], then the table
        bd = torch.from_numpy(bounds).to(dev)
        nat.check(lib.scpose_events_aedat4_pack(_ptr(t), _ptr(x), _ptr(y), _ptr(p), n, _ptr(bd), npk, h, w, int(stream_id), comp,
                                                _ptr(out), cap.value, _ptr(res[2:]), _ptr(res), _ptr(work), ws.value, _stream()),
                  "events_aedat4_pack")
        got = res.cpu().numpy()                                     # the one read-back
    _raise_status(who, int(got[1]), (h, w), _AEDAT4_WRITE_STATUS)
    return out[:int(got[0])], got[2:2 + 5 * npk].reshape(npk, 5).copy()


def lz4_frame_bytes(data, bounds=None):
    """A uint8 device tensor -> (uint8 device tensor, table): the bytes between bounds[k] and bounds[k + 1] (default: all of
    them, one piece) as records `int32 0, int32 size, LZ4 frame`, framed and compressed as pack_events_aedat4 frames a packet.
    table: int64 NumPy (n_pieces, 5), the record's offset and the frame's size in its first two columns."""
    who = "lz4_frame_bytes"
    if not torch.is_tensor(data) or data.dtype != torch.uint8:
        raise ValueError("%s: the bytes must be a uint8 device tensor" % who)
    _need_cuda(data)
    data = data.contiguous().view(-1)
    n = int(data.numel())
    bounds = _packet_bounds(who, (0, n) if bounds is None else bounds, n, "bytes")
    npk = int(bounds.size) - 1
    dev = data.device
    lib = nat.lib()
    ws, cap = c_size_t(), c_size_t()
    nat.check(lib.scpose_events_aedat4_frame_sizes(n, npk, ctypes.byref(ws), ctypes.byref(cap)), "events_aedat4_frame_sizes")
    with torch.cuda.device(dev):
        work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
        out = torch.empty(cap.value, dtype=torch.uint8, device=dev)
        res = torch.empty(2 + 5 * max(npk, 1), dtype=torch.int64, device=dev)
        bd = torch.from_numpy(bounds).to(dev)
        nat.check(lib.scpose_events_aedat4_frame(_ptr(data), n, _ptr(bd), npk, _ptr(out), cap.value, _ptr(res[2:]), _ptr(res),
                                                 _ptr(work), ws.value, _stream()), "events_aedat4_frame")
        got = res.cpu().numpy()
    _raise_status(who, int(got[1]), None, _AEDAT4_WRITE_STATUS)
    return out[:int(got[0])], got[2:2 + 5 * npk].reshape(npk, 5).copy()


# ------------------------------------------------------------------ image files (baseline JPEG, PNG) -> frames or network crops
JPEG_MAX_ROUNDS = 96          # launches of the relaxation (measured distribution and head-room)
_IMAGE_WORKSPACE = {}         # device index -> uint8 tensor, grown on demand (2 bytes per coefficient: too large to allocate per call)
_JPEG_WORKSPACE = _IMAGE_WORKSPACE      # its name before the PNG decoder shared it: the suite of the commit before the rename pokes it


def _image_workspace(dev, nbytes):
    ws = _IMAGE_WORKSPACE.get(dev.index)
    if ws is None or ws.numel() < nbytes:
        _IMAGE_WORKSPACE.pop(dev.index, None)
        ws = None
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        _IMAGE_WORKSPACE[dev.index] = ws
    return ws


def _crop_target(crop, n, dev):
    """crop = (minv float64 (n, 6), roi int32 (n, 4), out_h, out_w) -> (the crops to fill, the arguments minv .. crops of a
    scpose_*_decode_crop call, what those point to)"""
    minv, roi, oh, ow = crop
    d_minv = torch.from_numpy(np.ascontiguousarray(minv, dtype=np.float64)).to(dev, non_blocking=True)
    roi = np.ascontiguousarray(roi, dtype=np.int32)      # host memory: read before the call returns
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
    return out, (_ptr(d_minv), c_void_p(roi.ctypes.data), oh, ow, _ptr(out)), (d_minv, roi)


def _jpeg_decode_group(headers, files, rgb, dev, crop=None, max_rounds=JPEG_MAX_ROUNDS, out=None, y_out=None):
    """One device call on the current stream for images of one geometry; -> (frames, status list): scpose_jpeg_decode, or with
    crop (_crop_target) scpose_jpeg_decode_crop -> (crops, status list)."""
    h, w, mode = headers[0].geometry
    n = len(headers)
    desc, rows, data, max_subs = jr.pack_batch(headers, files)
    lib = nat.lib()
    ws = _query_bytes("jpeg_decode_workspace_bytes", n, h, w, jr.MODES[mode], max_subs)
    with torch.cuda.device(dev):
        d_desc = torch.from_numpy(desc).to(dev, non_blocking=True)
        d_rows = torch.from_numpy(rows).to(dev, non_blocking=True)
        d_data = torch.from_numpy(data).to(dev, non_blocking=True)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        work = _image_workspace(dev, ws)
        front = (_ptr(d_desc), _ptr(d_rows), int(rows.shape[0]), _ptr(d_data), int(data.size), n, h, w, jr.MODES[mode], int(max_subs),
                 0 if rgb else 1, int(max_rounds))
        if crop is None:
            if out is None:
                out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
            nat.check(lib.scpose_jpeg_decode(*front, _ptr(out), _ptr(y_out), _ptr(status), _ptr(work), ws, _stream()), "jpeg_decode")
        else:
            out, target, alive = _crop_target(crop, n, dev)
            nat.check(lib.scpose_jpeg_decode_crop(*front, *target, _ptr(status), _ptr(work), ws, _stream()), "jpeg_decode_crop")
        return out, status.tolist()


def _png_decode_group(headers, files, rgb, dev, crop=None, max_rounds=None):
    """One device call on the current stream for PNGs of one geometry; -> (frames, status list): scpose_png_decode, or with
    crop (_crop_target) scpose_png_decode_crop -> (crops, status list)."""
    h, w, channels = headers[0].geometry
    n = len(headers)
    desc, data = pr.pack_batch(headers, files)         # desc stays on the host: the library checks and uploads it
    lib = nat.lib()
    ws = _query_bytes("png_decode_workspace_bytes", n, h, w, channels)
    with torch.cuda.device(dev):
        d_data = torch.from_numpy(data).to(dev, non_blocking=True)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        work = _image_workspace(dev, ws)
        front = (c_void_p(desc.ctypes.data), _ptr(d_data), int(data.size), n, h, w, channels, 0 if rgb else 1)
        if crop is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
            nat.check(lib.scpose_png_decode(*front, _ptr(out), _ptr(status), _ptr(work), ws, _stream()), "png_decode")
        else:
            out, target, alive = _crop_target(crop, n, dev)
            nat.check(lib.scpose_png_decode_crop(*front, *target, _ptr(status), _ptr(work), ws, _stream()), "png_decode_crop")
        return out, status.tolist()                    # the copy back waits for the stream: desc has been read by then


def _jpeg_judge(who, i, st, rounds_cap):
    """One image's status word -> None: decoded on the device, or why the host decodes it; raises for a corrupt stream"""
    # not converged: the walk started from entries that are not the stream's, so CORRUPT says nothing; the host decides
    if st & nat.JPEG_NOT_CONVERGED:
        return "entry states not converged after %d rounds" % rounds_cap
    if st & nat.JPEG_CORRUPT:
        raise jr.JpegError("%s: file %d: corrupt or truncated entropy-coded data" % (who, i))
    return None


def _png_judge(who, i, st, rounds_cap):
    """The same for a PNG: the device never decides what a damaged file means"""
    if not st:
        return None
    names = [w for bit, w in ((nat.PNG_CORRUPT, "corrupt deflate stream"), (nat.PNG_CHECKSUM, "Adler-32 mismatch"),
                              (nat.PNG_FILTER, "filter type above 4")) if st & bit]
    return "device status %d (%s)" % (st, ", ".join(names))


def _pil_decode(data, rgb):
    """The host decoder of every image format: PIL's pixels as (H, W, 3) uint8, or whatever PIL raises."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        arr = np.array(im.convert("RGB"))              # a copy: the decoder's own array is read-only
    return arr if rgb else arr[:, :, ::-1].copy()


def _jpeg_host_decode(data, rgb, who, i):
    try:                                   # the message names decode_jpeg and no file, whoever calls: callers match on it
        return _pil_decode(data, rgb)
    except Exception as e:
        raise jr.JpegError("decode_jpeg: the host decoder cannot read the file either: %s" % e)


def _png_host_decode(data, rgb, who, i):
    try:
        return _pil_decode(data, rgb)
    except Exception as e:
        raise pr.PngError("%s: file %d: %s" % (who, i, e))


# What the batch driver asks of a device decoder: group(headers, files, rgb, dev, crop, rounds_cap) -> (tensor, status list), one
# call and one read-back; judge (above); host_decode(data, rgb, who, i) -> PIL's pixels, or the format's error with PIL's message;
# error, unsupported: what a file that cannot be decoded, or that fallback=False keeps from the host, raises.
_ImageFormat = collections.namedtuple("_ImageFormat", "group judge host_decode error unsupported")
_FORMATS = {
    "jpeg": _ImageFormat(_jpeg_decode_group, _jpeg_judge, _jpeg_host_decode, jr.JpegError, jr.UnsupportedJpeg),
    "png": _ImageFormat(_png_decode_group, _png_judge, _png_host_decode, pr.PngError, pr.UnsupportedPng),
}


def _image_device(device, who):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise nat.NativeError("%s needs a ROCm device (got %s); there is no CPU path" % (who, dev))
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _file_blobs(files, who):
    """files (bytes, uint8 arrays / tensors or paths) -> the bytes of each"""
    blobs = []
    for f in files:
        if isinstance(f, (bytes, bytearray, memoryview)):
            blobs.append(bytes(f))
        elif torch.is_tensor(f):
            blobs.append(f.cpu().numpy().tobytes())
        elif isinstance(f, np.ndarray):
            blobs.append(f.tobytes())
        else:
            with open(f, "rb") as fh:
                blobs.append(fh.read())
    if not blobs:
        raise ValueError("%s: no files" % who)
    return blobs


def _decode_files(who, files, kinds, rgb, dev, fallback, crop=None, max_rounds=None):
    """The batch driver of decode_jpeg, decode_png and decode_crop.  kinds = (jpeg, png): the device decoders on offer, as for
    image_read.sniff, which says per file who takes it.  crop: None for frames, else crop(indices, (h, w)) -> the crop argument of
    the group call for those files, all of that frame size.  Files are grouped by (decoder, geometry); every group is one call.
    -> (parts, host, facts).  parts: [(file indices, their rows of a group's tensor)], what the device decoded.  host: {index: reason},
    the files left to the host decoder (fallback=False: the first one raises instead); facts["host_px"] has their pixels.
    facts["rounds"]: per file the relaxation rounds used (0: no JPEG decoded on the device); facts["png"]: the indices png_decode.hip
    decoded; facts["device"]: per file whether the device decoded it."""
    blobs = _file_blobs(files, who)
    n, rounds_cap = len(blobs), JPEG_MAX_ROUNDS if max_rounds is None else int(max_rounds)
    heads, fmts, host, groups = [None] * n, [None] * n, {}, {}
    for i, b in enumerate(blobs):
        kind, heads[i], reason = image_read.sniff(b, *kinds)
        # a refusal is the PNG side's (its error classes, its host message) when the file is a PNG or no other decoder was on offer
        fmts[i] = _FORMATS[kind or ("png" if kinds[1] and (not kinds[0] or image_read.is_png(b)) else "jpeg")]
        if kind:
            groups.setdefault((kind, heads[i].geometry), []).append(i)
        elif fallback:
            host[i] = reason
        elif reason == image_read.BAD_CRC:
            raise fmts[i].error("%s: file %d: %s" % (who, i, reason))
        else:
            raise fmts[i].unsupported(reason)
    facts = {"rounds": [0] * n, "png": [], "device": [False] * n}
    parts = []
    for (kind, geom), idx in groups.items():
        fmt = _FORMATS[kind]
        out, status = fmt.group([heads[i] for i in idx], [blobs[i] for i in idx], rgb, dev, crop(idx, geom[:2]) if crop else None, rounds_cap)
        keep = []
        for row, i in enumerate(idx):
            facts["rounds"][i] = (status[row] >> 8) & 255          # a PNG's status word has no such byte
            reason = fmt.judge(who, i, status[row], rounds_cap)
            if reason is None:
                keep.append(row)
            elif fallback:
                host[i] = reason
            else:
                raise fmt.error("%s: file %d: %s" % (who, i, reason))
        if len(keep) < len(idx):
            out, idx = out[torch.tensor(keep, dtype=torch.int64, device=dev)], [idx[row] for row in keep]
        if idx:
            parts.append((idx, out))
            for i in idx:
                facts["device"][i] = True
            if kind == "png":
                facts["png"] += idx
    facts["host_px"] = {i: fmts[i].host_decode(blobs[i], rgb, who, i) for i in sorted(host)}
    return parts, host, facts


def _assemble(parts, n, dev):
    """parts [(indices, rows)] that cover 0 .. n - 1 -> the (n, ...) tensor; a part that is everything, in order, is returned itself"""
    if len(parts) == 1 and parts[0][0] == list(range(n)):
        return parts[0][1]
    with torch.cuda.device(dev):
        out = torch.empty((n,) + tuple(parts[0][1].shape[1:]), dtype=torch.uint8, device=dev)
        for idx, rows in parts:
            out.index_copy_(0, torch.tensor(idx, dtype=torch.int64, device=dev), rows)
    return out


def _decode_frames(who, files, kinds, rgb, device, fallback, max_rounds=None):
    """decode_jpeg and decode_png behind their info: -> ((N, H, W, 3) frames, host, facts) of _decode_files; one frame size or ValueError"""
    dev = _image_device(device, who)
    parts, host, facts = _decode_files(who, files, kinds, rgb, dev, fallback, max_rounds=max_rounds)
    sizes = {tuple(rows.shape[1:3]) for _, rows in parts} | {a.shape[:2] for a in facts["host_px"].values()}
    if len(sizes) != 1:
        raise ValueError("%s: the frames have different sizes %s: decode them in separate calls" % (who, sorted(sizes)))
    if host:
        parts.append((sorted(host), torch.from_numpy(np.stack([facts["host_px"][i] for i in sorted(host)])).to(dev)))
    return _assemble(parts, len(facts["rounds"]), dev), host, facts


def decode_jpeg(files, rgb=True, device=None, max_rounds=None, fallback=True):
    """Baseline JPEG files -> ((N, H, W, 3) uint8 frames on the device, info), decoded by csrc/jpeg_decode.hip bit for bit as
    libjpeg (PIL, cv2.imread) decodes them.  files: a list of bytes or of paths; all frames must have one size.  rgb: R, G, B
    order, else B, G, R (what cv2.imread returns).  Files are grouped by (height, width, sampling) and every group is one call.
    info = {"rounds": per image the relaxation rounds used (0: not decoded on the device), "fallback": {index: reason}}.
    A file jpeg_read.parse_jpeg refuses, or one whose entry states have not converged after max_rounds launches, is decoded by PIL
    on the host when `fallback`, else raises UnsupportedJpeg / JpegError.  A corrupt or truncated stream always raises JpegError."""
    out, host, facts = _decode_frames("decode_jpeg", files, (True, False), rgb, device, fallback, max_rounds)
    return out, {"rounds": facts["rounds"], "fallback": host}


def decode_png(files, rgb=True, device=None, fallback=True):
    """PNG files -> ((N, H, W, 3) uint8 frames on the device, info), decoded by csrc/png_decode.hip bit for bit as PIL's
    Image.open(f).convert("RGB") decodes them.  files: a list of bytes or of paths; all frames must have one size.  rgb: R, G, B order,
    else B, G, R.  Files are grouped by (height, width, channels) and every group is one call.
    info = {"device": per file whether the device decoded it, "fallback": {index: reason}}.
    A file png_read.parse_png refuses (interlaced, 1/2/4/16-bit, APNG, not a PNG), one that fails a chunk CRC and one whose status word
    is not 0 are the host decoder's: PIL returns pixels (bytes after the stream, say) or raises, and a raise becomes PngError with PIL's
    message -- the device never decides what a damaged file means.  fallback=False: UnsupportedPng / PngError at once."""
    out, host, facts = _decode_frames("decode_png", files, (False, True), rgb, device, fallback)
    return out, {"device": facts["device"], "fallback": host}


def decode_crop(files, trans, out_wh, rgb=True, device=None, max_rounds=None, fallback=True, png=False):
    """Image files -> ((N, H, W, 3) uint8 network crops on the device, info): row i is crop_warp(frame_i, trans[i], out_wh) of the frame
    PIL decodes from files[i] -- for a baseline JPEG, of decode_jpeg's frame -- bit for bit, without that frame: after the entropy
    decoding csrc/jpeg_decode.hip transforms only the blocks the warp's window (warp_window) can read and samples the planes.
    files as for decode_jpeg (frame sizes may differ); trans (N, 2, 3) as for crop_warp; out_wh = (W, H); rgb: the channel order.
    info as decode_jpeg's.  A file jpeg_read.parse_jpeg refuses (PNG, progressive JPEG, ...) and one whose entry states have not
    converged is decoded by PIL on the host when `fallback` and its row filled by crop_warp; a corrupt stream raises JpegError.
    png=True: a file parse_jpeg refuses is offered to png_read.parse_png; one it accepts is inflated, unfiltered and sampled by
    csrc/png_decode.hip (rounds 0), info gains "png": the indices decoded that way; a PNG whose status word is not 0 takes the PIL row
    (PngError when PIL raises, or at once without `fallback`).  png=False: a PNG is just a file parse_jpeg refuses.
    ValueError for a transform with a non-finite entry."""
    from .utils.transforms import invert_affine_cv
    dev = _image_device(device, "decode_crop")
    files = _file_blobs(files, "decode_crop")
    trans = np.asarray(trans, dtype=np.float64).reshape(len(files), 2, 3)
    _finite_affines("decode_crop", trans, len(files))           # ValueError naming the row, before anything is decoded
    ow, oh = int(out_wh[0]), int(out_wh[1])

    def crop(idx, frame_hw):
        minv = np.stack([np.asarray(invert_affine_cv(trans[i]), dtype=np.float64).reshape(6) for i in idx])
        return minv, np.array([warp_window(trans[i], (ow, oh), frame_hw) for i in idx], dtype=np.int32), oh, ow
    parts, host, facts = _decode_files("decode_crop", files, (True, bool(png)), rgb, dev, fallback, crop, max_rounds)
    if host:
        parts.append((sorted(host), crop_warp([facts["host_px"][i] for i in sorted(host)], trans[sorted(host)], (ow, oh), device=dev)))
    info = {"rounds": facts["rounds"], "fallback": host}
    if png:
        info["png"] = sorted(facts["png"])
    return _assemble(parts, len(files), dev), info


# ------------------------------------------------------------------ frames -> baseline JPEG files; the pose overlay
_JPEG_ENC_HUFF = {}           # device index -> the standard Huffman tables as uploaded (uint32 [4][256])


def _frames_u8(who, frames):
    _need_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError("%s: frames must be (N, H, W, 3) uint8 with N >= 1 (got %s %s)" % (who, tuple(frames.shape), frames.dtype))
    return frames.contiguous()


def encode_jpeg(frames, quality=75, subsampling="420", device=None, comment=None):
    """(N, H, W, 3) uint8 RGB frames -> list of N bytes objects, each the file PIL writes for the frame with
    save(format="JPEG", quality=quality, subsampling=...) and its other defaults, byte for byte (csrc/jpeg_encode.hip).
    subsampling: "420", "444" or "gray" (one component: Y of the three channels, PIL's convert("L")).  comment: the body of a COM
    segment in every file, where PIL's save(comment=...) puts it.  The streams are packed on the device; the host reads the
    offsets, then the packed bytes."""
    from . import jpeg_write as jw
    if torch.is_tensor(frames) and device is not None:
        frames = frames.to(device)
    elif not torch.is_tensor(frames):
        frames = torch.from_numpy(np.ascontiguousarray(frames)).to(device if device is not None else "cuda")
    frames = _frames_u8("encode_jpeg", frames)
    if subsampling not in jw.MODES:
        raise ValueError("encode_jpeg: subsampling=%r (420, 444, gray)" % (subsampling,))
    n, h, w = (int(v) for v in frames.shape[:3])
    head = jw.header(h, w, subsampling, quality, comment)
    mode = jw.MODES[subsampling]
    dev = frames.device
    lib = nat.lib()
    ws, cap = _query_bytes("jpeg_encode_workspace_bytes", n, h, w, mode), c_int64()
    nat.check(lib.scpose_jpeg_encode_capacity_bytes(n, h, w, mode, len(head), ctypes.byref(cap)), "jpeg_encode_capacity_bytes")
    with torch.cuda.device(dev):
        huff = _JPEG_ENC_HUFF.get(dev.index)
        if huff is None:
            huff = _JPEG_ENC_HUFF[dev.index] = torch.from_numpy(jw.huff_upload().view(np.int32)).to(dev)
        d_head = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
        out = torch.empty(cap.value, dtype=torch.uint8, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        work = _image_workspace(dev, ws)
        nat.check(lib.scpose_jpeg_encode(_ptr(frames), n, h, w, mode, int(quality), _ptr(huff), _ptr(d_head), len(head), _ptr(out),
                                         cap.value, _ptr(offsets), _ptr(status), _ptr(work), ws, _stream()), "jpeg_encode")
        off = offsets.tolist()
        bad = [i for i, st in enumerate(status.tolist()) if st]
        if bad:
            raise nat.NativeError("encode_jpeg: status %s for images %s" % (status.tolist(), bad))
        packed = out[:off[n]].cpu().numpy().tobytes()
    return [packed[off[i]:off[i + 1]] for i in range(n)]


def draw_overlays(frames, bboxes, points):
    """The pose overlay of pose_export.draw_overlay in place on (N, H, W, 3) uint8 RGB device frames: per frame the green outline of
    ImageDraw.rectangle([x, y, x + w, y + h], width=2), then a blue disc of radius 5 at (int(px), int(py)) for every point whose
    coordinates are finite.  bboxes (N, 4) ints x, y, w, h with w >= 1 and h >= 2; points (N, J, 2) float64.  -> frames."""
    _need_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("draw_overlays: frames must be contiguous (N, H, W, 3) uint8 (got %s %s)" % (tuple(frames.shape), frames.dtype))
    n, h, w = (int(v) for v in frames.shape[:3])
    bb = np.asarray(bboxes)
    if bb.shape != (n, 4) or not np.issubdtype(bb.dtype, np.integer):
        raise ValueError("draw_overlays: bboxes must be (%d, 4) integers (got %s %s)" % (n, bb.shape, bb.dtype))
    if (bb[:, 2] < 1).any() or (bb[:, 3] < 2).any() or (np.abs(bb.astype(np.int64)) >= 1 << 30).any():
        raise ValueError("draw_overlays: every box needs 1 <= w, 2 <= h and coordinates below 2^30")
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 3 or pts.shape[0] != n or pts.shape[2] != 2:
        raise ValueError("draw_overlays: points must be (%d, J, 2) (got %s)" % (n, pts.shape))
    j = int(pts.shape[1])
    with torch.cuda.device(frames.device):
        d_bb = torch.from_numpy(np.ascontiguousarray(bb, dtype=np.int32)).to(frames.device)
        d_pts = torch.from_numpy(pts).to(frames.device) if j else None
        nat.check(nat.lib().scpose_overlay_draw(_ptr(frames), n, h, w, _ptr(d_bb), _ptr(d_pts), j, _stream()), "overlay_draw")
    return frames


def resize_area(frames, out_hw, gray=True, channels="rgb"):
    """uint8 frames (F, H, W, 3) or (F, H, W) -> (F, h, w) gray frames, or with gray=False (F, h, w, 3) resized frames, on the device
    (csrc/resize_area.hip): cv2.resize(.., interpolation=cv2.INTER_AREA) per channel as resize_area.py restates it, then OpenCV's
    8-bit gray rule (4899 R + 9617 G + 1868 B + 8192) >> 14 on the rounded channels.  out_hw = (h, w) with h <= H and w <= W; the
    input's own size means gray only.  frames: a device tensor, or a host array that is uploaded.  channels: "rgb" or "bgr", which
    plane the R weight goes to.  One-channel frames are resized and `gray` is ignored.  The result is contiguous uint8, what
    DvsEmulator.emulate takes.  ValueError for a wrong dtype, rank or channel count and for an axis that would grow."""
    from . import resize_area as ra
    if channels not in ("rgb", "bgr"):
        raise ValueError("resize_area: channels=%r (rgb or bgr)" % (channels,))
    fr = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(np.asarray(frames)))
    if fr.dtype != torch.uint8 or fr.dim() not in (3, 4) or (fr.dim() == 4 and fr.shape[3] != 3):
        raise ValueError("resize_area: frames must be uint8 of shape (F, H, W, 3) or (F, H, W) (got %s %s)" % (fr.dtype, tuple(fr.shape)))
    f, H, W = (int(v) for v in fr.shape[:3])
    c = 3 if fr.dim() == 4 else 1
    if H < 1 or W < 1:
        raise ValueError("resize_area: empty frames %s" % (tuple(fr.shape),))
    rule, xrec, yrec = ra.plan((H, W), out_hw)                  # ValueError for a growing axis, before anything runs
    h, w = int(out_hw[0]), int(out_hw[1])
    if not fr.is_cuda:
        fr = fr.to(torch.device("cuda", torch.cuda.current_device()))
    fr = fr.contiguous()
    dev = fr.device
    with torch.cuda.device(dev):
        out = torch.empty((f, h, w) if gray or c == 1 else (f, h, w, 3), dtype=torch.uint8, device=dev)
        ws = _query_bytes("resize_area_workspace_bytes", h, w)
        work = torch.empty(ws, dtype=torch.uint8, device=dev)
        nat.check(nat.lib().scpose_resize_area_u8(_ptr(fr), f, H, W, c, _ptr(out), h, w, 1 if gray else 0, 1 if channels == "bgr" else 0, rule,
                                                  c_void_p(xrec.ctypes.data), c_void_p(yrec.ctypes.data), _ptr(work), ws, _stream()),
                  "resize_area_u8")
        torch.cuda.current_stream().synchronize()               # the tables are host memory: they stay until the stream has read them
    return out


class DvsEmulator:
    """Device DVS emulator (csrc/dvs_emulator.hip): see dvs_emulator().  The state lives in device memory between calls."""

    def __init__(self, h, w, device=None, **params):
        from . import dvs_emulator as de
        self._p = de.validate(h, w, **params)
        self.h, self.w = self._p["h"], self._p["w"]
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise nat.NativeError("dvs_emulator needs a ROCm device (got %s); there is no CPU path" % self.device)
        up = lambda a: torch.from_numpy(a).to(self.device) if a is not None else None
        self._maps = [up(self._p[k]) for k in ("pos_map", "neg_map", "noise_map")]
        self._lut = up(de.lin_log_table())
        self._state = torch.zeros(_query_bytes("dvs_state_bytes", self.h, self.w), dtype=torch.uint8, device=self.device)
        self._c = nat.DvsParams(self.h, self.w, self._p["pos"], self._p["neg"], self._maps[0].data_ptr() if self._maps[0] is not None else None,
                                self._maps[1].data_ptr() if self._maps[1] is not None else None,
                                self._maps[2].data_ptr() if self._maps[2] is not None else None, self._lut.data_ptr(),
                                self._p["cutoff_hz"], self._p["leak_rate_hz"], self._p["refractory_period_s"], self._p["max_iters"])
        self._t_prev = None
        self._per_frame = 0.25                 # events per pixel and frame seen so far: sizes the next call's columns
        self.last_status = 0

    def reset(self):
        """The next emulate() call initialises the state from its first frame again."""
        self._t_prev = None

    def state(self):
        """dict of the four state planes (base, lp0, lp1, tmem) as (h, w) float32 device tensors: copies, for inspection."""
        hw = self.h * self.w
        pl = (hw * 4 + 255) // 256 * 256
        return {k: self._state[256 + i * pl: 256 + i * pl + hw * 4].view(torch.float32).view(self.h, self.w).clone()
                for i, k in enumerate(("base", "lp0", "lp1", "tmem"))}

    def emulate(self, frames, t, capacity=None):
        """frames uint8 (F, h, w) and t float64 (F,) seconds: device tensors, or host arrays that are uploaded.  Returns
        (t int64 us, x int32, y int32, p int8, t_s float32) device tensors: the events of these frames in order, p == 1 for ON.
        The first call (and the first after reset()) takes its first frame as the reference's frame 0, which only initialises
        the state.  Stamps that do not increase raise ValueError before anything runs.  capacity: rows to provide for; by
        default sized from the event rate seen so far, and the call is repeated from a saved state when that was too small.  One
        small read-back per attempt, [n_events, status]."""
        from . import dvs_emulator as de
        if torch.is_tensor(frames):
            fr = frames.to(self.device)
        else:
            fr = torch.from_numpy(np.ascontiguousarray(np.asarray(frames))).to(self.device)
        if fr.dtype != torch.uint8 or fr.dim() != 3 or tuple(fr.shape[1:]) != (self.h, self.w):
            raise ValueError("dvs_emulator: frames must be uint8 of shape (F, %d, %d) (got %s %s)" % (self.h, self.w, fr.dtype, tuple(fr.shape)))
        fr = fr.contiguous()
        th = de.check_times(t.detach().cpu().numpy() if torch.is_tensor(t) else t, self._t_prev)
        if th.shape[0] != fr.shape[0]:
            raise ValueError("dvs_emulator: %d frames but %d stamps" % (fr.shape[0], th.shape[0]))
        lib = nat.lib()
        dev = self.device
        with torch.cuda.device(dev):
            if fr.shape[0] and self._t_prev is None:
                nat.check(lib.scpose_dvs_init(_ptr(self._state), _ptr(fr), c_double(float(th[0])), ctypes.byref(self._c), _stream()), "dvs_init")
                self._t_prev = float(th[0])
                fr, th = fr[1:], th[1:]
            f = int(fr.shape[0])
            if f == 0:
                return _empty_event_columns(0, dev) + (torch.empty(0, dtype=torch.float32, device=dev),)
            t_d = (t.to(dev, torch.float64)[-f:] if torch.is_tensor(t) else torch.from_numpy(th).to(dev)).contiguous()
            ws = _query_bytes("dvs_workspace_bytes", self.h, self.w, f, self._p["max_iters"])
            work = torch.empty(ws, dtype=torch.uint8, device=dev)
            cs = torch.empty(2, dtype=torch.int64, device=dev)
            fixed = capacity is not None
            cap = int(capacity) if fixed else max(4096, int(self._per_frame * 1.25 * f * self.h * self.w) + 1024)
            saved = None if fixed else self._state.clone()
            while True:
                cols = (torch.empty(cap, dtype=torch.float32, device=dev),) + _empty_event_columns(cap, dev)
                nat.check(lib.scpose_dvs_emulate(_ptr(self._state), _ptr(fr), _ptr(t_d), f, ctypes.byref(self._c), _ptr(cols[0]), _ptr(cols[1]),
                                                 _ptr(cols[2]), _ptr(cols[3]), _ptr(cols[4]), cap, _ptr(cs), _ptr(work), ws, _stream()),
                          "dvs_emulate")
                n, status = cs.tolist()                             # the one small read-back
                self.last_status = status
                if status & nat.DVS_TIME:
                    raise ValueError("dvs_emulator: a frame time is not later than its predecessor")
                if status & nat.DVS_ITERS:
                    self._t_prev = None
                    raise nat.NativeError("dvs_emulator: a frame needs more than max_iters=%d sub-iterations; the state was reset -- "
                                          "construct the emulator with a larger max_iters" % self._p["max_iters"])
                if status & nat.DVS_CAPACITY and not fixed:
                    self._state.copy_(saved)
                    cap = n
                    continue
                break
            self._t_prev = float(th[-1])
            if status & nat.DVS_CAPACITY:
                raise DvsCapacity("dvs_emulator: %d events do not fit the capacity of %d rows" % (n, cap), n, cols)
            self._per_frame = max(self._per_frame, n / float(f * self.h * self.w))
            return cols[1][:n], cols[2][:n], cols[3][:n], cols[4][:n], cols[0][:n]


class DvsCapacity(nat.NativeError):
    """emulate(capacity=...) produced more events than the capacity: .n_events is the full count, .columns the (t_s, t, x, y, p)
    buffers, whose first `capacity` rows are valid.  The state has advanced past the frames."""

    def __init__(self, msg, n_events, columns):
        super().__init__(msg)
        self.n_events, self.columns = n_events, columns


def dvs_emulator(h, w, pos_thres=0.2, neg_thres=0.2, cutoff_hz=0, leak_rate_hz=0, noise_rate_array=None, refractory_period_s=0,
                 shot_noise_rate_hz=0, leak_jitter_fraction=0, max_iters=1024, device=None):
    """The reference's DVS emulator core (v2e/v2ecore/emulator.py: EventEmulator.generate_events) on the device: intensity frames
    -> the event stream render_events takes.  pos_thres / neg_thres: scalars or (h, w) float32 arrays (dvs_emulator.
    draw_pixel_arrays draws them the way the reference does for sigma_thres > 0); noise_rate_array likewise, used with
    leak_rate_hz > 0.  shot_noise_rate_hz and leak_jitter_fraction must be 0: both draw random numbers every frame.  max_iters:
    the most sub-iterations (events of one polarity at one pixel) one frame may need.  Returns a DvsEmulator:
    .emulate(frames, t) -> (t, x, y, p, t_s), .reset().  Events of one sub-iteration come out as all ON pixels in row-major
    order, then all OFF pixels (the reference shuffles each such group of equal stamps); p is 1 for ON (the reference's +1) and 0
    for OFF (its -1)."""
    return DvsEmulator(h, w, device=device, pos_thres=pos_thres, neg_thres=neg_thres, cutoff_hz=cutoff_hz, leak_rate_hz=leak_rate_hz,
                       noise_rate_array=noise_rate_array, refractory_period_s=refractory_period_s, shot_noise_rate_hz=shot_noise_rate_hz,
                       leak_jitter_fraction=leak_jitter_fraction, max_iters=max_iters)


def _finite_affines(who, trans, n):
    """ValueError naming the first of the rows trans[0 .. n) that holds a NaN or an infinity, or whose inverse map does: the device's
    cast of a NaN to an integer and NumPy's differ, so such a row has no defined crop."""
    import numpy as np
    from .utils.transforms import invert_affine_cv
    with np.errstate(all="ignore"):
        for i in range(n):
            t = np.asarray(trans[i], dtype=np.float64)
            if not np.isfinite(t).all():
                raise ValueError("%s: transform %d holds a non-finite entry: %s" % (who, i, t.tolist()))
            if not np.isfinite(invert_affine_cv(t)).all():
                raise ValueError("%s: the inverse map of transform %d is not finite: %s" % (who, i, t.tolist()))


def warp_window(trans, out_wh, frame_hw):
    """[x0, y0, w, h]: a window of the frame that contains every pixel crop_warp reads for this affine (host side, NumPy); clipped to the
    frame (w or h may be 0: nothing of the frame is read).  The union of two boxes:
      * the corners of the output grid through the inverse map as the kernel derives it, in real numbers, with two pixels of margin and
        three on the far side.  While no term saturates, the fixed-point coordinate lies less than 1 px below the real one and a
        bilinear tap reads (x, x + 1), so this box holds every tap; it is the window the loader and the decoders have always been given.
      * the same corners in the kernel's own integers (csrc/bilinear_fixed.h: affine_source).  The row term sat((m1 y + m2) 1024) and
        the column term sat(m0 x 1024) are each monotone, and so are >> 5, >> 5 and the int16 clip: the smallest and the largest first
        tap of the whole grid are reached at x in {0, W - 1}, y in {0, H - 1}.  Once a term saturates at +-2^31 (2^21 px, as
        cv::saturate_cast<int> does) or the index at int16, the taps are no longer near the real coordinates -- a saturated row term
        plus a large negative column term lands inside the frame -- and only this box holds them.
    ValueError for a transform with a non-finite entry."""
    import numpy as np
    from .utils.transforms import invert_affine_cv, _sat_int
    _finite_affines("warp_window", [trans], 1)
    m = np.asarray(invert_affine_cv(trans), dtype=np.float64).reshape(2, 3)
    w, h = int(out_wh[0]), int(out_wh[1])
    fh, fw = int(frame_hw[0]), int(frame_hw[1])
    ex = np.array([0.0, w - 1.0]); ey = np.array([0.0, h - 1.0])
    cx = np.array([0.0, w - 1.0, 0.0, w - 1.0]); cy = np.array([0.0, 0.0, h - 1.0, h - 1.0])
    win = []
    for (mc, mr, mt), size in ((m[0], fw), (m[1], fh)):
        with np.errstate(all="ignore"):
            first = np.clip((_sat_int((mr * ey + mt) * 1024.0)[:, None] + 16 + _sat_int(mc * ex * 1024.0)[None, :]) >> 10, -32768, 32767)
            real = mc * cx + mr * cy + mt
        lo, hi = int(first.min()), int(first.max()) + 2
        if np.isfinite(real).all():                     # (finite entries can still overflow in the sum: then the exact box alone)
            real = np.clip(real, -2.0 ** 31, 2.0 ** 31)
            lo = min(lo, int(np.floor(real.min())) - 2); hi = max(hi, int(np.ceil(real.max())) + 3)
        lo = min(max(lo, 0), size); hi = min(max(hi, 0), size)
        win.append((lo, max(hi - lo, 0)))
    return [win[0][0], win[1][0], win[0][1], win[1][1]]


def basic_block(conv1, conv2, xb):
    """Fused BasicBlock relu(conv2(relu(conv1(x))) + x) on a blocked tensor (two Conv objects, 3x3 stride 1, C -> C)."""
    _need_cuda(xb)
    n, planes, h, w, _ = xb.shape
    out = torch.empty_like(xb)
    nat.check(nat.lib().scpose_basic_block_forward(conv1._h, conv2._h, _ptr(xb), n, h, w, _ptr(out), _stream()),
              "basic_block_forward")
    return out


def flip_merge(out, out_flipped, flip_pairs, shift):
    """(out + flip_back(out_flipped)) * 0.5 of the flip test (lib/core/function.py:347-366), on the device.
    out / out_flipped: (N,J,H,W) f32 device heatmaps of the frame and of its x-flipped copy."""
    _need_cuda(out, out_flipped)
    a, b = out.contiguous().float(), out_flipped.contiguous().float()
    n, j, h, w = a.shape
    perm = list(range(j))
    for p0, p1 in flip_pairs:
        perm[p0], perm[p1] = p1, p0
    perm_d = torch.tensor(perm, dtype=torch.int32, device=a.device)
    res = torch.empty_like(a)
    nat.check(nat.lib().scpose_flip_merge(_ptr(a), _ptr(b), _ptr(perm_d), n, j, h, w, int(bool(shift)), _ptr(res),
                                          _stream()), "flip_merge")
    return res


def heatmap_accumulate(acc, x, div=1.0):
    """In place acc = (acc + x) / div on the device: the ensemble sum / mean of validate_cv
    (lib/core/function.py:530-536).  acc, x: float32 device tensors of the same shape."""
    _need_cuda(acc, x)
    if acc.shape != x.shape or acc.dtype != torch.float32 or x.dtype != torch.float32:
        raise nat.NativeError("heatmap_accumulate: float32 tensors of one shape expected")
    if not acc.is_contiguous():
        raise nat.NativeError("heatmap_accumulate: acc must be contiguous (it is updated in place)")
    nat.check(nat.lib().scpose_heatmap_accumulate(_ptr(acc), _ptr(x.contiguous()), float(div), acc.numel(), _stream()),
              "heatmap_accumulate")
    return acc


# ------------------------------------------------------------------ PnP
def pnp_epnp_ransac(kp_xyc, landmarks, K, dist, conf_thr0=0.95, min_pts=15, thr_decay=0.8, thr_iters=100,
                    max_iters=10000, reproj_err=15.0, confidence=0.99, want_rvec=False, rows=None, refine_iters=0,
                    want_inliers=False):
    """kp_xyc (N,J,3) f32 device; landmarks (J,3), K (3,3), dist (5,) f64 device.
    Returns rot (N,3,3) f64, tvec (N,3) f64, status (N,) i32 [, rvec (N,3)] [, inliers (N,J) bool].
    rows: a contiguous (N,13) f64 device buffer -> the kernel writes [R (9), t (3), status] per frame straight into it
    (scpose_pnp_epnp_ransac_rows) and `rows` is returned: the block a rank all-gathers and copies to the host
    (`(rows, inliers)` with want_inliers).
    refine_iters (0..100): Levenberg-Marquardt iterations on each solved frame's final point set after the final fit
    (scpose_pnp_epnp_ransac_refine; 20 = cv2.solvePnPRefineLM's default).  want_inliers: also return that point set per frame,
    inliers[i, j] = landmark j was used.  With both at their defaults the existing entry points are called, as before."""
    _need_cuda(kp_xyc, landmarks, K, dist)
    kp = kp_xyc.contiguous().float()
    n, j, _ = kp.shape
    dev = kp.device
    lm = landmarks.contiguous().double()
    if lm.dim() != 2 or tuple(lm.shape) != (j, 3):
        raise nat.NativeError("pnp_epnp_ransac: landmarks must be (%d, 3) to match the keypoints, got %s" % (j, tuple(lm.shape)))
    Kd = K.contiguous().double()
    if Kd.numel() != 9:
        raise nat.NativeError("pnp_epnp_ransac: K must be a 3x3 camera matrix, got %s" % (tuple(K.shape),))
    # distortion vector: the kernel reads exactly (k1, k2, p1, p2, k3).  cv2 also accepts 4 coefficients (k3 = 0);
    # the 8/12/14-coefficient rational / thin-prism / tilted models are not implemented and must not be truncated.
    dd = dist.contiguous().double().reshape(-1) if dist is not None else torch.zeros(5, dtype=torch.float64, device=dev)
    if dd.numel() == 4:
        dd = torch.cat([dd, torch.zeros(1, dtype=torch.float64, device=dd.device)])
    elif dd.numel() != 5:
        raise nat.NativeError("pnp_epnp_ransac: %d distortion coefficients; supported are 4 or 5 (k1,k2,p1,p2[,k3])" % dd.numel())
    refine = refine_iters != 0 or want_inliers
    inl = torch.zeros((n,), dtype=torch.int64, device=dev) if want_inliers else None   # uint64 bit masks, landmark order
    if rows is not None:
        if want_rvec:     # the gather block has no rvec column: refuse instead of silently returning one tensor
            raise nat.NativeError("pnp_epnp_ransac: rows=... excludes want_rvec (the (N, 13) block is [R, t, status]); call without rows for rvec")
        if tuple(rows.shape) != (n, 13) or rows.dtype != torch.float64 or not rows.is_contiguous() or rows.device != dev:
            raise nat.NativeError("pnp_epnp_ransac: rows must be a contiguous float64 (%d, 13) tensor on %s" % (n, dev))
        if refine:
            nat.check(nat.lib().scpose_pnp_epnp_ransac_refine(_ptr(kp), _ptr(lm), _ptr(Kd), _ptr(dd), n, j, conf_thr0, min_pts,
                                                              thr_decay, thr_iters, max_iters, reproj_err, confidence,
                                                              int(refine_iters), None, None, None, None, _ptr(rows),
                                                              _ptr(inl), _stream()),
                      "pnp_epnp_ransac_refine")
            return (rows, _mask_bits(inl, j)) if want_inliers else rows
        nat.check(nat.lib().scpose_pnp_epnp_ransac_rows(_ptr(kp), _ptr(lm), _ptr(Kd), _ptr(dd), n, j, conf_thr0, min_pts, thr_decay,
                                                        thr_iters, max_iters, reproj_err, confidence, _ptr(rows), _stream()),
                  "pnp_epnp_ransac_rows")
        return rows
    rot = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
    tv = torch.empty((n, 3), dtype=torch.float64, device=dev)
    rv = torch.empty((n, 3), dtype=torch.float64, device=dev)
    st = torch.empty((n,), dtype=torch.int32, device=dev)
    if refine:
        nat.check(nat.lib().scpose_pnp_epnp_ransac_refine(_ptr(kp), _ptr(lm), _ptr(Kd), _ptr(dd), n, j, conf_thr0, min_pts,
                                                          thr_decay, thr_iters, max_iters, reproj_err, confidence,
                                                          int(refine_iters), _ptr(rot), _ptr(tv), _ptr(rv), _ptr(st), None,
                                                          _ptr(inl), _stream()),
                  "pnp_epnp_ransac_refine")
        out = (rot, tv, st, rv) if want_rvec else (rot, tv, st)
        return out + (_mask_bits(inl, j),) if want_inliers else out
    nat.check(nat.lib().scpose_pnp_epnp_ransac(_ptr(kp), _ptr(lm), _ptr(Kd), _ptr(dd), n, j, conf_thr0, min_pts, thr_decay,
                                               thr_iters, max_iters, reproj_err, confidence, _ptr(rot), _ptr(tv), _ptr(rv),
                                               _ptr(st), _stream()), "pnp_epnp_ransac")
    return (rot, tv, st, rv) if want_rvec else (rot, tv, st)


def _mask_bits(masks, j):
    """(N,) int64 holding uint64 landmark bit masks -> (N, J) bool."""
    return ((masks.unsqueeze(1) >> torch.arange(j, device=masks.device, dtype=torch.int64)) & 1).bool()


# ------------------------------------------------------------------ HRNet engine
HEAD_CODES = {"pose_hrnet": 0, "hrnet_cms": 1, "hrnet_cms_384": 2}     # include/scpose.h SCPOSE_HEAD_*


def desc_from_cfg(cfg, dtype="bf16", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """cfg: yacs-like node or plain dict with MODEL.NUM_JOINTS, MODEL.EXTRA.STAGE{2,3,4} and (optionally)
    MODEL.NAME in pose_hrnet / hrnet_cms / hrnet_cms_384 (the modules of landmark_regression/lib/models/)."""
    model = cfg["MODEL"]
    extra = model["EXTRA"]
    name = str(model["NAME"]) if "NAME" in model else "pose_hrnet"
    if name == "pose_resnet":
        return resnet_desc_from_cfg(cfg, dtype, mean, std)
    d = nat.HrnetDesc()
    if name not in HEAD_CODES:
        raise nat.NativeError("MODEL.NAME=%s: supported models are %s, pose_resnet" % (name, ", ".join(HEAD_CODES)))
    d.head = HEAD_CODES[name]
    d.num_joints = int(model["NUM_JOINTS"])
    d.final_conv_kernel = int(extra["FINAL_CONV_KERNEL"])
    d.num_stages = 3
    for si, name in enumerate(("STAGE2", "STAGE3", "STAGE4")):
        s = extra[name]
        if str(s["BLOCK"]) not in ("BASIC", "BOTTLENECK"):
            raise nat.NativeError("%s.BLOCK=%s: stage blocks are BASIC or BOTTLENECK" % (name, s["BLOCK"]))
        d.block[si] = 1 if str(s["BLOCK"]) == "BOTTLENECK" else 0
        d.num_modules[si] = int(s["NUM_MODULES"])
        d.num_branches[si] = int(s["NUM_BRANCHES"])
        for b in range(int(s["NUM_BRANCHES"])):
            d.num_blocks[si][b] = int(s["NUM_BLOCKS"][b])
            d.num_channels[si][b] = int(s["NUM_CHANNELS"][b])
    d.dtype = dtype_code(dtype)
    for i in range(3):
        d.mean[i] = mean[i]
        d.std[i] = std[i]
    return d


def resnet_desc_from_cfg(cfg, dtype="bf16", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """scpose_resnet_desc of MODEL.NAME pose_resnet: MODEL.EXTRA holds NUM_LAYERS, DECONV_WITH_BIAS, NUM_DECONV_LAYERS / FILTERS /
    KERNELS and FINAL_CONV_KERNEL (the POSE_RESNET node of landmark_regression/lib/config/models.py).  The library judges the
    values; only what the fixed-size descriptor cannot hold is refused here."""
    model = cfg["MODEL"]
    extra = model["EXTRA"]
    d = nat.ResnetDesc()
    d.num_joints = int(model["NUM_JOINTS"])
    d.final_conv_kernel = int(extra["FINAL_CONV_KERNEL"])
    d.num_layers = int(extra["NUM_LAYERS"])
    n = int(extra["NUM_DECONV_LAYERS"])
    filters, kernels = list(extra["NUM_DECONV_FILTERS"]), list(extra["NUM_DECONV_KERNELS"])
    if n > 4:
        raise nat.NativeError("EXTRA.NUM_DECONV_LAYERS=%d: at most 4 deconv layers" % n)
    if n > len(filters) or n > len(kernels):
        raise nat.NativeError("EXTRA.NUM_DECONV_LAYERS=%d but %d NUM_DECONV_FILTERS and %d NUM_DECONV_KERNELS" % (n, len(filters), len(kernels)))
    d.num_deconv_layers = n
    for i in range(n):
        d.deconv_filters[i] = int(filters[i])
        d.deconv_kernels[i] = int(kernels[i])
    d.deconv_with_bias = int(bool(extra["DECONV_WITH_BIAS"]))
    d.dtype = dtype_code(dtype)
    for i in range(3):
        d.mean[i] = mean[i]
        d.std[i] = std[i]
    return d


class HrnetEngine:
    """Owns a native scpose_hrnet handle built from a state_dict (host f32 copies are
    only needed during create) and a torch-allocated workspace arena."""

    def __init__(self, cfg, state_dict, dtype="bf16", allow_missing=False, device=None):
        if not torch.cuda.is_available():
            raise nat.NativeError("no ROCm device visible: the HRNet engine only runs on the GPU")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.desc = desc_from_cfg(cfg, dtype)
        self.num_joints = self.desc.num_joints
        names, ptrs, numels, keep = [], [], [], []
        for k, v in state_dict.items():
            if not torch.is_floating_point(v):
                continue
            t = v.detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            names.append(k.encode())
            ptrs.append(t.data_ptr())
            numels.append(t.numel())
        n = len(names)
        c_names = (c_char_p * n)(*names)
        c_ptrs = (c_void_p * n)(*ptrs)
        c_numels = (c_int64 * n)(*numels)
        h = c_void_p()
        with torch.cuda.device(self.device):
            resnet = isinstance(self.desc, nat.ResnetDesc)     # MODEL.NAME pose_resnet: the same handle type from its own create
            create = nat.lib().scpose_resnet_create if resnet else nat.lib().scpose_hrnet_create
            nat.check(create(ctypes.byref(self.desc), c_names, c_ptrs, c_numels, n, int(allow_missing), ctypes.byref(h)),
                      "resnet_create" if resnet else "hrnet_create")
        self._h = h
        self._ws = None

    def workspace_bytes(self, n, h, w):
        return _query_bytes("hrnet_workspace_bytes", self._h, n, h, w)

    @staticmethod
    def _input_format(x, who=None):
        """(fmt, n, h, w) of the input batch x: uint8 (N, H, W, 3) or float32 (N, 3, H, W).  who: the capture method that binds x
        by address and so refuses a dtype it would have to convert; the forward methods convert before they ask."""
        if x.dtype == torch.uint8:
            n, h, w, c = x.shape
            fmt = nat.IN_U8_NHWC
        elif x.dtype == torch.float32:
            n, c, h, w = x.shape
            fmt = nat.IN_F32_NCHW
        else:
            raise nat.NativeError("%s: input must be uint8 NHWC or float32 NCHW" % who)
        if c != 3:
            raise nat.NativeError("HRNet input must have 3 channels, got %d" % c)
        return fmt, n, h, w

    def _grow_workspace(self, n, h, w, device):
        need = self.workspace_bytes(n, h, w)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)

    def _heatmap_buffer(self, who, n, h, w, device, out):
        """out, checked against the heat-map shape of an (n, h, w) input, or a new buffer of that shape when out is None."""
        shape = (n, self.num_joints) + self.heatmap_size(h, w)
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=device)
        if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise nat.NativeError("%s: out must be contiguous float32 %s" % (who, shape))
        return out

    def heatmap_size(self, h, w):
        oh = c_int32(); ow = c_int32()
        nat.check(nat.lib().scpose_hrnet_heatmap_size(self._h, h, w, ctypes.byref(oh), ctypes.byref(ow)), "hrnet_heatmap_size")
        return oh.value, ow.value

    def stats(self, h, w):
        l = c_int32(); f = c_double(); by = c_double()
        nat.check(nat.lib().scpose_hrnet_stats(self._h, h, w, ctypes.byref(l), ctypes.byref(f), ctypes.byref(by)), "hrnet_stats")
        return {"launches": l.value, "flops_per_frame": f.value, "act_bytes_per_frame": by.value}

    def executed_stats(self, h, w):
        """stats()'s two work figures for what the launches do: a NUM_CHANNELS entry that is no multiple of 16 is carried at
        the next one (zero planes), so W18 / W30 / W40 / W44 execute more than stats() -- the network as described -- counts."""
        f = c_double(); by = c_double()
        nat.check(nat.lib().scpose_hrnet_executed_stats(self._h, h, w, ctypes.byref(f), ctypes.byref(by)), "hrnet_executed_stats")
        return {"flops_per_frame": f.value, "act_bytes_per_frame": by.value}

    def forward(self, x, out=None, profile=False):
        """x: float32 (N,3,H,W) normalised, or uint8 (N,H,W,3) raw RGB.  Returns f32 (N,J,H/4,W/4).
        profile=True records a HIP event around every launch (read with profile_read())."""
        _need_cuda(x)
        x = x.contiguous() if x.dtype == torch.uint8 else x.contiguous().float()
        fmt, n, h, w = self._input_format(x)
        self._grow_workspace(n, h, w, x.device)
        out = self._heatmap_buffer("hrnet_forward", n, h, w, x.device, out)
        fn = nat.lib().scpose_hrnet_forward_profiled if profile else nat.lib().scpose_hrnet_forward
        nat.check(fn(self._h, _ptr(x), fmt, n, h, w, _ptr(out), _ptr(self._ws), self._ws.numel(), _stream()), "hrnet_forward")
        self._last_hw = (h, w)
        return out

    def tail_fused(self, n, h, w):
        """True when a forward of this shape runs the last fuse sum + final_layer (+ decode) as one kernel (head_fused.hip)."""
        k = c_int32()
        nat.check(nat.lib().scpose_hrnet_tail_fused(self._h, n, h, w, ctypes.byref(k)), "hrnet_tail_fused")
        return bool(k.value)

    def forward_decode(self, x, center, scale, post_process=True, heatmaps=False, profile=False):
        """Key points straight from the forward (scpose_hrnet_forward_decode): (N, J, 3) [x_img, y_img, maxval], bit-identical
        to decode(forward(x), center, scale, post_process).  For pose_hrnet with a 1x1 final layer no heat-map is written
        unless heatmaps=True (then (preds, heatmaps) is returned); other heads always go through a heat-map buffer.
        profile=True records a HIP event around every launch (read with profile_read())."""
        _need_cuda(x, center, scale)
        x = x.contiguous() if x.dtype == torch.uint8 else x.contiguous().float()
        fmt, n, h, w = self._input_format(x)
        self._grow_workspace(n, h, w, x.device)
        oh, ow = self.heatmap_size(h, w)
        hm = None
        if heatmaps or not self.tail_fused(n, h, w):
            hm = torch.empty((n, self.num_joints, oh, ow), dtype=torch.float32, device=x.device)
        cc = center.contiguous().float(); ss = scale.contiguous().float()
        preds = torch.empty((n, self.num_joints, 3), dtype=torch.float32, device=x.device)
        fn = nat.lib().scpose_hrnet_forward_decode_profiled if profile else nat.lib().scpose_hrnet_forward_decode
        nat.check(fn(self._h, _ptr(x), fmt, n, h, w, _ptr(cc), _ptr(ss), int(bool(post_process)),
                     _ptr(preds), _ptr(hm) if hm is not None else None, _ptr(self._ws),
                     self._ws.numel(), _stream()), "hrnet_forward_decode")
        self._last_hw = (h, w)
        return (preds, hm) if heatmaps else preds

    def capture_decode(self, x, center, scale, post_process=True, concurrent=True, heatmaps=False):
        """capture() for forward_decode: x, center and scale are bound by address (refill them in place); .replay() returns
        the bound (N, J, 3) key-point buffer; .heatmaps is the bound heat-map buffer when one exists."""
        _need_cuda(x, center, scale)
        for t, name in ((x, "input"), (center, "center"), (scale, "scale")):
            if not t.is_contiguous():
                raise nat.NativeError("capture_decode: the %s buffer must be contiguous (it is bound by address)" % name)
        if center.dtype != torch.float32 or scale.dtype != torch.float32:
            raise nat.NativeError("capture_decode: center / scale must be float32")
        fmt, n, h, w = self._input_format(x, "capture_decode")
        oh, ow = self.heatmap_size(h, w)
        hm = None
        if heatmaps or not self.tail_fused(n, h, w):
            hm = torch.empty((n, self.num_joints, oh, ow), dtype=torch.float32, device=x.device)
        preds = torch.empty((n, self.num_joints, 3), dtype=torch.float32, device=x.device)
        return HrnetGraph(self, x, fmt, (n, h, w), preds, concurrent, decode=(center, scale, bool(post_process), hm))

    def capture(self, x, out=None, concurrent=True):
        """Record the forward of the input BUFFER x (uint8 NHWC or float32 NCHW, fixed shape) into a hipGraph and return
        an HrnetGraph: refill x in place (x.copy_(...)), call .replay(), read .out.  concurrent=True (1) records the
        independent ops (module branches, fuse rows, transition convs) on parallel graph branches; concurrent=2 only the
        fuse rows and transition convs (large batches, whose branch kernels each fill the chip); 0 / False none."""
        _need_cuda(x)
        if not x.is_contiguous():
            raise nat.NativeError("capture: the input buffer must be contiguous (it is bound by address)")
        fmt, n, h, w = self._input_format(x, "capture")
        out = self._heatmap_buffer("capture", n, h, w, x.device, out)
        return HrnetGraph(self, x, fmt, (n, h, w), out, concurrent)

    def tap_names(self):
        cap = 4096
        while True:   # every op output is a tap: W48 offers well over 4 KB of names; grow until the library accepts the buffer
            buf = ctypes.create_string_buffer(cap)
            rc = nat.lib().scpose_hrnet_tap_names(self._h, buf, cap)
            if rc == 0 or cap >= 1 << 24:
                break
            cap *= 4
        nat.check(rc, "hrnet_tap_names")
        return buf.value.decode().split(",")

    def forward_tap(self, x, tap):
        """Intermediate tensor `tap` ("stem2", "layer1", "stage3.1.out0", ...) of the forward of x as float32
        (N, C, h, w): the forward is run up to the op that produces it (unit-level parity against the oracle's taps)."""
        _need_cuda(x)
        x = x.contiguous() if x.dtype == torch.uint8 else x.contiguous().float()
        fmt, n, h, w = self._input_format(x)
        self._grow_workspace(n, h, w, x.device)
        c = c_int32(); oh = c_int32(); ow = c_int32()
        fn = nat.lib().scpose_hrnet_forward_tap
        nat.check(fn(self._h, None, fmt, n, h, w, tap.encode(), None, ctypes.byref(c), ctypes.byref(oh), ctypes.byref(ow), None, 0, None),
                  "hrnet_forward_tap")
        out = torch.empty((n, c.value, oh.value, ow.value), dtype=torch.float32, device=x.device)
        nat.check(fn(self._h, _ptr(x), fmt, n, h, w, tap.encode(), _ptr(out), None, None, None, _ptr(self._ws), self._ws.numel(), _stream()),
                  "hrnet_forward_tap")
        return out

    def profile_read(self):
        """Per-launch records of the last profiled forward: list of dicts
        {ms, flops_per_frame, bytes_per_frame, kind, a, cin, cout}."""
        cnt = c_int32()
        nat.check(nat.lib().scpose_hrnet_profile_read(self._h, 0, 0, 0, None, None, None, None, ctypes.byref(cnt)), "profile_read")
        k = cnt.value
        ms = np.zeros(k, dtype=np.float32); fl = np.zeros(k); by = np.zeros(k); sig = np.zeros((k, 4), dtype=np.int32)
        h, w = self._last_hw
        nat.check(nat.lib().scpose_hrnet_profile_read(self._h, h, w, k, c_void_p(ms.ctypes.data), c_void_p(fl.ctypes.data),
                                                      c_void_p(by.ctypes.data), c_void_p(sig.ctypes.data), ctypes.byref(cnt)),
                  "profile_read")
        return [{"ms": float(ms[i]), "flops_per_frame": float(fl[i]), "bytes_per_frame": float(by[i]),
                 "kind": int(sig[i, 0]), "a": int(sig[i, 1]), "cin": int(sig[i, 2]), "cout": int(sig[i, 3])} for i in range(k)]

    __call__ = forward

    @staticmethod
    def kernel_classes(recs):
        """Class name of every record of profile_read(): 'kind:a:cin:cout', with '@<output pixels per frame>' appended where one
        forward runs the same layer shape at two map sizes (the 48->48 stride-2 convs of the 96x96 -> 12x12 fuse chain), so
        that per-class statistics never mix launches with different work."""
        base = ["%d:%d:%d:%d" % (r["kind"], r["a"], r["cin"], r["cout"]) for r in recs]
        work = {}
        for b, r in zip(base, recs):
            work.setdefault(b, set()).add(r["flops_per_frame"])      # same layer shape, different map size (bytes alone also differ with a residual)
        out = []
        for b, r in zip(base, recs):
            if len(work[b]) > 1 and r["kind"] == 1:
                k = r["a"] // 10
                out.append("%s@%d" % (b, round(r["flops_per_frame"] / (2.0 * r["cin"] * r["cout"] * k * k))))
            else:
                out.append(b)
        return out

    def close(self):
        # captured graphs bake in this engine's packed-weight pointers: destroy them first, so that no graph can replay
        # kernels that read freed weights (their replay() raises afterwards)
        for ref in list(getattr(self, "_graphs", ())):
            g = ref()
            if g is not None:
                g.close()
        self._graphs = []
        if getattr(self, "_h", None):
            nat.lib().scpose_hrnet_destroy(self._h)
            self._h = None
        self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HrnetGraph:
    """A captured forward (scpose_hrnet_graph_*): fixed input / output / workspace buffers, one launch per replay."""

    def __init__(self, engine, x, fmt, nhw, out, concurrent, decode=None):
        n, h, w = nhw
        self.engine, self.x, self.out = engine, x, out
        self._ws = torch.empty(_query_bytes("hrnet_graph_workspace_bytes", engine._h, n, h, w), dtype=torch.uint8, device=x.device)       # owned by the graph: addresses are baked in
        torch.cuda.synchronize(x.device)     # create runs one eager forward on an internal stream: every pending write to x / out,
                                             # on any stream of x's device (not only the current one), must have landed
        g = c_void_p()
        self.heatmaps = None
        with torch.cuda.device(x.device):
            if decode is None:
                nat.check(nat.lib().scpose_hrnet_graph_create(engine._h, _ptr(x), fmt, n, h, w, _ptr(out), _ptr(self._ws), self._ws.numel(),
                                                              int(concurrent), ctypes.byref(g)), "hrnet_graph_create")
            else:   # out = the key-point buffer; the decode's inputs are bound like x
                self.center, self.scale, post, self.heatmaps = decode
                nat.check(nat.lib().scpose_hrnet_graph_create_decode(
                    engine._h, _ptr(x), fmt, n, h, w, _ptr(self.center), _ptr(self.scale), int(post), _ptr(out),
                    _ptr(self.heatmaps) if self.heatmaps is not None else None, _ptr(self._ws), self._ws.numel(), int(concurrent),
                    ctypes.byref(g)), "hrnet_graph_create_decode")
        self._g = g
        k = c_int32()
        nat.check(nat.lib().scpose_hrnet_graph_nodes(self._g, ctypes.byref(k)), "hrnet_graph_nodes")
        self.nodes = k.value
        import weakref
        if not hasattr(engine, "_graphs"):
            engine._graphs = []
        engine._graphs.append(weakref.ref(self))     # HrnetEngine.close() destroys its live graphs before its weights

    def replay(self):
        """Enqueue the captured forward on the current stream; returns the (bound) heat-map buffer."""
        if not getattr(self, "_g", None):
            raise RuntimeError("HrnetGraph.replay(): the graph (or its engine) has been closed")
        nat.check(nat.lib().scpose_hrnet_graph_launch(self._g, _stream()), "hrnet_graph_launch")
        return self.out

    def close(self):
        if getattr(self, "_g", None):
            nat.lib().scpose_hrnet_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
