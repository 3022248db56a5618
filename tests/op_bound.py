"""The per-op parity rule of the teacher-forced forward checks (tests/test_gpu_forward_ops.py, tests/test_gpu_conv.py).

An op y = round16(relu(sum w x + b + r)) with 16-bit x and w is compared with ref, the float64 result rounded once to the
16-bit grid (oracle/hrnet_ref.run_op(acc="f64")).  Products of two 16-bit values are exact in fp32, so an implementation
that accumulates in fp32 in ANY order (MFMA included) is off the exact sum by at most K 2^-24 S, S = conv(|x|, |w|) + |b| + |r|,
K = Cin k^2 + 2; its store and ref's can then land one grid step apart.  Hence, element-wise:

    |got - ref| <= u16(max(|got|, |ref|)) + E          (E: run_op's allowance; f32 outputs have no u16 term)

This bound is derived, not fitted: a correct kernel cannot fail it.  Two more statistics catch what it cannot:
  * the signed mean of sign(ref) (got - ref) / u16(ref) over ref != 0 is ~0 for round-to-nearest-even and about -0.5 for
    truncation;
  * the fraction of elements more than one grid step apart (asserted per op class in the GPU test, ~2x measured).
"""
import torch

from oracle import hrnet_ref as R

BIAS_LIMIT = 0.05


def u16(t, dtype):
    return R.u16(t, dtype)


def stats(got, ref, E, dtype, out_f32=False):
    """Returns a dict: n, hard-bound violations, max |d| / u16(max(|got|, |ref|)), max |d| / allowance, fraction differing,
    fraction more than one step u16(ref) apart, signed mean."""
    got, ref = got.double(), ref.double()
    d = got - ref
    unit = u16(ref, dtype)
    allow = E + (0.0 if out_f32 else u16(torch.maximum(got.abs(), ref.abs()), dtype))
    nz = ref != 0
    signed = (torch.sign(ref[nz]) * d[nz] / unit[nz]).mean().item() if nz.any() else 0.0
    big = u16(torch.maximum(got.abs(), ref.abs()), dtype)      # (u16(ref) at ref == 0 is the subnormal step: no scale to read)
    return {"n": d.numel(), "viol": int((d.abs() > allow).sum()), "max_ulp": (d.abs() / big).max().item() if d.numel() else 0.0,
            "use": (d.abs() / allow).max().item() if d.numel() else 0.0,
            "diff": (d != 0).double().mean().item(), "beyond": (d.abs() > unit).double().mean().item(), "signed": signed,
            "worst": (d.abs() - allow).max().item() if d.numel() else 0.0}


def check(got, ref, E, dtype, what, out_f32=False, bias_check=True):
    """Asserts the hard bound (every element) and, for 16-bit outputs, the rounding-bias bound; returns stats()."""
    s = stats(got, ref, E, dtype, out_f32)
    assert s["viol"] == 0, "%s: %d / %d elements beyond the arithmetic bound (worst excess %.3g, max %.2f steps)" % (
        what, s["viol"], s["n"], s["worst"], s["max_ulp"])
    if bias_check and not out_f32:
        assert abs(s["signed"]) <= BIAS_LIMIT, "%s: signed mean %.3f steps: biased rounding" % (what, s["signed"])
    return s


def conv_ref(x, w, b, stride, dtype, res=None, relu=False, store=True):
    """Single conv stage in float64 with its allowance: x, w (16-bit values), b, res as float tensors."""
    x, w, b = x.double(), w.double(), b.double()
    pad = (w.shape[-1] - 1) // 2
    v = torch.nn.functional.conv2d(x, w, b, stride, pad)
    S = torch.nn.functional.conv2d(x.abs(), w.abs(), b.abs(), stride, pad)
    if res is not None:
        v, S = v + res.double(), S + res.double().abs()
    if relu:
        v = torch.relu(v)
    E = (w.shape[1] * w.shape[2] * w.shape[3] + 2) * 2.0 ** -24 * S
    if store:
        v = v.to(R._DT[dtype]).double()
    return v, E, S
