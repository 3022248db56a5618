"""Parity of the MFMA implicit-GEMM convolution (csrc/conv_igemm.hip) through the C ABI
against torch's CPU float32 conv2d on identical 16-bit-rounded operands.

Tolerance: the kernel accumulates in fp32 and rounds once to bf16 (8 significand bits), so
agreement is required to 2 bf16 ulps of the result scale: |d| <= 1e-2*|ref| + 1e-2*rms(ref).
Also, element-wise against the float64 result rounded once (tests/op_bound.py): one grid step + K 2^-24 S, and no rounding
bias.
"""
import pytest
import torch
import torch.nn.functional as F

import op_bound as OB

pytestmark = pytest.mark.gpu

#        cin cout k s  H   W  N  res   relu
CASES = [
    (48, 48, 3, 1, 96, 96, 2, True, True),      # W48 branch 0 (mrep 3, nrep 4, single 6-plane chunk)
    (96, 96, 3, 1, 48, 48, 2, True, True),      # branch 1 (mrep 6)
    (192, 192, 3, 1, 24, 24, 2, True, True),    # branch 2 (2 Cout blocks, 24-wide tile, nrep 3)
    (384, 384, 3, 1, 12, 12, 3, True, True),    # branch 3 (4 Cout blocks, whole-image tile)
    (32, 32, 3, 1, 64, 64, 1, True, True),      # W32 branches
    (64, 64, 3, 1, 32, 32, 2, False, True),
    (128, 128, 3, 1, 16, 16, 2, True, False),
    (256, 256, 3, 1, 8, 8, 3, True, True),
    (64, 64, 3, 2, 192, 192, 1, False, True),   # stem conv2
    (64, 256, 1, 1, 96, 96, 1, False, False),   # layer1 1x1s
    (256, 64, 1, 1, 96, 96, 1, False, True),
    (64, 64, 1, 1, 32, 32, 2, False, True),
    (256, 48, 3, 1, 96, 96, 1, False, True),    # transition1
    (256, 96, 3, 2, 96, 96, 1, False, True),
    (48, 96, 3, 2, 96, 96, 2, False, False),    # fuse down paths
    (48, 48, 3, 2, 96, 96, 1, False, True),
    (96, 192, 3, 2, 48, 48, 2, False, False),
    (192, 384, 3, 2, 24, 24, 2, False, True),
    (96, 48, 1, 1, 48, 48, 2, False, False),    # fuse up paths (1x1)
    (384, 48, 1, 1, 12, 12, 2, False, False),
    (192, 96, 1, 1, 24, 24, 2, False, False),
    (48, 48, 3, 1, 20, 20, 2, True, True),      # ragged: tile overhangs the map
    (32, 64, 3, 2, 40, 40, 1, False, True),
    (16, 16, 3, 1, 6, 6, 2, True, True),        # tiny maps
    (16, 32, 3, 2, 2, 2, 3, False, False),
    (128, 16, 1, 1, 2, 2, 1, False, False),
    (80, 80, 3, 1, 16, 16, 1, True, True),      # Cout not on a 48/64/96 grid (padded block): conv_pipe, two tiles per weight chunk
    (80, 80, 3, 1, 20, 12, 3, True, True),      # ... one 20 x 12 tile per image, three images: the last work item has a single tile
    # 32x32x16-MFMA kernels (conv_m32 / conv_m32p): ragged maps, several Cout blocks, segment groups
    (96, 96, 3, 1, 20, 28, 3, True, True),
    (96, 192, 3, 1, 24, 24, 3, True, False),
    (192, 96, 3, 1, 10, 14, 5, False, True),
    (64, 128, 3, 1, 17, 9, 2, True, True),
    (32, 96, 3, 1, 12, 12, 7, True, True),      # 2 K-chunks only: single-role kernel, not producer/consumer
    (384, 384, 3, 1, 5, 5, 9, True, True),
    (96, 96, 3, 1, 1, 1, 4, True, True),
    # 48-row Cout blocks on the 16x16x32 consumers' 3 x 8 form (conv_m32p_kernel.h, M16 = 3): deep-K stride-1 layers with 48 output
    # channels (transition1 is the one in HRNet); residual epilogue, ragged maps, several images per work item, one-pixel maps
    (256, 48, 3, 1, 20, 28, 3, True, True),
    (128, 48, 3, 1, 24, 24, 2, True, False),
    (192, 48, 3, 1, 5, 7, 9, False, True),
    (256, 48, 3, 1, 1, 1, 4, True, True),
    # register-weight stride-2 kernel (conv_s2r.hip): every (Cin, channel-group) variant, ragged / odd maps, one-row maps
    (48, 192, 3, 2, 48, 48, 2, False, True),
    (48, 48, 3, 2, 18, 50, 3, False, False),
    (48, 96, 3, 2, 9, 7, 2, False, True),
    (32, 32, 3, 2, 64, 64, 1, False, True),
    (32, 128, 3, 2, 34, 22, 2, False, False),
    (64, 128, 3, 2, 32, 32, 2, False, True),
    (64, 32, 3, 2, 5, 33, 1, False, True),
    (64, 64, 3, 2, 1, 1, 5, False, False),
    (64, 64, 3, 1, 20, 12, 3, False, True),     # register-weight kernel, stride 1 (layer1's 3x3), ragged map
    (64, 64, 3, 1, 16, 16, 2, True, False),     # ... with a residual it stays on the 32x32x16 kernel
    # register-weight kernel for 96 input channels (conv_s2r12_kernel, 12 waves): Cout 96 (6 blocks x 2 row sets), 192, 384 (two
    # passes), ragged / odd / one-pixel maps, enough tiles for several per workgroup
    (96, 384, 3, 2, 24, 24, 2, False, True),
    (96, 96, 3, 2, 48, 48, 2, False, True),
    (96, 192, 3, 2, 18, 50, 3, False, False),
    (96, 192, 3, 2, 9, 7, 2, False, True),
    (96, 384, 3, 2, 1, 1, 5, False, False),
    (96, 192, 3, 2, 96, 96, 8, False, True),
    # stride 2 with channel counts outside the register-weight kernel's grid: producer/consumer kernel, 2-plane chunks
    (48, 64, 3, 2, 24, 24, 2, False, True),
    (96, 96, 3, 2, 20, 12, 2, False, False),
    (64, 96, 3, 2, 16, 16, 1, False, True),
    # streaming 1x1 kernel, one workgroup per CU (more than 80 KB of weights in LDS: built for 6 / 8 / 12 k-steps); and a shallow layer with
    # that many weights, which must fall back to conv_pipe instead of launching a two-per-CU variant past its LDS opt-in
    (384, 192, 1, 1, 12, 12, 3, False, False),
    (384, 96, 1, 1, 12, 12, 3, True, True),
    (128, 384, 1, 1, 10, 10, 2, False, True),
    (128, 512, 1, 1, 6, 6, 2, True, False),
]


def _rnd(t, dt):
    return t.to(dt).to(torch.float32)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%d-%d_k%d_s%d_%dx%d_n%d" % c[:7])
def test_conv_matches_cpu(gpu_ops, case, dtype):
    cin, cout, k, s, H, W, N, use_res, relu = case
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(1000 * cin + cout + k + s + H)
    x = _rnd(torch.randn(N, cin, H, W, generator=g), tdt)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    res = _rnd(torch.randn(N, cout, Ho, Wo, generator=g), tdt) if use_res else None

    ref = F.conv2d(x, _rnd(w, tdt), b, s, (k - 1) // 2)
    if res is not None:
        ref = ref + res
    if relu:
        ref = F.relu(ref)

    conv = gpu_ops.Conv(w, b, stride=s, dtype=dtype)
    xb = gpu_ops.to_blocked(x.cuda(), dtype)
    rb = gpu_ops.to_blocked(res.cuda(), dtype) if res is not None else None
    got = gpu_ops.from_blocked(conv(xb, residual=rb, relu=relu)).cpu()
    assert got.shape == ref.shape
    tol = 1e-2 * ref.abs() + 1e-2 * ref.pow(2).mean().sqrt()
    bad = (got - ref).abs() > tol
    assert not bad.any(), "max |d| %.4g (tol %.4g) at %d/%d elements" % (
        (got - ref).abs().max(), tol.min(), int(bad.sum()), bad.numel())
    ref64, E, _ = OB.conv_ref(x, _rnd(w, tdt), b, s, dtype, res=res, relu=relu)
    OB.check(got, ref64, E, dtype, "conv", bias_check=got.numel() >= 4096)


def test_conv_f32_nchw_output_with_joint_padding(gpu_ops):
    """final_layer: Cout = 11 joints (padded to 16 in the MFMA tile), float32 NCHW output, bias."""
    g = torch.Generator().manual_seed(5)
    x = _rnd(torch.randn(2, 48, 96, 96, generator=g), torch.bfloat16)
    w = torch.randn(11, 48, 1, 1, generator=g) / 48 ** 0.5
    b = torch.randn(11, generator=g)
    ref = F.conv2d(x, _rnd(w, torch.bfloat16), b)
    conv = gpu_ops.Conv(w, b, dtype="bf16")
    got = conv(gpu_ops.to_blocked(x.cuda()), out_nchw_f32=True).cpu()
    assert got.shape == (2, 11, 96, 96) and got.dtype == torch.float32
    assert (got - ref).abs().max() < 2e-4 * max(1.0, ref.abs().max().item())   # fp32 out: only summation order differs


def test_layout_roundtrip_is_exact(gpu_ops):
    x = _rnd(torch.randn(3, 40, 7, 9), torch.bfloat16)
    back = gpu_ops.from_blocked(gpu_ops.to_blocked(x.cuda())).cpu()
    assert torch.equal(back, x)


def test_fuse_sum_matches_reference_order(gpu_ops):
    """relu(x0 + up2(z1) + up4(z2) + up8(z3)) -- HighResolutionModule.forward :256-263."""
    g = torch.Generator().manual_seed(7)
    bf = torch.bfloat16
    x0 = _rnd(torch.randn(2, 48, 32, 32, generator=g), bf)
    zs = [_rnd(torch.randn(2, 48, 32 >> s, 32 >> s, generator=g), bf) for s in (1, 2, 3)]
    ref = x0.clone()
    for s, z in zip((1, 2, 3), zs):
        ref = ref + F.interpolate(z, scale_factor=2 ** s, mode="nearest")
    ref = _rnd(F.relu(ref), bf)
    terms = [gpu_ops.to_blocked(t.cuda()) for t in [x0] + zs]
    got = gpu_ops.from_blocked(gpu_ops.fuse_sum(terms, [0, 1, 2, 3], (32, 32))).cpu()
    assert torch.equal(got, ref)          # same fp32 sum order, one rounding: bit-exact


def test_bad_arguments_report_errors(gpu_ops):
    with pytest.raises(gpu_ops.nat.NativeError, match="multiple of 16"):
        gpu_ops.Conv(torch.zeros(8, 12, 3, 3))
    with pytest.raises(gpu_ops.nat.NativeError, match="kernel size"):
        gpu_ops.Conv(torch.zeros(16, 16, 5, 5))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(48, 96, 96, 2), (48, 24, 40, 3), (32, 64, 64, 2), (48, 7, 5, 4), (32, 16, 16, 1)],
                         ids=lambda s: "c%d_%dx%d_n%d" % s)
def test_fused_basic_block_matches_two_convs(gpu_ops, shape, dtype):
    """scpose_basic_block_forward (one kernel, intermediate tile in LDS) against the CPU float32 composition
    relu(conv2(round16(relu(conv1(x)))) + x) -- the intermediate is rounded to 16 bits exactly where the unfused
    path stores it -- and against the two unfused HIP launches."""
    C, H, W, N = shape
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(7 * C + H)
    x = _rnd(torch.randn(N, C, H, W, generator=g), tdt)
    w1 = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
    w2 = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b1 = torch.randn(C, generator=g) * 0.1
    b2 = torch.randn(C, generator=g) * 0.1
    mid = _rnd(F.relu(F.conv2d(x, _rnd(w1, tdt), b1, 1, 1)), tdt)
    ref = F.relu(F.conv2d(mid, _rnd(w2, tdt), b2, 1, 1) + x)
    c1 = gpu_ops.Conv(w1, b1, dtype=dtype)
    c2 = gpu_ops.Conv(w2, b2, dtype=dtype)
    xb = gpu_ops.to_blocked(x.cuda(), dtype)
    got = gpu_ops.from_blocked(gpu_ops.basic_block(c1, c2, xb)).cpu()
    two = gpu_ops.from_blocked(c2(c1(xb, relu=True), residual=xb, relu=True)).cpu()
    tol = 1.5e-2 * ref.abs() + 1.5e-2 * ref.pow(2).mean().sqrt()
    assert not ((got - ref).abs() > tol).any(), "fused vs CPU: max |d| %.4g" % (got - ref).abs().max()
    assert not ((got - two).abs() > tol).any(), "fused vs unfused HIP: max |d| %.4g" % (got - two).abs().max()
    # as a composite against float64: the intermediate's allowance (its fp32 error, then a grid step) carried through conv2
    mid64, E1, _ = OB.conv_ref(x, _rnd(w1, tdt), b1, 1, dtype, relu=True)
    E1 = E1 + OB.u16(mid64.abs() + E1, dtype)
    ref64, E2, _ = OB.conv_ref(mid64, _rnd(w2, tdt), b2, 1, dtype, res=x, relu=True)
    E2 = E2 + F.conv2d(E1, _rnd(w2, tdt).double().abs(), None, 1, 1)
    OB.check(got, ref64, E2, dtype, "fused block", bias_check=got.numel() >= 4096)


BLOCK_SPLIT_CODE = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, scpose
from importlib import import_module
ops = import_module('spacecraft-pose-estimation_amd.ops')
out = {}
for C, H, W in %(shapes)r:
    for dtype in ('bf16', 'f16'):
        g = torch.Generator().manual_seed(7 * C + H)
        x = torch.randn(%(n)d, C, H, W, generator=g)
        w1 = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
        w2 = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
        b1 = torch.randn(C, generator=g) * 0.1
        b2 = torch.randn(C, generator=g) * 0.1
        c1 = ops.Conv(w1, b1, dtype=dtype)
        c2 = ops.Conv(w2, b2, dtype=dtype)
        y = ops.from_blocked(ops.basic_block(c1, c2, ops.to_blocked(x.cuda(), dtype)))
        out['c%%d_%%dx%%d_%%s' %% (C, H, W, dtype)] = y.float().cpu().numpy()
np.savez(%(dst)r, **out)
"""


def test_fused_basic_block_frame_range_split(gpu_ops, tmp_path):
    """The fused BasicBlock addresses its tensor through 32-bit buffer descriptors, so a batch whose tensor reaches 4 GiB runs as
    several launches over frame ranges, both pointers advanced by the frame size.  The development switch SCPOSE_MAXN forces
    that split on five frames (ranges of 2, 2 and 1): same bits as one launch (sub-processes: switches are read once per process)."""
    import os
    import subprocess
    import sys
    import numpy as np
    from importlib import import_module
    nat = import_module("spacecraft-pose-estimation_amd._native")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shapes = [(48, 24, 40), (32, 16, 16)]

    def run(tag, extra_env):
        dst = str(tmp_path / (tag + ".npz"))
        env = {k: v for k, v in os.environ.items() if not k.startswith("SCPOSE_")}
        env.update(extra_env)
        code = BLOCK_SPLIT_CODE % dict(root=root, shapes=shapes, n=5, dst=dst)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        return np.load(dst), [ln for ln in r.stderr.splitlines() if ln.startswith("block ")]

    whole, _ = run("whole", {})
    # SCPOSE_DBG=32: the frame range of every launch is printed (common.h: for_frame_ranges)
    split, ranges = run("split", {"SCPOSE_DEV": "1", "SCPOSE_MAXN": "2", "SCPOSE_DBG": "32", "SCPOSE_LIB": nat.LIB_PATH})
    # the switch did switch: three launches per block, over frames 0..2, 2..4 and 4..5
    assert ranges == ["block %d %dx%d N=5: frames %s" % (C, H, W, fr) for C, H, W in shapes for _ in ("bf16", "f16")
                      for fr in ("0..2", "2..4", "4..5")], ranges
    assert len(whole.files) == 2 * len(shapes)
    for key in whole.files:
        a, b = torch.from_numpy(whole[key]), torch.from_numpy(split[key])
        assert a.shape[0] == 5 and torch.isfinite(a).all() and a.abs().max() > 0, key
        assert torch.equal(a, b), "%s: %d of %d elements differ" % (key, int((a != b).sum()), a.numel())


EQUIVARIANCE = [  # cin cout k s H   N  res   -- one shape per kernel family at batch sizes that fill the persistent grid
    (96, 96, 3, 1, 48, 96, True),      # conv_m32p, weights in producer registers
    (192, 192, 3, 1, 24, 128, True),   # conv_m32p, several K-chunks
    (384, 384, 3, 1, 12, 256, True),   # conv_m32p, two segments per work item
    (48, 96, 3, 2, 96, 64, False),     # conv_m32p stride 2
    (64, 64, 3, 1, 96, 48, False),     # conv_m32 (single role)
    (256, 48, 3, 1, 96, 32, False),
    (64, 256, 1, 1, 96, 32, True),     # conv_pipe 1x1, two workgroups per CU
    (48, 48, 3, 1, 96, 48, True),      # conv_pipe 3x3 (unfused branch-0 layer)
    (96, 192, 3, 2, 48, 128, False),   # conv_s2r12 (12 waves, register weights)
    (96, 384, 3, 2, 24, 256, False),   # ... two passes
    (192, 384, 3, 2, 24, 128, False),  # conv_m32p stride 2 (Cin >= 192 stays there)
]


@pytest.mark.parametrize("case", EQUIVARIANCE, ids=lambda c: "c%d-%d_k%d_s%d_%d_n%d" % c[:6])
def test_conv_is_equivariant_under_frame_permutation(gpu_ops, case):
    """A frame's result must not depend on its position in the batch, i.e. on which workgroup computes it
    (bit-exact): K-chunks and taps are accumulated in one fixed order everywhere."""
    cin, cout, k, s, H, N, use_res = case
    g = torch.Generator().manual_seed(cin + cout + H)
    conv = gpu_ops.Conv(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, torch.randn(cout, generator=g) * 0.1, stride=s)
    x = torch.randn(N, cin // 8, H, H, 8, generator=g).bfloat16().cuda()
    Ho = (H - 1) // s + 1
    r = torch.randn(N, cout // 8, Ho, Ho, 8, generator=g).bfloat16().cuda() if use_res else None
    perm = torch.randperm(N, generator=g).cuda()
    y = conv(x, residual=r, relu=True)
    yp = conv(x[perm].contiguous(), residual=r[perm].contiguous() if use_res else None, relu=True)
    assert torch.equal(yp, y[perm])
    # and a sub-batch gives the same frames (different grid size / items per workgroup)
    m = max(1, N // 3)
    ys = conv(x[:m].contiguous(), residual=r[:m].contiguous() if use_res else None, relu=True)
    assert torch.equal(ys, y[:m])


def test_development_switches_need_scpose_dev(gpu_ops):
    """A stray SCPOSE_* variable must not steer a production process: the ablation switch SCPOSE_DBG=1 (skip the MFMA
    loops) is ignored unless SCPOSE_DEV=1 is set too, and then the library says so on stderr.  The ablation paths exist
    only in the development build (libscpose_hip_dev.so, -DSCPOSE_DEV_BUILD): the shipped library ignores SCPOSE_DBG even
    with SCPOSE_DEV=1, because its kernels do not contain them."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import torch, scpose; from importlib import import_module; "
            "ops = import_module('spacecraft-pose-estimation_amd.ops'); g = torch.Generator().manual_seed(0); "
            "w = torch.randn(96, 96, 3, 3, generator=g) / 30; x = torch.randn(2, 12, 16, 16, 8, generator=g).bfloat16(); "
            "y = ops.Conv(w)(x.cuda()).float().cpu(); "
            "xr = x.float().permute(0, 1, 4, 2, 3).reshape(2, 96, 16, 16); "
            "ref = torch.nn.functional.conv2d(xr, w.bfloat16().float(), padding=1).reshape(2, 12, 8, 16, 16).permute(0, 1, 3, 4, 2); "
            "print('REL %%.4f' %% float((y - ref).norm() / ref.norm()))") % root

    def run(extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("SCPOSE_")}
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        rel = float([l for l in r.stdout.splitlines() if l.startswith("REL")][0].split()[1])
        return rel, r.stderr

    rel, err = run({"SCPOSE_DBG": "1"})
    assert rel < 1e-2 and "SCPOSE_DEV" not in err
    from importlib import import_module
    nat = import_module("spacecraft-pose-estimation_amd._native")
    assert nat.lib().scpose_is_dev_build() == 0          # this test process runs the shipped library
    rel, err = run({"SCPOSE_DBG": "1", "SCPOSE_DEV": "1", "SCPOSE_LIB": os.path.join(os.path.dirname(nat.DEV_LIB_PATH), nat.LIB_NAME)})
    assert rel < 1e-2 and "SCPOSE_DEV=1" in err          # shipped library: no ablation path to switch on
    if os.path.exists(nat.DEV_LIB_PATH):
        rel, err = run({"SCPOSE_DBG": "1", "SCPOSE_DEV": "1"})   # development build, picked up through SCPOSE_DEV=1
        assert rel > 0.5 and "SCPOSE_DEV=1" in err


#  cin cout k s  H   res    f32   tile-search switches, what the "m32" line of each launch must match (None: not a conv_m32 / conv_m32p layer)
RANGE_SPLIT = [  # one per kernel family under conv_launch: the channel pairs of EQUIVARIANCE (whose 64 -> 256 is the streaming 1x1 kernel's), a
    # conv_pipe 1x1, conv_s2r and final_layer's float32 NCHW output; N = 5, H x (H - 3) maps.  At these sizes the tile search takes the
    # small-tile producer/consumer forms (cp = 4, two 16-pixel columns; 64 -> 64 too): the two families it then never reaches are asked
    # for through its development switches, in the whole run and in the split run alike
    (96, 96, 3, 1, 20, True, False, {"SCPOSE_M32_CPMUL": "1", "SCPOSE_M16_NB": "6"}, "mr=3 nr=3 nb16=6 occ=3 cp=2 "),  # conv_m32p, weights in producer
    #                                                                    registers: one Cout block, six K-chunks of two planes, six 16-pixel columns
    (192, 192, 3, 1, 24, True, False, {}, r"mr=3 nr=\d nb16=[1-9] occ=3 "),  # conv_m32p, 16x16x32 consumers, several K-chunks, two Cout blocks
    (256, 48, 3, 1, 20, False, False, {}, r"mr=15 nr=\d nb16=[1-9] occ=3 "),  # conv_m32p, 48-row Cout blocks
    (192, 384, 3, 2, 24, False, False, {}, r"mr=3 nr=\d nb16=0 occ=3 "),   # conv_m32p stride 2 (Cin >= 192), 32x32x16 consumers
    (64, 64, 3, 1, 20, True, False, {"SCPOSE_M32_OCC": "2"}, r"mr=2 nr=\d nb16=0 occ=2 "),   # conv_m32 (single role), two workgroups per CU
    (64, 64, 3, 1, 20, True, False, {"SCPOSE_M32_OCC": "1"}, r"mr=2 nr=\d nb16=0 occ=1 "),   # conv_m32, one per CU: items of three tiles span frames
    (48, 48, 3, 1, 20, True, False, {}, None),     # conv_pipe 3x3 with residual
    (128, 384, 1, 1, 12, False, False, {}, None),  # conv_pipe 1x1 blocked (CASES: packed weights too large for the streaming kernel's variants)
    (48, 96, 3, 2, 24, False, False, {}, None),    # conv_s2r
    (96, 192, 3, 2, 24, False, False, {}, None),   # conv_s2r12
    (64, 256, 1, 1, 24, True, False, {}, None),    # streaming 1x1 with residual
    (48, 11, 1, 1, 24, False, True, {}, None),     # conv_pipe 1x1, float32 NCHW output, Cout = 11
]

RANGE_SPLIT_CODE = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, scpose
from importlib import import_module
ops = import_module('spacecraft-pose-estimation_amd.ops')
out = {}
for cin, cout, k, s, H, use_res, f32 in %(cases)r:
    for dtype in ('bf16', 'f16'):
        g = torch.Generator().manual_seed(cin + cout + H)
        conv = ops.Conv(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, torch.randn(cout, generator=g) * 0.1, stride=s, dtype=dtype)
        x = ops.to_blocked(torch.randn(5, cin, H, H - 3, generator=g).cuda(), dtype)
        Ho, Wo = (H - 1) // s + 1, (H - 4) // s + 1
        r = ops.to_blocked(torch.randn(5, cout, Ho, Wo, generator=g).cuda(), dtype) if use_res else None
        y = conv(x, out_nchw_f32=True) if f32 else ops.from_blocked(conv(x, residual=r, relu=True))
        out['c%%d-%%d_k%%d_s%%d_%%s' %% (cin, cout, k, s, dtype)] = y.float().cpu().numpy()
np.savez(%(dst)r, **out)
"""


def test_conv_frame_range_split(gpu_ops, tmp_path):
    """Every kernel under conv_launch addresses its tensors through 32-bit buffer descriptors; a batch whose tensor reaches 4 GiB
    runs as several launches over frame ranges, `in`, `res` and `out` advanced by their frame sizes, and inside a range the
    route is the one every smaller batch takes.  The development switch SCPOSE_MAXN forces that split on five frames (ranges of
    2, 2 and 1): same bits as one launch, for one layer per kernel family and both storage types (sub-processes: switches are
    read once per process; one pair per set of tile-search switches, all started together).  The tile choice every conv_m32 /
    conv_m32p launch prints names the family the row is there for.  Then the parity and equivariance cases of this file run
    under the switch as well."""
    import os
    import re
    import subprocess
    import sys
    import numpy as np
    from importlib import import_module
    nat = import_module("spacecraft-pose-estimation_amd._native")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SCPOSE_")}
    dev = {"SCPOSE_DEV": "1", "SCPOSE_LIB": nat.LIB_PATH, "SCPOSE_DBG": "32"}   # SCPOSE_DBG=32: every frame range and tile choice is printed

    def start(tag, cases, extra_env):
        dst = str(tmp_path / (tag + ".npz"))
        code = RANGE_SPLIT_CODE % dict(root=root, cases=[c[:7] for c in cases], dst=dst)
        return dst, subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                                     env=dict(clean, **extra_env), cwd=root)

    def finish(dst, proc):
        err = proc.communicate(timeout=900)[1]
        assert proc.returncode == 0, err[-3000:]
        return np.load(dst), err.splitlines()

    groups = {}   # tile-search switches -> the rows that run under them
    for case in RANGE_SPLIT:
        groups.setdefault(tuple(sorted(case[7].items())), []).append(case)
    started = [(cases, start("whole%d" % i, cases, dict(dev, **dict(sw)) if sw else {}),
                start("split%d" % i, cases, dict(dev, SCPOSE_MAXN="2", **dict(sw)))) for i, (sw, cases) in enumerate(groups.items())]
    for cases, whole_run, split_run in started:
        whole, whole_err = finish(*whole_run)
        split, split_err = finish(*split_run)
        # the switch did switch: three launches per case, over frames 0..2, 2..4 and 4..5
        ranges = [ln for ln in split_err if ln.startswith("conv ")]
        assert ranges == ["conv %d->%d k%d s%d %dx%d N=5: frames %s" % (cin, cout, k, s, H, H - 3, fr)
                          for cin, cout, k, s, H in (c[:5] for c in cases) for _ in ("bf16", "f16") for fr in ("0..2", "2..4", "4..5")], ranges
        # the kernel family of every launch: whole run (where it printed) and each range of the split run
        for cin, cout, k, s, H, _, _, sw, family in cases:
            for err, batches in ((whole_err, [5] if sw else []), (split_err, [2, 2, 1])):
                lines = [ln for ln in err if ln.startswith("m32 %d->%d " % (cin, cout))]
                assert [ln.split(":")[0].split()[-1] for ln in lines] == ["N=%d" % n for n in batches * 2 if family], lines
                assert all(re.search(family, ln) for ln in lines), (family, lines)
        assert len(whole.files) == 2 * len(cases)
        for key in whole.files:
            a, b = torch.from_numpy(whole[key]), torch.from_numpy(split[key])
            assert a.shape[0] == 5 and torch.isfinite(a).all() and a.abs().max() > 0, key
            assert torch.equal(a, b), "%s: %d of %d elements differ" % (key, int((a != b).sum()), a.numel())
    # parity with the CPU and frame-permutation equivariance on the split path
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_conv.py"), "-q", "-x", "-m", "gpu",
                        "-k", "(test_conv_matches_cpu and bf16) or equivariant"],
                       capture_output=True, text=True, env=dict(clean, SCPOSE_DEV="1", SCPOSE_MAXN="2", SCPOSE_LIB=nat.LIB_PATH), cwd=root, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout


@pytest.mark.parametrize("shape", [(32, 400, 1, 64, 24), (64, 256, 1, 96, 32), (96, 48, 1, 48, 64), (128, 64, 1, 32, 64),
                                   (192, 96, 1, 24, 64), (256, 64, 1, 96, 32), (384, 48, 1, 12, 64), (96, 96, 3, 48, 64)],
                         ids=lambda s: "c%d-%d_k%d_%d_n%d" % s)
def test_conv_is_run_to_run_deterministic(gpu_ops, shape):
    """Four launches on the same input give the same bits (every 1x1 variant -- streaming kernel for Cin <= 128, conv_pipe
    above -- and one 3x3 layer): no kernel depends on scheduling order or on uninitialised state."""
    cin, cout, k, H, N = shape
    g = torch.Generator().manual_seed(cin * 7 + cout)
    conv = gpu_ops.Conv(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, torch.randn(cout, generator=g) * 0.1)
    x = torch.randn(N, cin // 8, H, H, 8, generator=g).bfloat16().cuda()
    ys = [conv(x, relu=True) for _ in range(4)]
    assert all(torch.equal(y, ys[0]) for y in ys[1:])
