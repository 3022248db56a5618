"""The device JPEG decoder (csrc/jpeg_decode.hip) on the streams of tests/jpeg_stream_families.py -- tables per component,
every output-kernel edge, chosen fill bits and subsequence boundaries, runs to index 63, the extremes of the format, both ends
of the range limiters, the relaxation's worst case and the luma output of the C ABI: ops.decode_jpeg == PIL bit for bit and
the rounds are the restatement's, round for round.  tests/test_jpeg_streams.py shows on the CPU that each family holds its case."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_decode_restated as R
import jpeg_stream_families as F

pytestmark = pytest.mark.gpu
J = R.J


def decode_and_compare(gpu_ops, cases, rgb=True, **kw):
    """one call for files of one geometry -> info; every frame equals PIL, every round count the restatement's"""
    assert len({c.geometry for c in cases}) == 1
    got, info = gpu_ops.decode_jpeg([c.data for c in cases], rgb=rgb, fallback=False, **kw)
    got = got.cpu().numpy()
    bad = [c.name for i, c in enumerate(cases) if not np.array_equal(got[i], c.pil if rgb else c.pil[:, :, ::-1])]
    assert not bad, bad
    assert not info["fallback"]
    assert info["rounds"] == [c.relaxed[1] for c in cases], [c.name for c in cases]
    return info


def by_geometry(cases):
    groups = {}
    for c in cases:
        groups.setdefault(c.geometry, []).append(c)
    return list(groups.values())


def test_a_tables_per_component(gpu_ops):
    """three quantisation, three DC and three AC tables under ids 2, 0, 3; PIL's shared-chroma files ride in the same launch"""
    for group in by_geometry(F.family_a()):
        h, w, mode = group[0].geometry
        assert len(group) == 3
        pil = [F.Case("pil-%d" % q, R.fixture(mode, h, w, q, "noise", seed=q, **kw)) for q, kw in ((30, {}), (95, dict(restart_marker_blocks=1)))]
        decode_and_compare(gpu_ops, [group[0], pil[0], group[1], pil[1], group[2]])
        decode_and_compare(gpu_ops, group, rgb=False)


@pytest.mark.parametrize("mode", ("gray", "444", "420"))
def test_b_geometry(gpu_ops, mode):
    """chroma planes 1, 2 and 3 samples wide and 1 and 2 high, widths over 256 and 512, quads and single stores"""
    groups = by_geometry(F.family_b(mode))
    assert len(groups) == len(F.B_SIZES)
    for group in groups:
        assert len(group) == 4 and sum(c.written is None for c in group) == 1          # three hand-made files and PIL's
        for rgb in (True, False):
            decode_and_compare(gpu_ops, group, rgb=rgb)


@pytest.mark.parametrize("family", ("c", "d", "e", "f"))
def test_segment_ends_boundaries_runs_and_saturation(gpu_ops, family):
    for group in by_geometry(getattr(F, "family_" + family)()):
        decode_and_compare(gpu_ops, group)


def test_g_relaxation_worst_case(gpu_ops):
    worst, easy, wide = F.family_g()
    rounds = worst.relaxed[1]
    assert gpu_ops.JPEG_MAX_ROUNDS == R.DEFAULT_MAX_ROUNDS < rounds <= 250 and easy.relaxed[1] == 1
    files = [easy.data, worst.data]
    # the default cap: a status bit, PIL's pixels with the fallback, an error without it; the one-round neighbour is untouched
    got, info = gpu_ops.decode_jpeg(files)
    assert list(info["fallback"]) == [1] and "not converged" in info["fallback"][1]
    assert info["rounds"] == [1, R.DEFAULT_MAX_ROUNDS]
    assert np.array_equal(got[0].cpu().numpy(), easy.pil) and np.array_equal(got[1].cpu().numpy(), worst.pil)
    with pytest.raises(J.JpegError, match="not converged"):
        gpu_ops.decode_jpeg(files, fallback=False)
    # the cap raised: the device decodes it, in as many rounds as the file has subsequences
    info = decode_and_compare(gpu_ops, [easy, worst], max_rounds=250)
    assert info["rounds"] == [1, worst.stream.h.nsub]
    # restart segments on both sides of subsequence 256 and one across it: the segment search over a workgroup edge
    assert wide.stream.h.nsub > 256
    decode_and_compare(gpu_ops, [wide])


def abi_decode(gpu_ops, cases, bgr, with_y):
    """scpose_jpeg_decode with guard bytes after out, y_out and the workspace -> (out, y_out or None) as NumPy"""
    nat, dev = gpu_ops.nat, torch.device("cuda", torch.cuda.current_device())
    h, w, mode = cases[0].geometry
    n = len(cases)
    desc, rows, blob, max_subs = J.pack_batch([c.stream.h for c in cases], [c.data for c in cases])
    ws = ctypes.c_size_t()
    nat.check(nat.lib().scpose_jpeg_decode_workspace_bytes(n, h, w, J.MODES[mode], max_subs, ctypes.byref(ws)))
    guard = 256
    out = torch.full((n * h * w * 3 + guard,), 0xA5, dtype=torch.uint8, device=dev)
    y = torch.full((n * h * w + guard,), 0xC3, dtype=torch.uint8, device=dev)
    work = torch.full((ws.value + guard,), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_desc, d_rows, d_blob = (torch.from_numpy(a).to(dev) for a in (desc, rows, blob))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    nat.check(nat.lib().scpose_jpeg_decode(P(d_desc), P(d_rows), rows.shape[0], P(d_blob), blob.size, n, h, w, J.MODES[mode], max_subs,
                                           bgr, gpu_ops.JPEG_MAX_ROUNDS, P(out), P(y) if with_y else None, P(status), P(work), ws.value,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert all(s & 3 == 0 for s in status.tolist())
    assert bool((out[n * h * w * 3:] == 0xA5).all()) and bool((work[ws.value:] == 0x5A).all())
    if not with_y:
        assert bool((y == 0xC3).all())
    assert bool((y[n * h * w:] == 0xC3).all())
    return out[:n * h * w * 3].cpu().numpy().reshape(n, h, w, 3), y[:n * h * w].cpu().numpy().reshape(n, h, w) if with_y else None


@pytest.mark.parametrize("mode", ("gray", "444", "420"))
def test_h_luma_output_of_the_c_abi(gpu_ops, mode):
    """y_out: the luma plane cropped to H x W, by the quad stores (width 260) and the single stores (width 261, 31)"""
    groups = {g[0].geometry[:2]: g for g in by_geometry(F.family_b(mode))}
    for size in ((4, 260), (5, 261), (33, 31)):
        cases = groups[size][1:3] + groups[size][3:]                                   # restart intervals 1 and 3, and PIL's file
        assert len(cases) == 3
        for bgr in (0, 1):
            plain, _ = abi_decode(gpu_ops, cases, bgr, False)
            out, y = abi_decode(gpu_ops, cases, bgr, True)
            assert np.array_equal(out, plain)                                          # passing y_out changes nothing in out
            for i, c in enumerate(cases):
                assert np.array_equal(out[i], c.pil[:, :, ::-1] if bgr else c.pil), (c.name, bgr)
                luma = R.planes(c.stream, c.sequential[0])[0][:size[0], :size[1]]
                assert np.array_equal(y[i], luma), (c.name, bgr)
                if mode == "gray":
                    assert np.array_equal(y[i], out[i][:, :, 0])
