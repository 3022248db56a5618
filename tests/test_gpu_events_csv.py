"""events.csv parsed on the device (csrc/events_csv.hip) against tests/events_csv_restated.py and against the parent reader,
event_render.read_events_csv (the reference's pandas.read_csv call): element for element and in dtype on the grammar table and
the seeded corpora, the unsupported status on every rejected row, 3 M-event files in both styles, determinism, tile edges, the
two CLIs with and without --host_csv, the pandas fallback, and the chain file bytes -> poses."""
import ctypes
import filecmp
import io
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import events_csv_restated as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TILE = 4096                       # csrc/events_csv.hip: bytes per workgroup; 256 more are kept in LDS after it
DTYPES = [torch.int64, torch.int32, torch.int32, torch.int8]


@pytest.fixture(scope="module")
def er(scpose):
    from importlib import import_module
    return import_module("spacecraft-pose-estimation_amd.event_render")


def _oracle(er, data, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return er.read_events_csv(io.BytesIO(data), **kw)


def _check(gpu_ops, er, data, oracle=True, **kw):
    """device == restatement (== parent reader), element for element and in dtype; returns the device columns"""
    got = gpu_ops.parse_events_csv(data, **kw)
    assert [a.dtype for a in got] == DTYPES and all(a.is_cuda and a.dim() == 1 for a in got)
    want = R.parse(data, **kw)
    assert not isinstance(want, str), "the restatement answered %r" % (want,)
    for a, b in zip(got, want):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    if oracle:
        for a, b in zip(got, _oracle(er, data, **kw)):
            a = a.cpu().numpy()
            assert a.shape == b.shape and np.array_equal(a.astype(np.int64), b)
    return got


@pytest.mark.parametrize("name,data,ws", R.ACCEPTED, ids=[c[0] for c in R.ACCEPTED])
def test_accepted_rows(gpu_ops, er, name, data, ws):
    for flags in ({}, {"swap_xy": True}, {"microseconds_timestamp": True}, {"swap_xy": True, "milliseconds_timestamp": True}):
        _check(gpu_ops, er, data, delim_whitespace=ws, **flags)


@pytest.mark.parametrize("name,data,ws", R.REJECTED, ids=[c[0] for c in R.REJECTED])
def test_rejected_rows_raise_unsupported(gpu_ops, name, data, ws):
    with pytest.raises(gpu_ops.UnsupportedCsv):
        gpu_ops.parse_events_csv(data, delim_whitespace=ws)
    good = R.corpus_white(1, 500) if ws else R.corpus_comma(1, 500)          # the bad line deep inside a good file
    with pytest.raises(gpu_ops.UnsupportedCsv):
        gpu_ops.parse_events_csv(good + data + good, delim_whitespace=ws, swap_xy=True)


@pytest.mark.parametrize("style,flags", [("comma", {}), ("comma", {"milliseconds_timestamp": True}),
                                         ("white", {"swap_xy": True}),
                                         ("white", {"swap_xy": True, "microseconds_timestamp": True})])
def test_seeded_corpus(gpu_ops, er, style, flags):
    """the corpora of tests/test_events_csv.py: accepted grammar only, so UnsupportedCsv here is a failure"""
    gen = R.corpus_comma if style == "comma" else R.corpus_white
    data = gen(20261016, 200000, final_line_end=False)
    got = _check(gpu_ops, er, data, delim_whitespace=style == "white", **flags)
    assert got[0].numel() == 200000


@pytest.mark.parametrize("style", ["comma", "white"])
def test_three_million_events_twice(gpu_ops, er, style):
    ws = style == "white"
    data = (R.corpus_white if ws else R.corpus_comma)(3, 3000000, padding=False)
    flags = {"delim_whitespace": ws, "swap_xy": ws}
    a = gpu_ops.parse_events_csv(data, **flags)
    b = gpu_ops.parse_events_csv(data, **flags)
    assert a[0].numel() == 3000000
    assert all(torch.equal(u, v) for u, v in zip(a, b))                       # two runs are bitwise equal
    for u, v in zip(a, _oracle(er, data, **flags)):
        u = u.cpu().numpy()
        assert u.shape == v.shape and np.array_equal(u.astype(np.int64), v)
    want = R.parse(data, **flags)
    for u, v in zip(a, want):
        u = u.cpu().numpy()
        assert u.dtype == v.dtype and np.array_equal(u, v)


def test_deterministic_on_the_padded_corpus(gpu_ops):
    data = R.corpus_comma(9, 300000)
    dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    a = gpu_ops.parse_events_csv(dev)
    b = gpu_ops.parse_events_csv(dev)
    c = gpu_ops.parse_events_csv(data)
    assert all(torch.equal(u, v) and torch.equal(u, w) for u, v, w in zip(a, b, c))
    # a view that does not start on a 16-byte boundary
    shifted = torch.cat([torch.zeros(3, dtype=torch.uint8, device="cuda"), dev])[3:]
    d = gpu_ops.parse_events_csv(shifted)
    assert all(torch.equal(u, v) for u, v in zip(a, d))


def test_tile_edges(gpu_ops, er):
    row = b"1234567,101,202,1\n"
    n = len(row)
    # a line straddles every tile edge (18 does not divide 4096), the size is not a multiple of the tile, no final line end
    data = (row * 1000)[:-1]
    assert len(data) % TILE != 0 and TILE % n != 0
    got = _check(gpu_ops, er, data)
    assert got[0].numel() == 1000
    # a line end as the last byte of a tile, as the first byte of the next one, '\r' | '\n' split by the edge
    for pad in (TILE - 1, TILE, TILE + 1):                                    # the line end starts at byte pad - 1
        head = b"#" + b"c" * (pad - n - 2) + b"\n"
        assert len(head) + n - 1 == pad - 1
        for end in (b"\n", b"\r\n", b"\r"):
            data = head + row[:-1] + end + row * 3
            _check(gpu_ops, er, data)
    # exactly one tile, one tile and one byte, and a digit run across the edge in whitespace mode
    for size in (TILE, TILE + 1, 2 * TILE, 2 * TILE - 1):
        body = row * (size // n)
        data = body + b"#" + b"x" * (size - len(body) - 1)
        assert len(data) == size
        _check(gpu_ops, er, data)
    data = b"0.000001 5 6 1\n" * 3000
    _check(gpu_ops, er, data, delim_whitespace=True)
    # a line longer than tile + halo: blanks and a comment of 6000 bytes after a row, then rows
    data = row[:-1] + b" " * 3000 + b"# " + b"z" * 6000 + b"\n" + row * 5
    _check(gpu_ops, er, data)
    # a field longer than the halo is parsed from global memory (an integer column: any length of zeros is the same number)
    data = b"0" * 5000 + b"7,1,2,1\n" + row * 300
    _check(gpu_ops, er, data)
    # a rejected line that straddles the edge
    with pytest.raises(gpu_ops.UnsupportedCsv):
        gpu_ops.parse_events_csv(row * 227 + b"12,3e4,5,1\n" + row * 300)


def test_tiny_files(gpu_ops, er):
    for data in (b"", b"\n", b"#", b" ", b"\r"):
        got = _check(gpu_ops, er, data)
        assert got[0].numel() == 0
    with pytest.raises(gpu_ops.UnsupportedCsv):
        gpu_ops.parse_events_csv(b"1")
    got = _check(gpu_ops, er, b"1,2,3,4")
    assert [int(v[0]) for v in got] == [1, 2, 3, 4]
    got = _check(gpu_ops, er, b"1 2 3 4", delim_whitespace=True, swap_xy=True)
    assert [int(v[0]) for v in got] == [1, 3, 2, 4]


def test_path_and_device_inputs(gpu_ops, er, tmp_path):
    data = R.corpus_white(4, 5000)
    path = tmp_path / "events.csv"
    path.write_bytes(data)
    a = gpu_ops.parse_events_csv(str(path), delim_whitespace=True, swap_xy=True)
    b = _check(gpu_ops, er, data, delim_whitespace=True, swap_xy=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    with pytest.raises(ValueError):
        gpu_ops.parse_events_csv(torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(gpu_ops.nat.NativeError):
        gpu_ops.parse_events_csv(torch.zeros(4, dtype=torch.uint8))


def test_c_abi_directly(gpu_ops, er):
    """through ctypes: caller-owned buffers, the capacity status, the unsupported status, exact row count"""
    nat = gpu_ops.nat; lib = nat.lib()
    data = R.corpus_comma(12, 20000)
    want = R.parse(data, milliseconds_timestamp=True)
    buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    n = buf.numel()
    ws = ctypes.c_size_t()
    nat.check(lib.scpose_events_csv_workspace_bytes(n, ctypes.byref(ws)))
    work = torch.empty(ws.value, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda v: ctypes.c_void_p(v.data_ptr())

    def run(src, nbytes, cap, t_div=0.0):
        cols = [torch.full((cap + 8,), -7, dtype=d, device="cuda") for d in DTYPES]
        cs = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        nat.check(lib.scpose_events_csv_parse(P(src), nbytes, 0, 0, t_div, P(cols[0]), P(cols[1]), P(cols[2]), P(cols[3]), cap, P(cs),
                                              P(work), ws.value, st))
        return cols, cs.tolist()

    cols, (rows, status) = run(buf, n, 20000, 1000.0)
    assert (rows, status) == (20000, 0)
    for c, w in zip(cols, want):
        assert np.array_equal(c[:rows].cpu().numpy(), w)
        assert (c[rows:] == -7).all()                                         # nothing is written past the rows
    cols, (rows, status) = run(buf, n, 19999)
    assert (rows, status) == (0, nat.CSV_CAPACITY) and all((c[19999:] == -7).all() for c in cols)
    bad = torch.from_numpy(np.frombuffer(data + b"1,2,3\n", np.uint8).copy()).cuda()
    nat.check(lib.scpose_events_csv_workspace_bytes(bad.numel(), ctypes.byref(ws)))
    work = torch.empty(ws.value, dtype=torch.uint8, device="cuda")
    _, (rows, status) = run(bad, bad.numel(), 20001)
    assert (rows, status) == (0, nat.CSV_UNSUPPORTED)
    _, (rows, status) = run(buf, 0, 0)
    assert (rows, status) == (0, 0)


def _scene_files(folder):
    out = {}
    for dp, _, files in os.walk(str(folder)):
        for f in files:
            if not f.endswith(".csv"):
                out[os.path.relpath(os.path.join(dp, f), str(folder))] = os.path.join(dp, f)
    return out


def _same_trees(a, b):
    fa, fb = _scene_files(a), _scene_files(b)
    assert sorted(fa) == sorted(fb) and len(fa) > 2
    for k in fa:
        assert filecmp.cmp(fa[k], fb[k], shallow=False), k


def _events_text(rng, n, h, w, exponent=False):
    t = np.sort(rng.integers(1000000, 1000000 + 165000, n)); x = rng.integers(-4, w + 4, n); y = rng.integers(-4, h + 4, n)
    p = rng.integers(0, 2, n)
    lines = [b"%d,%d,%d,%d\n" % (t[i], x[i], y[i], p[i]) for i in range(n)]
    if exponent:
        lines[n // 2] = b"%d,%de0,%d,%d\n" % (t[n // 2], x[n // 2], y[n // 2], p[n // 2])     # same value, outside the device grammar
    return b"# t,x,y,p\n" + b"".join(lines)


@pytest.mark.parametrize("exponent", [False, True], ids=["device", "fallback"])
def test_convert_aedats_with_and_without_host_csv(gpu_ops, tmp_path, exponent):
    h, w = 120, 160
    text = _events_text(np.random.default_rng(21), 60000, h, w, exponent)
    if exponent:
        with pytest.raises(gpu_ops.UnsupportedCsv):
            gpu_ops.parse_events_csv(text)
    else:
        assert gpu_ops.parse_events_csv(text)[0].numel() == 60000           # the device parser takes this text: no fallback below
    from importlib import import_module
    syn = import_module("spacecraft-pose-estimation_amd.synthetic")
    K = syn.SPEEDPLUS_K.copy(); K[0] *= w / 1920.0; K[1] *= h / 1200.0
    calib = tmp_path / "calibration.json"
    calib.write_text(json.dumps({"intrinsics": {"camera_matrix": K.tolist(), "distortion_coefficients": syn.SPEEDPLUS_DIST.tolist()}}))
    for tag, extra in (("dev", []), ("host", ["--host_csv"])):
        scene = tmp_path / tag / "scene0"
        scene.mkdir(parents=True)
        (scene / "events.csv").write_bytes(text)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "v2e", "convert_aedats.py"), "--scenes_dir", str(tmp_path / tag),
                            "--calibration_file_path", str(calib), "--image_width", str(w), "--image_height", str(h)] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "scene0: 16 frames" in r.stdout
    _same_trees(tmp_path / "dev", tmp_path / "host")


@pytest.mark.parametrize("exponent", [False, True], ids=["device", "fallback"])
def test_e2v_with_and_without_host_csv(gpu_ops, tmp_path, exponent):
    h, w = 120, 160
    text = _events_text(np.random.default_rng(22), 60000, h, w, exponent)
    if exponent:
        with pytest.raises(gpu_ops.UnsupportedCsv):
            gpu_ops.parse_events_csv(text)
    else:
        assert gpu_ops.parse_events_csv(text)[0].numel() == 60000           # the device parser takes this text: no fallback below
    src = tmp_path / "events.csv"
    src.write_bytes(text)
    for tag, extra in (("dev", []), ("host", ["--host_csv"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(ROOT, "v2e", "e2v.py"), "--events_file", str(src), "--output_folder", str(out),
                            "--output_width", str(w), "--output_height", str(h), "--dvs_exposure", "duration", "10000"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "e2v: 16 frames" in r.stdout
    _same_trees(tmp_path / "dev", tmp_path / "host")
    assert any(k.endswith("-frame_times.txt") for k in _scene_files(tmp_path / "dev"))


def test_bytes_to_poses_equals_the_host_parsed_chain(gpu_ops, er, scpose):
    """file bytes -> parse_events_csv -> render_events -> crop_warp -> forward -> decode -> PnP == the same chain started from
    the arrays the parent reader gives, exactly"""
    from importlib import import_module
    syn = import_module("spacecraft-pose-estimation_amd.synthetic")
    tr = import_module("spacecraft-pose-estimation_amd.utils.transforms")
    h, w = 120, 160
    rng = np.random.default_rng(3)
    n = 40000
    t = np.sort(rng.integers(0, 85000, n)); x = rng.integers(0, w, n); y = rng.integers(0, h, n); p = rng.integers(0, 2, n)
    text = b"".join(b"%d, %d, %d, %d\r\n" % (t[i], x[i], y[i], p[i]) for i in range(n))
    K = syn.SPEEDPLUS_K.copy(); K[0] *= w / 1920.0; K[1] *= h / 1200.0
    dist = syn.SPEEDPLUS_DIST.copy()
    cfg = syn.hrnet_cfg(16, 11, 64, modules=(1, 1, 1))
    eng = gpu_ops.HrnetEngine(cfg, syn.random_checkpoint(cfg, seed=0), dtype="bf16", device="cuda:0")

    def chain(td, xd, yd):
        d, names = gpu_ops.render_events(td, xd, yd, None, (h, w), K=K, dist=dist)
        nf = len(names)
        c = np.tile(np.array([[w / 2.0, h / 2.0]], np.float32), (nf, 1)); s = np.full((nf, 2), 0.5, np.float32)
        trans = np.stack([tr.get_affine_transform(c[i], s[i], 0, (64, 64)) for i in range(nf)])
        crops = gpu_ops.crop_warp(d, trans, (64, 64))
        kp = eng.forward_decode(crops, torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda(), True)
        rot, tv, st = gpu_ops.pnp_epnp_ransac(kp, torch.from_numpy(syn.TANGO_LANDMARKS).cuda(), torch.from_numpy(K).cuda(),
                                              torch.from_numpy(dist).cuda())
        return names, kp.clone(), rot.clone(), tv.clone(), st.clone()

    td, xd, yd, _ = gpu_ops.parse_events_csv(torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda())
    ht, hx, hy, _ = _oracle(er, text)
    a = chain(td, xd, yd)
    b = chain(torch.from_numpy(ht).cuda(), torch.from_numpy(hx.astype(np.int32)).cuda(), torch.from_numpy(hy.astype(np.int32)).cuda())
    eng.close()
    assert a[0] == b[0] and len(a[0]) == 8
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)
    assert torch.isfinite(a[1]).all()
