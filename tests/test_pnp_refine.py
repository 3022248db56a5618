"""Levenberg-Marquardt pose refinement (scpose_pnp_epnp_ransac_refine, csrc/pnp.hip lm_refine): the parts that need no device.

  * the entry point is declared, bound and exported, and rejects bad arguments before touching a device;
  * the NumPy restatement of the kernel's algorithm (tests/pnp_lm_restated.py) reaches the least-squares minimum SciPy finds
    (tests/pnp_independent.py) and never raises the cost -- so the GPU tests that pin the kernel to the restatement
    (tests/test_gpu_pnp_refine.py) pin it to that minimum as well;
  * the CLIs expose --pnp_refine as an optional extension whose default keeps the reference's poses.
"""
import argparse
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle import pnp_ref as P
import pnp_independent as I
import pnp_lm_restated as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat(scpose):
    from importlib import import_module
    n = import_module("spacecraft-pose-estimation_amd._native")
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return n


def rot_dist(Ra, Rb):
    """Geodesic angle through the quaternion of Ra^T Rb: resolves 1e-12 rad, where arccos of the trace stops at ~1e-8."""
    return float(Rotation.from_matrix(Ra.T @ Rb).magnitude())


def test_refine_entry_is_declared_bound_and_exported(nat):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scpose.h")).read(), flags=re.S)
    assert re.search(r"\bscpose_pnp_epnp_ransac_refine\s*\(", text)
    assert "scpose_pnp_epnp_ransac_refine" in nat.SYMBOLS
    assert hasattr(nat.lib(), "scpose_pnp_epnp_ransac_refine")
    assert nat.ABI_VERSION == 7 and nat.lib().scpose_abi_version() == 7


def _call(nat, n=0, refine_iters=0, arrays=True, rows=False, j=11):
    buf = (ctypes.c_double * 16)()
    ist = (ctypes.c_int32 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rot = tv = st = None
    if arrays:
        rot, tv, st = p, p, ctypes.cast(ist, ctypes.c_void_p)
    return nat.lib().scpose_pnp_epnp_ransac_refine(None, None, None, None, n, j, 0.95, 15, 0.8, 100, 10000, 15.0, 0.99,
                                                     refine_iters, rot, tv, None, st, p if rows else None, None, None)


@pytest.mark.parametrize("iters", [-1, 101])
def test_refine_iters_out_of_range_is_an_error_without_a_device(nat, iters):
    assert _call(nat, refine_iters=iters) == -1
    assert b"refine_iters" in nat.lib().scpose_last_error()


def test_refine_needs_exactly_one_output_form(nat):
    assert _call(nat, arrays=True, rows=True) == -1
    assert b"output form" in nat.lib().scpose_last_error()
    assert _call(nat, arrays=False, rows=False) == -1
    assert _call(nat, arrays=True, rows=False, refine_iters=100) == 0      # an empty batch with valid arguments is a no-op
    assert _call(nat, arrays=False, rows=True, refine_iters=0) == 0


def _frames(n, seed, noise, outliers=0.0):
    rng = np.random.default_rng(seed)
    kp, Rs, ts = P.synth_keypoints(n, rng, noise, outliers)
    return kp, Rs, ts, rng


@pytest.mark.parametrize("npts", [11, 6, 4])
def test_restatement_reaches_the_scipy_minimum_and_never_raises_the_cost(npts):
    """Run to its fixed point (eps = 0, 100 iterations), the restatement sits on the least-squares minimum: SciPy's LM started
    there moves it by no more than 1e-8 (rad / relative; MINPACK's own last step: its xtol = 1e-12 stops one step short of where
    a further Newton step is below 1e-12, measured up to 4e-9 rad), and SciPy started where the restatement started lands on it
    to SciPy's own tolerance.  With the kernel's stop rule (FLT_EPSILON, 20 iterations) it stops within 1e-6 rad / 1e-7 relative of
    that minimum (the last step taken is <= FLT_EPSILON |p|), at a cost within 1e-9 (relative) of SciPy's.  The cost never rises."""
    kp, Rs, ts, rng = _frames(24, 7 + npts, 1.0)
    X = P.LANDMARKS[:npts]
    X32 = X.astype(np.float32).astype(np.float64)
    worst = {"fixed_r": 0.0, "fixed_t": 0.0, "scipy_r": 0.0, "stop_r": 0.0, "stop_t": 0.0}
    for i in range(len(kp)):
        uv = kp[i, :npts, :2].astype(np.float32).astype(np.float64)
        # start away from the optimum, like an algebraic solution: 5 mrad and 1 % of the distance
        r0 = Rotation.from_matrix(Rs[i]).as_rotvec() + rng.normal(0, 5e-3, 3)
        t0 = ts[i] * (1 + rng.normal(0, 1e-2, 3))
        trace = []
        r, t = L.refine(r0, t0, X, uv, P.CAMERA_K, P.CAMERA_DIST, iters=100, trace=trace, eps=0)
        c0 = L.cost(np.concatenate([r0, t0]), X32, uv, P.CAMERA_K, P.CAMERA_DIST)
        assert all(b <= a for a, b in zip([c0] + trace, trace)), "the cost rose: %s" % trace
        R = L.rodrigues(r)
        Rf, tf = I.refine(R, t, X32, uv, P.CAMERA_K, P.CAMERA_DIST)            # SciPy from the restatement's answer
        worst["fixed_r"] = max(worst["fixed_r"], rot_dist(R, Rf))
        worst["fixed_t"] = max(worst["fixed_t"], np.linalg.norm(t - tf) / np.linalg.norm(tf))
        Rl, tl = I.refine(L.rodrigues(r0), t0, X32, uv, P.CAMERA_K, P.CAMERA_DIST)   # SciPy from the same start
        worst["scipy_r"] = max(worst["scipy_r"], rot_dist(R, Rl))
        trace = []
        rs, ts_ = L.refine(r0, t0, X, uv, P.CAMERA_K, P.CAMERA_DIST, iters=20, trace=trace)
        assert all(b <= a for a, b in zip([c0] + trace, trace)), "the cost rose: %s" % trace
        worst["stop_r"] = max(worst["stop_r"], rot_dist(L.rodrigues(rs), R))
        worst["stop_t"] = max(worst["stop_t"], np.linalg.norm(ts_ - t) / np.linalg.norm(t))
        assert L.cost(np.concatenate([rs, ts_]), X32, uv, P.CAMERA_K, P.CAMERA_DIST) <= \
            (1 + 1e-9) * I.rms(Rl, tl, X32, uv, P.CAMERA_K, P.CAMERA_DIST) ** 2 * npts
    print(npts, {k: "%.1e" % v for k, v in worst.items()})
    assert worst["fixed_r"] <= 1e-8 and worst["fixed_t"] <= 1e-8, worst
    assert worst["scipy_r"] <= 1e-6, worst
    assert worst["stop_r"] <= 1e-6 and worst["stop_t"] <= 1e-7, worst


def test_restatement_twenty_iterations_converge_from_the_epnp_pose():
    """The default budget (20, --pnp_refine lm) from the EPnP + RANSAC pose of the C oracle, on its inlier set."""
    kp, Rs, ts, _ = _frames(32, 3, 1.0, 0.1)
    o = P.solve_batch(kp)
    worst = 0.0
    for i in np.nonzero(o["status"] > 0)[0]:
        uv = kp[i, :, :2].astype(np.float64)
        m = I.inlier_mask(o["R"][i], o["t"][i], P.LANDMARKS, uv, P.CAMERA_K, P.CAMERA_DIST)
        r, t = L.refine(o["rvec"][i], o["t"][i], P.LANDMARKS[m], uv[m], P.CAMERA_K, P.CAMERA_DIST, iters=20)
        X32 = P.LANDMARKS[m].astype(np.float32).astype(np.float64)
        Rl, _ = I.refine(L.rodrigues(r), t, X32, uv[m], P.CAMERA_K, P.CAMERA_DIST)
        worst = max(worst, rot_dist(L.rodrigues(r), Rl))
        assert I.rms(L.rodrigues(r), t, X32, uv[m], P.CAMERA_K, P.CAMERA_DIST) <= \
            I.rms(o["R"][i], o["t"][i], X32, uv[m], P.CAMERA_K, P.CAMERA_DIST)
    assert worst <= 1e-6, worst


def _surface(path, monkeypatch):
    class Done(Exception):
        pass
    got = {}

    def parse(self, args=None, namespace=None):
        got["parser"] = self
        raise Done()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    spec = importlib.util.spec_from_file_location("cli_surface_" + os.path.basename(path).replace(".", "_"), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(Done):
        (mod.parse_args([]) if hasattr(mod, "parse_args") else mod.main())
    monkeypatch.undo()
    return {a.dest: a for a in got["parser"]._actions}


@pytest.mark.parametrize("path", ["pose_estimation/export_predicted_poses_real.py", "evaluate_pipeline.py"])
def test_clis_expose_pnp_refine(path, monkeypatch):
    acts = _surface(os.path.join(ROOT, path), monkeypatch)
    a = acts["pnp_refine"]
    assert a.option_strings == ["--pnp_refine"] and a.required is False and a.default == "none"
    assert tuple(a.choices) == ("none", "lm")
