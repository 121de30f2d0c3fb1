"""Optimizer::OptimizeSim3 on the device (orbx_optimize_sim3, csrc/orbx_optimize_sim3.hip) against tests/optsim3_ref.py, the numpy float64
restatement of reference src/Optimizer.cc:1364-1590 and the vendored g2o.  No C entry point of the compiled reference reaches OptimizeSim3, so
the restatement is tied down on the CPU by the scenes' ground truth, by an independent scipy solve and by the reference's Sim3::log(); every
stage of the device is then checked against the restatement fed with the device's OWN upstream outputs."""
import ctypes
import functools
import math
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import optsim3_ref as osr
import sim3_ref as sr
from test_initializer import REF, ROOT

ERR_ARG, ERR_CAPACITY, ERR_NODEVICE, ERR_STATE = -1, -3, -4, -5
F32, F64 = np.float32, np.float64
TH2 = 10.0                  # LoopClosing::ComputeSim3 calls OptimizeSim3(..., 10, mbFixScale)
NEAR = 1e-6                 # pairs with a tested chi2 within this relative distance of th2 are left out of the classification checks
EXCLUDED_CAP = 0.05
PERTURBATIONS = 6

# What moving every camera-point coordinate by ONE double ulp (up or down, at random; PERTURBATIONS draws per scene and estimate) does to one restated
# linearisation, the largest over the scenes, at the input estimate and at the restatement's final one: errors in pixels; chi2 relative to
# max(1, chi2); the Jacobian relative to its largest entry (g2o's central differences magnify a change of a few ulps of an error by 1 / (2e-9):
# this is the reference's own noise); H relative to its largest entry; b[i] relative to sqrt(H[i][i]) + 1.  The device is held to 4 times these.
# test_bounds_are_the_measured_ones recomputes them.
LIN_MEASURED = dict(errors=2.27e-13, chi2=2.11e-13, jac=2.46e-7, H=6.21e-8, b=7.60e-6)
LIN_BOUND = {k: 4 * v for k, v in LIN_MEASURED.items()}
# The same perturbations through the whole restated optimisation: the largest change of quat (up to sign), t and s over the scenes, and 4 times it.
E2E_MEASURED = 3.30e-8
E2E_BOUND = 4 * E2E_MEASURED

K2_OTHER = (435.2, 435.2, 320.5, 241.0)
# (name, pairs, fix_scale, kind, make_scene arguments); the seeds are in SEEDS.  Pairs 0 (nothing to do), 9 (below the floor: round one runs, return 0), 10 without
# outliers (the floor, accepted), 12 with outliers (below 10 after the removal: return 0 with removed_first set), 63 / 64 / 65 (the wave edge),
# 256 / 257 (a thread's second pair), 300 (several waves), each with and without fix_scale; K1 != K2; no outliers (nBad == 0: round two has 5
# iterations); noise-free (a round ends in Terminate: rho == 0 or ten trials); a tenth of the points behind camera 2.
# Seeds: the first for which the restatement alone meets _screen (test_seeds_are_the_first_screened).
_COUNTS = ((0, "zero", {}), (9, "zero", {}), (10, "floor", {}), (12, "zero_removed", dict(outliers=0.3)), (63, "outliers", dict(outliers=0.1)),
           (64, "outliers", dict(outliers=0.1)), (65, "outliers", dict(outliers=0.1)), (256, "outliers", dict(outliers=0.1)), (257, "outliers", dict(outliers=0.1)),
           (300, "outliers", dict(outliers=0.1)))
SCENES = [("%s_%d" % ("fix" if fs else "free", n), n, fs, kind, kw) for n, kind, kw in _COUNTS for fs in (False, True)] + [
    ("k2_100", 100, False, "outliers", dict(outliers=0.1, k2=K2_OTHER)),
    ("clean_100", 100, False, "clean", {}),
    ("noisefree_50", 50, False, "terminate", dict(noise=0.0)),
    ("behind_100", 100, False, "behind", dict(outliers=0.1, behind=0.1)),
]
NAMES = [s[0] for s in SCENES]
SEEDS = {name: 0 for name in NAMES}
RUN_NAMES = [s[0] for s in SCENES if s[1] > 0]
ZERO_NAMES = [s[0] for s in SCENES if s[3] in ("zero", "zero_removed")]
BATCH = ("free_300", "free_12", "free_0", "fix_65")      # mixed sizes; one returns 0, one has n = 0


def _gpu():
    import torch
    return torch.cuda.is_available()


@functools.lru_cache(maxsize=None)
def _orbx():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd")


def _row(name):
    return [s for s in SCENES if s[0] == name][0]


def _make(name, seed):
    _, n, fs, kind, kw = _row(name)
    return osr.make_scene(n, seed, fix_scale=fs, **kw)


def _screen(name, seed):
    """what the GPU tests rely on, on the restatement alone: no tested chi2 within NEAR of th2, and the path the scene is there for"""
    _, n, fs, kind, kw = _row(name)
    p = _make(name, seed)
    P = osr.Problem(p, TH2, fs)
    r = osr.optimize_sim3(P)
    if osr.near_threshold(r, P.th2, NEAR).any():
        return False
    if kind == "zero":
        return r["returned_zero"] and r["n_inliers"] == 0
    if kind == "zero_removed":
        return r["returned_zero"] and 0 < r["n_bad"] and n - r["n_bad"] < 10
    if kind == "floor":
        return not r["returned_zero"] and r["n_bad"] == 0 and r["n_inliers"] == 10
    if kind == "clean":
        return not r["returned_zero"] and r["n_bad"] == 0 and r["stats"][1, 0] <= 5
    if kind == "terminate":
        return not r["returned_zero"] and any(w in ("rho0", "trials") for w in r["why"])
    ok = not r["returned_zero"] and r["n_bad"] > 0 and r["n_inliers"] >= 0.7 * n
    if kind == "behind":
        ok = ok and int((P.x3dc2[:, 2] < 0).sum()) == n // 10
    return ok


def _first_seed(name):
    for seed in range(200):
        if _screen(name, seed):
            return seed
    raise AssertionError("no seed for " + name)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _make(name, SEEDS[name])


def _problem(name, x3dc1=None, x3dc2=None):
    return osr.Problem(_scene(name), TH2, _row(name)[2], x3dc1, x3dc2)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return osr.optimize_sim3(_problem(name))


def _ulp_moved(P, name, g):
    """the problem with every camera-point coordinate moved by one double ulp, up or down"""
    mv = lambda X: np.nextafter(X, np.where(g.integers(0, 2, X.shape) == 1, np.inf, -np.inf))      # noqa: E731
    return _problem(name, mv(P.X1), mv(P.X2))


def _lin_dev(a, b):
    """the five deviations of LIN_MEASURED between two linearisations"""
    H = np.abs(b["H"])
    return dict(errors=float(np.abs(a["errors"] - b["errors"]).max()),
                chi2=float((np.abs(a["chi2"] - b["chi2"]) / np.maximum(1.0, np.abs(b["chi2"]))).max()),
                jac=float(np.abs(a["jac"] - b["jac"]).max() / np.abs(b["jac"]).max()),
                H=float(np.abs(a["H"] - b["H"]).max() / H.max()),
                b=float((np.abs(a["b"] - b["b"]) / (np.sqrt(np.diag(H)) + 1.0)).max()))


def _est_dev(Sa, Sb):
    qa, qb = np.array(Sa[0]), np.array(Sb[0])
    return max(float(min(np.abs(qa - qb).max(), np.abs(qa + qb).max())), float(np.abs(np.array(Sa[1]) - np.array(Sb[1])).max()), abs(Sa[2] - Sb[2]))


@functools.lru_cache(maxsize=None)
def _measure_bounds():
    lin = dict(errors=0.0, chi2=0.0, jac=0.0, H=0.0, b=0.0)
    e2e, flips = 0.0, 0
    for name in RUN_NAMES:
        P, r = _problem(name), _ref(name)
        g = np.random.default_rng(12345)
        kept = ~r["removed_first"]
        bases = [(P.S0, None, osr.linearize(P, P.S0))] + ([] if r["returned_zero"] else [(r["S"], kept, osr.linearize(P, r["S"], kept))])
        for _ in range(PERTURBATIONS):
            Q = _ulp_moved(P, name, g)
            for S, act, base in bases:
                d = _lin_dev(osr.linearize(Q, S, act), base)
                lin = {k: max(lin[k], d[k]) for k in lin}
            rq = osr.optimize_sim3(Q)
            e2e = max(e2e, _est_dev(rq["S"], r["S"]))
            flips += int((rq["removed_first"] != r["removed_first"]).sum() + (rq["removed_final"] != r["removed_final"]).sum())
    return lin, e2e, flips


# ---------------------------------------------------------------------------------------------------------------------------------------
# without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_create_without_a_device(orbx):
    L = orbx.load_library()
    for sym in ("orbx_sim3_optimizer_create", "orbx_sim3_optimizer_destroy", "orbx_optimize_sim3", "orbx_optimize_sim3_linearize", "orbx_sim3_optimizer_last_timing"):
        assert hasattr(L, sym), sym
    assert callable(orbx.sim3_opt_problem) and all(hasattr(orbx.Sim3Optimizer, k) for k in ("OptimizeSim3", "linearize", "last_timing"))
    assert "orbx_optimize_sim3" in (ROOT / "__graft_entry__.py").read_text()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbx_sim3_optimizer_create.argtypes = [ci, ci, ci, ctypes.POINTER(vp)]
    L.orbx_sim3_optimizer_destroy.argtypes = [vp]
    L.orbx_sim3_optimizer_destroy.restype = None
    L.orbx_last_error.restype = ctypes.c_char_p
    h = vp()
    assert L.orbx_sim3_optimizer_create(0, 0, 100, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_sim3_optimizer_create(0, 8, 0, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_sim3_optimizer_create(0, 8, 1 << 20, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_sim3_optimizer_create(0, 8, 100, None) == ERR_ARG
    rc = L.orbx_sim3_optimizer_create(0, 8, 100, ctypes.byref(h))
    if _gpu():
        assert rc == 0 and h.value
        L.orbx_sim3_optimizer_destroy(h)
    else:
        assert rc == ERR_NODEVICE and not h.value
        assert len(L.orbx_last_error()) > 0
        with pytest.raises(orbx.OrbxError) as e:
            orbx.Sim3Optimizer()
        assert e.value.code == ERR_NODEVICE
    L.orbx_optimize_sim3.argtypes = [vp, vp, ci, vp]
    L.orbx_optimize_sim3_linearize.argtypes = [vp, vp, vp, vp, ctypes.c_double, vp, vp, vp, vp, vp, vp]
    L.orbx_sim3_optimizer_last_timing.argtypes = [vp, vp, vp]
    assert L.orbx_optimize_sim3(None, None, 1, None) == ERR_ARG
    assert L.orbx_optimize_sim3_linearize(None, None, None, None, 1.0, None, None, None, None, None, None) == ERR_ARG
    assert L.orbx_sim3_optimizer_last_timing(None, None, None) == ERR_ARG


@pytest.mark.skipif(not os.access(REF / "include" / "Optimizer.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-DOPTIMIZER_H", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "OptimizeSim3_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "OptimizeSim3_hip.cc").read_text()
    for piece in ("int OptimizeSim3_hip(", "OptimizeSim3All(", "orbx_optimize_sim3(", "GetIndexInKeyFrame(", "isBad()", "mvInvLevelSigma2[", "mvKeysUn[", "shim_error.h"):
        assert piece in text, piece
    head = (shim / "OptimizeSim3_hip.h").read_text()
    assert "OptimizeSim3_hip(" in head and "OptimizeSim3All(" in head
    assert "OptimizeSim3_hip" not in (ROOT / "oracle" / "Makefile").read_text()


def test_seeds_are_the_first_screened():
    for name in NAMES:
        assert SEEDS[name] == _first_seed(name), name


def test_bounds_are_the_measured_ones():
    lin, e2e, flips = _measure_bounds()
    print("one-ulp camera points through one linearisation: %s; through the optimisation: %.3g, %d flipped classifications" % (
        ", ".join("%s %.3g" % kv for kv in lin.items()), e2e, flips))
    assert flips == 0
    for k, got in lin.items():
        assert LIN_MEASURED[k] / 1.25 <= got <= LIN_MEASURED[k] * 1.25, (k, got)
    assert E2E_MEASURED / 1.25 <= e2e <= E2E_MEASURED * 1.25, e2e
    assert LIN_BOUND == {k: 4 * v for k, v in LIN_MEASURED.items()} and E2E_BOUND == 4 * E2E_MEASURED


@pytest.mark.parametrize("name", RUN_NAMES)
def test_restatement_recovers_the_scene(name):
    """ground truth: the refined similarity is nearer the scene's than the estimate it started from (0.02 rad, 0.03 m and 2 % away), in rotation and in
    translation, once there are a wave's pairs or more; the noise-free scene is recovered to the float rounding of its inputs (1e-5)"""
    _, n, fs, kind, kw = _row(name)
    p, r = _scene(name), _ref(name)
    truth = dict(R=p["truth"][0], t=p["truth"][1], s=p["truth"][2])
    e0 = sr.similarity_error(p["R12"], p["t12"], p["s12"], truth)
    e1 = sr.similarity_error(osr.quat_to_R(r["S"][0]), r["S"][1], r["S"][2], truth)
    print(name, "start", e0, "refined", e1, "inliers", r["n_inliers"], "bad", r["n_bad"], r["stats"].ravel(), r["why"])
    if r["returned_zero"]:
        assert r["S"] == _problem(name).S0
        return
    assert (r["removed_first"] | r["removed_final"])[p["outlier"]].all()
    if n >= 63:
        assert e1[0] < e0[0] / 2 and e1[1] < e0[1] / 2 and (fs or e1[2] < e0[2] / 2)
    if kind == "terminate":
        assert math.radians(e1[0]) < 1e-5 and e1[1] < 1e-5 and e1[2] < 1e-5


@pytest.mark.parametrize("name", ["free_64", "fix_300", "k2_100", "clean_100", "behind_100"])
def test_restatement_against_an_independent_solve(name):
    """scipy.optimize.least_squares with analytic residuals sqrt(w) e on the final inlier set (every chi2 <= th2 = Huber's delta^2 there: the robust
    cost is the plain one), started at the restatement's result S and parametrised as Sim3(u) * S: the driver stops once three iterations in a row
    gain less than 0.1 % of chi2, so the restatement's cost is held to 0.5 % above the optimum's and the optimum to |u| < 1e-2."""
    from scipy.optimize import least_squares
    P, r = _problem(name), _ref(name)
    keep = ~(r["removed_first"] | r["removed_final"])
    S, fs = r["S"], P.fix_scale

    def res(u):
        T = osr.oplus(S, list(u[:6]) + [0.0 if fs else u[6]], fs)
        e12, e21 = osr.errors_at(P, T)
        return np.concatenate([(np.sqrt(P.w1)[:, None] * e12)[keep].ravel(), (np.sqrt(P.w2)[:, None] * e21)[keep].ravel()])

    sol = least_squares(res, np.zeros(7), method="lm", xtol=1e-14, ftol=1e-14, gtol=1e-14)
    c0, c1 = float((res(np.zeros(7)) ** 2).sum()), float((sol.fun ** 2).sum())
    print(name, "cost at the restatement's result %.9g, at scipy's optimum %.9g, |u| %.3g" % (c0, c1, np.abs(sol.x).max()))
    assert c1 <= c0 <= c1 * 1.005 and np.abs(sol.x).max() < 1e-2


def test_restated_log_inverts_the_restated_exponential():
    """Sim3::log() (sim3.h:148-230) of the restated exponential, in all four branches and on both sides of each 1e-5 switch.
    omega and sigma come back to 1e-9, or to theta^3 where log takes its d > 1 - eps branch (theta up to ~4.5e-3: omega = deltaR / 2 there).
    upsilon comes back to 1e-9 where both functions use the same branch's A, B, C.  For 1e-5 <= theta < ~4.5e-3 the exponential uses the general
    formulas and log the small-angle ones: A and B then differ by O(theta^2), and for |sigma| >= 1e-5 by the reference's small-angle
    B = (sigma^2 / 2 - sigma + 1) s / sigma^3, which grows like sigma^-3 (it multiplies Omega^2 = O(theta^2)): upsilon is held to
    2 (1 + s / |sigma|^3) theta^2 |upsilon| there, which says nothing for a tiny sigma - the reference's two functions do not invert each other there."""
    seen = set()
    g = np.random.default_rng(7)
    for theta in (0.0, 0.99e-5, 1.01e-5, 1e-3, 0.4):
        for sigma in (0.0, 0.99e-5, -0.99e-5, 1.01e-5, -1.01e-5, 0.2, -0.3):
            ax = g.normal(size=3)
            u = np.concatenate([theta * ax / np.linalg.norm(ax), g.normal(size=3), [sigma]])
            S, be = osr.sim3_exp(u)
            v, bl = osr.sim3_log(S)
            seen.add(be)
            assert be[0] == bl[0] == (abs(sigma) < 1e-5) and be[1] == (theta < 1e-5) and bl[1] == (theta < 4e-3)
            assert np.abs(v - u)[[0, 1, 2, 6]].max() <= max(1e-9, theta ** 3), (theta, sigma, v - u)
            tol = 1e-9
            if bl[1] and not be[1]:
                tol = max(1e-9, 2 * (1 + (0.0 if be[0] else S[2] / abs(sigma) ** 3)) * theta ** 2 * np.abs(u[3:6]).max())
            assert np.abs(v - u)[3:6].max() <= tol, (theta, sigma, v - u)
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _handle():
    return _orbx().Sim3Optimizer(max_problems=4, max_pairs=512)


def _run(name):
    return _handle().OptimizeSim3([_scene(name)], th2=TH2, fix_scale=_row(name)[2], full=True)[0]


_dev = functools.lru_cache(maxsize=None)(_run)      # host copies only


@functools.lru_cache(maxsize=None)
def _ref_fed(name):
    """the restatement fed with the device's own camera points"""
    d = _dev(name)
    return osr.optimize_sim3(_problem(name, d.x3dc1, d.x3dc2))


def _b64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def _result_bits(r):
    return [np.ascontiguousarray(v).tobytes() for v in (np.int64(r.n_inliers), np.int64(r.n_bad), r.quat, r.t, np.float64(r.s), r.r12, r.removed_first, r.removed_final,
                                                        r.chi2_round1, r.chi2_round2, r.stats, r.x3dc1, r.x3dc2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUN_NAMES)
def test_camera_points(name):
    d, P = _dev(name), _problem(name)
    assert d.x3dc1.shape == P.x3dc1.shape and (d.x3dc1.view(np.uint32) == P.x3dc1.view(np.uint32)).all()
    assert (d.x3dc2.view(np.uint32) == P.x3dc2.view(np.uint32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUN_NAMES)
def test_one_linearisation(name):
    """at the input estimate over all pairs, and at the device's final estimate over the pairs round one kept"""
    _, n, fs, kind, kw = _row(name)
    d, p = _dev(name), _scene(name)
    P = _problem(name, d.x3dc1, d.x3dc2)
    cases = [(P.S0, None)]
    if d.n_inliers > 0 or not _ref(name)["returned_zero"]:
        cases.append(((list(d.quat), list(d.t), d.s), ~d.removed_first))
    for S, act in cases:
        got = _handle().linearize(p, S[0], S[1], S[2], active=act, th2=TH2, fix_scale=fs)
        want = osr.linearize(P, S, act)
        dev = _lin_dev(got, want)
        print(name, "all pairs" if act is None else "kept pairs", ", ".join("%s %.3g (%.3g)" % (k, v, LIN_BOUND[k]) for k, v in dev.items()))
        for k, v in dev.items():
            assert v <= LIN_BOUND[k], (k, v)
        if fs:
            assert (got["jac"][:, :, 6] == 0).all() and (got["H"][6] == 0).all() and (got["H"][:, 6] == 0).all() and got["b"][6] == 0
        if act is not None:
            off = np.repeat(~act, 2)
            assert (got["jac"][off] == 0).all() and (got["errors"][off] == 0).all() and (got["chi2"][off] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUN_NAMES)
def test_end_to_end(name):
    d, r = _dev(name), _ref_fed(name)
    dev = _est_dev((list(d.quat), list(d.t), d.s), r["S"])
    print(name, "estimate %.3g (%.3g); iterations %s against %s; robust chi2 %s against %s" % (dev, E2E_BOUND, d.stats[:, 0], r["stats"][:, 0], d.stats[:, 1], r["stats"][:, 1]))
    assert dev <= E2E_BOUND
    # a trial whose chi2 gain is within rounding of a switch (rho's sign, the three-strikes 0.1 %) can fall on either side: one iteration, as in test_pose_optimization.py
    assert (np.abs(d.stats[:, 0] - r["stats"][:, 0]) <= 1).all()
    assert np.abs(d.r12.astype(F64) - osr.quat_to_R(list(d.quat))).max() <= 2.0 ** -23


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUN_NAMES)
def test_classification(name):
    _, n, fs, kind, kw = _row(name)
    d, r = _dev(name), _ref_fed(name)
    near = osr.near_threshold(r, float(F32(TH2)), NEAR)
    assert near.mean() <= EXCLUDED_CAP
    ok = ~near
    assert (d.removed_first[ok] == r["removed_first"][ok]).all() and (d.removed_final[ok] == r["removed_final"][ok]).all()
    tested1 = r["chi2_round1"] >= 0
    assert ((d.chi2_round1 >= 0) == tested1).all() and ((d.chi2_round2 >= 0) == (r["chi2_round2"] >= 0))[ok].all()
    if not near.any():
        assert d.n_bad == r["n_bad"] == int(d.removed_first.sum()) and d.n_inliers == r["n_inliers"]
        if d.n_inliers:
            assert d.n_inliers == n - d.n_bad - int(d.removed_final.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ZERO_NAMES)
def test_return_zero(name):
    _, n, fs, kind, kw = _row(name)
    d = _handle().OptimizeSim3([_scene(name)], th2=TH2, fix_scale=fs, full=True)[0]
    P = _problem(name)
    assert d.n_inliers == 0
    assert (_b64(d.quat) == _b64(P.S0[0])).all() and (_b64(d.t) == _b64(P.S0[1])).all() and _b64(d.s) == _b64(P.S0[2])
    if n == 0:
        assert d.n_bad == 0 and len(d.removed_first) == 0 and (d.stats == 0).all()
        return
    r = _ref_fed(name)
    ok = ~osr.near_threshold(r, float(F32(TH2)), NEAR)
    assert ok.all() and (d.removed_first == r["removed_first"]).all() and not d.removed_final.any() and d.n_bad == r["n_bad"]
    assert d.stats[0, 0] >= 1 and (d.stats[1] == 0).all() and (d.chi2_round2 == -1).all()
    if kind == "zero_removed":
        assert d.removed_first.any()


@pytest.mark.gpu
def test_batch_equals_alone_bit_for_bit():
    h = _handle()
    fs = False
    scenes = [_scene(nm) for nm in BATCH]
    # (fix_65 is a fix_scale scene run free here: the flag belongs to the call)
    together = h.OptimizeSim3(scenes, th2=TH2, fix_scale=fs, full=True)
    alone = [h.OptimizeSim3([s], th2=TH2, fix_scale=fs, full=True)[0] for s in scenes]
    zeros = 0
    for a, b, nm in zip(together, alone, BATCH):
        assert _result_bits(a) == _result_bits(b), nm
        zeros += a.n_inliers == 0
    assert zeros >= 2 and together[0].n_inliers > 0 and len(together[2].removed_first) == 0
    assert h.last_timing()[1] == 1


@pytest.mark.gpu
def test_repeated_calls_give_the_same_bits():
    h, s = _handle(), _scene("free_257")
    first = _result_bits(h.OptimizeSim3([s], th2=TH2, full=True)[0])
    for _ in range(19):
        assert _result_bits(h.OptimizeSim3([s], th2=TH2, full=True)[0]) == first


@pytest.mark.gpu
def test_python_round_trip():
    """Sim3Solver's first event -> sim3_opt_problem -> Sim3Optimizer on a test_sim3_solver.py scene: the refined similarity carries the scene's points at
    least as near their true places as the event alone"""
    orbx = _orbx()
    c = sr.scene(300, 1, scale=1.7, outliers=0.3)
    sets = sr.draw_sets(300, 300, 1001)
    solved = orbx.Sim3Solver(max_candidates=1, max_matches=512, max_iterations=300).Solve([c], sets=[sets], min_inliers=20)[0]
    assert solved.first_event >= 0
    inl = solved.inliers_first
    # SearchBySim3's matches: the event's inliers, observed where the TRUE points project (map 2 carries the scene's position noise), half a pixel of noise
    g = np.random.default_rng(5)
    tr = c["truth"]
    X1c = c["world1"].astype(F64) @ c["Rcw1"].astype(F64).T + c["tcw1"].astype(F64)
    X2c = (X1c - tr["t"]) @ tr["R"] / tr["s"]
    pr = lambda X, K: np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)      # noqa: E731
    m = dict(world1=c["world1"][inl], world2=c["world2"][inl], obs1=(pr(X1c, c["K1"]) + g.normal(0, 0.5, (300, 2)))[inl], obs2=(pr(X2c, c["K2"]) + g.normal(0, 0.5, (300, 2)))[inl],
             inv_sigma2_1=1.0 / c["sigma2_1"][inl], inv_sigma2_2=1.0 / c["sigma2_2"][inl])
    p = orbx.sim3_opt_problem(c, solved, m)
    r = _handle().OptimizeSim3([p], th2=TH2)[0]
    it = solved.first_event
    e0 = sr.similarity_error(solved.r12[it], solved.t12[it], solved.s12[it], tr)
    e1 = sr.similarity_error(r.r12, r.t, r.s, tr)
    # one figure for "how well": the RMS distance between the scene's points of map 2 carried into map 1 and their true places there (a
    # smaller rotation error can come with a larger scale error: the three components are printed, not compared one by one)
    transfer = lambda R, t, s: float(np.sqrt(((float(s) * X2c @ np.asarray(R, F64).T + np.asarray(t, F64) - X1c) ** 2).sum(1).mean()))      # noqa: E731
    t0, t1 = transfer(solved.r12[it], solved.t12[it], solved.s12[it]), transfer(r.r12, r.t, r.s)
    print("first event (deg, |dt|, |ds|):", e0, "transfer RMS %.6g; refined:" % t0, e1, "transfer RMS %.6g; inliers %d of %d" % (t1, r.n_inliers, int(inl.sum())))
    assert r.n_inliers >= 20 and t1 <= t0
    assert r.T12().shape == (4, 4) and not r.removed.all()


@pytest.mark.gpu
def test_error_paths():
    orbx = _orbx()
    h = orbx.Sim3Optimizer(max_problems=2, max_pairs=64)
    good, big = _scene("free_64"), _scene("free_65")
    with pytest.raises(orbx.OrbxError) as e:
        h.OptimizeSim3([big], th2=TH2)
    assert e.value.code == ERR_CAPACITY
    with pytest.raises(orbx.OrbxError) as e:
        h.OptimizeSim3([good, good, good], th2=TH2)
    assert e.value.code == ERR_CAPACITY
    keep = []
    h._L.orbx_last_error.restype = ctypes.c_char_p
    P, n = h._problem(good, keep, TH2, False)
    res = (orbx.Sim3OptResult * 1)()
    for field, value, code in (("world1", None, ERR_ARG), ("obs2", None, ERR_ARG), ("inv_sigma2_1", None, ERR_ARG), ("n", -1, ERR_ARG), ("fx1", float("nan"), ERR_ARG),
                               ("cy2", float("inf"), ERR_ARG), ("n", 65, ERR_CAPACITY)):
        Q, _ = h._problem(good, keep, TH2, False)
        setattr(Q, field, value)
        assert h._L.orbx_optimize_sim3(h._h, ctypes.byref(Q), 1, res) == code, field
        assert len(h._L.orbx_last_error()) > 0
    assert h._L.orbx_optimize_sim3(h._h, ctypes.byref(P), 0, res) == ERR_ARG
    assert h._L.orbx_optimize_sim3(h._h, None, 1, res) == ERR_ARG
    r = h.OptimizeSim3([good], th2=TH2)[0]      # the handle stays usable
    assert r.n_inliers == _ref("free_64")["n_inliers"] or osr.near_threshold(_ref("free_64"), float(F32(TH2)), NEAR).any()
    h.close()
