"""Optimizer::OptimizeEssentialGraph on the device (orbx_optimize_essential_graph, csrc/orbx_essential_graph.hip) against tests/essential_graph_ref.py,
the numpy float64 restatement of reference src/Optimizer.cc:1017-1339 and the vendored g2o.  No C entry point of the compiled reference reaches this
function, so the restatement is tied down on the CPU (the loop closes, an independent scipy solve, a dense solve, log against exp); every stage of the
device is then checked against the restatement fed with the device's OWN upstream outputs."""
import ctypes
import functools
import math
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import essential_graph_ref as eg
from test_initializer import REF, ROOT

ERR_ARG, ERR_CAPACITY, ERR_NODEVICE, ERR_STATE = -1, -3, -4, -5
F64 = np.float64
PERTURBATIONS = 6
EPS64 = float(np.finfo(F64).eps)

# What moving every input pose component (est and meas: q, t, s of every keyframe) by ONE double ulp, up or down at random, PERTURBATIONS draws per
# scene, does to the restatement, the largest over the scenes: the errors; chi2 relative to max(1, chi2); the Jacobians and H relative to their largest
# entry (g2o's central differences magnify a change of a few ulps of an error by 1 / (2e-9): this is the reference's own noise); b[i] relative to
# sqrt(H[i][i]) + 1; x of the first solve (lambda = 1e-16) relative to max(1, |x|); the final q (up to sign), t and s, relative to max(1, |value|).  The
# device is held to 4 times these.  test_bounds_are_the_measured_ones recomputes them.
# Per scene: the scenes differ by orders of magnitude in conditioning (300 steps of scale drift make the free 300 scene's translations thousands of units long).
STAGES = ("errors", "chi2", "jac", "H", "b", "x", "est")
MEASURED = {
    'n2_free': dict(errors=1.89e-15, chi2=1.54e-16, jac=7.23e-08, H=8.29e-08, b=2.4e-09, x=6.53e-09, est=2.37e-08),
    'n2_fix': dict(errors=1.33e-15, chi2=3.61e-16, jac=5.69e-08, H=3.08e-08, b=6.92e-09, x=2.26e-08, est=1.12e-08),
    'n3_first_free': dict(errors=3.33e-15, chi2=1.21e-15, jac=2.18e-07, H=1.24e-07, b=2.8e-08, x=1.44e-07, est=1.07e-07),
    'n3_first_fix': dict(errors=3.77e-15, chi2=3.89e-16, jac=2.43e-07, H=8.71e-08, b=2.34e-08, x=1.69e-07, est=7.53e-08),
    'n3_middle_free': dict(errors=3.33e-15, chi2=1.21e-15, jac=2.02e-07, H=1.24e-07, b=1.28e-08, x=7.98e-08, est=3.73e-08),
    'n3_middle_fix': dict(errors=3.77e-15, chi2=3.89e-16, jac=2.01e-07, H=8.71e-08, b=1.39e-08, x=5.93e-08, est=2.99e-08),
    'n3_last_free': dict(errors=3.33e-15, chi2=1.21e-15, jac=2.38e-07, H=1.58e-07, b=2.8e-08, x=2.61e-08, est=2.92e-08),
    'n3_last_fix': dict(errors=3.77e-15, chi2=3.89e-16, jac=2.74e-07, H=2.04e-07, b=2.34e-08, x=4.69e-08, est=2.51e-08),
    'n9_free': dict(errors=5.77e-15, chi2=6.55e-15, jac=3.09e-07, H=1.49e-07, b=5.53e-07, x=6.06e-07, est=5.01e-07),
    'n9_fix': dict(errors=7.11e-15, chi2=2.11e-15, jac=3.04e-07, H=1.6e-07, b=4.99e-08, x=5.88e-07, est=3.13e-07),
    'n64_free': dict(errors=4.97e-14, chi2=1.51e-15, jac=1.01e-06, H=4.73e-07, b=6.7e-05, x=0.000272, est=0.000651),
    'n64_fix': dict(errors=4.09e-14, chi2=5.26e-15, jac=7.9e-07, H=1.71e-07, b=2.2e-06, x=1.33e-05, est=7.88e-06),
    'n65_free': dict(errors=5.33e-14, chi2=1.55e-15, jac=7.74e-07, H=3.88e-07, b=6.7e-05, x=0.000242, est=0.000283),
    'n65_fix': dict(errors=4.44e-14, chi2=2.3e-15, jac=7.79e-07, H=2.71e-07, b=2.06e-06, x=1.12e-05, est=1.1e-05),
    'n300_free': dict(errors=1.15e-12, chi2=6.75e-15, jac=2.14e-06, H=4.54e-07, b=0.00245, x=1.12, est=0.133),
    'n300_fix': dict(errors=3.13e-13, chi2=2.02e-16, jac=6.48e-07, H=2.85e-07, b=0.000241, x=0.00344, est=0.00444),
}
BOUND = {name: {k: 4 * v for k, v in m.items()} for name, m in MEASURED.items()}

# (name, N, make_scene arguments): 2 = one free vertex; 3 = a chain with the fixed vertex first, in the middle, last; 9 = a ring inside one tile with
# the duplicated pair and the isolated vertex; 64 / 65 = the wave edge of the per-vertex and per-edge kernels; 300 = band 6, K = 4, one older kind-1
# loop edge, several panels and workgroups, ~1800 edges.  Each with and without fix_scale.
# The 300 scene drifts in scale by 0.01 +- 0.0115 per step, not by the 0.03 +- 0.02 of the others: 300 steps of 3 % are a factor of 8000 between the two
# ends of the loop, on which the restated Levenberg driver takes two steps and gives up (chi2 1.0e6 -> 1.9e4) and a one-ulp change of the inputs moves
# the result by 20 - bounds taken there would check nothing.  With 1 % the whole trajectory drifts by e^3, as a 100-keyframe one does at 3 %.
_BASE = (("n2", 2, {}), ("n3_first", 3, dict(fixed=0)), ("n3_middle", 3, dict(fixed=1)), ("n3_last", 3, dict(fixed=2)),
         ("n9", 9, dict(K=2, duplicate=True, isolated=True, points=40)), ("n64", 64, dict(points=70)), ("n65", 65, {}),
         ("n300", 300, dict(K=4, band=6, old_loop=True, points=300, scale_drift=(0.01, 0.2 / 300 ** 0.5))))
SCENES = [("%s_%s" % (name, "fix" if fs else "free"), n, fs, kw) for name, n, kw in _BASE for fs in (False, True)]
NAMES = [s[0] for s in SCENES]
# the first seed for which the restatement alone meets _screen (test_seeds_are_the_first_screened)
SEEDS = {'n2_free': 0, 'n2_fix': 6, 'n3_first_free': 1, 'n3_first_fix': 2, 'n3_middle_free': 1, 'n3_middle_fix': 2, 'n3_last_free': 1, 'n3_last_fix': 2, 'n9_free': 0,
         'n9_fix': 1, 'n64_free': 0, 'n64_fix': 0, 'n65_free': 1, 'n65_fix': 0, 'n300_free': 1, 'n300_fix': 16}
SMALL = [s[0] for s in SCENES if s[1] <= 65]


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
    _, n, fs, kw = _row(name)
    return eg.make_scene(n, seed, fix_scale=fs, **kw)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _make(name, SEEDS[name])


def _ref(name):
    return _runs(name, SEEDS[name])[0]


def _log_of(r):
    """what the device's log is compared with: trials per iteration, whether each iteration's last trial was accepted, the ending"""
    return [int(l[0]) for l in r["log"]], [bool(a[-1]) for a in r["accepts"]], r["ended"]


def _ulp_moved(G, g):
    mv = lambda X: np.nextafter(X, np.where(g.integers(0, 2, X.shape) == 1, np.inf, -np.inf))      # noqa: E731
    return G.with_poses(mv(G.est), mv(G.meas))


@functools.lru_cache(maxsize=None)
def _moved(name, seed):
    """the PERTURBATIONS one-ulp neighbours of a scene"""
    G = _make(name, seed)[0]
    g = np.random.default_rng(12345)
    return [_ulp_moved(G, g) for _ in range(PERTURBATIONS)]


@functools.lru_cache(maxsize=None)
def _run_of(name, seed, k):
    """the restated run of a scene (k < 0) or of its neighbour k (shared by the screen and the bounds)"""
    return eg.optimize(_make(name, seed)[0] if k < 0 else _moved(name, seed)[k])


def _runs(name, seed):
    return _run_of(name, seed, -1), [(Q, _run_of(name, seed, k)) for k, Q in enumerate(_moved(name, seed))]


def _screen(name, seed):
    """what the GPU tests rely on, on the restatement alone: chi2 falls, and the trial log (accept or reject per trial, trials per iteration, the
    ending) is the same under every one-ulp perturbation of the inputs (the draws stop at the first that differs)"""
    r = _run_of(name, seed, -1)
    if not r["chi2"][1] < r["chi2"][0]:
        return False
    for k in range(PERTURBATIONS):
        q = _run_of(name, seed, k)
        if _log_of(q) != _log_of(r) or q["accepts"] != r["accepts"]:
            return False
    return True


def _first_seed(name):
    for seed in range(200):
        if _screen(name, seed):
            return seed
    raise AssertionError("no seed for " + name)


def _rel(a, b):
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if np.size(a) else 0.0


def _lin_dev(a, b):
    """the deviations of MEASURED between two linearisations (a against b)"""
    H = np.concatenate([b["h_diag"].reshape(-1), b["h_off"].reshape(-1)])
    Ha = np.concatenate([a["h_diag"].reshape(-1), a["h_off"].reshape(-1)])
    dg = np.sqrt(np.abs(np.einsum("nii->ni", b["h_diag"]))) + 1.0
    return dict(errors=float(np.abs(a["errors"] - b["errors"]).max()), chi2=abs(a["chi2"] - b["chi2"]) / max(1.0, abs(b["chi2"])),
                jac=float(np.abs(a["jac"] - b["jac"]).max() / np.abs(b["jac"]).max()), H=float(np.abs(Ha - H).max() / np.abs(H).max()),
                b=float((np.abs(a["b"] - b["b"]) / dg).max()))


def _est_dev(A, B):
    A, B = np.asarray(A), np.asarray(B)
    dq = np.minimum(np.abs(A[:, :4] - B[:, :4]).max(1), np.abs(A[:, :4] + B[:, :4]).max(1)).max()
    return max(float(dq), _rel(A[:, 4:], B[:, 4:]))


def _first_x(G, lin):
    """x of lambda = 1e-16 by vertex"""
    ok, x = eg.sparse_solve(lin["sym"], lin["Hb"], lin["bp"], 1e-16)
    out = np.zeros((G.N, 7))
    out[lin["sym"]["order"]] = x
    return ok, out


@functools.lru_cache(maxsize=None)
def _measure_bounds():
    out = {}
    for name in NAMES:
        m = {k: 0.0 for k in STAGES}
        G = _scene(name)[0]
        r, moved = _runs(name, SEEDS[name])
        base = eg.linearize(G, G.est)
        bx = _first_x(G, base)[1]
        for Q, rq in moved:
            lin = eg.linearize(Q, Q.est)
            d = _lin_dev(lin, base)
            d["x"] = _rel(_first_x(Q, lin)[1], bx)
            d["est"] = _est_dev(rq["est"], r["est"])
            m = {k: max(m[k], d[k]) for k in m}
        out[name] = m
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def _bind(L):
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbx_essential_graph_create.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.orbx_essential_graph_destroy.argtypes = [vp]
    L.orbx_essential_graph_destroy.restype = None
    L.orbx_optimize_essential_graph.argtypes = [vp, vp, vp]
    L.orbx_essential_graph_linearize.argtypes = [vp] * 10
    L.orbx_essential_graph_solve.argtypes = [vp, ctypes.c_double, vp, vp]
    L.orbx_essential_graph_last_timing.argtypes = [vp, vp, vp, vp]
    L.orbx_last_error.restype = ctypes.c_char_p


def test_exports_and_create_without_a_device(orbx):
    L = orbx.load_library()
    for sym in ("orbx_essential_graph_create", "orbx_essential_graph_destroy", "orbx_optimize_essential_graph", "orbx_essential_graph_linearize",
                "orbx_essential_graph_solve", "orbx_essential_graph_last_timing"):
        assert hasattr(L, sym), sym
    assert callable(orbx.essential_graph_edges) and all(hasattr(orbx.EssentialGraphOptimizer, k) for k in ("OptimizeEssentialGraph", "linearize", "solve", "last_timing"))
    assert "orbx_optimize_essential_graph" in (ROOT / "__graft_entry__.py").read_text()
    _bind(L)
    h = ctypes.c_void_p()
    assert L.orbx_essential_graph_create(0, 0, 10, 0, 10, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_essential_graph_create(0, 8, -1, 0, 10, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_essential_graph_create(0, 8, 10, -1, 10, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_essential_graph_create(0, 8, 10, 0, 0, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_essential_graph_create(0, 8, 10, 0, 10, None) == ERR_ARG
    rc = L.orbx_essential_graph_create(0, 8, 10, 0, 36, ctypes.byref(h))
    if _gpu():
        assert rc == 0 and h.value
        L.orbx_essential_graph_destroy(h)
    else:
        assert rc == ERR_NODEVICE and not h.value
        assert len(L.orbx_last_error()) > 0
        with pytest.raises(orbx.OrbxError) as e:
            orbx.EssentialGraphOptimizer(8, 10)
        assert e.value.code == ERR_NODEVICE


def test_error_paths_without_a_device(orbx):
    L = orbx.load_library()
    _bind(L)
    assert L.orbx_optimize_essential_graph(None, None, None) == ERR_ARG
    assert L.orbx_essential_graph_linearize(*[None] * 10) == ERR_ARG
    assert L.orbx_essential_graph_solve(None, 1.0, None, None) == ERR_ARG
    assert L.orbx_essential_graph_last_timing(None, None, None, None) == ERR_ARG
    with pytest.raises(ValueError):
        orbx.EssentialGraphOptimizer._problem(dict(est=np.zeros((2, 8)), meas=np.zeros((3, 8)), fixed=0, edges=[]), [], False, 20, 1e-16)
    with pytest.raises(ValueError):
        orbx.EssentialGraphOptimizer._problem(dict(est=np.zeros((2, 8)), fixed=0, edges=[], points=np.zeros((2, 3)), ref=[0]), [], False, 20, 1e-16)


@pytest.mark.skipif(not os.access(REF / "include" / "Optimizer.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-DOPTIMIZER_H", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "EssentialGraph_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "EssentialGraph_hip.cc").read_text()
    for piece in ("void OptimizeEssentialGraph_hip(", "orbx_optimize_essential_graph(", "isBad()", "GetCovisiblesByWeight(", "GetLoopEdges()", "hasChild(", "mnCorrectedReference",
                  "mMutexMapUpdate", "SetPose(", "SetWorldPos(", "UpdateNormalAndDepth()", "shim_error.h"):
        assert piece in text, piece
    assert "OptimizeEssentialGraph_hip(" in (shim / "EssentialGraph_hip.h").read_text()
    assert "EssentialGraph_hip" not in (ROOT / "oracle" / "Makefile").read_text()


def _kf(i, parent=None, children=(), loops=(), cov=(), weights=None, bad=False):
    ang = 0.1 * i
    R = np.array([[math.cos(ang), -math.sin(ang), 0.0], [math.sin(ang), math.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    return dict(id=i, parent=parent, children=set(children), loop_edges=set(loops), covisibles=list(cov), weights=dict(weights or {}), bad=bad, Rcw=R, tcw=[0.5 * i, 0.0, 0.1])


def test_edge_selection_rules(orbx):
    """hand-built keyframes that hit every rule of :1106-1262; ids are not contiguous, keyframe 30 is bad"""
    w = lambda **k: {int(a[1:]): b for a, b in k.items()}      # noqa: E731
    kfs = [
        _kf(0, children=[10], cov=[10, 20, 70], weights=w(k10=300, k20=150, k70=120)),
        _kf(10, parent=0, children=[20], cov=[0, 20, 40], weights=w(k0=300, k20=250, k40=120)),
        _kf(20, parent=10, children=[40], cov=[10, 0, 30, 40], weights=w(k10=250, k0=150, k30=140, k40=200)),
        _kf(30, parent=20, bad=True, cov=[20], weights=w(k20=140)),
        _kf(40, parent=20, children=[50], loops=[70], cov=[20, 10, 50, 30], weights=w(k20=200, k10=120, k50=180, k30=110)),
        _kf(50, parent=40, children=[60], cov=[40, 60, 20, 0], weights=w(k40=180, k60=170, k20=99, k0=100)),
        _kf(60, parent=50, children=[70], cov=[50, 70, 10], weights=w(k50=170, k70=160, k10=130)),
        _kf(70, parent=60, loops=[40, 0], cov=[60, 0, 40, 10, 50], weights=w(k60=160, k0=120, k40=115, k10=105, k50=101)),
    ]
    ident = [0.0, 0.0, 0.0, 1.0]
    corrected = {70: ident + [1.0, 2.0, 3.0, 1.1], 60: ident + [0.9, 2.0, 3.0, 1.1]}
    non_corrected = {70: ident + [4.0, 5.0, 6.0, 1.0], 60: ident + [3.5, 5.0, 6.0, 1.0]}
    # LoopConnections: (70, 0) is the (current, loop) pair with weight 120; (70, 10) has weight 105 -> kept; (60, 0) has no weight -> skipped;
    # (60, 10) weight 130 -> kept and later dedupes the covisibility edge (60, 10)
    lc = {70: [0, 10], 60: [0, 10]}
    kfs[7]["weights"][0] = 50      # below min_feat, yet kept: the (current, loop) pair
    g = orbx.essential_graph_edges(kfs, loop_kf=0, cur_kf=70, corrected=corrected, non_corrected=non_corrected, loop_connections=lc)
    ids = list(g["ids"])
    assert ids == [0, 10, 20, 40, 50, 60, 70] and g["fixed"] == 0
    ix = {k: n for n, k in enumerate(ids)}
    E = lambda i, j, k: (ix[i], ix[j], k)      # noqa: E731
    want = [E(70, 0, 0), E(70, 10, 0), E(60, 10, 0),                      # LoopConnections; (60, 0) is below min_feat
            E(10, 0, 1),                                                  # 10: parent; covisibles 0 (parent), 20 / 40 (larger ids)
            E(20, 10, 1), E(20, 0, 1),                                    # 20: parent, covisible 0; 30 is bad, 40 a child
            E(40, 20, 1), E(40, 10, 1),                                   # 40: parent; loop edge 70 is larger; covisible 10; 50 a child; 30 bad
            E(50, 40, 1), E(50, 0, 1),                                    # 50: parent; 60 a child; 20 has weight 99; 0 has exactly min_feat
            E(60, 50, 1),                                                 # 60: parent; 70 a child; (60, 10) already inserted
            E(70, 60, 1), E(70, 0, 1), E(70, 40, 1), E(70, 50, 1)]        # 70: parent; loop edges 0, 40 in id order (0 repeats its LoopConnections pair); covisible 0
    #                                                                       has weight 50 now and is a loop edge, 40 a loop edge, (70, 10) inserted, 50 weight 101
    assert [tuple(int(v) for v in e) for e in g["edges"]] == want
    assert (g["est"][ix[70]] == corrected[70]).all() and (g["meas"][ix[70]] == non_corrected[70]).all()
    assert (g["meas"][ix[20]] == g["est"][ix[20]]).all() and g["est"][ix[20], 7] == 1.0
    ang = 0.1 * 20
    assert np.allclose(g["est"][ix[20], :4], [0.0, 0.0, math.sin(ang / 2), math.cos(ang / 2)], atol=1e-15) and (g["est"][ix[20], 4:7] == [10.0, 0.0, 0.1]).all()
    # the order of GetCovisiblesByWeight is kept
    kfs[7]["covisibles"], kfs[7]["loop_edges"] = [50, 10, 60], set()
    g2 = orbx.essential_graph_edges(kfs, 0, 70, corrected, non_corrected, {})
    assert [tuple(int(v) for v in e) for e in g2["edges"]][-3:] == [E(70, 60, 1), E(70, 50, 1), E(70, 10, 1)]


def test_seeds_are_the_first_screened():
    for name in NAMES:
        assert SEEDS[name] == _first_seed(name), name


def test_bounds_are_the_measured_ones():
    for name, m in _measure_bounds().items():
        print(name, "one-ulp input poses through the restatement: " + ", ".join("%s %.3g" % kv for kv in m.items()))
        for k, got in m.items():
            assert MEASURED[name][k] / 1.25 <= got <= MEASURED[name][k] * 1.25, (name, k, got)
        assert BOUND[name] == {k: 4 * v for k, v in MEASURED[name].items()}


def _loop_distance(V, tru, cur, loop):
    """rotation angle, largest translation component and |log scale| between the relative pose of (cur, loop) in V and in the truth"""
    R, t, s = eg.relative(V, cur, loop)
    Rt, tt, st = eg.relative(tru, cur, loop)
    return math.acos(max(-1.0, min(1.0, 0.5 * (np.trace(R @ Rt.T) - 1.0)))), float(np.abs(t - tt).max()), abs(math.log(s / st))


# One step of drift at two sigma: 0.06 rad, 0.16, and 0.03 + 2 * 0.02 = 0.07 of log-scale.
LOOP_DISTANCE = (0.06, 0.16, 0.07)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_closes_the_loop(name):
    """ground truth, every scene: chi2 falls, and the relative pose of the current and the loop keyframe ends within LOOP_DISTANCE of the truth - one
    step's drift at two sigma in rotation, translation and log-scale, whatever the trajectory has accumulated (up to 0.5 rad, 60 units and e^3).
    From nine keyframes on it also ends no further away than HALF of what the uncorrected trajectory has accumulated: the optimisation spreads the
    loop's discrepancy over the trajectory."""
    (G, tru), r = _scene(name), _ref(name)
    assert r["chi2"][1] < r["chi2"][0]
    before, after = _loop_distance(G.meas, tru, G.N - 1, 0), _loop_distance(r["est"], tru, G.N - 1, 0)
    print(name, "chi2 %.4g -> %.4g" % r["chi2"], "loop before", before, "after", after, _log_of(r))
    assert all(a <= d for a, d in zip(after, LOOP_DISTANCE)), after
    if G.N >= 9:
        assert after[0] <= 0.5 * before[0] and after[1] <= 0.5 * before[1] and (G.fix_scale or after[2] <= 0.5 * before[2])


def _scipy_min(G, r, V0):
    """scipy's Levenberg-Marquardt on the edge errors over oplus updates of V0 -> (chi2, estimates)"""
    from scipy.optimize import least_squares
    sym, M = r["sym"], eg.measurements(G)
    dof = 6 if G.fix_scale else 7

    def upd(p):
        x = np.zeros((sym["nf"], 7))
        x[:, :dof] = p.reshape(sym["nf"], dof)
        return eg.apply_update(G, sym, V0, x)
    sol = least_squares(lambda p: eg.errors_at(G, M, upd(p)).ravel(), np.zeros(sym["nf"] * dof), method="lm", xtol=1e-14, ftol=1e-14, gtol=1e-14)
    return float((sol.fun ** 2).sum()), upd(sol.x), float(np.abs(sol.x).max())


@pytest.mark.parametrize("name", ["n9_free", "n9_fix", "n3_middle_free"])
def test_restatement_against_scipy(name):
    """an independent scipy.optimize.least_squares on the same residual, over the same oplus parametrisation, started from the INPUT estimates and
    from the restated result.  Both reach the minimum the restated driver stops next to: each chi2 is at most 5 % below the restated one and not above
    it by more than 1e-6 (scipy stops on its own forward-difference gradient), the two agree to 0.1 % - the gain below which the driver itself counts
    an iteration as no progress -, and all three sets of estimates are within 0.05 of one another in every component.
    The restated driver does not end ON the minimum: with lambda_init = 1e-16 every trial is a Gauss-Newton step (lambda stays below 1e-3 through its
    ten doublings), and the run ends at the first step that does not lower chi2, or after three gains below 0.1 %."""
    G, r = _scene(name)[0], _ref(name)
    chi_a, est_a, _ = _scipy_min(G, r, G.est)
    chi_b, est_b, step = _scipy_min(G, r, r["est"])
    print(name, "restated chi2 %.12g, scipy from the input %.12g, from the restated result %.12g (step %.3g), estimates %.3g / %.3g / %.3g apart" % (
        r["chi2"][1], chi_a, chi_b, step, _est_dev(est_a, r["est"]), _est_dev(est_b, r["est"]), _est_dev(est_a, est_b)))
    for chi in (chi_a, chi_b):
        assert chi <= r["chi2"][1] * (1 + 1e-6) and r["chi2"][1] - chi <= 0.05 * r["chi2"][1]
    assert abs(chi_a - chi_b) <= 1e-3 * chi_b
    assert _est_dev(est_a, r["est"]) <= 0.05 and _est_dev(est_b, r["est"]) <= 0.05 and _est_dev(est_a, est_b) <= 0.05 and step <= 0.05


def test_pinned_elementary_functions_against_numpy():
    """the kernels' own exp, sin, cos, log and acos, as restated, against numpy's over the ranges the reductions cover: within 4 ulps (of the result;
    of one for sin and cos next to their zeros, where libm's own reductions differ)"""
    def ulps(a, b, floor=0.0):
        return float((np.abs(a - b) / np.maximum(np.spacing(np.abs(b)), floor)).max())
    g = np.random.default_rng(7)
    x = np.concatenate([g.uniform(-20, 20, 200000), [0.0, 1e-9, -1e-9, 1e-300]])
    assert ulps(eg.eg_exp(x), np.exp(x)) <= 4
    t = np.concatenate([g.uniform(0, 4, 200000), [0.0, 1e-9, 1e-5, math.pi]])
    s, c = eg.eg_sincos(t)
    assert ulps(s, np.sin(t), EPS64 / 2) <= 4 and ulps(c, np.cos(t), EPS64 / 2) <= 4
    v = np.concatenate([np.exp(g.uniform(-20, 20, 200000)), [1.0, 0.5, 2.0, 1 + 1e-12, 1 - 1e-12]])
    assert ulps(eg.eg_log(v), np.log(v), EPS64 / 2) <= 4 and eg.eg_log(1.0) == 0.0
    d = np.concatenate([g.uniform(-1, 1, 200000), 1 - np.logspace(-15, -1, 2000), [1.0, -1.0, 0.5, -0.5, 0.0]])
    assert ulps(eg.eg_acos(d), np.arccos(d)) <= 4 and eg.eg_acos(1.0) == 0.0
    u = [0.3, -0.2, 0.5, 1.0, -2.0, 0.5, 0.2]
    import optsim3_ref as osr
    assert np.abs(eg.pack(eg.sim3_exp(u)[0], 1) - eg.pack(osr.sim3_exp(u)[0], 1)).max() <= 1e-15


@pytest.mark.parametrize("name", SMALL)
def test_sparse_solve_equals_dense(name):
    G = _scene(name)[0]
    lin = eg.linearize(G, G.est)
    H, b = eg.dense_system(lin["sym"], lin["Hb"], lin["bp"])
    for lam in (1e-16, 1.0):
        ok, x = eg.sparse_solve(lin["sym"], lin["Hb"], lin["bp"], lam)
        assert ok
        A = H + lam * np.eye(len(H))
        keep = np.ones(len(H), bool)
        if G.fix_scale:      # the seventh rows are exactly zero: x = 0 / lambda there, and the rest decouples
            assert (x[:, 6] == 0).all() and (H[6::7] == 0).all()
            keep[6::7] = False
        A = A[keep][:, keep]
        xd = np.linalg.solve(A, b[keep])
        tol = 16 * np.linalg.cond(A) * EPS64 * max(1.0, np.abs(xd).max())
        print(name, lam, "sparse - dense %.3g (%.3g)" % (np.abs(x.ravel()[keep] - xd).max(), tol))
        assert np.abs(x.ravel()[keep] - xd).max() <= tol


def test_isolated_vertex_and_duplicates():
    G = _scene("n9_free")[0]
    lin = eg.linearize(G, G.est)
    iso = 9 // 2 + 1
    assert not (G.edges[:, :2] == iso).any() and (lin["h_diag"][iso] == 0).all() and (lin["b"][iso] == 0).all()
    pairs = [tuple(sorted(e[:2])) for e in G.edges.tolist()]
    assert len(pairs) > len(set(pairs))      # the duplicated pairs are there
    r = _ref("n9_free")
    assert (r["est"][iso] == G.est[iso]).all() and (r["est"][G.fixed] == G.est[G.fixed]).all()


def test_log_inverts_exp_on_all_four_branches():
    seen = set()
    for theta in (0.0, 3e-6, 1e-3, 0.7, 2.5):
        for sigma in (0.0, 4e-6, -2e-3, 0.3):
            u = np.array([0.3, -0.5, 0.8]) / math.sqrt(0.98) * theta
            u = np.concatenate([u, [0.4, -1.1, 2.0], [sigma]])
            S, be = eg.sim3_exp(u)
            v, bl = eg.sim3_log_v(eg.unpack(eg.pack(S, 1)))
            seen.add((bool(bl[0][0]), bool(bl[1][0])))
            assert bool(bl[0][0]) == (abs(sigma) < 1e-5) and bool(bl[1][0]) == (math.cos(theta) > 1 - 1e-5)
            # omega and sigma: inside d > 1 - eps (theta < 4.5e-3) log takes omega = deltaR / 2, exact to theta^3
            assert np.abs(v[0] - u)[[0, 1, 2, 6]].max() <= max(1e-9, theta ** 3), (theta, sigma, v[0] - u)
            # the translation: where log is inside d > 1 - eps and exp outside theta < eps (1e-5 <= theta < 4.5e-3) the two use different A and B;
            # the reference's series B for |sigma| >= eps is s (sigma^2 / 2 - sigma + 1) / sigma^3 (it lacks the "- 1"), so W differs by up to
            # (1 + s / |sigma|^3) theta^2 there - the reference's own behaviour, kept
            tol = 1e-9
            if bl[1][0] and not be[1]:
                tol = max(1e-9, 2 * (1 + (0.0 if be[0] else S[2] / abs(sigma) ** 3)) * theta ** 2 * np.abs(u[3:6]).max())
            assert np.abs(v[0] - u)[3:6].max() <= tol, (theta, sigma, v[0] - u)
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _handle():
    return _orbx().EssentialGraphOptimizer(max_keyframes=320, max_edges=2048, max_points=512)


def _run(name, handle=None):
    G = _scene(name)[0]
    return (handle or _handle()).OptimizeEssentialGraph(G, fix_scale=G.fix_scale, full=True)


_dev = functools.lru_cache(maxsize=None)(_run)


@functools.lru_cache(maxsize=None)
def _dev_lin(name):
    G = _scene(name)[0]
    h = _handle()
    lin = h.linearize(G, fix_scale=G.fix_scale)
    return lin, h.solve(1e-16), h.solve(1.0)


def _blocks_of(G, sym, lin):
    """the device's H and b in the restatement's block layout"""
    nf = sym["nf"]
    Hb = np.zeros((nf + sym["nOff"], 7, 7))
    Hb[:nf] = lin["h_diag"][sym["order"]]
    index = {(int(sym["rowIdx"][k]), q): nf + k for q in range(nf) for k in range(int(sym["colPtr"][q]), int(sym["colPtr"][q + 1]))}
    for e in range(G.E):
        pi, pj = int(sym["pos"][G.edges[e, 0]]), int(sym["pos"][G.edges[e, 1]])
        if pi >= 0 and pj >= 0:
            Hb[index[(max(pi, pj), min(pi, pj))]] = lin["h_off"][e] if pi > pj else lin["h_off"][e].T
    return Hb, lin["b"][sym["order"]]


def _bits(r):
    return [np.ascontiguousarray(v).tobytes() for v in (r.est, r.Tiw, r.inv, r.points, np.array(r.chi2), r.trials, r.iter_chi2, r.iter_lambda, r.iter_rho, r.order)] + [r.ended, r.fill_blocks]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_measurements(name):
    G = _scene(name)[0]
    got, want = _dev_lin(name)[0]["meas"], eg.measurements(G)
    assert got.shape == want.shape and (got.view(np.uint64) == want.view(np.uint64)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_linearisation(name):
    G = _scene(name)[0]
    got = _dev_lin(name)[0]
    want = eg.linearize(G, G.est, got["meas"])
    dev = _lin_dev(got, want)
    print(name, ", ".join("%s %.3g (%.3g)" % (k, v, BOUND[name][k]) for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= BOUND[name][k], (k, v)
    assert (got["jac"][G.edges[:, 0] == G.fixed, 0] == 0).all() and (got["jac"][G.edges[:, 1] == G.fixed, 1] == 0).all()
    assert (got["h_diag"][G.fixed] == 0).all() and (got["b"][G.fixed] == 0).all()
    if G.fix_scale:
        assert (got["jac"][..., 6] == 0).all() and (got["h_diag"][:, 6] == 0).all() and (got["h_diag"][:, :, 6] == 0).all() and (got["b"][:, 6] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_solve(name):
    """x at lambda = 1e-16 and 1 against the restated solve of the device's own H and b, and the residual of the device's x"""
    G = _scene(name)[0]
    lin, s0, s1 = _dev_lin(name)
    sym = eg.symbolic(G)
    Hb, bp = _blocks_of(G, sym, lin)
    H, b = eg.dense_system(sym, Hb, bp)
    for lam, (ok, x) in ((1e-16, s0), (1.0, s1)):
        wok, wx = eg.sparse_solve(sym, Hb, bp, lam)
        assert ok and wok
        xp = x[sym["order"]]
        dev = _rel(xp, wx)
        r = (H @ xp.ravel() + lam * xp.ravel()) - b
        nb, na = np.linalg.norm(b), math.sqrt(np.linalg.norm(H) ** 2 + lam * lam * len(b))
        res = float(np.linalg.norm(r) / nb)
        # normwise backward error of a stable solve: |r| <= c n eps (|A| |x| + |b|), c = 8
        res_bound = 8 * len(b) * EPS64 * (1.0 + na * np.linalg.norm(xp) / nb)
        print(name, "lambda %g: x %.3g (%.3g), residual / |b| %.3g (%.3g)" % (lam, dev, BOUND[name]["x"], res, res_bound))
        assert dev <= BOUND[name]["x"] and res <= res_bound
        assert (x[G.fixed] == 0).all()
        if G.fix_scale:
            assert (x[:, 6] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_end_to_end(name):
    """The device's exp, sin, cos, log and acos are its own series (EgMath), restated bit for bit, so the two runs differ only where the order of an
    operation does; with the device library's functions two scenes ended their last iteration differently (a chi2 gain of 1e-14 decided by an ulp of
    acos).  Bit-equality of the estimates is printed, not asserted: the bound is the one-ulp sensitivity."""
    G = _scene(name)[0]
    d = _dev(name)
    want = eg.optimize(G, M=_dev_lin(name)[0]["meas"])
    dev = _est_dev(d.est, want["est"])
    trials, accepted, ended = _log_of(want)
    print(name, "bit-equal" if (d.est.view(np.uint64) == want["est"].view(np.uint64)).all() else "not bit-equal", "estimate %.3g (%.3g); chi2 %s against %s; trials %s against %s; %s against %s" % (dev, BOUND[name]["est"], d.chi2, want["chi2"], list(d.trials), trials, d.ended, ended))
    assert d.iterations == want["iterations"] and list(d.trials) == trials and d.ended == ended
    assert [bool(r > 0.0) for r in d.iter_rho] == accepted
    assert dev <= BOUND[name]["est"]
    assert abs(d.chi2[0] - want["chi2"][0]) <= BOUND[name]["chi2"] * max(1.0, want["chi2"][0])
    assert (d.est[G.fixed] == G.est[G.fixed]).all()
    # every elementary function is restated, so nothing is left to differ: the estimates agree in every bit (the bound above is the contract of the
    # issue; this is what the pinned arithmetic delivers, and it is what holds the scenes whose one-ulp sensitivity is large)
    assert (d.est.view(np.uint64) == want["est"].view(np.uint64)).all()
    # the write-back of the device's OWN estimates, bit for bit
    Tiw, inv, pts = eg.write_back(G, d.est)
    assert (d.Tiw.view(np.uint32) == Tiw.view(np.uint32)).all() and (d.inv.view(np.uint64) == inv.view(np.uint64)).all()
    assert d.points.shape == pts.shape and (d.points.view(np.uint32) == pts.view(np.uint32)).all()
    if len(pts):
        assert G.ref[0] == -1 and (d.points[0] == G.points[0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_reported_order_and_fill(name):
    G, d = _scene(name)[0], _dev(name)
    assert sorted(d.order.tolist()) == [v for v in range(G.N) if v != G.fixed]
    assert d.fill_blocks == eg.symbolic(G, d.order)["fill"]
    nf = G.N - 1
    if G.N == 300:
        print(name, "fill %d of %d" % (d.fill_blocks, nf * (nf + 1) // 2))
        assert d.fill_blocks < 0.25 * (nf * (nf + 1) // 2)


@pytest.mark.gpu
def test_repeated_call_gives_the_same_bits():
    for name in ("n65_free", "n9_fix"):
        assert _bits(_run(name)) == _bits(_dev(name))


@pytest.mark.gpu
def test_two_scenes_on_one_handle_equal_fresh_handles():
    a, b = _run("n64_free"), _run("n9_fix")      # back to back on the shared handle, the larger first
    for name, got in (("n64_free", a), ("n9_fix", b)):
        h = _orbx().EssentialGraphOptimizer(max_keyframes=70, max_edges=300, max_points=100)
        assert _bits(_run(name, h)) == _bits(got)
        h.close()


@pytest.mark.gpu
def test_python_round_trip():
    """keyframe dicts -> essential_graph_edges -> the device: the scene's edges, the repeated parent edge once"""
    G = _scene("n9_free")[0]
    ids = [3 * v + 1 for v in range(G.N)]
    kfs = [dict(id=ids[v], parent=None, children=set(), loop_edges=set(), covisibles=[], weights={}, bad=False, Rcw=np.eye(3), tcw=np.zeros(3)) for v in range(G.N)]
    lc = {}
    for i, j, kind in G.edges.tolist():
        if kind == 0:
            lc.setdefault(ids[i], []).append(ids[j])
            kfs[i]["weights"][ids[j]] = 150
        elif kfs[i]["parent"] is None:
            kfs[i]["parent"] = ids[j]
            kfs[j]["children"].add(ids[i])
        else:
            kfs[i]["covisibles"].append(ids[j])
            kfs[i]["weights"][ids[j]] = 200 - len(kfs[i]["covisibles"])
    g = _orbx().essential_graph_edges(kfs, ids[G.fixed], ids[G.N - 1], {ids[v]: G.est[v] for v in range(G.N)}, {ids[v]: G.meas[v] for v in range(G.N)}, lc)
    assert sorted(map(tuple, g["edges"].tolist())) == sorted(set(map(tuple, G.edges.tolist())))
    r = _handle().OptimizeEssentialGraph(g, fix_scale=False, full=True)
    assert r.est.shape == (G.N, 8) and r.Tiw.shape == (G.N, 3, 4) and r.chi2[1] < r.chi2[0] and r.ended in ("iterations", "trials", "rho0", "three")
    ms, launches, solve_ms = _handle().last_timing()
    assert ms > 0 and launches >= 6 and 0 < solve_ms <= ms


@pytest.mark.gpu
def test_error_paths():
    orbx = _orbx()
    G = _scene("n9_free")[0]
    h = orbx.EssentialGraphOptimizer(max_keyframes=9, max_edges=G.E, max_points=4, max_fill_blocks=40)
    with pytest.raises(orbx.OrbxError) as e:
        h.solve(1.0)
    assert e.value.code == ERR_STATE
    with pytest.raises(orbx.OrbxError) as e:
        h.last_timing()
    assert e.value.code == ERR_STATE

    def code(**kw):
        g = dict(est=G.est, meas=G.meas, fixed=G.fixed, edges=G.edges)
        g.update(kw)
        with pytest.raises(orbx.OrbxError) as ei:
            h.OptimizeEssentialGraph(g)
        return ei.value.code
    bad = lambda row: np.concatenate([G.edges, np.array([row], np.int32)])[1:]      # noqa: E731
    assert code(fixed=9) == ERR_ARG and code(fixed=-1) == ERR_ARG
    assert code(edges=bad([9, 0, 1])) == ERR_ARG and code(edges=bad([0, -1, 1])) == ERR_ARG
    assert code(edges=bad([3, 3, 1])) == ERR_ARG and code(edges=bad([3, 2, 2])) == ERR_ARG
    est = G.est.copy()
    est[4, 7] = 0.0
    assert code(est=est) == ERR_ARG
    est[4, 7] = float("nan")
    assert code(est=est) == ERR_ARG
    assert code(points=np.zeros((1, 3)), ref=[9]) == ERR_ARG and code(points=np.zeros((1, 3)), ref=[-2]) == ERR_ARG
    assert code(points=np.zeros((5, 3)), ref=[0] * 5) == ERR_CAPACITY
    assert code(edges=np.concatenate([G.edges, G.edges[:1]])) == ERR_CAPACITY
    assert code(est=np.concatenate([G.est, G.est[:1]]), meas=None) == ERR_CAPACITY
    tight = orbx.EssentialGraphOptimizer(max_keyframes=9, max_edges=G.E, max_fill_blocks=eg.symbolic(G)["fill"] - 1)
    with pytest.raises(orbx.OrbxError) as e:
        tight.OptimizeEssentialGraph(dict(est=G.est, meas=G.meas, fixed=G.fixed, edges=G.edges))
    assert e.value.code == ERR_CAPACITY and "fill" in str(e.value)
    tight.close()
    # the handle stays usable; no edge and a lone fixed vertex are not errors
    r = h.OptimizeEssentialGraph(dict(est=G.est, meas=G.meas, fixed=G.fixed, edges=G.edges), full=True)
    assert _bits(r)[:3] == _bits(_dev("n9_free"))[:3]
    r0 = h.OptimizeEssentialGraph(dict(est=G.est, fixed=G.fixed, edges=np.zeros((0, 3), np.int32)))
    assert (r0.est == G.est).all() and r0.iterations == 0 and r0.chi2 == (0.0, 0.0)
    r1 = h.OptimizeEssentialGraph(dict(est=G.est[:1], fixed=0, edges=[]))
    assert (r1.est == G.est[:1]).all() and len(r1.order) == 0
    h.close()
