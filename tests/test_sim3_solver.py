"""Sim3Solver on the device (orbx_sim3_solve and friends, Python Sim3Solver, shim/Sim3Solver_hip.cc).

Expected values come from the numpy restatement in tests/sim3_ref.py.  Every device stage is checked against the restatement fed with the
device's OWN upstream outputs, so a stage's allowance never has to cover the stages before it; two end-to-end checks tie the chain to the
float64 form of the restatement on screened sets and scenes.
"""
import ctypes
import functools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import sim3_ref as sr
from test_initializer import REF, ROOT

ERR_ARG, ERR_CAPACITY, ERR_NODEVICE, ERR_STATE = -1, -3, -4, -5
F32, F64 = np.float32, np.float64
ULP1 = 2.0 ** -23      # one float ulp of 1
GAP = 1e-3             # sets whose two largest eigenvalues of N are relatively closer leave the eigenvector undetermined (three nearly collinear points)
EXCLUDED_CAP = 0.05

# Largest difference between the float32 and the float64 form of the restatement over the gap-screened sets of every scene below (entries of R; t
# relative to max(1, |t|); s), and 4 times it: the factor of RANK2 / DECOMP in test_initializer.py.  test_bounds_are_the_measured_ones recomputes them.
MODEL_R_MEASURED, MODEL_T_MEASURED, MODEL_S_MEASURED = 2.41e-5, 1.34e-4, 3.09e-7
MODEL_R_BOUND, MODEL_T_BOUND, MODEL_S_BOUND = 4 * MODEL_R_MEASURED, 4 * MODEL_T_MEASURED, 4 * MODEL_S_MEASURED
# The float64 restatement's first event against the scene's similarity, the largest over the scenes that have one (rotation in degrees, |t - t_true|,
# |s / s_true - 1|), and 1.25 times it.
FIRST_ROT_MEASURED, FIRST_T_MEASURED, FIRST_S_MEASURED = 0.911, 0.0724, 0.0033
FIRST_ROT_TOL, FIRST_T_TOL, FIRST_S_TOL = 1.25 * FIRST_ROT_MEASURED, 1.25 * FIRST_T_MEASURED, 1.25 * FIRST_S_MEASURED

# (name, kind, matches, iterations, seed, min_inliers, fix_scale, scene scale, outlier share).
# Matches 3, 19, 20, 21, 63, 64, 65, 300, 1000: the minimum, below / at / above min_inliers, a wave less one, a wave, a wave and one, several waves,
# many.  Iterations 1, 7, 300.  Seeds: the first seed for which the restatement alone keeps the share of gap-excluded sets under EXCLUDED_CAP and
# meets test_scenes_are_screened (no count falls on different sides of min_inliers in the float32 and the float64 form).
SCENES = [
    ("general_3", "general", 3, 1, 1, 2, False, 1.7, 0.0),
    ("general_19", "general", 19, 7, 1, 20, False, 1.7, 0.3),       # n < min_inliers: no iterations, bNoMore at once
    ("general_20", "general", 20, 7, 1, 20, False, 1.7, 0.3),       # count > 20 cannot happen
    ("general_21", "general", 21, 7, 1, 20, False, 1.7, 0.3),
    ("general_63", "general", 63, 300, 1, 20, False, 1.7, 0.3),
    ("general_64", "general", 64, 300, 1, 20, False, 1.7, 0.3),
    ("general_65", "general", 65, 7, 1, 20, False, 1.7, 0.3),
    ("general_300", "general", 300, 300, 1, 20, False, 1.7, 0.3),
    ("general_1000", "general", 1000, 300, 1, 20, False, 1.7, 0.3),
    ("fix_64", "general", 64, 7, 1, 20, True, 1.0, 0.3),
    ("fix_300", "general", 300, 300, 1, 20, True, 1.0, 0.3),
    ("behind_300", "behind", 300, 7, 1, 20, False, 1.7, 0.3),       # a tenth of the points behind camera 2
    ("z0_65", "z0", 65, 7, 1, 20, False, 1.7, 0.3),                 # points on camera 1's z = 0 plane: invz = 1 / 0
    ("noevent_100", "general", 100, 300, 1, 20, False, 1.7, 0.9),   # ten true pairs: no iteration reaches min_inliers
]
NAMES = [s[0] for s in SCENES]
ITER_NAMES = [s[0] for s in SCENES if s[2] >= s[5]]                 # scenes that run iterations
BATCH = ("general_300", "general_19", "noevent_100")                # mixed n; one below min_inliers, one that never reaches an event


def _gpu():
    import torch
    return torch.cuda.is_available()


@functools.lru_cache(maxsize=None)
def _orbx():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd")


def _row(name):
    return [s for s in SCENES if s[0] == name][0]


@functools.lru_cache(maxsize=None)
def _scene(name):
    _, kind, n, it, seed, mi, fs, scale, outl = _row(name)
    c = sr.scene(n, seed, scale=scale, outliers=outl, kind=kind)
    c["sets"] = sr.draw_sets(n, it, seed + 1000)
    return c


@functools.lru_cache(maxsize=None)
def _ref(name, form="f32"):
    _, _, _, _, _, mi, fs, _, _ = _row(name)
    c = _scene(name)
    return sr.solve(c, c["sets"], mi, fs, form)


@functools.lru_cache(maxsize=None)
def _handle():
    return _orbx().Sim3Solver(max_candidates=4, max_matches=1024, max_iterations=300)


def _solve(name):
    _, _, _, _, _, mi, fs, _, _ = _row(name)
    c = _scene(name)
    r = _handle().Solve([c], sets=[c["sets"]], min_inliers=mi, fix_scale=fs, full=True)[0]
    r.masks = np.array([r.inliers(it) for it in range(r.iterations)], bool).reshape(r.iterations, r.n)      # before another call overwrites them
    return r


_dev = functools.lru_cache(maxsize=None)(_solve)      # host copies only: nothing of a cached result reads the device again


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _con(d):
    return {k: getattr(d, k) for k in ("x3dc1", "x3dc2", "p1im1", "p2im2", "max_err1", "max_err2")}


# ---------------------------------------------------------------------------------------------------------------------------------------
# without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_create_without_a_device(orbx):
    L = orbx.load_library()
    for sym in ("orbx_sim3_solver_create", "orbx_sim3_solver_destroy", "orbx_sim3_solve", "orbx_sim3_inliers", "orbx_sim3_check_models", "orbx_sim3_ransac_iterations",
                "orbx_sim3_last_timing"):
        assert hasattr(L, sym), sym
    assert callable(orbx.sim3_sets) and hasattr(orbx.Sim3Solver, "Solve") and hasattr(orbx.Sim3Solver, "CheckModels") and hasattr(orbx.Sim3Solver, "last_timing")
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbx_sim3_solver_create.argtypes = [ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.orbx_sim3_solver_destroy.argtypes = [vp]
    L.orbx_sim3_solver_destroy.restype = None
    L.orbx_last_error.restype = ctypes.c_char_p
    h = vp()
    assert L.orbx_sim3_solver_create(0, 0, 1000, 300, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_sim3_solver_create(0, 8, 2, 300, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_sim3_solver_create(0, 8, 1 << 20, 300, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_sim3_solver_create(0, 8, 1000, 0, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_sim3_solver_create(0, 8, 1000, 300, None) == ERR_ARG
    rc = L.orbx_sim3_solver_create(0, 8, 1000, 300, ctypes.byref(h))
    if _gpu():
        assert rc == 0 and h.value
        L.orbx_sim3_solver_destroy(h)
    else:
        assert rc == ERR_NODEVICE and not h.value
        assert len(L.orbx_last_error()) > 0
        with pytest.raises(orbx.OrbxError) as e:
            orbx.Sim3Solver()
        assert e.value.code == ERR_NODEVICE
    L.orbx_sim3_solve.argtypes = [vp, vp, ci, vp]
    L.orbx_sim3_inliers.argtypes = [vp, ci, ci, vp]
    L.orbx_sim3_check_models.argtypes = [vp, vp, vp, vp, ci, vp, vp]
    L.orbx_sim3_last_timing.argtypes = [vp, vp, vp]
    assert L.orbx_sim3_solve(None, None, 1, None) == ERR_ARG
    assert L.orbx_sim3_inliers(None, 0, 0, None) == ERR_ARG
    assert L.orbx_sim3_check_models(None, None, None, None, 1, None, None) == ERR_ARG
    assert L.orbx_sim3_last_timing(None, None, None) == ERR_ARG


def test_ransac_iterations(orbx):
    for n in range(20, 2001):
        assert orbx.sim3_ransac_iterations(0.99, 20, 300, n) == sr.ransac_iterations(0.99, 20, 300, n), n
    assert orbx.sim3_ransac_iterations(0.99, 20, 300, 20) == 1           # min_inliers == n
    assert orbx.sim3_ransac_iterations(0.99, 20, 300, 21) == sr.ransac_iterations(0.99, 20, 300, 21) > 1
    assert orbx.sim3_ransac_iterations(0.99, 20, 300, 2000) == 300       # the cap
    for prob, mi, mx, n in ((0.5, 6, 100, 11), (0.999, 100, 1000, 150), (0.9, 3, 5, 400)):
        assert orbx.sim3_ransac_iterations(prob, mi, mx, n) == sr.ransac_iterations(prob, mi, mx, n)


def test_sim3_sets(orbx):
    script, want = sr.sets_example()
    it = iter(script)
    seen = []

    def randint(lo, hi):
        seen.append((lo, hi))
        return next(it)
    assert orbx.sim3_sets(6, 3, randint).tolist() == want
    assert seen == [(0, 5), (0, 4), (0, 3)] * 3
    g = np.random.default_rng(3)
    s = orbx.sim3_sets(40, 200, lambda lo, hi: g.integers(lo, hi + 1))
    assert s.shape == (200, 3) and s.dtype == np.int32 and s.min() >= 0 and s.max() < 40
    assert all(len(set(r)) == 3 for r in s.tolist())
    assert (s == sr.draw_sets(40, 200, 3)).all()
    with pytest.raises(ValueError):
        orbx.sim3_sets(2, 1, lambda lo, hi: lo)


class _StubSolver:
    def __init__(self, masks):
        self.masks = masks

    def _inliers(self, candidate, iteration, n):
        return self.masks[iteration]


def _candidate(orbx, count, masks, min_inliers, n, indices1, mN1):
    """a Sim3Candidate of the package over explicit per-iteration outputs (no device)"""
    it = len(count)
    ev, first, best = sr.scan_events(count, min_inliers)
    g = np.random.default_rng(5)
    out = dict(count=np.asarray(count, np.int32), r12=g.normal(size=(it, 3, 3)).astype(F32), t12=g.normal(size=(it, 3)).astype(F32), s12=g.uniform(1, 2, it).astype(F32),
               is_event=ev, first_event=first, best_iteration=best, no_more=bool(n < min_inliers or first < 0),
               inliers_first=masks[first] if first >= 0 else np.zeros(n, bool))
    return orbx.Sim3Candidate(_StubSolver(masks), 0, out, n, mN1, indices1, min_inliers), out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_iterate_replay_equals_a_straight_loop(orbx, seed):
    g = np.random.default_rng(seed)
    n, it, mi = 40, 57, 20
    count = g.integers(15, 30, it).astype(np.int32)
    count[10], count[11] = count[:10].max(), count[:10].max()      # a tie: >= takes the later one, twice
    masks = np.zeros((it, n), bool)
    for k in range(it):
        masks[k, g.permutation(n)[:count[k]]] = True
    idx, mN1 = 2 * np.arange(n) + 1, 2 * n + 3
    ev, first, best = sr.scan_events(count, mi)
    assert ev.sum() >= 2 and ev[11] == (count[11] > mi)
    for chunk in (1, 5, 7, 1000):
        cand, out = _candidate(orbx, count, masks, mi, n, idx, mN1)
        ref = sr.Solver(count, masks, out["r12"], out["t12"], out["s12"], n, mi, idx, mN1)
        events, guard = [], 0
        while guard < 1000:
            guard += 1
            a, b = cand.iterate(chunk), ref.iterate(chunk)
            assert (a[0] is None) == (b[0] is None) and a[1] == b[1] and a[3] == b[3] and (a[2] == b[2]).all()
            if a[0] is not None:
                assert _same_bits(a[0], b[0])
                events.append(cand.mnIterations - 1)
                assert _same_bits(cand.GetEstimatedRotation(), out["r12"][events[-1]]) and cand.GetEstimatedScale() == out["s12"][events[-1]]
                assert a[2].sum() == count[events[-1]] and a[2][idx[masks[events[-1]]]].all()
            if a[1]:
                break
        assert events == np.flatnonzero(ev).tolist()      # the straight loop's events, whatever the chunking
        assert cand._best == best and ref.best == best
    few, _ = _candidate(orbx, count[:0], masks[:0], 50, n, idx, mN1)
    assert few.iterate(5)[:2] == (None, True) and few.iterate(5)[3] == 0


def test_round_robin_restatement():
    """the restated loop of LoopClosing::ComputeSim3 on three scripted candidates: one discarded at once, one after its iterations, one asked again after a success"""
    n, mi = 30, 20
    mk = lambda count: sr.Solver(np.asarray(count, np.int32), np.ones((len(count), n), bool), np.zeros((len(count), 3, 3), F32), np.zeros((len(count), 3), F32), np.ones(len(count), F32), n, mi)
    a = mk([5, 25, 3, 25, 4, 4, 4, 4, 4, 4, 26, 1])
    b = sr.Solver(np.zeros(0, np.int32), np.zeros((0, 10), bool), np.zeros((0, 3, 3), F32), np.zeros((0, 3), F32), np.zeros(0, F32), 10, mi)
    c = mk([7] * 11)
    hits = []
    log = sr.round_robin([a, b, c], lambda i, k: hits.append((i, k)) or len(hits) == 3)
    assert [(e[0], e[1], e[2]) for e in log] == [(0, False, 25), (1, True, 0), (2, False, 0), (0, False, 25), (2, False, 0), (0, False, 0), (2, True, 0), (0, False, 26)]
    assert hits == [(0, 25), (0, 25), (0, 26)]


@pytest.mark.skipif(not os.access(REF / "include" / "Sim3Solver.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-DOPTIMIZER_H", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "Sim3Solver_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "Sim3Solver_hip.cc").read_text()
    for piece in ("Sim3Solver::Sim3Solver(", "void Sim3Solver::SetRansacParameters(", "cv::Mat Sim3Solver::iterate(", "cv::Mat Sim3Solver::find(", "Sim3Solver::GetEstimatedRotation(",
                  "Sim3Solver::GetEstimatedTranslation(", "Sim3Solver::GetEstimatedScale(", "orbx_sim3_solve(", "orbx_sim3_inliers(", "orbx_sim3_ransac_iterations(",
                  "DUtils::Random::RandomInt(", "SolveAll("):
        assert piece in text, piece
    assert "SolveAll(" in (shim / "Sim3Solver_hip.h").read_text()
    assert "Sim3Solver_hip" not in (ROOT / "oracle" / "Makefile").read_text()


def test_jacobi_sweeps_settled():
    """two sweeps fewer than ORBX_SIM3_JACOBI_SWEEPS and two more give the same float bits on every set of every scene"""
    text = (ROOT / "include" / "orbx.h").read_text()
    assert "#define ORBX_SIM3_JACOBI_SWEEPS %d\n" % sr.SWEEPS in text
    systems = 0
    for name in ITER_NAMES:
        r = _ref(name)
        q = [sr.jacobi_eig4(r["nmat"], k) for k in (sr.SWEEPS - 2, sr.SWEEPS, sr.SWEEPS + 2)]
        assert (_bits(q[0]) == _bits(q[1])).all() and (_bits(q[1]) == _bits(q[2])).all(), name
        assert (_bits(q[1]) == _bits(r["quat"])).all()
        systems += len(q[0])
    assert systems == sum(s[3] for s in SCENES if s[2] >= s[5]) > 1800


def _screened_sets(name):
    r64 = _ref(name, "f64")
    return r64["gap"] >= GAP


def _measure_bounds():
    dR = dt = ds = 0.0
    first = [0.0, 0.0, 0.0]
    for name in ITER_NAMES:
        a, b, ok = _ref(name), _ref(name, "f64"), _screened_sets(name)
        if ok.any():
            dR = max(dR, float(np.abs(a["r12"] - b["r12"]).reshape(len(ok), -1).max(1)[ok].max()))
            dt = max(dt, float((np.abs(a["t12"] - b["t12"]).max(1) / np.maximum(1.0, np.linalg.norm(b["t12"], axis=1)))[ok].max()))
            ds = max(ds, float(np.abs(a["s12"] - b["s12"])[ok].max()))
        fe = b["first_event"]
        if fe >= 0:
            e = sr.similarity_error(b["r12"][fe], b["t12"][fe], b["s12"][fe], _scene(name)["truth"])
            first = [max(x, y) for x, y in zip(first, e)]
    return (dR, dt, ds), tuple(first)


def test_bounds_are_the_measured_ones():
    (dR, dt, ds), (fr, ft, fs) = _measure_bounds()
    print("float32 against float64 form on gap-screened sets: R %.3g, t %.3g, s %.3g; float64 first events against the scenes: %.3g deg, %.3g, %.3g" % (dR, dt, ds, fr, ft, fs))
    for got, const in ((dR, MODEL_R_MEASURED), (dt, MODEL_T_MEASURED), (ds, MODEL_S_MEASURED), (fr, FIRST_ROT_MEASURED), (ft, FIRST_T_MEASURED), (fs, FIRST_S_MEASURED)):
        assert const / 1.25 <= got <= const * 1.25, (got, const)
    assert (MODEL_R_BOUND, MODEL_T_BOUND, MODEL_S_BOUND) == (4 * MODEL_R_MEASURED, 4 * MODEL_T_MEASURED, 4 * MODEL_S_MEASURED)
    assert (FIRST_ROT_TOL, FIRST_T_TOL, FIRST_S_TOL) == (1.25 * FIRST_ROT_MEASURED, 1.25 * FIRST_T_MEASURED, 1.25 * FIRST_S_MEASURED)


@pytest.mark.parametrize("name", NAMES)
def test_scenes_are_screened(name):
    """what the GPU tests rely on, asserted on the restatement alone"""
    _, kind, n, it, seed, mi, fs, _, _ = _row(name)
    a, b = _ref(name), _ref(name, "f64")
    if n < mi:
        assert len(a["count"]) == 0 and a["no_more"] and a["first_event"] == -1 and a["best_iteration"] == -1
        return
    assert len(a["count"]) == it
    ok = _screened_sets(name)
    assert (~ok).sum() <= EXCLUDED_CAP * it, "%d of %d sets excluded" % ((~ok).sum(), it)
    # no count falls on different sides of min_inliers in the two forms, so the events are the same events
    assert ((a["count"] > mi) == (b["count"] > mi)).all()
    assert a["first_event"] == b["first_event"]
    # the quaternion's sign does not reach the rotation beyond the rounding of the float angle-axis vector: for -q its length is 2 pi minus the
    # angle, up to 2 pi, so each component rounds by up to half an ulp of [4, 8) = 2^-22, and R moves by no more than the vector does: sqrt(3) * 2^-22
    q = a["quat"]
    if ok.any():
        assert np.abs(sr.rotation_from_quat(q) - sr.rotation_from_quat(-q))[ok].max() <= 2.0 ** -21
    if name in ("general_20", "general_21", "noevent_100"):
        assert a["first_event"] == -1 and a["no_more"] and a["best_iteration"] >= 0
    if name in ("general_63", "general_64", "general_300", "general_1000", "fix_300"):
        assert a["first_event"] >= 0 and a["is_event"].sum() >= 2      # an event after an event
    if name == "behind_300":
        assert (a["x3dc2"][:, 2] < 0).sum() >= 10
    if name == "z0_65":
        assert (a["x3dc1"][:, 2] == 0).sum() >= 1 and not np.isfinite(a["p1im1"]).all()
    if name == "general_300":
        # a product with 9.210 that has a fractional part: 1.44 * 9.21 = 13.26 -> 13
        s = _scene(name)["sigma2_1"]
        prod = F64(9.210) * s.astype(F64)
        assert (prod != np.floor(prod)).any() and (a["max_err1"] == np.floor(prod).astype(F32)).all() and (a["max_err1"] < prod).any()


def test_some_scene_updates_the_best_on_a_tie():
    ties = 0
    for name in ITER_NAMES:
        c = _ref(name)["count"]
        best = 0
        for k in c:
            ties += int(k == best and best > 0)
            best = max(best, int(k))
    assert ties >= 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# on the device, stage by stage
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_constructor(name):
    d, r = _dev(name), _ref(name)
    for k in ("x3dc1", "x3dc2", "p1im1", "p2im2", "max_err1", "max_err2"):
        assert _same_bits(getattr(d, k), r[k]), k
    assert d.iterations == len(r["count"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_model_inputs(name):
    d = _dev(name)
    N = sr.model_inputs(d.x3dc1, d.x3dc2, d.sets)[4]
    assert _same_bits(d.nmat, N)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_quaternion(name):
    d = _dev(name)
    q, gap = sr.eigh_quat(d.nmat)
    ok = gap >= GAP
    assert (~ok).sum() <= EXCLUDED_CAP * d.iterations
    sign = np.where((q * d.quat.astype(F64)).sum(1) < 0, -1.0, 1.0)[:, None]
    diff = np.abs(d.quat.astype(F64) - sign * q).max(1)
    print("%s: quaternion against eigh %.3g on %d of %d sets" % (name, diff[ok].max() if ok.any() else 0.0, ok.sum(), len(ok)))
    assert (diff[ok] <= ULP1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_rotation(name):
    d = _dev(name)
    R = sr.rotation_from_quat(d.quat).astype(F32)
    fin = np.isfinite(R).all((1, 2))
    assert (np.isfinite(d.r12).all((1, 2)) == fin).all()
    diff = np.abs(d.r12[fin].astype(F64) - R[fin].astype(F64))
    print("%s: rotation against the double restatement %.3g" % (name, diff.max() if fin.any() else 0.0))
    assert (diff <= ULP1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_scale_translation_transforms(name):
    d = _dev(name)
    fs = _row(name)[6]
    Pr1, Pr2, O1, O2, _ = sr.model_inputs(d.x3dc1, d.x3dc2, d.sets)
    s, t, T12, T21 = sr.model_from_rotation(d.r12, Pr1, Pr2, O1, O2, fs)
    assert _same_bits(d.s12, s) and _same_bits(d.t12, t) and _same_bits(d.t12m, T12) and _same_bits(d.t21m, T21)
    if fs:
        assert (d.s12 == 1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_inliers(name):
    d = _solve(name)      # a solve of its own: the masks are read again behind CheckModels
    c = _scene(name)
    count, inl = sr.check_inliers(_con(d), c["K1"], c["K2"], d.t12m, d.t21m)
    assert (d.count == count).all()
    assert (d.masks == inl).all()
    if d.first_event >= 0:
        assert (d.inliers_first == inl[d.first_event]).all()
    else:
        assert not d.inliers_first.any()
    cm_count, cm_inl = _handle().CheckModels(c, d.t12m, d.t21m)
    assert (cm_count == count).all() and (cm_inl == inl).all()
    # the masks of the solve survive CheckModels
    last = d.iterations - 1
    assert (d.inliers(last) == inl[last]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_events(name):
    d = _dev(name)
    mi = _row(name)[5]
    ev, first, best = sr.scan_events(d.count, mi)
    assert (d.is_event == ev).all() and d.first_event == first and d.best_iteration == best
    assert d.no_more == (d.n < mi or first < 0)


def _depth_problem():
    """30 pairs on the optical axis at depths 1..30, both maps the same, identity poses: a pure x translation by delta moves the pair at depth z by
    fx * delta / z pixels in both images, so delta_k = (30 - k + 0.5) * sqrt(13) / fx leaves exactly the k deepest pairs under the limit 13"""
    n = 30
    w = np.zeros((n, 3), F32)
    w[:, 2] = np.arange(1, n + 1)
    K = (500.0, 500.0, 320.0, 240.0)
    c = dict(Rcw1=np.eye(3, dtype=F32), tcw1=np.zeros(3, F32), Rcw2=np.eye(3, dtype=F32), tcw2=np.zeros(3, F32), K1=K, K2=K, world1=w, world2=w.copy(),
             sigma2_1=np.full(n, 1.44, F32), sigma2_2=np.full(n, 1.44, F32))

    def models(counts):
        T12, T21 = np.tile(np.eye(4, dtype=F32), (len(counts), 1, 1)), np.tile(np.eye(4, dtype=F32), (len(counts), 1, 1))
        for j, k in enumerate(counts):
            delta = (n - k + 0.5) * np.sqrt(13.0) / 500.0
            T12[j, 0, 3], T21[j, 0, 3] = delta, -delta
        return T12, T21
    return c, models


@pytest.mark.gpu
def test_scripted_counts_tie_and_event_after_event():
    orbx = _orbx()
    c, models = _depth_problem()
    script = [5, 22, 3, 22, 21, 25, 25, 0, 30, 29]      # events at 1, 3 (a tie: >= takes the later one), 5, 6 (tie), 8
    T12, T21 = models(script)
    count, inl = _handle().CheckModels(c, T12, T21)
    rc, ri = sr.check_inliers(sr.constructor(c), c["K1"], c["K2"], T12, T21)
    assert count.tolist() == script == rc.tolist() and (inl == ri).all()
    assert all((inl[j] == (np.arange(30) >= 30 - k)).all() for j, k in enumerate(script))
    ev, first, best = sr.scan_events(count, 20)
    assert np.flatnonzero(ev).tolist() == [1, 3, 5, 6, 8] and first == 1 and best == 8
    cand, out = _candidate(orbx, count, inl, 20, 30, np.arange(30), 30)
    got = []
    while True:
        T, no_more, vb, k = cand.iterate(5)
        if T is not None:
            got.append((cand.mnIterations - 1, k, vb.sum()))
        if no_more:
            break
    assert got == [(1, 22, 22), (3, 22, 22), (5, 25, 25), (6, 25, 25), (8, 30, 30)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# on the device, end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_model_end_to_end(name):
    d, b = _dev(name), _ref(name, "f64")
    ok = b["gap"] >= GAP
    if not ok.any():
        return
    dR = np.abs(d.r12.astype(F64) - b["r12"]).reshape(len(ok), -1).max(1)[ok].max()
    dt = (np.abs(d.t12.astype(F64) - b["t12"]).max(1) / np.maximum(1.0, np.linalg.norm(b["t12"], axis=1)))[ok].max()
    ds = np.abs(d.s12.astype(F64) - b["s12"])[ok].max()
    print("%s: device against the float64 form: R %.3g (bound %.3g), t %.3g (%.3g), s %.3g (%.3g)" % (name, dR, MODEL_R_BOUND, dt, MODEL_T_BOUND, ds, MODEL_S_BOUND))
    assert dR <= MODEL_R_BOUND and dt <= MODEL_T_BOUND and ds <= MODEL_S_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_first_event_end_to_end(name):
    d, a = _dev(name), _ref(name)
    assert d.first_event == a["first_event"]
    if d.first_event < 0:
        assert d.no_more
        return
    fe = d.first_event
    rot, dt, ds = sr.similarity_error(d.r12[fe], d.t12[fe], d.s12[fe], _scene(name)["truth"])
    print("%s: first event %d recovers the similarity to %.3g deg, %.3g, %.3g" % (name, fe, rot, dt, ds))
    assert rot <= FIRST_ROT_TOL and dt <= FIRST_T_TOL and ds <= FIRST_S_TOL


def _batch_args():
    cs = [_scene(n) for n in BATCH]
    mi, fs = _row(BATCH[0])[5], _row(BATCH[0])[6]
    assert all(_row(n)[5] == mi and _row(n)[6] == fs for n in BATCH)
    return cs, mi, fs


@pytest.mark.gpu
def test_batch_equals_alone():
    cs, mi, fs = _batch_args()
    alone = []
    for c in cs:
        r = _handle().Solve([c], sets=[c["sets"]], min_inliers=mi, fix_scale=fs, full=True)[0]
        r.masks = np.array([r.inliers(it) for it in range(r.iterations)], bool).reshape(r.iterations, r.n)
        alone.append(r)
    both = _handle().Solve(cs, sets=[c["sets"] for c in cs], min_inliers=mi, fix_scale=fs, full=True)
    assert _handle().last_timing()[1] == 4
    assert [b.n for b in both] == [300, 19, 100] and both[1].iterations == 0 and both[1].no_more and both[2].no_more and both[2].first_event == -1 and both[0].first_event >= 0
    for a, b in zip(alone, both):
        for k in ("r12", "t12", "s12", "x3dc1", "x3dc2", "p1im1", "p2im2", "max_err1", "max_err2", "nmat", "quat", "t12m", "t21m"):
            assert _same_bits(getattr(a, k), getattr(b, k)), k
        assert (a.count == b.count).all() and (a.is_event == b.is_event).all() and (a.inliers_first == b.inliers_first).all()
        assert (a.first_event, a.best_iteration, a.no_more) == (b.first_event, b.best_iteration, b.no_more)
        masks = np.array([b.inliers(it) for it in range(b.iterations)], bool).reshape(b.iterations, b.n)
        assert (masks == a.masks).all()


@pytest.mark.gpu
def test_round_robin_replay():
    cs, mi, fs = _batch_args()
    hits = []

    def run(solvers, stop_at):
        del hits[:]
        return sr.round_robin(solvers, lambda i, k: hits.append(i) or len(hits) == stop_at)
    for stop_at in (1, 3, 10 ** 6):      # OptimizeSim3 accepts the first Sim3; the third; never: every candidate ends on bNoMore
        cand = _handle().Solve(cs, sets=[c["sets"] for c in cs], min_inliers=mi, fix_scale=fs)
        masks = [np.array([b.inliers(it) for it in range(b.iterations)], bool).reshape(b.iterations, b.n) for b in cand]
        ref = [sr.Solver(b.count, m, b.r12, b.t12, b.s12, b.n, mi, c["indices1"], c["mN1"]) for b, m, c in zip(cand, masks, cs)]
        got, want = run(cand, stop_at), run(ref, stop_at)
        assert got == want
        successes = [e for e in got if e[4] is not None]
        assert len(successes) >= min(stop_at, 2) and all(e[0] == 0 for e in successes)
        if stop_at == 1:
            assert len(got) == 1                                                    # the first candidate's first visit ends the loop
        else:
            assert len(successes) >= 2                                              # asked again after a success
            assert (1, True, 0, (), None, None) in got                              # discarded at once: n < min_inliers
        if stop_at == 10 ** 6:
            assert sorted(e[0] for e in got if e[1]) == [0, 1, 2]                   # everybody ends on bNoMore
            assert sum(1 for e in got if e[0] == 2) == 60                           # 300 iterations, five at a time


@pytest.mark.gpu
def test_error_paths():
    orbx = _orbx()
    h = _handle()
    c = _scene("general_65")
    sets = c["sets"]

    def code(fn):
        with pytest.raises(orbx.OrbxError) as e:
            fn()
        return e.value.code
    assert code(lambda: h.Solve([c] * 5, sets=[sets] * 5)) == ERR_CAPACITY                                   # candidates
    big = sr.scene(1025, 1)
    assert code(lambda: h.Solve([big], sets=[sr.draw_sets(1025, 3, 1)])) == ERR_CAPACITY                     # matches
    assert code(lambda: h.Solve([c], sets=[sr.draw_sets(65, 301, 1)])) == ERR_CAPACITY                       # iterations
    assert code(lambda: h.Solve([], sets=[])) == ERR_ARG                                                     # ncandidates < 1
    bad = sets.copy()
    bad[3, 1] = 65
    assert code(lambda: h.Solve([c], sets=[bad])) == ERR_ARG                                                 # outside [0, n)
    bad = sets.copy()
    bad[2, 0] = -1
    assert code(lambda: h.Solve([c], sets=[bad])) == ERR_ARG
    bad = sets.copy()
    bad[6, 2] = bad[6, 0]
    assert code(lambda: h.Solve([c], sets=[bad])) == ERR_ARG                                                 # repeated inside a set
    two = sr.scene(3, 1, outliers=0.0)
    two = dict(two, world1=two["world1"][:2], world2=two["world2"][:2], sigma2_1=two["sigma2_1"][:2], sigma2_2=two["sigma2_2"][:2])
    assert code(lambda: h.Solve([two], sets=[np.array([[0, 1, 0]], np.int32)], min_inliers=1)) == ERR_ARG    # n < 3 with iterations requested
    assert code(lambda: h.CheckModels(c, np.zeros((301, 4, 4), F32), np.zeros((301, 4, 4), F32))) == ERR_CAPACITY
    assert code(lambda: h.CheckModels(c, np.zeros((0, 4, 4), F32), np.zeros((0, 4, 4), F32))) == ERR_ARG
    # the handle is still usable, and says what the restatement says
    mi, fs = _row("general_65")[5], _row("general_65")[6]
    r = h.Solve([c], sets=[sets], min_inliers=mi, fix_scale=fs)[0]
    ref = _ref("general_65")
    assert r.first_event == ref["first_event"] and (r.count == ref["count"]).all()
    assert code(lambda: r._solver._inliers(0, 7, r.n)) == ERR_ARG and code(lambda: r._solver._inliers(1, 0, r.n)) == ERR_ARG
    fresh = orbx.Sim3Solver(max_candidates=1, max_matches=64, max_iterations=8)
    assert code(lambda: fresh._inliers(0, 0, 3)) == ERR_STATE and code(fresh.last_timing) == ERR_STATE
    fresh.close()


@pytest.mark.gpu
def test_default_sets_and_determinism():
    c = _scene("general_300")
    h = _handle()
    a = h.Solve([c], rng=np.random.default_rng(7))[0]
    b = h.Solve([c], rng=np.random.default_rng(7))[0]
    assert a.iterations == sr.ransac_iterations(0.99, 20, 300, 300) == len(a.sets)
    assert (a.sets == sr.draw_sets(300, a.iterations, 7)).all()
    assert (a.count == b.count).all() and _same_bits(a.r12, b.r12) and _same_bits(a.t12, b.t12) and _same_bits(a.s12, b.s12)
    ms, launches = h.last_timing()
    assert launches == 4 and ms > 0
