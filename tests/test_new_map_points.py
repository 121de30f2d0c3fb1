"""New map points on the device: the per-match geometry of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:423-596,
orbx_triangulate_matches) and the chain over the neighbour keyframes (orbx_create_new_map_points), against tests/triangulate_ref.py.

Contract: status exact on every match that does not sit on a threshold (`near`, at most 5 % of a scene); x3d of the stereo paths bit-equal;
x3d of the triangulation path within X3D_BOUND of the float64-SVD restatement, relative to the point's distance from KF1's centre; the
created list = the accepted slots in (neighbour, idx1) order; the chain = the sequential loop over the CPU restatement of
SearchForTriangulation, the restated geometry and the mask update."""
import ctypes
import functools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import triangulate_ref as tr

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
ERR_ARG, ERR_CAPACITY, ERR_NODEVICE = -1, -3, -4

# Largest error of a FLOAT32 SVD (numpy.linalg.svd on the float32 A) against the float64 SVD over the accepted triangulated matches of
# PAIR_SCENES, relative to the point's distance from KF1's centre, times 4 (half an ulp per coordinate before any algorithm error; the
# reference's own float Jacobi is no more accurate than LAPACK's).  Measured: 1.27e-7 -> 5.1e-7.
# test_x3d_bound_is_the_measured_one recomputes it.
X3D_MEASURED = 1.27e-7
X3D_BOUND = 4 * X3D_MEASURED
JACOBI_SWEEPS = 6       # TRI_JACOBI_SWEEPS of csrc/orbx_triangulate.hip

# (name, pair_scene arguments).  Feature counts 1 / 63 / 64 / 65 / 300 / 1000: one lane, a wave less one, a wave, a wave and one, two
# workgroups, four.  "through": KF2 stands beyond the points (they are behind it: z2 <= 0 on the stereo path).
PAIR_SCENES = [
    ("side_mono_300", dict(seed=1, n=300, baseline="side")),
    ("forward_mono_1000", dict(seed=2, n=1000, baseline="forward")),
    ("short_mono_65", dict(seed=3, n=65, baseline="short")),
    ("side_mixed_64", dict(seed=4, n=64, baseline="side", stereo_frac=0.5)),
    ("short_mixed_300", dict(seed=5, n=300, baseline="short", stereo_frac=0.5)),
    ("short_stereo_63", dict(seed=6, n=63, baseline="short", stereo_frac=1.0)),
    ("forward_stereo_300", dict(seed=7, n=300, baseline="forward", stereo_frac=1.0)),
    ("through_stereo_300", dict(seed=8, n=300, baseline=(0.0, 0.0, -12.0), stereo_frac=1.0)),
    ("axis_mono_300", dict(seed=9, n=300, baseline="axis")),
    ("tiny_stereo_noisy_kf2_300", dict(seed=11, n=300, baseline="tiny", stereo_frac=1.0, noise=0.05, noise2=3.0, depth=(3.0, 5.0), wrong=0.0)),      # (the chi2 test of KF2)
    ("one_feature", dict(seed=10, n=1, baseline="side", wrong=0.0)),
]
# near-degenerate geometry for the sweep count only: points 100 baselines away, motion along the optical axis, parallax at the 0.9998 bound
DEGENERATE_SCENES = [
    dict(seed=21, n=1000, baseline="far", depth=(0.3, 0.5), noise=0.05, stereo_frac=1.0, mbf=0.4),      # (a stereo flag lifts the 0.9998 gate)
    dict(seed=22, n=1000, baseline="axis", noise=0.1),
    dict(seed=23, n=1000, baseline=(0.1, 0.0, 0.0), depth=(4.9, 5.1), noise=0.02),      # atan(0.1 / 5) = 0.02 rad: cos = 0.9998
]
# (name, chain_scene arguments): KF1 sizes 1, 63, 64, 65, 300, 1000; K = 1, 3, 20; mono / mixed / all stereo; a neighbour without
# features; a pair without matches (see _chain).  Seeds: no match of a neighbour before the last sits on a threshold
# (test_chain_scenes_are_screened) and, for "order", the sequential chain differs from independent pairs.
CHAIN_SCENES = [
    ("one", dict(seed=100, n=1, K=1)),
    ("n63_mono", dict(seed=101, n=63, K=3)),
    ("n64_mixed", dict(seed=102, n=64, K=3, stereo_frac=0.5)),
    ("n65_stereo", dict(seed=203, n=65, K=3, stereo_frac=1.0)),
    ("order", dict(seed=104, n=300, K=3, baselines=["side", "side", "forward"])),
    ("n1000_mono", dict(seed=4005, n=1000, K=3)),
    ("k20", dict(seed=306, n=300, K=20)),
    ("empty_neighbour", dict(seed=107, n=300, K=3, n2=[300, 0, 300])),
    ("no_matches", dict(seed=108, n=65, K=2)),
]


@functools.lru_cache(maxsize=None)
def _orbx():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd")


@functools.lru_cache(maxsize=None)
def _pair(name):
    kw = dict(PAIR_SCENES)[name]
    p = tr.pair_scene(_orbx(), **kw)
    return p, tr.triangulate(p["g1"], p["g2"], p["o1"], p["o2"], p["idx1"], p["idx2"])


@functools.lru_cache(maxsize=None)
def _handmade():
    """pairs made on purpose: w == 0, depth <= 0 on a stereo flag, dist == 0, a point behind each camera; ten matches of each"""
    orbx = _orbx()
    pairs = []
    # w == 0: both optical centres' rays through the principal points and a second "pose" whose third row is sheared (not a rotation): the rays
    # are 5.7 degrees apart (cos 0.995 < 0.9998: triangulate) and the third column of A is exactly 0, so the null vector is (0, 0, 1, 0)
    # (translations at which LAPACK's float64 SVD returns that vector with an exact 0 too; at tx = 0.3 it returns w = -4.9e-32)
    for i in range(1, 11):
        T2 = np.eye(4)
        T2[2, 0], T2[0, 3], T2[1, 3] = 0.1, 0.3 + 0.05 * i, 0.1
        g1, g2 = tr.make_geom(np.eye(4)), tr.make_geom(T2)
        k = np.zeros(1, orbx.KEYPOINT_DTYPE)
        k["x"], k["y"] = 320, 240
        o = dict(kps=k, raw=None, u_right=None, depth=None)
        pairs.append(dict(g1=g1, g2=g2, o1=o, o2=dict(o), idx1=np.zeros(1, np.int32), idx2=np.zeros(1, np.int32)))
    # depth <= 0 under a stereo flag: cos(2 atan2(mb/2, -0.05)) is far below the rays' cosine, so UnprojectStereo of KF1 is chosen and fails
    p = tr.pair_scene(orbx, seed=31, n=64, baseline="short", stereo_frac=1.0, wrong=0.0)
    p["o1"] = dict(p["o1"], depth=p["o1"]["depth"].copy())
    p["o1"]["depth"][p["idx1"][:12]] = -0.05
    pairs.append(p)
    # dist == 0: KF2's centre put onto the point that KF1's stereo observation unprojects to (the centre enters nothing before the scale test)
    q = tr.pair_scene(orbx, seed=32, n=64, baseline="short", stereo_frac=1.0, wrong=0.0, noise=0.1)
    r = tr.triangulate(q["g1"], q["g2"], q["o1"], q["o2"], q["idx1"], q["idx2"])
    for j in np.nonzero(r["status"] == tr.STEREO1)[0][:10]:
        pairs.append(dict(q, g2=dict(q["g2"], center=r["x3d"][j].copy()), idx1=q["idx1"][j:j + 1], idx2=q["idx2"][j:j + 1]))
    # behind KF1: swapped correspondences of a sideways pair triangulate behind the cameras; behind KF2: the "through" scene
    pairs.append(tr.pair_scene(orbx, seed=33, n=64, baseline="side", wrong=1.0))
    pairs.append(tr.pair_scene(orbx, seed=34, n=64, baseline=(0.0, 0.0, -12.0), stereo_frac=1.0, wrong=0.0))
    pairs.append(dict(pairs[-1], idx1=np.zeros(0, np.int32), idx2=np.zeros(0, np.int32)))      # a pair without matches inside the CSR
    return pairs, tr.restate_pairs(pairs)


@functools.lru_cache(maxsize=None)
def _chain(name):
    kw = dict(CHAIN_SCENES)[name]
    sc = tr.chain_scene(_orbx(), **kw)
    if name == "no_matches":      # the second neighbour's descriptors are unrelated: nothing within TH_LOW
        nb = sc["neighbours"][1]
        nb["desc"] = np.random.default_rng(5).integers(0, 256, nb["desc"].shape, dtype=np.uint8)
    return sc


@functools.lru_cache(maxsize=None)
def _chain_want(name, sequential=True):
    return tr.expected_chain(oracle_lib, oracle_lib.Oracle(), _chain(name), sequential=sequential)


def _accepted(status):
    return (status >= tr.TRIANGULATED) & (status <= tr.STEREO2)


def _rel_err(a, b, dist):
    return np.linalg.norm(a.astype(np.float64) - b.astype(np.float64), axis=-1) / dist


# ---------------------------------------------------------------------------------------------------------------------------------------
# without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_null_arguments_are_errors(orbx):
    L = orbx.load_library()
    for sym in ("orbx_triangulate_matches", "orbx_create_new_map_points", "orbx_new_points_last_timing"):
        assert hasattr(L, sym), sym
    L.orbx_triangulate_matches.argtypes = [ctypes.c_void_p] * 4
    L.orbx_create_new_map_points.argtypes = [ctypes.c_void_p] * 6
    L.orbx_new_points_last_timing.argtypes = [ctypes.c_void_p] * 4
    assert L.orbx_triangulate_matches(None, None, None, None) == ERR_ARG
    assert L.orbx_create_new_map_points(None, None, None, None, None, None) == ERR_ARG
    assert L.orbx_new_points_last_timing(None, None, None, None) == ERR_ARG
    assert hasattr(orbx.ORBmatcher, "TriangulateMatches") and hasattr(orbx.ORBmatcher, "CreateNewMapPoints")


def test_no_cpu_fallback(orbx):
    """the calls take an orbx_matcher, and a matcher cannot be made without a device"""
    import torch
    if torch.cuda.is_available():
        orbx.ORBmatcher(0.6, False, max_features=64).close()
    else:
        with pytest.raises(orbx.OrbxError) as e:
            orbx.ORBmatcher(0.6, False, max_features=64)
        assert e.value.code == ERR_NODEVICE


@pytest.mark.skipif(not os.access(REF / "include" / "LocalMapping.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-DOPTIMIZER_H", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "LocalMapping_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    assert "int CreateNewMapPoints(LocalMapping *lm);" in (shim / "LocalMapping_hip.h").read_text()
    assert "orbx_create_new_map_points(" in (shim / "LocalMapping_hip.cc").read_text()
    assert "LocalMapping_hip" not in (ROOT / "oracle" / "Makefile").read_text()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement and the scenes (CPU)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in PAIR_SCENES])
def test_pair_scenes_are_screened(name):
    _, r = _pair(name)
    assert r["near"].sum() <= 0.05 * len(r["near"]), (int(r["near"].sum()), len(r["near"]))      # (under 20 matches: none)


def test_handmade_cases_take_their_branches():
    pairs, r = _handmade()
    h = np.bincount(r["status"], minlength=13)
    print(dict(zip(tr.NAMES, h)))
    for code in (tr.W_ZERO, tr.DEPTH_INVALID, tr.DIST_ZERO, tr.BEHIND1, tr.BEHIND2):
        assert h[code] >= 10, (tr.NAMES[code], h)
    assert (r["status"][:10] == tr.W_ZERO).all()
    assert r["near"].sum() <= 0.05 * len(r["near"])


def test_status_histogram_covers_every_branch():
    h = np.zeros(13, np.int64)
    for name, _ in PAIR_SCENES:
        h += np.bincount(_pair(name)[1]["status"], minlength=13)
    h += np.bincount(_handmade()[1]["status"], minlength=13)
    print(dict(zip(tr.NAMES, h)))
    for code in range(tr.TRIANGULATED, 13):      # the three accepting paths and every rejecting `continue`
        assert h[code] >= 10, (tr.NAMES[code], h)


def test_x3d_bound_is_the_measured_one():
    worst = 0.0
    for name, _ in PAIR_SCENES:
        _, r = _pair(name)
        m = r["status"] == tr.TRIANGULATED
        if m.any():
            worst = max(worst, float(_rel_err(r["x3d"][m], r["x3d32"][m], r["dist1"][m]).max()))
    print("float32 SVD against float64 SVD, relative to the distance: %.3g" % worst)
    assert X3D_MEASURED / 1.25 <= worst <= X3D_MEASURED * 1.25
    assert X3D_BOUND == 4 * X3D_MEASURED


def test_jacobi_sweeps_settled():
    """the device's Jacobi (restated in float64): the result stops changing two sweeps before JACOBI_SWEEPS, on the test scenes and on
    near-degenerate ones, and agrees with the float64 SVD far inside the bound"""
    orbx = _orbx()
    scenes = [_pair(n)[0] for n, _ in PAIR_SCENES] + [tr.pair_scene(orbx, **kw) for kw in DEGENERATE_SCENES]
    total = 0
    for p in scenes:
        want = tr.triangulate(p["g1"], p["g2"], p["o1"], p["o2"], p["idx1"], p["idx2"])
        got = {s: tr.triangulate(p["g1"], p["g2"], p["o1"], p["o2"], p["idx1"], p["idx2"], null_vector=lambda A, s=s: tr.jacobi_null(A, s))
               for s in (JACOBI_SWEEPS - 2, JACOBI_SWEEPS)}
        a, b = got[JACOBI_SWEEPS - 2], got[JACOBI_SWEEPS]
        assert np.array_equal(a["status"], b["status"])
        assert np.array_equal(a["x3d"].view(np.uint32), b["x3d"].view(np.uint32))
        m = (want["status"] == tr.TRIANGULATED) & (b["status"] == tr.TRIANGULATED)
        total += int(m.sum())
        if m.any():
            assert _rel_err(b["x3d"][m], want["x3d"][m], want["dist1"][m]).max() <= X3D_BOUND
        ok = ~want["near"]
        assert np.array_equal(b["status"][ok], want["status"][ok])
    assert total > 1000


@pytest.mark.parametrize("name", [n for n, _ in CHAIN_SCENES])
def test_chain_scenes_are_screened(oracle, name):
    """no match of a neighbour before the last sits on a threshold (its outcome would change the later searches), the last neighbour's
    are left out of the comparison, at most 5 % of them"""
    w = _chain_want(name)
    K = len(w["nmatches"])
    assert w["near"][:K - 1].sum() == 0
    assert w["near"][K - 1].sum() <= 0.05 * int(w["nmatches"][K - 1])
    if name == "no_matches":
        assert w["nmatches"][0] > 0 and w["nmatches"][1] == 0
    elif name == "empty_neighbour":
        assert w["nmatches"][1] == 0 and w["nmatches"][2] > 0
    elif name != "one":
        assert w["nmatches"][0] > 10 and len(w["created"]) > 5


def test_chain_depends_on_the_order(oracle):
    """a feature of KF1 that got its point from neighbour k is gone for neighbour k+1, and the KF2 feature it would have taken is free for
    another: K independent searches on the initial mask give other matches for a later neighbour"""
    seq, par = _chain_want("order"), _chain_want("order", False)
    assert np.array_equal(seq["matches"][0], par["matches"][0])
    later = (seq["matches"][1:] != par["matches"][1:])
    assert later.any()
    created1 = [c[1] for c in seq["created"] if c[0] == 0]
    assert (seq["matches"][1:, created1] == -1).all() and (par["matches"][1:, created1] >= 0).any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------------------------
def _check_geometry(got, want):
    ok = ~want["near"]
    print("near: %d of %d; status histogram %s" % (int(want["near"].sum()), len(ok), dict(zip(tr.NAMES, np.bincount(want["status"], minlength=13)))))
    assert np.array_equal(got["status"][ok], want["status"][ok]), np.nonzero(got["status"] != want["status"])[0]
    st = ok & ((want["status"] == tr.STEREO1) | (want["status"] == tr.STEREO2))
    assert np.array_equal(got["x3d"][st].view(np.uint32), want["x3d"][st].view(np.uint32))
    t = ok & (want["status"] == tr.TRIANGULATED)
    if t.any():
        e = _rel_err(got["x3d"][t], want["x3d"][t], want["dist1"][t])
        print("triangulated x3d against the float64 SVD: max %.3g, median %.3g (bound %.3g)" % (e.max(), np.median(e), X3D_BOUND))
        assert e.max() <= X3D_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in PAIR_SCENES])
def test_triangulate_matches(orbx, name):
    p, want = _pair(name)
    mt = orbx.ORBmatcher(0.6, False, max_features=1024)
    got = mt.TriangulateMatches([p])
    _check_geometry(got, want)


@pytest.mark.gpu
def test_triangulate_matches_ragged_pairs(orbx):
    """all the scenes as one call (CSR over the pairs) and the hand-made cases, a pair without matches among them"""
    pairs = [_pair(n)[0] for n, _ in PAIR_SCENES]
    want = {k: np.concatenate([_pair(n)[1][k] for n, _ in PAIR_SCENES]) for k in ("status", "x3d", "near", "dist1")}
    mt = orbx.ORBmatcher(0.6, False, max_features=1024)
    got = mt.TriangulateMatches(pairs)
    assert got["offset"][-1] == len(want["status"])
    _check_geometry(got, want)
    hp, hw = _handmade()
    got = mt.TriangulateMatches(hp)
    _check_geometry(got, hw)
    assert (got["status"][:10] == tr.W_ZERO).all() and (got["x3d"][:10] == 0).all()


def _check_chain(got, want, K, n1):
    assert got["pairs_done"] == K
    assert np.array_equal(got["nmatches"], want["nmatches"])
    assert np.array_equal(got["matches"], want["matches"][:, :n1])
    ok = ~want["near"][:, :n1]
    assert np.array_equal(got["status"][ok], want["status"][:, :n1][ok])
    # the created list = the accepted slots of the status array in (neighbour, idx1) order
    kk, ii = np.nonzero(_accepted(got["status"]))
    c = got["created"]
    assert got["count"] == len(kk) == len(c)
    assert np.array_equal(c["neighbour"], kk) and np.array_equal(c["idx1"], ii)
    assert np.array_equal(c["idx2"], got["matches"][kk, ii]) and np.array_equal(c["path"], got["status"][kk, ii])
    xyz = np.stack([c["x"], c["y"], c["z"]], 1) if len(c) else np.zeros((0, 3), np.float32)
    assert np.array_equal(xyz.view(np.uint32), got["x3d"][kk, ii].view(np.uint32))
    # ... and equals the expected one where no near match is involved
    wl = [e for e in want["created"] if not want["near"][e[0], e[1]]]
    gl = [(int(e["neighbour"]), int(e["idx1"]), int(e["idx2"]), int(e["path"])) for e in c if not want["near"][e["neighbour"], e["idx1"]]]
    assert gl == [e[:4] for e in wl]
    for e, g in zip(wl, [e for e in c if not want["near"][e["neighbour"], e["idx1"]]]):
        gx, wx = np.array([g["x"], g["y"], g["z"]], np.float32), np.array(e[4:], np.float32)
        if e[3] == tr.TRIANGULATED:
            d1 = np.linalg.norm(wx.astype(np.float64))      # KF1 sits at the origin in the chain scenes
            assert np.linalg.norm(gx.astype(np.float64) - wx.astype(np.float64)) / d1 <= X3D_BOUND
        else:
            assert np.array_equal(gx.view(np.uint32), wx.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in CHAIN_SCENES])
def test_chain(orbx, oracle, name):
    sc, want = _chain(name), _chain_want(name)
    n1, K = len(sc["kf1"]["kps"]), len(sc["neighbours"])
    mt = orbx.ORBmatcher(0.6, False, max_features=max(n1, sc["cap2"], 64))
    got = mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"])
    _check_chain(got, want, K, n1)
    ms, launches, _ = mt.new_points_last_timing()
    assert launches == 4 * K + 1 and ms > 0
    again = mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"], full=False)      # the handle's buffers are reused; the list alone
    assert again["count"] == got["count"] and np.array_equal(again["created"], got["created"])


@pytest.mark.gpu
def test_chain_with_spare_capacity(orbx, oracle):
    """KF1's feature set wider than its feature count (capacity 77 for 63 features, not a multiple of 8; the neighbours 80 for 63): the
    staging keeps capacity-sized device arrays behind count-sized host arrays, the slot stride exceeds n1"""
    sc, want = _chain("n63_mono"), _chain_want("n63_mono")
    mt = orbx.ORBmatcher(0.6, False, max_features=128)
    got = mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"], capacity1=77, capacity2=80)
    _check_chain(got, want, 3, 63)


@pytest.mark.gpu
def test_chain_stops_when_a_keyframe_waits(orbx, oracle):
    """stop_flag set before the call: the first neighbour runs (the reference checks for i > 0 only), the others do not"""
    sc = _chain("order")
    want = tr.expected_chain(oracle_lib, oracle, sc, stop_after=1)
    n1, K = len(sc["kf1"]["kps"]), len(sc["neighbours"])
    mt = orbx.ORBmatcher(0.6, False, max_features=max(n1, sc["cap2"]))
    flag = np.ones(1, np.uint8)
    got = mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"], stop_flag=flag)
    assert flag[0] == 1
    assert got["pairs_done"] == 1 and (got["nmatches"][1:] == 0).all() and (got["matches"][1:] == -1).all() and (got["status"][1:] == 0).all()
    assert got["nmatches"][0] == want["nmatches"][0] and np.array_equal(got["matches"][0], want["matches"][0])
    assert got["count"] == len([e for e in want["created"] if e[0] == 0])
    assert mt.new_points_last_timing()[1] == 5


@pytest.mark.gpu
def test_capacity_and_argument_errors(orbx):
    sc = _chain("n63_mono")
    mt = orbx.ORBmatcher(0.6, False, max_features=64)
    with pytest.raises(orbx.OrbxError) as e:      # a neighbour set wider than the matcher
        mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"], capacity2=65)
    assert e.value.code == ERR_CAPACITY
    with pytest.raises(orbx.OrbxError) as e:      # the created list may need one entry per KF1 feature
        mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"], created_capacity=10)
    assert e.value.code == ERR_CAPACITY
    bad = dict(sc["kf1"], g=dict(sc["kf1"]["g"], scale_factors=np.ones(13, np.float32), level_sigma2=np.ones(13, np.float32)))
    with pytest.raises(orbx.OrbxError) as e:      # more pyramid levels than the tables hold
        mt.CreateNewMapPoints(bad, sc["neighbours"])
    assert e.value.code == ERR_ARG
    p = dict(_pair("side_mixed_64")[0])
    p["idx2"] = p["idx2"].copy()
    p["idx2"][0] = 64
    with pytest.raises(orbx.OrbxError) as e:      # a match past the end of KF2
        mt.TriangulateMatches([p])
    assert e.value.code == ERR_ARG
    got = mt.TriangulateMatches([_pair("side_mono_300")[0]])      # the geometry alone is not sized by the matcher's max_features
    assert np.array_equal(got["status"][~_pair("side_mono_300")[1]["near"]], _pair("side_mono_300")[1]["status"][~_pair("side_mono_300")[1]["near"]])
    L = orbx.load_library()
    L.orbx_create_new_map_points.argtypes = [ctypes.c_void_p] * 6
    assert L.orbx_create_new_map_points(mt._h, None, None, None, None, None) == ERR_ARG
    L.orbx_triangulate_matches.argtypes = [ctypes.c_void_p] * 4
    assert L.orbx_triangulate_matches(mt._h, None, None, None) == ERR_ARG
    got = mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"])      # the handle still works
    assert got["pairs_done"] == 3
