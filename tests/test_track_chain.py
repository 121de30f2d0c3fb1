"""A tracked frame on the device: Tracking::TrackWithMotionModel (reference src/Tracking.cc:1370-1421) and Tracking::TrackLocalMap (:1454-1489) as
one launch chain each (orbx_track_with_motion_model / orbx_track_local_map, csrc/orbx_track.hip).

CPU: the restatement's loops against a line-by-line translation, the scenes' construction conditions through the restatement, the shim compiles.
gpu: the chains (1) equal - bit for bit, index for index, in every result field - the existing entry points composed with the restatement's glue on the
host, (2) also where the host's upper bound on the number of correspondences is loose (the pose kernel's instantiation is decided on the device), (3) equal the CPU restatement (pose to 1e-5:
orbx_pose_optimization's contract), (4) at the edges of the control flow, (5) and refuse bad arguments without a launch."""
import ctypes
import functools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import track_ref
import track_scenes as ts

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
TH = {"mono": 15.0, "stereo": 7.0, "mixed": 15.0}      # :1374-1378


# ---------------------------------------------------------------------------------------------------------------------
# the three ways to run a scene: CPU restatement, composition of the existing device calls, the chain
# ---------------------------------------------------------------------------------------------------------------------
def cpu_motion(oracle, fr, last, meta, ori=1):
    return track_ref.motion_model(lambda th: oracle_lib.search_by_projection_last(oracle, fr, last, th, meta["mono"], ori), lambda p: oracle_lib.pose_optimization(oracle, p),
                                  fr, last, meta["th"], ts.INV_SIGMA2)


def _dev_motion_args(orbx, fr, last):
    return dict(fr, kps=ts.struct_kps(orbx, fr["kps7"])), dict(last, kps=ts.struct_kps(orbx, last["kps7"]), valid=(last["valid"] == 1).astype(np.uint8))


def composed_motion(orbx, mt, po, fr, last, meta):
    frame, lastd = _dev_motion_args(orbx, fr, last)
    return track_ref.motion_model(lambda th: mt.SearchByProjectionLast(frame, lastd, th, meta["mono"]), lambda p: po.PoseOptimization([p])[0], fr, last, meta["th"], ts.INV_SIGMA2)


def chain_motion(orbx, mt, fr, last, meta):
    frame, lastd = _dev_motion_args(orbx, fr, last)
    return mt.TrackWithMotionModel(frame, lastd, meta["th"], meta["mono"], ts.INV_SIGMA2)


def _points(sc):
    return {k: sc[k] for k in ("pos", "normal", "max_distance", "min_distance", "desc", "has_obs")}


def cpu_local(oracle, fr, sc, nnratio=0.8):
    def search():
        fv = track_ref.is_in_frustum(sc["Tcw"], sc["cam"], (0.0, float(ts.W), 0.0, float(ts.H)), ts.LOG_SCALE, 8, sc)
        if len(fr["kps7"]) == 0 or len(sc["pos"]) == 0:
            return 0, np.full(len(fr["kps7"]), -1, np.int32), fv
        nm, a = oracle_lib.search_by_projection(oracle, fr, dict(fv, desc=sc["desc"], has_obs=sc["has_obs"]), sc["th"], nnratio)
        return nm, a, fv
    return track_ref.local_map(search, lambda p: oracle_lib.pose_optimization(oracle, p), fr, sc["Tcw"], sc["cam"], _points(sc), fr["held"], fr["held_pos"], ts.INV_SIGMA2,
                               sc["stereo"])


def composed_local(orbx, mt, po, fr, sc):
    frame = dict(fr, kps=ts.struct_kps(orbx, fr["kps7"]))

    def search():
        if len(fr["kps7"]) == 0:
            return 0, np.zeros(0, np.int32), None
        return mt.SearchLocalPoints(frame, sc["Tcw"], sc["cam"], ts.LOG_SCALE, _points(sc), sc["th"])
    return track_ref.local_map(search, lambda p: po.PoseOptimization([p])[0], fr, sc["Tcw"], sc["cam"], _points(sc), fr["held"], fr["held_pos"], ts.INV_SIGMA2, sc["stereo"])


def chain_local(orbx, mt, fr, sc):
    frame = dict(fr, kps=ts.struct_kps(orbx, fr["kps7"]))
    return mt.TrackLocalMap(frame, sc["Tcw"], sc["cam"], ts.LOG_SCALE, _points(sc), sc["th"], fr["held"], fr["held_pos"], ts.INV_SIGMA2, sc["stereo"])


MOTION_INTS = ("nmatches_search", "wide", "n_correspondences", "pose_inliers", "nmatches", "nmatches_map", "ran_pose")
MOTION_ARRAYS = ("matches", "search_matches", "discarded")
LOCAL_INTS = ("nmatches", "n_correspondences", "pose_inliers", "inliers_map", "inliers_all")
LOCAL_ARRAYS = ("assigned", "outlier", "found", "cleared")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.uint64)


def assert_same(got, want, ints, arrays, bits, tag=""):
    for k in ints:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    for k in arrays:
        assert len(got[k]) == len(want[k]) and (np.asarray(got[k]) == np.asarray(want[k])).all(), (tag, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[:8])
    gp, wp = np.asarray(got["pose"], np.float32), np.asarray(want["pose"], np.float32)
    if bits:
        assert (_bits(gp) == _bits(wp)).all(), (tag, "pose", np.abs(gp - wp).max())
        assert (_bits(np.asarray(got["stats"], np.float64)) == _bits(np.asarray(want["stats"], np.float64))).all(), (tag, "stats", got["stats"], want["stats"])
    else:
        assert np.abs(gp.astype(np.float64) - wp).max() <= 1e-5, (tag, "pose", np.abs(gp.astype(np.float64) - wp).max())
    if "frustum" in want and want["frustum"] is not None:
        ok = want["frustum"]["in_view"] > 0
        assert (got["frustum"]["in_view"] == want["frustum"]["in_view"]).all(), tag
        for k in ("proj_x", "proj_y", "proj_xr", "view_cos"):
            assert (_bits(got["frustum"][k][ok]) == _bits(want["frustum"][k][ok])).all(), (tag, k)
        assert (got["frustum"]["level"][ok] == want["frustum"]["level"][ok]).all(), tag


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement and the scenes
# ---------------------------------------------------------------------------------------------------------------------
def test_discard_and_statistics_loops_equal_the_reference_lines():
    rng = np.random.default_rng(5)
    for rep in range(40):
        n, nl = int(rng.integers(0, 60)), 40
        mvp = np.where(rng.random(n) < 0.6, rng.integers(0, nl, n), -1).astype(np.int32)
        outl, obs_last = (rng.random(n) < 0.4).astype(np.uint8), (rng.random(nl) < 0.7).astype(np.uint8)
        nm = int((mvp >= 0).sum()) + int(rng.integers(0, 3))
        # :1402-1421, line by line
        want_mvp, want_disc, nmatches, nmap = mvp.copy(), np.zeros(n, np.uint8), nm, 0
        for i in range(n):
            if want_mvp[i] >= 0:
                if outl[i]:
                    want_mvp[i] = -1
                    want_disc[i] = 1
                    nmatches -= 1
                elif obs_last[mvp[i]] > 0:
                    nmap += 1
        got = track_ref.discard(mvp, outl, obs_last, nm)
        assert (got[0] == want_mvp).all() and (got[1] == want_disc).all() and got[2:] == (nmatches, nmap)
        # :1460-1489, line by line
        has, observed = (mvp >= 0).astype(np.uint8), (rng.random(n) < 0.7).astype(np.uint8)
        for stereo in (0, 1):
            found, cleared, imap, iall = np.zeros(n, np.uint8), np.zeros(n, np.uint8), 0, 0
            for i in range(n):
                if has[i]:
                    if not outl[i]:
                        found[i] = 1
                        iall += 1
                        if observed[i]:
                            imap += 1
                    elif stereo:
                        cleared[i] = 1
            got = track_ref.statistics(has, outl, observed, stereo)
            assert (got[0] == found).all() and (got[1] == cleared).all() and got[2:] == (imap, iall)


@functools.lru_cache(maxsize=None)
def wide_scene():
    return ts.motion_scene(101, n_last=300, clutter=200, sensor="mono", wrong=0.0, off_px=22.0, max_octave=2)


@functools.lru_cache(maxsize=None)
def fail_scene():
    return ts.motion_scene(102, n_last=300, clutter=200, sensor="mono", wrong=0.0, off_px=120.0, max_octave=2)


@functools.lru_cache(maxsize=None)
def outlier_scene(sensor):
    return ts.motion_scene({"mono": 111, "stereo": 112, "mixed": 113}[sensor], sensor=sensor, th=TH[sensor])


@functools.lru_cache(maxsize=None)
def local_outlier_scene(sensor):
    return ts.local_scene({"mono": 121, "stereo": 122, "mixed": 123}[sensor], sensor=sensor)


def _pass1(oracle, fr, last, meta, th=None):
    return oracle_lib.search_by_projection_last(oracle, fr, last, meta["th"] if th is None else th, meta["mono"], 1)


def exact_matches_scene(oracle, target):
    """Exactly `target` matches after pass 1 (valid flags trimmed with the restatement)."""
    fr, last, meta = ts.motion_scene(131, n_last=120, clutter=100, sensor="mixed", wrong=0.0)
    return fr, ts.trim_valid(fr, last, lambda l: _pass1(oracle, fr, l, meta)[0], target), meta


BOUNDARY = (255, 256, 257, 512, 513, 1025)


@functools.lru_cache(maxsize=None)
def boundary_scene(target, loose):
    """Exactly `target` correspondences.  tight: every valid last-frame point is matched and N > target, so the host's bound min(N, valid) IS the count;
    loose: N = 2000 features and 2000 valid last-frame points (the extra ones behind the camera), so the bound - and the instantiation - is larger."""
    extra = 2000 - target if loose else 40
    return ts.motion_scene(140 + target, n_last=target, clutter=extra, behind=extra if loose else 0, sensor="mixed", clean=True)


def test_scenes_meet_their_construction_conditions(oracle):
    fr, last, meta = wide_scene()
    assert _pass1(oracle, fr, last, meta)[0] < 20 <= _pass1(oracle, fr, last, meta, 2 * meta["th"])[0]
    fr, last, meta = fail_scene()
    assert _pass1(oracle, fr, last, meta)[0] < 20 and _pass1(oracle, fr, last, meta, 2 * meta["th"])[0] < 20
    for sensor in ("mono", "stereo", "mixed"):
        fr, last, meta = outlier_scene(sensor)
        r = cpu_motion(oracle, fr, last, meta)
        assert r["ran_pose"] == 1 and r["discarded"].sum() >= 5 and r["nmatches"] >= 20 and 0 < r["nmatches_map"] < r["nmatches"], (sensor, r["discarded"].sum(), r["nmatches"])
        assert (r["search_matches"] == -2).any() or sensor != "mixed"
        fl, sc = local_outlier_scene(sensor)
        r = cpu_local(oracle, fl, sc)
        assert r["outlier"].sum() >= 5 and r["found"].sum() >= 20 and r["nmatches"] >= 20 and 0 < r["inliers_map"] < r["inliers_all"], (sensor, r["outlier"].sum(), r["found"].sum())
        assert (r["cleared"].sum() > 0) == (sensor == "stereo")
    for target in (19, 20):
        fr, last, meta = exact_matches_scene(oracle, target)
        assert _pass1(oracle, fr, last, meta)[0] == target


@pytest.mark.parametrize("target", BOUNDARY)
def test_boundary_scenes_have_exactly_their_correspondences(oracle, target):
    for loose in (False, True):
        fr, last, meta = boundary_scene(target, loose)
        nm, a = _pass1(oracle, fr, last, meta)
        assert nm == target and (a >= 0).sum() == target, (target, loose, nm)
        bound = min(len(fr["kps7"]), int((last["valid"] == 1).sum()))
        assert bound == (2000 if loose else target)


@pytest.mark.skipif(not os.access(REF / "include" / "Tracking.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-include", str(REF / "include" / "Tracking.h"), "-I" + str(ROOT / "include"), "-fsyntax-only", str(shim / "Tracking_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_makes_the_calls_it_claims_and_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "Tracking_hip.cc").read_text()
    for piece in ("orbx_track_with_motion_model(", "orbx_track_local_map(", "MapPointAccess", "shim_error.h", "orbx_shim::Fail(", "SetPose(", "IncreaseFound()", "mbTrackInView",
                  "mnLastFrameSeen", "mvbOutlier"):
        assert piece in text, piece
    assert "Tracking_hip" not in (ROOT / "oracle" / "Makefile").read_text()
    assert "Tracking_hip" in (ROOT / "INTEGRATION.md").read_text()


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _handles(ori=1):
    import importlib
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    return orbx.ORBmatcher(0.8, bool(ori), max_features=4096), orbx.PoseOptimizer(max_frames=1, max_features=4096)


@pytest.mark.gpu
@pytest.mark.parametrize("sensor", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("ori", [0, 1])
def test_motion_chain_equals_the_existing_calls(orbx, sensor, ori):
    mt, po = _handles(ori)
    fr, last, meta = outlier_scene(sensor)
    want, got = composed_motion(orbx, mt, po, fr, last, meta), chain_motion(orbx, mt, fr, last, meta)
    assert want["ran_pose"] == 1 and want["discarded"].sum() >= 5 and want["nmatches"] >= 20
    assert_same(got, want, MOTION_INTS, MOTION_ARRAYS, True, (sensor, ori))


@pytest.mark.gpu
@pytest.mark.parametrize("sensor,sensor_stereo", [("mono", 0), ("stereo", 1), ("mixed", 0), ("mixed", 1)])
def test_local_chain_equals_the_existing_calls(orbx, sensor, sensor_stereo):
    mt, po = _handles()
    fr, sc = local_outlier_scene(sensor)
    sc = dict(sc, stereo=bool(sensor_stereo))
    want, got = composed_local(orbx, mt, po, fr, sc), chain_local(orbx, mt, fr, sc)
    assert want["outlier"].sum() >= 5 and want["found"].sum() >= 20 and (want["cleared"].sum() > 0) == bool(sensor_stereo)
    assert_same(got, want, LOCAL_INTS, LOCAL_ARRAYS, True, (sensor, sensor_stereo))


@pytest.mark.gpu
@pytest.mark.parametrize("target", BOUNDARY)
def test_instantiation_boundaries(orbx, target):
    """The count is known on the device only; the host knows min(N, valid points): tight = the count itself, loose = 2000.  The chain enqueues one launch
    per instantiation of k_pose_opt up to the bound's, each gated on its range of the device count, so the counts on both sides of 256 / 512 / 1024 take
    different launches of the same chain.  (Run once with the instantiation chosen from the bound instead - eight edges per thread for 2000 - this test
    passed too: thread t owns edges t, t + 256, .., dead slots are zeros, the reduction's order is fixed.  That form cost up to 70 us)"""
    mt, po = _handles()
    for loose in (False, True):
        fr, last, meta = boundary_scene(target, loose)
        want, got = composed_motion(orbx, mt, po, fr, last, meta), chain_motion(orbx, mt, fr, last, meta)
        assert got["n_correspondences"] == target == want["n_correspondences"] and got["ran_pose"] == 1
        assert_same(got, want, MOTION_INTS, MOTION_ARRAYS, True, (target, loose))


@pytest.mark.gpu
@pytest.mark.parametrize("target", [256, 257])
def test_instantiation_boundaries_local_map(orbx, target):
    """The same for TrackLocalMap, whose bound is min(N, held + local points): `target` held features and nothing found, once alone (the bound is the
    count) and once with 1500 local points behind the camera (a larger bound: more gated launches)."""
    mt, po = _handles()
    fr, sc = ts.local_scene(150 + target, m=0, n_held=target, clutter=20, wrong=0.1)
    want, got = composed_local(orbx, mt, po, fr, sc), chain_local(orbx, mt, fr, sc)
    assert got["n_correspondences"] == target
    assert_same(got, want, LOCAL_INTS, LOCAL_ARRAYS, True, (target, "tight"))
    rng = np.random.default_rng(target)
    m = 1500
    away = dict(pos=(np.asarray(sc["Tcw"]).reshape(4, 4)[:3, :3].T @ (np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), -rng.uniform(2, 8, m)], 1)
                                                                   - np.asarray(sc["Tcw"]).reshape(4, 4)[:3, 3]).T).T.astype(np.float32),
                normal=np.tile(np.float32([0, 0, 1]), (m, 1)), max_distance=np.full(m, 10, np.float32), min_distance=np.full(m, 1, np.float32),
                desc=rng.integers(0, 256, (m, 32), dtype=np.uint8), has_obs=np.ones(m, np.uint8))
    sc2 = dict(sc, **away)
    want2, got2 = composed_local(orbx, mt, po, fr, sc2), chain_local(orbx, mt, fr, sc2)
    assert got2["n_correspondences"] == target and got2["nmatches"] == 0 and not got2["frustum"]["in_view"].any()
    assert_same(got2, want2, LOCAL_INTS, LOCAL_ARRAYS, True, (target, "loose"))
    assert (_bits(got2["pose"]) == _bits(got["pose"])).all() and (got2["outlier"] == got["outlier"]).all()      # the same problem under two bounds


@pytest.mark.gpu
@pytest.mark.parametrize("sensor", ["mono", "stereo", "mixed"])
def test_chains_equal_the_cpu_restatement(orbx, oracle, sensor):
    mt, _ = _handles()
    fr, last, meta = outlier_scene(sensor)
    assert_same(chain_motion(orbx, mt, fr, last, meta), cpu_motion(oracle, fr, last, meta), MOTION_INTS, MOTION_ARRAYS, False, sensor)
    fl, sc = local_outlier_scene(sensor)
    assert_same(chain_local(orbx, mt, fl, sc), cpu_local(oracle, fl, sc), LOCAL_INTS, LOCAL_ARRAYS, False, sensor)


@pytest.mark.gpu
def test_motion_chain_control_flow(orbx, oracle):
    mt, po = _handles()
    # the wide scene: pass 2 counts, with the matches of a 2 * th call
    fr, last, meta = wide_scene()
    got = chain_motion(orbx, mt, fr, last, meta)
    frame, lastd = _dev_motion_args(orbx, fr, last)
    nm2, a2 = mt.SearchByProjectionLast(frame, lastd, 2 * meta["th"], meta["mono"])
    assert got["wide"] == 1 and got["ran_pose"] == 1 and got["nmatches_search"] == nm2 >= 20 and (got["search_matches"] == a2).all()
    assert_same(got, composed_motion(orbx, mt, po, fr, last, meta), MOTION_INTS, MOTION_ARRAYS, True, "wide")
    # the fail scene: nothing behind the searches runs
    fr, last, meta = fail_scene()
    got = chain_motion(orbx, mt, fr, last, meta)
    assert got["ran_pose"] == 0 and got["wide"] == 1 and got["nmatches_map"] == 0 and got["pose_inliers"] == 0 and not got["discarded"].any()
    assert (_bits(got["pose"]) == _bits(np.asarray(fr["Tcw"], np.float32))).all()
    assert_same(got, composed_motion(orbx, mt, po, fr, last, meta), MOTION_INTS, MOTION_ARRAYS, True, "fail")
    # exactly 19 and exactly 20 matches after pass 1
    for target in (19, 20):
        fr, last, meta = exact_matches_scene(oracle, target)
        got = chain_motion(orbx, mt, fr, last, meta)
        assert got["wide"] == (1 if target == 19 else 0) and (got["nmatches_search"] == 20 or target == 19)
        assert_same(got, composed_motion(orbx, mt, po, fr, last, meta), MOTION_INTS, MOTION_ARRAYS, True, target)
    # no feature at all; no valid last-frame point
    fr, last, meta = outlier_scene("mixed")
    empty = dict(fr, kps7=fr["kps7"][:0], desc=fr["desc"][:0], u_right=fr["u_right"][:0], occupied=fr["occupied"][:0])
    got = chain_motion(orbx, mt, empty, last, meta)
    assert got["ran_pose"] == 0 and got["nmatches"] == 0 and len(got["matches"]) == 0 and (_bits(got["pose"]) == _bits(np.asarray(fr["Tcw"], np.float32))).all()
    none = dict(last, valid=np.zeros_like(last["valid"]))
    got = chain_motion(orbx, mt, fr, none, meta)
    assert got["ran_pose"] == 0 and got["wide"] == 1 and got["nmatches_search"] == 0 and (got["matches"] == -1).all() and (got["search_matches"] == -1).all()
    assert_same(got, composed_motion(orbx, mt, po, fr, none, meta), MOTION_INTS, MOTION_ARRAYS, True, "no valid point")


@pytest.mark.gpu
def test_local_chain_control_flow(orbx):
    mt, po = _handles()

    def both(fr, sc, tag):
        want, got = composed_local(orbx, mt, po, fr, sc), chain_local(orbx, mt, fr, sc)
        assert_same(got, want, LOCAL_INTS, LOCAL_ARRAYS, True, tag)
        return got
    # no local point: the held features alone; 1 and 2 correspondences take k_pose_opt's n < 3 path (the pose comes back unchanged)
    for n_held in (1, 2, 150):
        fr, sc = ts.local_scene(160 + n_held, m=0, n_held=n_held, clutter=50)
        got = both(fr, sc, ("held only", n_held))
        assert got["n_correspondences"] == n_held and got["nmatches"] == 0
        if n_held < 3:
            assert got["pose_inliers"] == 0 and (_bits(got["pose"]) == _bits(sc["Tcw"])).all() and not got["outlier"].any()
    # nothing held
    fr, sc = ts.local_scene(171, m=400, n_held=0, clutter=200)
    got = both(fr, sc, "nothing held")
    assert got["n_correspondences"] == (got["assigned"] >= 0).sum() >= 20
    # every correspondence an outlier: forty features far apart all hold ONE world point, which projects to one pixel under any pose - at most one of them can fit
    fr, sc = ts.local_scene(172, m=0, n_held=40, clutter=0, wrong=0.0)
    fr = dict(fr, held_pos=np.tile(fr["held_pos"][np.flatnonzero(fr["held"])[0]], (len(fr["held"]), 1)))
    got = both(fr, sc, "all outliers")
    assert got["n_correspondences"] == 40 and got["outlier"].sum() >= 39 and got["pose_inliers"] == 40 - got["outlier"].sum()
    # no feature at all: the frustum test still runs
    fr, sc = local_outlier_scene("mixed")
    empty = dict(fr, kps7=fr["kps7"][:0], desc=fr["desc"][:0], u_right=fr["u_right"][:0], occupied=fr["occupied"][:0], held=fr["held"][:0], held_pos=fr["held_pos"][:0])
    got = chain_local(orbx, mt, empty, sc)
    want = track_ref.is_in_frustum(sc["Tcw"], sc["cam"], (0.0, float(ts.W), 0.0, float(ts.H)), ts.LOG_SCALE, 8, sc)
    assert got["n_correspondences"] == 0 and (got["frustum"]["in_view"] == want["in_view"]).all() and want["in_view"].sum() > 20
    assert (_bits(got["pose"]) == _bits(sc["Tcw"])).all()


@pytest.mark.gpu
def test_no_state_is_left_between_calls(orbx, oracle):
    """Two chain calls in a row on one handle with different sizes, an existing entry point of the matcher in between, and both chains interleaved."""
    mt, po = _handles()
    big, small = outlier_scene("mixed"), ts.motion_scene(181, n_last=90, clutter=30, sensor="stereo", th=7.0)
    want_big, want_small = composed_motion(orbx, mt, po, *big), composed_motion(orbx, mt, po, *small)
    fl, sc = local_outlier_scene("stereo")
    want_local = composed_local(orbx, mt, po, fl, sc)
    frame, lastd = _dev_motion_args(orbx, big[0], big[1])
    for step in range(2):
        assert_same(chain_motion(orbx, mt, *big), want_big, MOTION_INTS, MOTION_ARRAYS, True, ("big", step))
        assert_same(chain_motion(orbx, mt, *small), want_small, MOTION_INTS, MOTION_ARRAYS, True, ("small", step))
        nm, a = mt.SearchByProjectionLast(frame, lastd, 15.0, False)
        assert nm == want_big["nmatches_search"] and (a == want_big["search_matches"]).all()
        assert_same(chain_local(orbx, mt, fl, sc), want_local, LOCAL_INTS, LOCAL_ARRAYS, True, ("local", step))
    assert_same(chain_motion(orbx, mt, *wide_scene()), composed_motion(orbx, mt, po, *wide_scene()), MOTION_INTS, MOTION_ARRAYS, True, "wide after")


@pytest.mark.gpu
def test_bad_arguments_are_errors_not_launches(orbx):
    mt, _ = _handles()
    L = mt._L
    fr, last, meta = outlier_scene("mixed")
    # nlevels out of range (the wrapper passes len(scale_factors))
    frame, lastd = _dev_motion_args(orbx, fr, last)
    with pytest.raises(orbx.OrbxError) as e:
        mt.TrackWithMotionModel(dict(frame, scale_factors=np.ones(65, np.float32)), lastd, 15.0, False, np.ones(65, np.float32))
    assert e.value.code == -1
    # NULL arguments
    for fn, nargs in ((L.orbx_track_with_motion_model, 10), (L.orbx_track_local_map, 14)):
        fn.argtypes = None
        fn.restype = ctypes.c_int
        args = [mt._h] + [ctypes.c_void_p(None)] * (nargs - 1)
        if nargs == 10:
            args[4], args[6], args[7], args[8] = 8, ctypes.c_float(15.0), 0, 1
        else:
            args[5], args[6], args[7], args[8], args[12] = 8, ctypes.c_float(0.5), ctypes.c_float(3.0), ctypes.c_float(0.8), 0
        assert fn(*args) == -1 and len(L.orbx_last_error()) > 0
    fl, sc = local_outlier_scene("mixed")
    with pytest.raises(orbx.OrbxError) as e:      # the frustum arguments and the scale factors must name the same levels, 1..12
        mt.TrackLocalMap(dict(fl, kps=ts.struct_kps(orbx, fl["kps7"]), scale_factors=np.ones(13, np.float32)), sc["Tcw"], sc["cam"], ts.LOG_SCALE, _points(sc), 3.0, fl["held"],
                         fl["held_pos"], np.ones(13, np.float32), False)
    assert e.value.code == -1
    # more than 8192 possible correspondences: refused before anything is staged or launched
    big = orbx.ORBmatcher(0.8, True, max_features=9000)
    n = 8200
    rng = np.random.default_rng(9)
    k7 = np.zeros((n, 7), np.float32)
    k7[:, 0], k7[:, 1], k7[:, 2], k7[:, 6] = rng.uniform(5, 635, n), rng.uniform(5, 475, n), 31, -1
    frb = dict(kps7=k7, kps=ts.struct_kps(orbx, k7), desc=np.zeros((n, 32), np.uint8), u_right=np.full(n, -1, np.float32), occupied=np.zeros(n, np.uint8), scale_factors=ts.SCALES,
               width=ts.W, height=ts.H, Tcw=np.eye(4, dtype=np.float32), cam=ts.CAM)
    lastb = dict(Tcw=np.eye(4, dtype=np.float32), valid=np.ones(n, np.uint8), pos=np.ones((n, 3), np.float32), desc=np.zeros((n, 32), np.uint8), has_obs=np.ones(n, np.uint8),
                 kps=ts.struct_kps(orbx, k7))
    with pytest.raises(orbx.OrbxError) as e:
        big.TrackWithMotionModel(frb, lastb, 15.0, True, ts.INV_SIGMA2)
    assert e.value.code == -3
    with pytest.raises(orbx.OrbxError) as e:
        big.TrackLocalMap(frb, np.eye(4, dtype=np.float32), ts.CAM, ts.LOG_SCALE, dict(pos=np.zeros((0, 3), np.float32), normal=np.zeros((0, 3), np.float32),
                          max_distance=np.zeros(0, np.float32), min_distance=np.zeros(0, np.float32), desc=np.zeros((0, 32), np.uint8), has_obs=np.zeros(0, np.uint8)),
                          3.0, np.ones(n, np.uint8), np.ones((n, 3), np.float32), ts.INV_SIGMA2, False)
    assert e.value.code == -3
    big.close()
    # the handle still works
    assert chain_motion(orbx, mt, fr, last, meta)["ran_pose"] == 1
