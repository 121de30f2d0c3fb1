"""Covisibility on the device (csrc/orbx_covis.hip, orbx_covis_*, Covisibility) against tests/covis_ref.py, a literal restatement of the counting in
KeyFrame::UpdateConnections, Tracking::UpdateLocalKeyFrames and LocalMapping::KeyFrameCulling.  CPU tests: the restatement on hand-made cases, the vacuity
guards of the scenes, the restatement against the compiled reference, the ABI without a device, the shim.  GPU tests: every field of every result equals
the restatement: integers, no tolerance, no excluded case."""
import ctypes
import functools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import covis_ref as cr
import covis_scenes as cs
from test_initializer import REF, ROOT

ERR_ARG, ERR_CAPACITY, ERR_NODEVICE = -1, -3, -4
CONN_FIELDS = ("counter_offset", "counter_kf", "counter_weight", "n_max", "kf_max", "conn_offset", "conn_kf", "conn_weight")
CULL_FIELDS = ("n_mps", "n_redundant", "culled", "point_bad", "point_obs")


def _gpu():
    import torch
    return torch.cuda.is_available()


@functools.lru_cache(maxsize=None)
def _orbx():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd")


def _same(got, want, fields, where):
    for k in fields:
        g, w = np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
        assert len(g) == len(w) and (g.astype(np.int64) == w.astype(np.int64)).all(), (where, k, g[:40], w[:40])


# ---------------------------------------------------------------------------------------------------------------------
# the restatement on hand-made cases (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def _shared(weights, ranks=None, bad_points=(), dup=0, flags=None, frame=False):
    """slot 0 owns the list; slot k >= 1 shares weights[k - 1] distinct points with it (point p is seen by every k with weights[k - 1] > p)"""
    NK = len(weights) + 1
    kfs = [[] for _ in range(NK)]
    for p in range(max(list(weights) + [1])):
        kfs[0].append((p, 0, 0))
        for k, w in enumerate(weights):
            if w > p:
                kfs[k + 1].append((p, 0, 0))
    entries = list(kfs[0]) + [kfs[0][0]] * dup
    kfs[0] = entries
    bad = np.zeros(max(list(weights) + [1]), np.uint8)
    bad[list(bad_points)] = 1
    return _orbx().covis_slice(kfs, lists=[(-1, entries) if frame else 0], n_points=len(bad), point_bad=bad, ranks=ranks, flags=flags)


def test_restated_threshold_fallback_and_ties():
    r = cr.update_connections_list(_shared([14, 15, 16, 3]), 0)
    assert r["counter"] == [(1, 14), (2, 15), (3, 16), (4, 3)] and (r["n_max"], r["kf_max"]) == (16, 3)
    assert r["conn"] == [(3, 16), (2, 15)]                                  # 14 stays out, 15 is in
    r = cr.update_connections_list(_shared([14, 9, 14]), 0)
    assert r["conn"] == [(1, 14)] and (r["n_max"], r["kf_max"]) == (14, 1)    # nothing reaches th: the single best, the FIRST of the tie in map order
    r = cr.update_connections_list(_shared([14, 9, 14], ranks=[50, 40, 30, 20]), 0)
    assert r["counter"] == [(3, 14), (2, 9), (1, 14)] and r["conn"] == [(3, 14)] and r["kf_max"] == 3      # ... which is the lowest RANK, not the lowest slot
    r = cr.update_connections_list(_shared([20, 17, 20, 17, 20], ranks=[0, 5, 1, 4, 2, 3]), 0)
    assert (r["n_max"], r["kf_max"]) == (20, 5)                               # arg-max: lowest rank of the tie (slot 5 has rank 3, slots 3 and 1 ranks 4 and 5)
    assert r["conn"] == [(1, 20), (3, 20), (5, 20), (4, 17), (2, 17)]         # ordered list: highest rank first within a weight
    assert cr.update_connections_list(_shared([20, 17]), 0, 21)["conn"] == [(1, 20)] and cr.update_connections_list(_shared([20, 17]), 0, 17)["conn"] == [(1, 20), (2, 17)]


def test_restated_duplicate_bad_and_empty():
    r = cr.update_connections_list(_shared([15], dup=1), 0)
    assert r["counter"] == [(1, 16)]                                          # both entries of a repeated point count
    r = cr.update_connections_list(_shared([15], bad_points=(0, 3)), 0)
    assert r["counter"] == [(1, 13)] and r["conn"] == [(1, 13)]               # bad points are skipped
    s = _orbx().covis_slice([[(0, 0, 0)], []], lists=[1, 0], n_points=1)
    assert cr.update_connections_list(s, 0) == dict(counter=[], n_max=0, kf_max=-1, conn=[])      # an empty list
    assert cr.update_connections_list(s, 1) == dict(counter=[], n_max=0, kf_max=-1, conn=[])      # only the owner sees the point
    # a Frame's vote: no self-exclusion, and a bad keyframe is no candidate but stays in the counter
    r = cr.update_connections_list(_shared([20, 18], flags=[0, 4, 0], frame=True), 0)
    assert r["counter"] == [(0, 20), (1, 20), (2, 18)] and (r["n_max"], r["kf_max"]) == (20, 0)
    r = cr.update_connections_list(_shared([20, 18], flags=[4, 4, 0], frame=True), 0)
    assert (r["n_max"], r["kf_max"]) == (18, 2) and r["conn"] == [(1, 20), (0, 20), (2, 18)]
    u = cr.update_local_keyframes(_shared([20, 18], flags=[4, 4, 0]))
    assert list(u["kf_max"]) == [2] and list(u["counter_weight"]) == [20, 20, 18]


def _cull_case(n_mps, n_red, stereo=False, flags=0, extra=3):
    """slot 0's list: n_red points seen by 0 and `extra` others, n_mps - n_red seen by 0 alone (twice through a stereo observation when `stereo`)"""
    kfs = [[] for _ in range(1 + extra)]
    for p in range(n_mps):
        kfs[0].append((p, 0, 0))
        if p < n_red:
            for k in range(1, 1 + extra):
                kfs[k].append((p, 0, 1 if stereo and k == 1 else 0))
    fl = np.zeros(1 + extra, np.uint8)
    fl[0] = flags
    return _orbx().covis_slice(kfs, lists=[0], n_points=n_mps, flags=fl)


@pytest.mark.parametrize("n", [10, 20, 1000])
def test_restated_culling_threshold_is_the_double_product(n):
    at = cr.keyframe_culling(_cull_case(n, 9 * n // 10))
    assert (int(at["n_mps"][0]), int(at["n_redundant"][0]), int(at["culled"][0])) == (n, 9 * n // 10, 0)       # exactly 0.9 nMPs: not culled
    above = cr.keyframe_culling(_cull_case(n, 9 * n // 10 + 1))
    assert (int(above["n_redundant"][0]), int(above["culled"][0])) == (9 * n // 10 + 1, 1)
    r = 9 * n // 10 + 1
    assert (above["point_obs"][:r] == 3).all() and not above["point_bad"][:r].any()                            # erased: 4 -> 3 observations
    assert (above["point_obs"][r:] == 0).all() and above["point_bad"][r:].all()                                # the points it saw alone are gone with it


def test_restated_culling_observations_flags_and_octaves():
    # two mono others + the owner = 3 observations: not > 3; a stereo other makes it 4, but still only two other observers
    assert int(cr.keyframe_culling(_cull_case(10, 10, extra=2))["n_redundant"][0]) == 0
    assert int(cr.keyframe_culling(_cull_case(10, 10, extra=2, stereo=True))["n_redundant"][0]) == 0
    r = cr.keyframe_culling(_cull_case(10, 10, stereo=True))
    assert int(r["culled"][0]) == 1 and (r["point_obs"] == 4).all()                                              # 1 + 2 + 1 + 1, minus the owner's 1
    r = cr.keyframe_culling(_cull_case(10, 10, flags=1))
    assert (int(r["n_mps"][0]), int(r["culled"][0])) == (0, 0) and (r["point_obs"] == 4).all()                   # mnId == 0: skipped
    r = cr.keyframe_culling(_cull_case(10, 10, flags=2))
    assert int(r["culled"][0]) == 1 and (r["point_obs"] == 4).all()                                              # mbNotErase: reported, nothing erased
    # the owner's stereo observation counts 2, in Observations() and in the erase
    kfs = [[(p, 0, 1) for p in range(10)]] + [[(p, 0, 0) for p in range(10)] for _ in range(2)] + [[(p, 0, 0) for p in range(5)]]
    r = cr.keyframe_culling(_orbx().covis_slice(kfs, lists=[0], n_points=10))
    assert (int(r["n_redundant"][0]), int(r["culled"][0])) == (5, 0)
    kfs[3] = [(p, 0, 0) for p in range(10)]
    r = cr.keyframe_culling(_orbx().covis_slice(kfs, lists=[0], n_points=10))
    assert int(r["culled"][0]) == 1 and (r["point_obs"] == 3).all() and not r["point_bad"].any()
    # octaves: an observer two octaves coarser does not count, one octave coarser does; depth: a far point is not counted at all
    kfs = [[(p, 1, 0, 0 if p == 9 else 1) for p in range(10)]] + [[(p, 2, 0) for p in range(10)] for _ in range(2)] + [[(p, 3, 0) for p in range(10)]]
    r = cr.keyframe_culling(_orbx().covis_slice(kfs, lists=[0], n_points=10))
    assert (int(r["n_mps"][0]), int(r["n_redundant"][0])) == (9, 0)
    kfs[3] = [(p, 0, 0) for p in range(10)]
    assert int(cr.keyframe_culling(_orbx().covis_slice(kfs, lists=[0], n_points=10))["n_redundant"][0]) == 9


def test_scene_vacuity_guards():
    s = cs.cascade_scene()
    seq, ind = cr.keyframe_culling(s), cr.keyframe_culling(s, sequential=False)
    assert tuple(int(c) for c in seq["culled"]) == cs.CASCADE_CULLED
    assert int(s["kf_flags"][5]) & 2 and seq["culled"][5] and seq["culled"][[1, 2]].all() and seq["culled"][7]      # the uncullable one sits between the culls
    assert (seq["culled"] != ind["culled"]).any() and (seq["n_mps"] != ind["n_mps"]).any()
    assert ((seq["point_bad"] == 1) & (np.asarray(s["point_bad"]) == 0)).sum() >= 1 and not ind["point_bad"].any()
    for K in (1, 2, 12):
        assert cr.keyframe_culling(cs.all_culled_scene(K))["culled"].all()
        assert not cr.keyframe_culling(cs.no_cull_scene(K))["culled"].any()
    assert 1 <= cr.keyframe_culling(cs.random_cull_scene(3))["culled"].sum() < 12
    t = cr.update_connections(cs.tie_scene())
    assert cs.ties_at_or_above(t["conn_weight"], t["conn_offset"]) >= 20
    big = cr.update_connections(cs.connect_scene(1, 63))
    assert (np.diff(big["conn_offset"]) > 1).any() and (big["kf_max"] == -1).any()


def _window_slice(orbx, w):
    octv = np.rint(np.log(1.0 / np.asarray(w["edge_inv_sigma2"], np.float64)) / (2 * np.log(1.2))).astype(np.int32)
    kfs = [[] for _ in range(w["K"])]
    for e in range(w["E"]):
        kfs[int(w["edge_kf"][e])].append((int(w["edge_point"][e]), int(octv[e]), int(w["edge_obs"][e, 2] >= 0)))
    return orbx.covis_slice(kfs, lists=[w["K"] - 1], n_points=w["P"])


def _slam_lib():
    import oracle_lib
    return oracle_lib.slam_lib()


@pytest.mark.skipif(_slam_lib() is None or not hasattr(_slam_lib(), "orbslam_local_ba"), reason="oracle/_ref/liborbslam.so (the compiled reference) not built")
@pytest.mark.parametrize("cfg", [dict(K=10, P=300, seed=21, max_obs=6, n_fixed=0, stereo_frac=1.0), dict(K=16, P=1200, seed=5, max_obs=5, n_fixed=0)])
def test_restatement_against_the_compiled_update_connections(orbx, cfg):
    """the local keyframes of Optimizer::LocalBundleAdjustment are GetVectorCovisibleKeyFrames() of the keyframe whose UpdateConnections ran last"""
    import oracle_lib
    w = orbx.lba_synth.make_window(**cfg)
    ref_kf = w["K"] - 1
    role = oracle_lib.ref_local_ba_on_map(w, ref_kf)["role"]
    want = set(int(k) for k in np.flatnonzero(role == 1)) - {ref_kf}
    r = cr.update_connections_list(_window_slice(orbx, w), 0)
    assert len(want) >= 1 and set(k for k, _ in r["conn"]) == want


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a device, the shim
# ---------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("orbx_covis_create", "orbx_covis_destroy", "orbx_covis_update_connections", "orbx_covis_keyframe_culling", "orbx_covis_last_timing")


def test_exports_and_create_without_a_device(orbx):
    L = orbx.load_library()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
    assert all(hasattr(orbx.Covisibility, k) for k in ("UpdateConnections", "KeyFrameCulling", "UpdateLocalKeyFrames", "last_timing")) and hasattr(orbx, "covis_slice")
    assert "orbx_covis_update_connections" in (ROOT / "__graft_entry__.py").read_text()
    assert "orbx_covis.hip" in orbx.build_mod.HIP_SOURCES
    assert orbx.COVIS_LDS_KEYFRAMES == cs.LDS_NK and ("#define ORBX_COVIS_LDS_KEYFRAMES %d" % cs.LDS_NK) in (ROOT / "include" / "orbx.h").read_text()
    L.orbx_covis_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.orbx_last_error.restype = ctypes.c_char_p
    h = ctypes.c_void_p()
    assert L.orbx_covis_create(0, None) == ERR_ARG
    rc = L.orbx_covis_create(0, ctypes.byref(h))
    if _gpu():
        assert rc == 0 and h.value
        L.orbx_covis_destroy.argtypes = [ctypes.c_void_p]
        L.orbx_covis_destroy(h)
    else:
        assert rc == ERR_NODEVICE and not h.value and len(L.orbx_last_error()) > 0
        with pytest.raises(orbx.OrbxError) as e:
            orbx.Covisibility()
        assert e.value.code == ERR_NODEVICE


def _call_raw(orbx, h, s, culling=False, th=15, cap=1 << 16):
    L = orbx.load_library()
    L.orbx_covis_update_connections.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.orbx_covis_keyframe_culling.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    keep = []
    S, _ = orbx.covis_marshal(s, keep)
    Q, M = S.num_lists, S.num_points
    if culling:
        o = dict(n_mps=np.zeros(Q + 1, np.int32), n_redundant=np.zeros(Q + 1, np.int32), culled=np.zeros(Q + 1, np.uint8), point_bad=np.zeros(M + 1, np.uint8),
                 point_obs=np.zeros(M + 1, np.int32))
        R = orbx.CovisCulling(*[o[k].ctypes.data for k in CULL_FIELDS])
        return L.orbx_covis_keyframe_culling(h, ctypes.byref(S), ctypes.byref(R)), o
    o = {k: np.full((Q + 2) if k in ("counter_offset", "conn_offset", "n_max", "kf_max") else cap + 1, -7, np.int32) for k in CONN_FIELDS}
    R = orbx.CovisConnections(o["counter_offset"].ctypes.data, o["counter_kf"].ctypes.data, o["counter_weight"].ctypes.data, cap, o["n_max"].ctypes.data,
                              o["kf_max"].ctypes.data, o["conn_offset"].ctypes.data, o["conn_kf"].ctypes.data, o["conn_weight"].ctypes.data, cap)
    return L.orbx_covis_update_connections(h, ctypes.byref(S), th, ctypes.byref(R)), o


def test_argument_errors_come_back_as_errors(orbx):
    """the slice is checked before the handle is looked at, so a machine without a device sees the same errors (there through a NULL handle, which a
    good slice reports as such)"""
    L = orbx.load_library()
    L.orbx_last_error.restype = ctypes.c_char_p
    L.orbx_covis_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.orbx_covis_destroy.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    have = L.orbx_covis_create(0, ctypes.byref(h)) == 0
    assert have == _gpu()
    good = cs.connect_scene(2, 65, (16, 40), (1,))
    owned = cs.cascade_scene()
    cases = []
    for key, idx, val, word in (("obs_offset", 3, 10 ** 6, "obs_offset decreases"), ("list_offset", 1, 10 ** 6, "list_offset decreases"), ("obs_offset", 0, 1, "start at 0"),
                                ("obs_offset", -1, 10 ** 6, "num_obs"), ("obs_kf", 5, 65, "obs_kf"), ("obs_kf", 5, -1, "obs_kf"), ("list_point", 2, 10 ** 6, "list_point"),
                                ("list_kf", 0, 65, "list_kf"), ("list_kf", 0, -2, "list_kf"), ("kf_rank", 7, int(good["kf_rank"][8]), "same rank")):
        bad = {k: np.array(v, copy=True) for k, v in good.items()}
        bad[key][idx] = val
        cases.append((bad, False, word))
    frame = {k: np.array(v, copy=True) for k, v in owned.items()}
    frame["list_kf"][3] = -1
    twice = {k: np.array(v, copy=True) for k, v in owned.items()}
    twice["list_kf"][3] = twice["list_kf"][4]
    cases += [(frame, True, "list_kf"), (twice, True, "two lists")]
    for bad, culling, word in cases:
        rc, o = _call_raw(orbx, h if have else None, bad, culling)
        assert rc == ERR_ARG and word in L.orbx_last_error().decode(), (word, rc, L.orbx_last_error())
    for s, culling in ((good, False), (owned, True)):
        rc, o = _call_raw(orbx, h if have else None, s, culling)
        assert (rc == 0) if have else (rc == ERR_ARG and "NULL handle" in L.orbx_last_error().decode())      # the slices are fine, and the handle is unharmed
    if have:
        L.orbx_covis_destroy(h)


def test_null_arguments_are_errors(orbx):
    L = orbx.load_library()
    L.orbx_covis_update_connections.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.orbx_covis_keyframe_culling.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.orbx_covis_last_timing.argtypes = [ctypes.c_void_p] * 3
    L.orbx_covis_destroy.argtypes = [ctypes.c_void_p]
    assert L.orbx_covis_update_connections(None, None, 15, None) == ERR_ARG
    assert L.orbx_covis_keyframe_culling(None, None, None) == ERR_ARG
    assert L.orbx_covis_last_timing(None, None, None) == ERR_ARG
    L.orbx_covis_destroy(None)
    with pytest.raises(ValueError):
        bad = dict(cs.tie_scene())
        bad["obs_octave"] = bad["obs_octave"][:-1]
        orbx.covis_marshal(bad, [])


def test_covis_slice_helper(orbx):
    s = orbx.covis_slice([[(1, 2, 1), (0, 0, 0), (1, 3, 0)], [(0, 1, 0, 0)]], lists=[1, 0, (-1, [(1, 4, 0, 0)])], ranks=[9, 3], flags=[0, 2])
    assert list(s["obs_offset"]) == [0, 2, 3] and list(s["obs_kf"]) == [0, 1, 0] and list(s["obs_octave"]) == [0, 1, 2] and list(s["obs_stereo"]) == [0, 0, 1]
    assert list(s["list_offset"]) == [0, 1, 4, 5] and list(s["list_kf"]) == [1, 0, -1] and list(s["list_point"]) == [0, 1, 0, 1, 1]
    assert list(s["list_octave"]) == [1, 2, 0, 3, 4] and list(s["list_close"]) == [0, 1, 1, 1, 0] and list(s["kf_rank"]) == [9, 3] and list(s["kf_flags"]) == [0, 2]


@pytest.mark.skipif(not os.access(REF / "include" / "KeyFrame.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "Covisibility_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "Covisibility_hip.cc").read_text()
    for piece in ("orbx_covis_update_connections(", "orbx_covis_keyframe_culling(", "MapPointAccess.h", "AddConnection(", "ChangeParent(", "RefreshCovisibles(", "SetBadFlag()",
                  "mConnectedKeyFrameWeights", "mvpOrderedConnectedKeyFrames", "mvOrderedWeights", "mbFirstConnection", "shim_error.h"):
        assert piece in text, piece
    head = (shim / "Covisibility_hip.h").read_text()
    for piece in ("class Covisibility_hip", "UpdateConnections(", "KeyFrameCulling(", "UpdateLocalKeyFrames("):
        assert piece in head, piece
    assert "Covisibility_hip" not in (ROOT / "oracle" / "Makefile").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    assert "Covisibility_hip" in integ and "orbx_covis_update_connections" in integ


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dev():
    return _orbx().Covisibility()


@functools.lru_cache(maxsize=None)
def _want_conn(NK):
    return cr.update_connections(cs.connect_scene(NK, NK))


@pytest.mark.gpu
@pytest.mark.parametrize("NK", cs.SWEEP_NK)
def test_update_connections_sweep(orbx, NK):
    """Q = 7 (owned and Frame lists of 0, 1, 14, 15, 16, 1500 and 40 entries in one call) and Q = 1 (the 1500-entry list and the empty list alone);
    a batch equals the same lists one call each, bit for bit"""
    s, want = cs.connect_scene(NK, NK), _want_conn(NK)
    got = _dev().UpdateConnections(s)
    _same(got, want, CONN_FIELDS, NK)
    ms, launches = _dev().last_timing()
    assert launches == 2 and ms > 0
    for q in range(len(cs.SWEEP_SIZES)):
        one = _dev().UpdateConnections(cs.one_list(s, q))
        a, b = int(want["counter_offset"][q]), int(want["counter_offset"][q + 1])
        c, d = int(want["conn_offset"][q]), int(want["conn_offset"][q + 1])
        ref = dict(counter_offset=[0, b - a], counter_kf=got["counter_kf"][a:b], counter_weight=got["counter_weight"][a:b], n_max=got["n_max"][q:q + 1],
                   kf_max=got["kf_max"][q:q + 1], conn_offset=[0, d - c], conn_kf=got["conn_kf"][c:d], conn_weight=got["conn_weight"][c:d])
        _same(one, ref, CONN_FIELDS, (NK, q))


@pytest.mark.gpu
def test_update_connections_ties_thresholds_and_frames(orbx):
    s = cs.tie_scene()
    _same(_dev().UpdateConnections(s), cr.update_connections(s), CONN_FIELDS, "ties")
    for th in (1, 14, 16, 21, 22, 10 ** 6):
        _same(_dev().UpdateConnections(s, th=th), cr.update_connections(s, th), CONN_FIELDS, ("ties", th))
    for NK in (2, 65, cs.LDS_NK + 1):
        t = cs.connect_scene(NK, NK)
        _same(_dev().UpdateLocalKeyFrames(t), cr.update_local_keyframes(t), ("counter_offset", "counter_kf", "counter_weight", "n_max", "kf_max"), ("frame", NK))


@pytest.mark.gpu
@pytest.mark.parametrize("NK,Q", [(cs.LDS_NK + 1, 70), (64, 4100)])
def test_update_connections_more_lists_than_workgroups(orbx, NK, Q):
    """beyond the LDS limit 64 workgroups stride over the lists and reuse their histogram rows; within it 4096 workgroups do"""
    s = cs.connect_scene(7, NK, (40, 3, 16, 0, 25) * (Q // 5), tuple(range(1, Q, 7)))
    _same(_dev().UpdateConnections(s), cr.update_connections(s), CONN_FIELDS, (NK, Q))


CULL_SCENES = dict(cascade=cs.cascade_scene, all1=lambda: cs.all_culled_scene(1), all2=lambda: cs.all_culled_scene(2), all12=lambda: cs.all_culled_scene(12),
                   all2_empty_first=lambda: cs.all_culled_scene(2, True), none1=lambda: cs.no_cull_scene(1), none2=lambda: cs.no_cull_scene(2),
                   none12=lambda: cs.no_cull_scene(12), random3=lambda: cs.random_cull_scene(3), random4=lambda: cs.random_cull_scene(4),
                   random5_k30=lambda: cs.random_cull_scene(5, 30, 2500))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CULL_SCENES))
def test_keyframe_culling(orbx, name):
    s = CULL_SCENES[name]()
    want = cr.keyframe_culling(s)
    got = _dev().KeyFrameCulling(s)
    _same(got, want, CULL_FIELDS, name)
    # c erasing culls: staging + init + (c + 1) evaluations + c erases; the last evaluation is not needed when the last list is the last cull
    Q = len(s["list_kf"])
    c = int((want["culled"].astype(bool) & ((np.asarray(s["kf_flags"])[np.asarray(s["list_kf"])] & 2) == 0)).sum())
    last = Q - 1 - int(np.argmax((want["culled"].astype(bool) & ((np.asarray(s["kf_flags"])[np.asarray(s["list_kf"])] & 2) == 0))[::-1])) if c else -1
    assert _dev().last_timing()[1] == 2 * c + 3 - (1 if last == Q - 1 else 0)
    again = _dev().KeyFrameCulling(s)      # no state leaks from call to call on one handle
    _same(again, got, CULL_FIELDS, (name, "again"))


@pytest.mark.gpu
def test_calls_interleave_on_one_handle_without_leaking_state(orbx):
    a, b = cs.cascade_scene(), cs.connect_scene(63, 63)
    r1 = _dev().KeyFrameCulling(a)
    _same(_dev().UpdateConnections(b), _want_conn(63), CONN_FIELDS, "between")
    _same(_dev().KeyFrameCulling(cs.all_culled_scene(12)), cr.keyframe_culling(cs.all_culled_scene(12)), CULL_FIELDS, "between")
    _same(_dev().KeyFrameCulling(a), r1, CULL_FIELDS, "after")
    assert tuple(int(c) for c in r1["culled"]) == cs.CASCADE_CULLED


@pytest.mark.gpu
def test_capacity_error_and_recovery(orbx):
    s, want = cs.connect_scene(63, 63), _want_conn(63)
    n, m = int(want["counter_offset"][-1]), int(want["conn_offset"][-1])
    for kw in (dict(counter_capacity=n - 1), dict(conn_capacity=m - 1), dict(counter_capacity=0, conn_capacity=0)):
        with pytest.raises(orbx.OrbxError) as e:
            _dev().UpdateConnections(s, **kw)
        assert e.value.code == ERR_CAPACITY
    _same(_dev().UpdateConnections(s, counter_capacity=n, conn_capacity=m), want, CONN_FIELDS, "exact capacity")
    h = ctypes.c_void_p()
    L = orbx.load_library()
    L.orbx_covis_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    assert L.orbx_covis_create(0, ctypes.byref(h)) == 0
    rc, o = _call_raw(orbx, h, s, cap=m - 1)
    assert rc == ERR_CAPACITY and all((o[k] == -7).all() for k in CONN_FIELDS)      # nothing was written
    rc, o = _call_raw(orbx, h, s)
    assert rc == 0
    L.orbx_covis_destroy.argtypes = [ctypes.c_void_p]
    L.orbx_covis_destroy(h)


@pytest.mark.gpu
def test_c_abi_through_ctypes_agrees_with_the_class(orbx):
    L = orbx.load_library()
    L.orbx_covis_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.orbx_covis_destroy.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    assert L.orbx_covis_create(0, ctypes.byref(h)) == 0
    s = cs.connect_scene(300, 300)
    got = _dev().UpdateConnections(s)
    rc, o = _call_raw(orbx, h, s)
    Q = len(s["list_kf"])
    n, m = int(o["counter_offset"][Q]), int(o["conn_offset"][Q])
    raw = dict(counter_offset=o["counter_offset"][:Q + 1], counter_kf=o["counter_kf"][:n], counter_weight=o["counter_weight"][:n], n_max=o["n_max"][:Q], kf_max=o["kf_max"][:Q],
               conn_offset=o["conn_offset"][:Q + 1], conn_kf=o["conn_kf"][:m], conn_weight=o["conn_weight"][:m])
    assert rc == 0
    _same(raw, got, CONN_FIELDS, "raw connections")
    c = cs.cascade_scene()
    rc, o = _call_raw(orbx, h, c, culling=True)
    assert rc == 0
    M = len(c["point_bad"])
    _same(dict(n_mps=o["n_mps"][:12], n_redundant=o["n_redundant"][:12], culled=o["culled"][:12], point_bad=o["point_bad"][:M], point_obs=o["point_obs"][:M]),
          _dev().KeyFrameCulling(c), CULL_FIELDS, "raw culling")
    L.orbx_covis_destroy(h)
