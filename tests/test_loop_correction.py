"""Loop correction on the device (csrc/orbx_loop_correct.hip, orbx_loop_*, LoopCorrection) against tests/loop_ref.py, the literal restatement of
LoopClosing::CorrectLoop's Sim3 propagation and of the map update after global BA.  CPU tests: the restatement against float64 4x4 matrices and its
invariants, hand-made cases, the vacuity guards of the scenes, the ABI without a device, the shim.  GPU tests: every field of every result equals
the restatement - integers equal, floats and doubles bit for bit, no tolerance, no excluded case."""
import ctypes
import functools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import loop_ref as lr
import loop_scenes as ls
import optsim3_ref as g2o
from test_initializer import REF, ROOT

ERR_ARG, ERR_NODEVICE = -1, -4
SIM3_FIELDS = ("noncorrected", "corrected", "tiw", "ow_new", "scw_mat", "pos", "corrected_by", "normal", "max_dist", "min_dist", "updated")
GBA_FIELDS = ("tcw_gba", "reached", "pos", "moved")
f4, f8 = np.float32, np.float64


def _gpu():
    import torch
    return torch.cuda.is_available()


@functools.lru_cache(maxsize=None)
def _orbx():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a.astype(np.int64)


def _same(got, want, fields, where):
    for k in fields:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.reshape(-1).shape == w.reshape(-1).shape, (where, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(_bits(g).reshape(-1) != _bits(w).reshape(-1))
        assert len(bad) == 0, (where, k, len(bad), bad[:8], g.reshape(-1)[bad[:8]], w.reshape(-1)[bad[:8]])


def _T64(T12):
    T = np.eye(4)
    T[:3] = np.asarray(T12, f8).reshape(3, 4)
    return T


def _sim3_matrix(row):
    """[[s R, t], [0, 1]] of (q, t, s) by the textbook quaternion formula on the normalised quaternion"""
    q = np.asarray(row[:4], f8) / np.linalg.norm(row[:4])
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = row[7] * R, row[4:7]
    return S


# ---------------------------------------------------------------------------------------------------------------------
# the restatement tied to something other than itself (CPU)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,s", [(11, 1.0), (12, 1.1), (13, 0.8)])
def test_restated_correct_loop_against_float64_matrices(seed, s):
    """new P = inv(S_corrected) S_old P with float64 4x4 matrices, and: the camera coordinates of the new point in the corrected SE3 pose are the old
    camera coordinates / s.  Both within 1e-5 of the point's depth in the correcting keyframe: float32 rounding of inputs and outputs is 6e-8 per
    operation over about a dozen operations on coordinates of the depth's magnitude, the rest is margin."""
    p = ls.sim3_scene(8, 200, seed, s=s)
    r = lr.correct_loop(p)
    group, cur = p["group_kf"], p["current"]
    Scw, Tcur = _sim3_matrix(p["scw"]), _T64(p["tcw"][group[cur]])
    n = 0
    for g, k in enumerate(group):
        Tiw = _T64(p["tcw"][k])
        Scorr = Scw if g == cur else Tiw @ np.linalg.inv(Tcur) @ Scw
        assert np.abs(_sim3_matrix(r["corrected"][g]) - Scorr).max() <= 1e-5 * max(1.0, np.abs(Scorr[:3, 3]).max())
        assert np.abs(_sim3_matrix(r["noncorrected"][g]) - Tiw).max() <= 1e-5 * max(1.0, np.abs(Tiw[:3, 3]).max())
        Tn = _T64(r["tiw"][g])
        for i in np.flatnonzero(r["corrected_by"] == g):
            P = np.append(p["pos"][i].astype(f8), 1.0)
            old = Tiw @ P
            depth = old[2]
            assert depth > 1.0, "the scene keeps the group's points in front of the group"
            want = np.linalg.inv(Scorr) @ old
            newP = np.append(r["pos"][i].astype(f8), 1.0)
            assert np.abs(newP - want)[:3].max() <= 1e-5 * depth, (g, i)
            assert np.abs((Tn @ newP)[:3] - old[:3] / s).max() <= 1e-5 * depth, (g, i)
            n += 1
    assert n > 100
    # the Sim3 pieces are tests/optsim3_ref.py's group operations, the 4x4 product the stand-in's
    g = (cur + 1) % len(group)
    _, Twc = lr.set_pose(lr.mat44(p["tcw"][group[cur]]))
    Tic = lr.matmul(lr.mat44(p["tcw"][group[g]]), Twc)
    Scw3 = ([float(v) for v in p["scw"][:4]], [float(v) for v in p["scw"][4:7]], float(p["scw"][7]))
    want = g2o.sim3_mul(g2o.sim3_from_Rts(Tic[:3, :3].astype(f8), Tic[:3, 3].astype(f8), 1.0), Scw3)
    assert (_bits(r["corrected"][g]) == _bits(np.array(list(want[0]) + list(want[1]) + [want[2]]))).all()
    assert (_bits(r["corrected"][cur]) == _bits(np.asarray(p["scw"], f8))).all()
    assert np.abs(Twc.astype(f8) @ _T64(p["tcw"][group[cur]]) - np.eye(4)).max() <= 1e-5 * max(1.0, np.abs(Twc[:3, 3]).max())


@pytest.mark.parametrize("seed", [21, 22])
def test_restated_propagate_gba_invariants(seed):
    """A non-optimised keyframe keeps its pose relative to its parent, Tchild_new inv(Tparent_new) = Tchild_old inv(Tparent_old); a re-projected point
    keeps its camera coordinates in its reference keyframe.  1e-5 relative to the magnitude of the operands (the larger translation, at least 1;
    the point's depth): two float products and a transposed-rotation product per edge, 6e-8 per operation, the rest is margin."""
    p = ls.gba_scene(60, 400, seed)
    r = lr.propagate_gba(p)
    n = 0
    for c, k in enumerate(p["parent"]):
        if k < 0 or not r["reached"][c]:
            continue
        assert r["reached"][k]
        if p["in_gba"][c]:
            assert (_bits(r["tcw_gba"][c]) == _bits(p["tcw_gba"][c])).all()
            continue
        Tc, Tk, Gc, Gk = _T64(p["tcw"][c]), _T64(p["tcw"][k]), _T64(r["tcw_gba"][c]), _T64(r["tcw_gba"][k])
        scale = max(1.0, np.abs(Tc[:3, 3]).max(), np.abs(Tk[:3, 3]).max(), np.abs(Gk[:3, 3]).max())
        assert np.abs(Gc @ np.linalg.inv(Gk) - Tc @ np.linalg.inv(Tk)).max() <= 1e-5 * scale, (c, k)
        n += 1
    assert n >= 8
    two = np.flatnonzero(r["moved"] == 2)
    assert len(two) > 50
    for i in two:
        k = p["point_ref"][i]
        old = _T64(p["tcw"][k]) @ np.append(p["pos"][i].astype(f8), 1.0)
        new = _T64(r["tcw_gba"][k]) @ np.append(r["pos"][i].astype(f8), 1.0)
        assert old[2] > 1.0 and np.abs(new - old).max() <= 1e-5 * old[2], i
    one = np.flatnonzero(r["moved"] == 1)
    assert len(one) and (_bits(r["pos"][one]) == _bits(p["pos_gba"][one])).all()
    zero = np.flatnonzero(r["moved"] == 0)
    assert len(zero) and (_bits(r["pos"][zero]) == _bits(p["pos"][zero])).all()


# ---------------------------------------------------------------------------------------------------------------------
# hand-made cases of the restatement (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def _hand(group, cur, lists, obs, M, bad=(), done=(), s=1.2):
    base = ls.sim3_scene(3, M, 5, s=s, n_out=2, permute=False, special_lists=False)      # five keyframes; the group and the lists are replaced
    flat = [k for o in obs for k in o]
    off = np.zeros(M + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in obs])
    flag = lambda idx: np.array([1 if i in idx else 0 for i in range(M)], np.uint8)      # noqa: E731
    loff = np.zeros(len(group) + 1, np.int32)
    loff[1:] = np.cumsum([len(l) for l in lists])
    base.update(group_kf=np.array(group, np.int32), current=cur, list_offset=loff, list_point=np.array([i for l in lists for i in l], np.int32).reshape(-1),
                obs_offset=off, obs_kf=np.array(flat, np.int32).reshape(-1), point_bad=flag(bad), point_done=flag(done), point_ref=np.zeros(M, np.int32))
    return base


def test_restated_first_in_group_order_wins_and_skips():
    # the group order is 2, 0, 1 (not the slot order) and the current keyframe is second in it
    p = _hand([2, 0, 1], 1, [[1, -1, 4], [0, 1, 2, 3, 4], [1, 2, 5]], [[0], [0, 1, 2], [3], [0], [2, 4], []], 6, bad=(2,), done=(3,))
    r = lr.correct_loop(p)
    assert list(r["corrected_by"]) == [1, 0, -1, -1, 0, 2]          # point 1: slot 2's list comes first; 2 is bad, 3 is done; the NULL entry is skipped
    assert list(r["updated"]) == [1, 1, 0, 0, 1, 0]                 # point 5 moved without observations: UpdateNormalAndDepth returns early
    for i in (2, 3):
        assert (_bits(r["pos"][i]) == _bits(p["pos"][i])).all() and not r["normal"][i].any() and r["max_dist"][i] == 0
    assert (_bits(r["pos"][5]) != _bits(p["pos"][5])).any() and not r["normal"][5].any()
    assert (_bits(r["corrected"][1]) == _bits(p["scw"])).all() and (r["corrected"][0] != p["scw"]).any()
    assert r["noncorrected"][:, 7].tolist() == [1.0, 1.0, 1.0] and np.allclose(r["corrected"][:, 7], 1.2)
    # with the slot order as the group order the same lists give another corrector
    q = _hand([0, 1, 2], 1, [[0, 1, 2, 3, 4], [1, 2, 5], [1, -1, 4]], [[0], [0, 1, 2], [3], [0], [2, 4], []], 6, bad=(2,), done=(3,))
    assert list(lr.correct_loop(q)["corrected_by"]) == [0, 0, -1, -1, 0, 1]


def test_restated_centres_follow_the_order_of_set_pose():
    """point 0 is moved by group position 1 and seen by the keyframes at positions 0 (already re-posed), 1 (itself: not yet) and 2 (not yet)"""
    p = _hand([3, 1, 4], 0, [[], [0], [0]], [[3, 1, 4, 0]], 1)
    p["point_ref"][:] = 3
    r = lr.correct_loop(p)
    assert list(r["corrected_by"]) == [1]
    ow = np.array(p["ow"], f4)
    ow[3] = r["ow_new"][0]
    want = lr.update_normal_and_depth(r["pos"][0], [3, 1, 4, 0], ow, 3, p["ref_scale"][0], p["top_scale"][0])
    assert (_bits(want[0]) == _bits(r["normal"][0])).all() and _bits(want[1]) == _bits(r["max_dist"][0]) and _bits(want[2]) == _bits(r["min_dist"][0])
    old = lr.update_normal_and_depth(r["pos"][0], [3, 1, 4, 0], np.asarray(p["ow"], f4), 3, p["ref_scale"][0], p["top_scale"][0])
    assert (_bits(old[0]) != _bits(r["normal"][0])).any() and _bits(old[1]) != _bits(r["max_dist"][0])      # the reference keyframe's centre moved too


def test_restated_gba_tree_cases():
    s = ls.gba_scene(6, 12, 3, n_free=0, n_out=0)
    s["parent"] = np.array([-1, 0, 1, 2, -2, 4], np.int32)
    s["in_gba"] = np.array([1, 0, 1, 0, 1, 0], np.uint8)
    s["point_ref"] = np.array([0, 1, 2, 3, 4, 5] * 2, np.int32)
    s["point_in_gba"][:] = 0
    s["point_in_gba"][6:9] = 1
    s["point_bad"][:] = 0
    s["point_bad"][11] = 1
    r = lr.propagate_gba(s)
    assert list(r["reached"]) == [1, 1, 1, 1, 0, 0]
    assert (_bits(r["tcw_gba"][2]) == _bits(s["tcw_gba"][2])).all()      # an optimised child under a non-optimised parent keeps its pose
    for c, k in ((1, 0), (3, 2)):                                          # ... and its non-optimised child chains from it
        _, Twc = lr.set_pose(lr.mat44(s["tcw"][k]))
        want = lr.matmul(lr.matmul(lr.mat44(s["tcw"][c]), Twc), lr.mat44(r["tcw_gba"][k]))
        assert (_bits(want[:3].reshape(12)) == _bits(r["tcw_gba"][c])).all() and (want[3] == [0, 0, 0, 1]).all()
    assert list(r["moved"]) == [2, 2, 2, 2, 0, 0, 1, 1, 1, 2, 0, 0]      # the points of the unreached keyframes 4 and 5 stay, also where 4 was optimised
    assert (_bits(r["pos"][[4, 5, 10, 11]]) == _bits(s["pos"][[4, 5, 10, 11]])).all()


# ---------------------------------------------------------------------------------------------------------------------
# the scenes are not vacuous (CPU)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sim3_case(name):
    big = (1, 63, 64, 65, 300)
    p = dict(g1=lambda: ls.sim3_scene(1, 40, 31, s=1.0), g3=lambda: ls.sim3_scene(3, 60, 32, s=1.1, big=big), g64=lambda: ls.sim3_scene(64, 300, 33, s=0.9),
             g65=lambda: ls.sim3_scene(65, 300, 34, s=1.0), m0=lambda: ls.sim3_scene(3, 0, 35), slot_order=lambda: ls.sim3_scene(7, 80, 36, permute=False),
             no_entries=lambda: _no_entries())[name]()
    return p, lr.correct_loop(p)


def _no_entries():
    p = ls.sim3_scene(4, 10, 37)
    p["list_offset"] = np.zeros(5, np.int32)
    p["list_point"] = np.zeros(0, np.int32)
    return p


SIM3_CASES = ("g1", "g3", "g64", "g65", "m0", "slot_order", "no_entries")


def test_sim3_scene_vacuity_guards():
    scales = set()
    for name in ("g3", "g64", "g65"):
        p, r = _sim3_case(name)
        G = len(p["group_kf"])
        gpos = {int(k): g for g, k in enumerate(p["group_kf"])}
        moved = np.flatnonzero(r["corrected_by"] >= 0)
        both = []
        for i in moved:
            o = [int(k) for k in p["obs_kf"][p["obs_offset"][i]:p["obs_offset"][i + 1]]]
            c = int(r["corrected_by"][i])
            if any(k in gpos and gpos[k] < c for k in o) and any(k in gpos and gpos[k] > c for k in o) and any(k not in gpos for k in o):
                both.append(i)
        assert len(both) >= 0.2 * len(moved) and len(moved) >= 30, (name, len(both), len(moved))
        ow_new = np.array(p["ow"], f4)
        ow_new[p["group_kf"]] = r["ow_new"]
        for i in both:      # neither all-old nor all-new centres give the restatement's normal
            o = p["obs_kf"][p["obs_offset"][i]:p["obs_offset"][i + 1]]
            for ow in (np.asarray(p["ow"], f4), ow_new):
                alt = lr.update_normal_and_depth(r["pos"][i], o, ow, int(p["point_ref"][i]), p["ref_scale"][i], p["top_scale"][i])
                assert (_bits(alt[0]) != _bits(r["normal"][i])).any(), (name, i)
        assert (r["branch"] != 3).any() and (r["branch"] == 3).sum() >= 2, (name, r["branch"])      # a non-trace branch of Quaterniond(Matrix3d)
        assert list(np.sort(p["group_kf"])) != list(p["group_kf"]) and p["current"] != 0
        sizes = np.diff(p["list_offset"])
        assert (sizes == 0).any() and (sizes == 1).any()
        assert (r["corrected_by"] == -1).any() and p["point_bad"].any() and p["point_done"].any() and (p["list_point"] == -1).any()
        inlist = [set(p["list_point"][p["list_offset"][g]:p["list_offset"][g + 1]]) for g in range(G)]
        assert all(0 in l for g, l in enumerate(inlist) if sizes[g] > 0)      # a point in every (non-empty) list
        scales.add(float(p["scw"][7]))
    assert 1.0 in scales and len(scales) >= 2
    assert sorted(set(np.diff(_sim3_case("g3")[0]["obs_offset"])[:5])) == [1, 63, 64, 65, 300]
    assert _sim3_case("g1")[1]["corrected_by"].max() == 0 and len(_sim3_case("m0")[1]["pos"]) == 0


@functools.lru_cache(maxsize=None)
def _gba_case(name):
    p = dict(n1=lambda: ls.gba_scene(1, 1, 41), chain1=lambda: ls.chain_scene(1, 63, 42), chain3=lambda: ls.chain_scene(3, 64, 43), chain40=lambda: ls.chain_scene(40, 65, 44),
             tree65=lambda: ls.gba_scene(65, 0, 45), tree300=lambda: ls.gba_scene(300, 5000, 46), two_origins=lambda: ls.gba_scene(40, 100, 47, origins=2))[name]()
    return p, lr.propagate_gba(p)


GBA_CASES = ("n1", "chain1", "chain3", "chain40", "tree65", "tree300", "two_origins")


def test_gba_scene_vacuity_guards():
    p, r = _gba_case("tree300")
    assert sorted(set(r["moved"])) == [0, 1, 2] and not r["reached"].all() and r["reached"].sum() > 200
    free = np.flatnonzero((p["in_gba"] == 0) & (r["reached"] == 1) & (p["parent"] >= 0))
    assert len(free) >= 20 and (p["in_gba"][p["parent"][free]] == 0).sum() >= 5      # chains of non-optimised keyframes inside the tree
    assert not (r["tcw_gba"][r["reached"] == 1] == 777.0).any()                       # the sentinel of a non-optimised pose reaches no reached result
    for name, k in (("chain1", 1), ("chain3", 3), ("chain40", 40)):
        p, r = _gba_case(name)
        assert r["reached"].all() and (p["in_gba"] == 0).sum() == k + 1 and (r["moved"] == 2).sum() >= 40 and not (r["tcw_gba"] == 777.0).any()
    assert (_gba_case("two_origins")[0]["parent"] == -1).sum() == 2


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a device, the shim
# ---------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("orbx_loop_create", "orbx_loop_destroy", "orbx_loop_correct_sim3", "orbx_loop_propagate_gba", "orbx_loop_last_timing")


def test_exports_and_create_without_a_device(orbx):
    L = orbx.load_library()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
    assert all(hasattr(orbx.LoopCorrection, k) for k in ("CorrectLoop", "PropagateGBA", "last_timing")) and hasattr(orbx, "loop_marshal")
    assert all(hasattr(orbx, k) for k in ("LoopSim3Problem", "LoopSim3Result", "LoopGbaProblem", "LoopGbaResult"))
    assert "orbx_loop_correct_sim3" in (ROOT / "__graft_entry__.py").read_text()
    assert "orbx_loop_correct.hip" in orbx.build_mod.HIP_SOURCES
    L.orbx_loop_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.orbx_last_error.restype = ctypes.c_char_p
    h = ctypes.c_void_p()
    assert L.orbx_loop_create(0, None) == ERR_ARG
    rc = L.orbx_loop_create(0, ctypes.byref(h))
    if _gpu():
        assert rc == 0 and h.value
        L.orbx_loop_destroy.argtypes = [ctypes.c_void_p]
        L.orbx_loop_destroy(h)
    else:
        assert rc == ERR_NODEVICE and not h.value and len(L.orbx_last_error()) > 0
        with pytest.raises(orbx.OrbxError) as e:
            orbx.LoopCorrection()
        assert e.value.code == ERR_NODEVICE


def _call_raw(orbx, h, p, null=None):
    L = orbx.load_library()
    L.orbx_loop_correct_sim3.argtypes = [ctypes.c_void_p] * 3
    L.orbx_loop_propagate_gba.argtypes = [ctypes.c_void_p] * 3
    keep = []
    P, _ = orbx.loop_marshal(p, keep)
    if null:
        setattr(P, null, None)
    sim3 = isinstance(P, orbx.LoopSim3Problem)
    sizes = dict(G=P.num_group, M=P.num_points) if sim3 else dict(n=P.num_keyframes, M=P.num_points)
    fields = orbx.LOOP_SIM3_FIELDS if sim3 else orbx.LOOP_GBA_FIELDS
    o = {k: np.zeros((sizes[s] + 1, w), dt) for k, dt, s, w in fields}
    R = (orbx.LoopSim3Result if sim3 else orbx.LoopGbaResult)(*[o[k].ctypes.data for k, _, _, _ in fields])
    rc = (L.orbx_loop_correct_sim3 if sim3 else L.orbx_loop_propagate_gba)(h, ctypes.byref(P), ctypes.byref(R))
    return rc, {k: (o[k][:sizes[s]] if w > 1 else o[k][:sizes[s], 0]) for k, _, s, w in fields}


def test_argument_errors_come_back_as_errors(orbx):
    """the problem is checked before the handle is looked at, so a machine without a device sees the same errors (there through a NULL handle, which a
    good problem reports as such)"""
    L = orbx.load_library()
    L.orbx_last_error.restype = ctypes.c_char_p
    L.orbx_loop_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.orbx_loop_destroy.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    have = L.orbx_loop_create(0, ctypes.byref(h)) == 0
    assert have == _gpu()
    good, tree = ls.sim3_scene(5, 30, 51), ls.gba_scene(20, 30, 52)
    NK, G, M, n = len(good["tcw"]), 5, 30, 20
    cases = []
    for key, idx, val, word in (("list_offset", 0, 1, "list_offset does not start at 0"), ("list_offset", 2, 10 ** 6, "list_offset decreases"), ("list_offset", -1, 10 ** 6, "num_entries"),
                                ("obs_offset", 0, 1, "obs_offset does not start at 0"), ("obs_offset", 3, 10 ** 6, "obs_offset decreases"), ("obs_offset", -1, 10 ** 6, "num_obs"),
                                ("group_kf", 0, NK, "group_kf"), ("group_kf", 0, -1, "group_kf"), ("group_kf", 1, int(good["group_kf"][3]), "two group entries"),
                                ("obs_kf", 4, NK, "obs_kf"), ("obs_kf", 4, -1, "obs_kf"), ("list_point", 2, M, "list_point"), ("list_point", 2, -2, "list_point"),
                                ("point_ref", 7, NK, "point_ref"), ("point_ref", 7, -1, "point_ref"), ("current", None, G, "current"), ("current", None, -1, "current"),
                                ("scw", 7, 0.0, "positive"), ("scw", 7, -1.0, "positive"), ("scw", 1, np.nan, "finite"), ("tcw", 13, np.inf, "finite"), ("ow", 2, np.nan, "finite"),
                                ("pos", 5, np.nan, "finite")):
        bad = {k: np.array(v, copy=True) for k, v in good.items()}
        if idx is None:
            bad[key] = val
        else:
            bad[key].reshape(-1)[idx] = val
        cases.append((bad, None, word))
    cases += [(good, k, "NULL") for k in ("tcw", "ow", "group_kf", "scw", "list_offset", "list_point", "pos", "point_bad", "point_done", "point_ref", "ref_scale", "top_scale",
                                           "obs_offset", "obs_kf")]
    loop2 = {k: np.array(v, copy=True) for k, v in tree.items()}
    loop2["parent"][5], loop2["parent"][9] = 9, 5
    self1 = {k: np.array(v, copy=True) for k, v in tree.items()}
    self1["parent"][7] = 7
    no_origin = {k: np.array(v, copy=True) for k, v in tree.items()}
    no_origin["parent"][0] = -2
    for key, idx, val, word in (("parent", 3, n, "parent"), ("parent", 3, -3, "parent"), ("point_ref", 2, n, "point_ref"), ("point_ref", 2, -2, "point_ref"), ("tcw", 30, np.nan, "finite"),
                                ("tcw_gba", 1, np.inf, "finite"), ("pos", 0, np.nan, "finite"), ("pos_gba", 4, np.nan, "finite")):
        bad = {k: np.array(v, copy=True) for k, v in tree.items()}
        bad[key].reshape(-1)[idx] = val
        cases.append((bad, None, word))
    cases += [(loop2, None, "own ancestor"), (self1, None, "own ancestor"), (no_origin, None, "no origin")]
    cases += [(tree, k, "NULL") for k in ("parent", "tcw", "tcw_gba", "in_gba", "pos", "pos_gba", "point_in_gba", "point_bad", "point_ref")]
    for bad, null, word in cases:
        rc, _ = _call_raw(orbx, h if have else None, bad, null)
        assert rc == ERR_ARG and word in L.orbx_last_error().decode(), (word, null, rc, L.orbx_last_error())
    for p, want, fields in ((good, lr.correct_loop, SIM3_FIELDS), (tree, lr.propagate_gba, GBA_FIELDS)):
        rc, o = _call_raw(orbx, h if have else None, p)
        if have:      # the problems are fine, and the handle is unharmed
            assert rc == 0
            _same(o, want(p), fields, "after the errors")
        else:
            assert rc == ERR_ARG and "NULL handle" in L.orbx_last_error().decode()
    if have:
        L.orbx_loop_destroy(h)


def test_null_arguments_are_handled(orbx):
    L = orbx.load_library()
    L.orbx_loop_correct_sim3.argtypes = [ctypes.c_void_p] * 3
    L.orbx_loop_propagate_gba.argtypes = [ctypes.c_void_p] * 3
    L.orbx_loop_last_timing.argtypes = [ctypes.c_void_p] * 3
    L.orbx_loop_destroy.argtypes = [ctypes.c_void_p]
    assert L.orbx_loop_correct_sim3(None, None, None) == ERR_ARG
    assert L.orbx_loop_propagate_gba(None, None, None) == ERR_ARG
    assert L.orbx_loop_last_timing(None, None, None) == ERR_ARG
    L.orbx_loop_destroy(None)
    with pytest.raises(ValueError):
        bad = dict(ls.sim3_scene(3, 5, 1))
        bad["ref_scale"] = bad["ref_scale"][:-1]
        orbx.loop_marshal(bad, [])
    with pytest.raises(ValueError):
        bad = dict(ls.gba_scene(3, 5, 1))
        bad["in_gba"] = bad["in_gba"][:-1]
        orbx.loop_marshal(bad, [])


@pytest.mark.skipif(not os.access(REF / "include" / "KeyFrame.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-DOPTIMIZER_H", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "LoopClosing_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "LoopClosing_hip.cc").read_text()
    for piece in ("orbx_loop_correct_sim3(", "orbx_loop_propagate_gba(", "MapPointAccess.h", "shim_error.h", "SetWorldPos(", "SetPose(", "mnCorrectedByKF", "mnCorrectedReference",
                  "mTcwGBA", "mTcwBefGBA", "mnBAGlobalForKF", "mvpKeyFrameOrigins", "GetMapPointMatches()"):
        assert piece in text, piece
    head = (shim / "LoopClosing_hip.h").read_text()
    for piece in ("class LoopCorrection_hip", "CorrectLoopPropagate(", "PropagateGBA("):
        assert piece in head, piece
    assert "LoopClosing_hip" not in (ROOT / "oracle" / "Makefile").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    assert "LoopClosing_hip" in integ and "orbx_loop_correct_sim3" in integ and "orbx_loop_propagate_gba" in integ


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dev():
    return _orbx().LoopCorrection()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SIM3_CASES)
def test_correct_loop_equals_the_restatement(orbx, name):
    """G = 1 (the current keyframe alone), 3, 64 and 65; an empty list and a list of one; M = 0; points with 1, 63, 64, 65 and 300 observers; a point in
    every list; permuted and slot group orders; no list entry at all"""
    p, want = _sim3_case(name)
    got = _dev().CorrectLoop(p)
    _same(got, want, SIM3_FIELDS, name)
    ms, launches = _dev().last_timing()
    M, S = len(p["pos"]), len(p["list_point"])      # staging, the group, the claims (with entries), the points (with points), the results
    assert launches == 3 + (1 if M else 0) + (1 if M and S else 0) and ms > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", GBA_CASES)
def test_propagate_gba_equals_the_restatement(orbx, name):
    """n = 1; chains of 1, 3 and 40 non-optimised keyframes; branching trees at n = 65 and 300; M = 0, 1, 63, 64, 65 and 5000; two origins"""
    p, want = _gba_case(name)
    got = _dev().PropagateGBA(p)
    _same(got, want, GBA_FIELDS, name)
    ms, launches = _dev().last_timing()
    assert launches == 3 and ms > 0


@pytest.mark.gpu
def test_buffers_grow_from_call_to_call(orbx):
    dev = orbx.LoopCorrection()
    for name in ("g1", "g3", "g65", "g1"):
        _same(dev.CorrectLoop(_sim3_case(name)[0]), _sim3_case(name)[1], SIM3_FIELDS, ("grow", name))
    for name in ("n1", "chain3", "tree300", "chain40"):
        _same(dev.PropagateGBA(_gba_case(name)[0]), _gba_case(name)[1], GBA_FIELDS, ("grow", name))
    _same(dev.CorrectLoop(_sim3_case("g64")[0]), _sim3_case("g64")[1], SIM3_FIELDS, ("grow", "after gba"))
    dev.close()


@pytest.mark.gpu
def test_the_same_call_twice_gives_identical_bits(orbx):
    p = _sim3_case("g65")[0]
    a, b = _dev().CorrectLoop(p), _dev().CorrectLoop(p)
    _same(a, b, SIM3_FIELDS, "twice")
    q = _gba_case("tree300")[0]
    a, b = _dev().PropagateGBA(q), _dev().PropagateGBA(q)
    _same(a, b, GBA_FIELDS, "twice")


@pytest.mark.gpu
def test_c_abi_through_ctypes_agrees_with_the_class_and_null_results(orbx):
    L = orbx.load_library()
    L.orbx_loop_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.orbx_loop_destroy.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    assert L.orbx_loop_create(0, ctypes.byref(h)) == 0
    for p, want, fields in ((_sim3_case("g3") + (SIM3_FIELDS,)), (_gba_case("chain3") + (GBA_FIELDS,))):
        rc, o = _call_raw(orbx, h, p)
        assert rc == 0
        _same(o, want, fields, "raw")
        keep = []
        P, _ = orbx.loop_marshal(p, keep)
        sim3 = isinstance(P, orbx.LoopSim3Problem)
        fn = L.orbx_loop_correct_sim3 if sim3 else L.orbx_loop_propagate_gba
        assert fn(h, ctypes.byref(P), None) == 0                                                  # no result struct
        R = (orbx.LoopSim3Result if sim3 else orbx.LoopGbaResult)()
        assert fn(h, ctypes.byref(P), ctypes.byref(R)) == 0                                       # every result pointer NULL
    L.orbx_loop_destroy(h)
