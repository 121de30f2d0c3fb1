"""Steps 2 and 3 of LocalMapping::SearchInNeighbors on the device (orbx_search_in_neighbors / orbx_fuse_apply, csrc/orbx_fuse_chain.hip) against the literal
sequential restatement tests/fuse_chain_ref.py.  CPU: the restatement on hand-made cases of every branch, against the compiled reference's ORBmatcher::Fuse,
the vacuity guards of the scenes, the ABI without a device, the shim.  gpu: every field of every result equals the restatement - no tolerance."""
import ctypes
import math
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import fuse_chain_ref as fr
import fuse_chain_scenes as fs
import oracle_lib

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
ERR_ARG, ERR_CAPACITY = -1, -3
A, RBH, RH, HB = fr.ADDED, fr.REPLACED_BY_HOLDER, fr.REPLACED_HOLDER, fr.HOLDER_BAD


def _orbx():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd")


# ---------------------------------------------------------------------------------------------------------------------
# hand-made cases: (name, slice, keyframe slot, list, best_idx, best_dist[, active]).  Keyframe slot 0 is the one fused into; searchable
# keyframes 0 and 1; slots 2.. are other observers.  Ranks reverse the slots unless given.
# ---------------------------------------------------------------------------------------------------------------------
def hand_cases(orbx):
    H = lambda *a, **k: fs.hand_slice(orbx, *a, **k)      # noqa: E731
    c = []
    # add: point 0 (observed by keyframe 1) gains (0, 2)
    c.append(("add", H({0: [-1, -1, -1], 1: [0]}, 1), 0, [0], [2], [10]))
    # a stereo feature adds 2
    c.append(("add_stereo", H({0: [-1, -1], 1: [0]}, 1, stereo={0: {1}}), 0, [0], [1], [10]))
    # the holder has more observations: the list point is replaced by the holder
    c.append(("replaced_by_holder", H({0: [1], 1: [0]}, 2, other_obs=[(1, 2, 0, 0), (0, 3, 0, 0), (1, 4, 0, 0)]), 0, [0], [0], [20]))
    # the list point has more: the holder is replaced
    c.append(("replaced_holder", H({0: [1], 1: [0]}, 2, other_obs=[(0, 2, 0, 0), (0, 3, 1, 0)]), 0, [0], [0], [20]))
    # equal Observations(): the holder is replaced
    c.append(("equal", H({0: [1], 1: [0]}, 2), 0, [0], [0], [50]))
    # the holder is bad: nothing changes, nFused counts
    c.append(("holder_bad", H({0: [1], 1: [0]}, 2, bad=[0, 1]), 0, [0], [0], [5]))
    # both points are observed by keyframe 2: the loser's observation there is erased (point 0 loses: 2 observations against 3)
    c.append(("conflict_erase", H({0: [1, -1], 1: [0, 1]}, 2, other_obs=[(0, 2, 4, 0), (1, 2, 7, 0)]), 0, [0], [0], [9]))
    # ... and in a searchable keyframe: kf_point of the erased feature becomes -1 (keyframe 1 holds both)
    c.append(("conflict_erase_searchable", H({0: [1], 1: [0, 1]}, 2, other_obs=[(1, 2, 0, 0)]), 0, [0], [0], [9]))
    # two list points pick the same empty feature: the first adds, the second is replaced by it (first has 2 observations then, second 1) ...
    c.append(("same_empty_second_replaced", H({0: [-1], 1: [0, 1]}, 2), 0, [0, 1], [0, 0], [10, 11]))
    # ... or replaces it (the second has more observations)
    c.append(("same_empty_second_replaces", H({0: [-1], 1: [0, 1]}, 2, other_obs=[(1, 2, 0, 0), (1, 3, 0, 0)]), 0, [0, 1], [0, 0], [10, 11]))
    # a point that goes bad before its turn: entry 0 replaces point 1 (the holder), entry 1 is point 1
    c.append(("bad_before_turn", H({0: [1, -1], 1: [0]}, 2, other_obs=[(0, 2, 0, 0)]), 0, [0, 1], [0, 1], [10, 10]))
    # a -1 and a duplicate in the list, an entry that is not active, one beyond TH_LOW
    c.append(("null_duplicate", H({0: [-1, -1, -1], 1: [0, 1, 2]}, 3), 0, [-1, 0, 0, 1, 2], [0, 0, 1, 1, 2], [10, 10, 10, 51, 10], [1, 1, 1, 1, 0]))
    # a stereo observation moves: point 1 (held by 0 at a stereo feature, and by keyframe 2) is replaced by point 0 with three observations
    c.append(("stereo_moves", H({0: [1], 1: [0]}, 2, other_obs=[(0, 2, 0, 1), (0, 3, 0, 0), (1, 4, 0, 1)], stereo={0: {0}}), 0, [0], [0], [10]))
    # a bad observer keyframe takes no part in the new descriptor; ranks given
    c.append(("bad_observer", H({0: [1], 1: [0]}, 2, other_obs=[(0, 2, 0, 0), (0, 3, 0, 0), (1, 4, 0, 0), (1, 5, 0, 0)], kf_bad=[0, 0, 1, 0, 1, 0], ranks=[50, 10, 40, 20, 30, 0]),
              0, [0], [0], [10]))
    return [x if len(x) == 7 else x + ([1] * len(x[3]),) for x in c]


def _apply_ref(case):
    _, sl, kf, lst, bi, bd, act = case
    return fr.fuse_apply(sl, kf, lst, act, bi, bd)


def test_restatement_on_hand_made_cases(orbx):
    r = {c[0]: _apply_ref(c) for c in hand_cases(orbx)}
    rows = lambda name: [tuple(int(v) for v in row) for row in r[name]["log"]]      # noqa: E731
    kfp = lambda name, i: r[name]["kf_point"][i].tolist()                           # noqa: E731
    assert rows("add") == [(0, 0, 0, 2, A, -1)] and kfp("add", 0) == [-1, -1, 0] and r["add"]["point_obs"].tolist() == [2] and r["add"]["nfused"].tolist() == [1]
    # ranks reverse the slots: the observation of keyframe 0 comes behind the one of keyframe 1
    assert r["add"]["obs_kf"].tolist() == [0, 1] and r["add"]["obs_idx"].tolist() == [2, 0]
    assert r["add_stereo"]["point_obs"].tolist() == [3] and r["add_stereo"]["obs_stereo"].tolist() == [1, 0]
    x = r["replaced_by_holder"]
    assert rows("replaced_by_holder") == [(0, 0, 0, 0, RBH, 1)] and x["point_bad"].tolist() == [1, 0] and x["replaced"].tolist() == [1, -1]
    assert x["point_obs"].tolist() == [2, 5] and x["kf_point"][1].tolist() == [1] and x["obs_offset"].tolist() == [0, 0, 5]
    x = r["replaced_holder"]
    assert rows("replaced_holder") == [(0, 0, 0, 0, RH, 1)] and x["point_bad"].tolist() == [0, 1] and x["kf_point"][0].tolist() == [0] and x["point_obs"].tolist() == [4, 1]
    assert rows("equal") == [(0, 0, 0, 0, RH, 1)] and r["equal"]["replaced"].tolist() == [-1, 0]
    x = r["holder_bad"]
    assert rows("holder_bad") == [(0, 0, 0, 0, HB, 1)] and x["nfused"].tolist() == [1] and x["kf_point"][0].tolist() == [1] and x["point_obs"].tolist() == [1, 1]
    x = r["conflict_erase"]
    assert rows("conflict_erase") == [(0, 0, 0, 0, RBH, 1)] and x["conflict_erases"] == 2 and x["point_obs"].tolist() == [2, 3]      # keyframes 1 and 2 observe both
    assert x["kf_point"][1].tolist() == [-1, 1] and x["obs_offset"].tolist() == [0, 0, 3]
    x = r["conflict_erase_searchable"]
    assert x["conflict_erases"] == 1 and x["kf_point"][1].tolist() == [-1, 1] and x["kf_point"][0].tolist() == [1]
    x = r["same_empty_second_replaced"]
    assert rows("same_empty_second_replaced") == [(0, 0, 0, 0, A, -1), (0, 1, 1, 0, RBH, 0)] and x["point_bad"].tolist() == [0, 1] and x["kf_point"][1].tolist() == [0, -1]
    assert x["conflict_erases"] == 1 and x["nfused"].tolist() == [2]
    x = r["same_empty_second_replaces"]
    assert rows("same_empty_second_replaces") == [(0, 0, 0, 0, A, -1), (0, 1, 1, 0, RH, 0)] and x["point_bad"].tolist() == [1, 0] and x["kf_point"][0].tolist() == [1]
    x = r["bad_before_turn"]
    assert rows("bad_before_turn") == [(0, 0, 0, 0, RH, 1)] and x["nfused"].tolist() == [1] and x["kf_point"][0].tolist() == [0, -1]
    x = r["null_duplicate"]
    assert rows("null_duplicate") == [(0, 1, 0, 0, A, -1)] and x["nfused"].tolist() == [1] and x["kf_point"][0].tolist() == [0, -1, -1]
    x = r["stereo_moves"]
    assert rows("stereo_moves") == [(0, 0, 0, 0, RH, 1)] and x["point_obs"].tolist() == [4 + 2 + 2, 4] and x["obs_stereo"].sum() == 3
    # the found / visible counters of the loser go to the winner
    sl = hand_cases(orbx)[2][1]
    x = r["replaced_by_holder"]
    assert x["found"][1] == sl["found"][0] + sl["found"][1] and x["visible"][1] == sl["visible"][0] + sl["visible"][1]


def test_descriptor_rule_and_bad_observers(orbx):
    """ComputeDistinctiveDescriptors after Replace: the median at sorted position (N - 1) / 2, the first strictly smallest one, observers that are bad left out"""
    case = [c for c in hand_cases(orbx) if c[0] == "bad_observer"][0]
    sl = case[1]
    r = _apply_ref(case)
    st = fr.State(sl)
    assert [int(k) for k in r["log"][0]] == [0, 0, 0, 0, RH, 1]
    o0, o1 = r["obs_offset"][0], r["obs_offset"][1]
    kfs = r["obs_kf"][o0:o1].tolist()
    assert kfs == [5, 1, 3, 4, 2, 0]      # ascending rank 0, 10, 20, 30, 40, 50
    pool = {(int(kf), int(i)): d for kf, i, d in zip(sl["obs_kf"], sl["obs_idx"], sl["obs_desc"])}
    descs = [pool[(kf, int(i))] for kf, i in zip(kfs, r["obs_idx"][o0:o1]) if not st.kf_bad[kf]]
    assert len(descs) == 4
    med = [sorted(fr.hamming(a, b) for b in descs)[1] for a in descs]
    assert (r["desc"][0] == descs[med.index(min(med))]).all()
    # N = 0: the descriptor is kept
    sl2 = fs.hand_slice(orbx, {0: [1], 1: [0]}, 2, kf_bad=[1, 1])
    r2 = fr.fuse_apply(sl2, 0, [0], [1], [0], [10])
    assert (r2["desc"][0] == sl2["desc"][0]).all() and r2["point_bad"].tolist() == [0, 1]


def _chain_shapes():
    # (seed, T, M, mode, repeat, bad observer)
    return [(1, 3, 150, "mixed", False, False), (2, 3, 130, "mono", False, True), (3, 6, 110, "stereo", True, False), (4, 6, 100, "mixed", True, True)]


_CHAIN = {}


def _chain(orbx, cfg):
    """the scene and its restatement, computed once"""
    if cfg not in _CHAIN:
        seed, T, M, mode, rep, bo = cfg
        sl, cur, tg = fs.chain_scene(orbx, seed, T=T, M=M, mode=mode, repeat=rep, bad_observer=bo)
        _CHAIN[cfg] = (sl, cur, tg, fr.search_in_neighbors(sl, cur, tg))
    return _CHAIN[cfg]


@pytest.mark.parametrize("cfg", _chain_shapes())
def test_scene_vacuity_guards(orbx, cfg):
    sl, cur, tg, want = _chain(orbx, cfg)
    kinds = np.bincount(want["log"][:, 4], minlength=4)
    assert (kinds >= 5).all() and want["conflict_erases"] >= 5, (kinds, want["conflict_erases"])
    assert 150 <= len(sl["bad"]) <= 400 and all(64 <= len(k["kps"]) <= 200 for k in sl["searchable"])
    assert len(tg) == (7 if cfg[4] else 3) and (not cfg[4] or len(set(tg)) < len(tg))
    assert len(want["candidates"]) == len(set(want["candidates"].tolist())) and (want["nfused"] > 0).all()
    assert -1 in fr.State(sl).kf_point[0]
    # independent calls would fuse differently: some call's log differs from what the same call gives on the INITIAL state
    differ = 0
    for c, t in enumerate(tg):
        st, log = fr.State(sl), []
        fr.fuse(st, st.sidx[t], list(st.kf_point[st.sidx[cur]]), c, log)
        mine = [tuple(r) for r in want["log"][want["log"][:, 0] == c].tolist()]
        differ += mine != [tuple(r) for r in log]
    assert differ >= 1
    # the gather removes duplicates: the targets hold more good points than there are candidates
    st = fr.State(sl)
    assert sum(1 for t in tg for p in st.kf_point[st.sidx[t]] if p >= 0) > len(want["candidates"])
    if cfg[3] != "mono":
        assert want["obs_stereo"].sum() > 0 and any((k["u_right"] >= 0).any() for k in sl["searchable"])
    if cfg[5]:
        assert np.asarray(sl["kf_bad"]).sum() == 1


def test_descriptor_change_changes_a_later_match(orbx):
    """a Replace in target t rewrites the winner's descriptor, and target t + 1 then matches where the old descriptor would not have.  The current keyframe's point
    starts with a descriptor 45 bits from its feature in target 0 and further than TH_LOW from its feature in target 1; replacing target 0's weak holder gives it
    the distinctive descriptor of its observations, which is close to both."""
    info = {}
    sl, cur, tg = fs.chain_scene(orbx, 31, T=2, M=80, mode="mixed", present=1.0, info=info)
    rng = np.random.default_rng(1)
    desc = np.asarray(sl["desc"]).copy()
    mine = []
    for j in np.flatnonzero(info["cat"] == 2):
        p, f0, f1 = info["old"][j], info["feature"][(1, int(j))], info["feature"][(2, int(j))]
        d0, d1 = sl["searchable"][1]["desc"][f0], sl["searchable"][2]["desc"][f1]
        same = np.flatnonzero(np.unpackbits(d0 ^ d1) == 0)
        if fr.hamming(d0, d1) < 6:
            continue
        bits = np.unpackbits(d0)
        bits[rng.choice(same, 45, replace=False)] ^= 1
        desc[p] = np.packbits(bits)
        mine.append(p)
    sl = dict(sl, desc=desc)
    want = fr.search_in_neighbors(sl, cur, tg)
    lst = want["list"][1].tolist()
    hit = 0
    for p in mine:
        i = lst.index(p)
        rows0 = [r for r in want["log"].tolist() if r[0] == 0 and r[2] == p and r[4] == RH]
        if not rows0 or not want["active"][1][i]:
            continue
        st = fr.State(sl)      # the old descriptor against target 1, everything else as prepared
        bi0, bd0 = fr.search(st, st.sidx[tg[1]], [p], {k: want[k][1][i:i + 1] for k in ("active", "u", "v", "ur", "level", "radius")})
        hit += int(want["best_dist"][1][i] <= fr.TH_LOW < bd0[0] and any(r[0] == 1 and r[2] == p for r in want["log"].tolist()))
    assert hit >= 3


def test_search_restatement_equals_the_compiled_one(orbx, oracle):
    """the numpy search of the restatement against oracle/match_oracle.cc's, on the prepare values of a chain's calls"""
    sl, cur, tg, want = _chain(orbx, _chain_shapes()[0])
    st = fr.State(sl)
    for c, t in enumerate(tg):
        k = sl["searchable"][st.sidx[t]]
        lst = want["list"][c]
        pts = dict(u=want["u"][c], v=want["v"][c], ur=want["ur"][c], level=want["level"][c], radius=want["radius"][c], active=want["active"][c],
                   desc=np.array([sl["desc"][max(int(p), 0)] for p in lst], np.uint8))
        if c > 0:
            continue      # (later calls search with rewritten descriptors; the first call's are the slice's)
        kf = dict(kps=k["kps"], desc=k["desc"], u_right=k["u_right"], inv_level_sigma2=k["inv_level_sigma2"], width=640, height=480)
        bi, bd = oracle_lib.fuse_best(oracle, kf, pts, True)
        assert (bi == want["best_idx"][c]).all() and (bd == want["best_dist"][c]).all() and (bd <= fr.TH_LOW).sum() > 20


@pytest.mark.skipif(oracle_lib.slam_lib() is None, reason="oracle/_ref/liborbslam.so not built (needs the reference sources)")
@pytest.mark.parametrize("seed", [51, 52])
def test_one_call_equals_the_compiled_reference(orbx, seed):
    """ORBmatcher::Fuse of the reference on real KeyFrame / MapPoint objects (oracle/refslam_wrap.cc:orbslam_fuse): nfused, the target's holders, bad, replaced and
    the prepare values, bit for bit"""
    from test_fuse import _scene, _sim3
    kf, Tt, sk, Ts, P, cdesc, rng = _scene(orbx, seed)
    n, nc, n_exist = len(kf["kps"]), len(P), 120
    holder = np.full(n, -1, np.int32)
    holder[rng.choice(n, n_exist, replace=False)] = np.arange(n_exist)
    exist_obs = rng.integers(0, 5, n_exist).astype(np.int32)
    cand_obs = rng.integers(0, 4, nc).astype(np.int32)
    lst = np.concatenate([rng.permutation(nc), rng.integers(0, nc, 60)]).astype(np.int32)
    lst[rng.choice(len(lst), 25, replace=False)] = -1
    want = oracle_lib.ref_fuse(1, kf, Tt, _sim3(Tt), holder, exist_obs, sk, Ts, P, cdesc, cand_obs, lst, 3.0, False)
    # the same map as a slice: slot 0 the target, 1 the source keyframe, 2..5 the four extra observers; candidates 0..nc-1, existing points behind them
    f32 = np.float32
    T = np.asarray(Tt, f32)
    ow = np.zeros(3, f32)
    for r in range(3):
        o = (-T[0, r]) * T[0, 3]
        o = o + (-T[1, r]) * T[1, 3]
        o = o + (-T[2, r]) * T[2, 3]
        ow[r] = o
    pos = np.concatenate([np.asarray(P, f32), np.array([[0, 0, 2.0 + k] for k in range(n_exist)], f32)])
    octv = np.concatenate([np.asarray(sk["octave"]), np.full(n_exist, sk["octave"][0])])
    dist = np.array([f32(math.sqrt(sum(float(c) * float(c) for c in p))) for p in pos], f32)
    nrm = np.array([[f32(float(c) / math.sqrt(sum(float(q) * float(q) for q in p))) for c in p] for p in pos], f32)
    rawmax = (dist * fs.SF[octv]).astype(f32)
    NP = nc + n_exist
    pts = dict(pos=pos, normal=nrm, raw_max_dist=rawmax, max_dist=(f32(1.2) * rawmax).astype(f32), min_dist=(f32(0.8) * (rawmax / fs.SF[7]).astype(f32)).astype(f32),
               desc=np.concatenate([cdesc, np.tile(cdesc[0], (n_exist, 1))]), bad=np.zeros(NP, np.uint8), visible=np.ones(NP, np.int32), found=np.ones(NP, np.int32))
    kfp = np.where(holder >= 0, nc + holder, -1).astype(np.int32)
    target = dict(slot=0, kps=kf["kps"], desc=kf["desc"], u_right=kf["u_right"], kf_point=kfp, Tcw=T, ow=ow, cam=fs.CAM, bounds=fs.BOUNDS, scale_factors=fs.SF,
                  inv_level_sigma2=kf["inv_level_sigma2"], log_scale_factor=f32(math.log(float(f32(1.2)))))
    other = [(c, 1, c, 0, cdesc[c]) for c in range(nc)] + [(c, 2 + e, c, 0, cdesc[c]) for c in range(nc) for e in range(min(int(cand_obs[c]), 4))]
    for k in range(n_exist):
        i = 1 + (k % (nc - 1))
        other += [(nc + k, 2 + e, i, 0, cdesc[i]) for e in range(min(int(exist_obs[k]), 4))]
    sl = orbx.fuse_slice([target], pts, other, num_keyframes=6)
    st, log, keep = fr.State(sl), [], []
    nfused = fr.fuse(st, 0, [int(p) for p in lst], 0, log, keep)
    assert nfused == want["nfused"] and nfused > 200
    got_holder = np.array([-1 if p < 0 else (p if p < nc else 1000000 + p - nc) for p in st.kf_point[0]], np.int32)
    assert (got_holder == want["holder"]).all()
    assert (np.array(st.bad[:nc], np.uint8) == want["bad"]).all() and want["bad"].sum() > 5
    rep = np.array([-1 if p < 0 else (p if p < nc else 1000000 + p - nc) for p in st.replaced[:nc]], np.int32)
    assert (rep == want["replaced"]).all()
    # the prepare values of the reference are those of every candidate against the untouched target
    prep = fr.prepare(fr.State(sl), 0, list(range(nc)))
    pw = want["points"]
    assert (prep["active"] == pw["active"]).all() and 0 < prep["active"].sum() < nc
    on = prep["active"] > 0
    for k in ("u", "v", "ur", "radius"):
        assert (prep[k][on].view(np.uint32) == np.asarray(pw[k], f32)[on].view(np.uint32)).all(), k
    assert (prep["level"][on] == pw["level"][on]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a device, the shim
# ---------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("orbx_search_in_neighbors", "orbx_fuse_apply", "orbx_search_in_neighbors_last_timing")


def _bind(orbx):
    L = orbx.load_library()
    L.orbx_last_error.restype = ctypes.c_char_p
    L.orbx_search_in_neighbors.argtypes = [ctypes.c_void_p, ctypes.POINTER(orbx.FuseSlice), ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(orbx.FuseResult)]
    L.orbx_fuse_apply.argtypes = [ctypes.c_void_p, ctypes.POINTER(orbx.FuseSlice), ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.POINTER(orbx.FuseResult)]
    return L


def _bad_slices(orbx):
    base = fs.hand_slice(orbx, {0: [1, -1], 1: [0, 1]}, 2, other_obs=[(0, 2, 4, 0), (1, 2, 7, 0)])
    out = []

    def mod(name, text, **kw):
        s = dict(base)
        s.update(kw)
        out.append((name, s, text))
    mod("rank", "same rank", kf_rank=np.array([1, 1, 2], np.int32))
    mod("offset", "obs_offset", obs_offset=np.array([0, 3, 5], np.int32)[::-1].copy())
    mod("obs_kf", "no keyframe slot", obs_kf=np.array([9] + list(base["obs_kf"][1:]), np.int32))
    o = np.asarray(base["obs_kf"]).copy()
    o[[0, 1]] = o[[1, 0]]
    mod("order", "ascending rank", obs_kf=o)
    k1 = dict(base["searchable"][1], kf_point=np.array([0, -1], np.int32))
    mod("consistency", "hold", searchable=[base["searchable"][0], k1])
    k0 = dict(base["searchable"][0], kf_point=np.array([1, 0], np.int32))
    mod("unobserved", "observe their keyframe", searchable=[k0, base["searchable"][1]])
    k0 = dict(base["searchable"][0], kf_point=np.array([1, 5], np.int32))
    mod("point", "no point", searchable=[k0, base["searchable"][1]])
    mod("twice", "searchable twice", searchable=[base["searchable"][0], dict(base["searchable"][1], slot=0)])
    return base, out


def test_exports_and_bad_arguments_without_a_device(orbx):
    L = _bind(orbx)
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
    assert all(hasattr(orbx.ORBmatcher, k) for k in ("SearchInNeighbors", "FuseApply", "search_in_neighbors_last_timing")) and hasattr(orbx, "fuse_slice") and hasattr(orbx, "fuse_marshal")
    assert "orbx_search_in_neighbors" in (ROOT / "__graft_entry__.py").read_text() and "orbx_fuse_chain.hip" in orbx.build_mod.HIP_SOURCES
    R = orbx.FuseResult()
    assert L.orbx_search_in_neighbors(None, None, 0, None, 0, ctypes.byref(R)) == ERR_ARG and b"NULL slice" in L.orbx_last_error()
    assert L.orbx_fuse_apply(None, None, 0, None, None, None, None, 0, ctypes.byref(R)) == ERR_ARG and b"NULL slice" in L.orbx_last_error()
    base, bad = _bad_slices(orbx)
    keep = []
    S, _ = orbx.fuse_marshal(base, keep)
    assert L.orbx_search_in_neighbors(None, ctypes.byref(S), 0, None, 0, None) == ERR_ARG and b"NULL result" in L.orbx_last_error()
    assert L.orbx_search_in_neighbors(None, ctypes.byref(S), 0, None, 0, ctypes.byref(R)) == ERR_ARG and b"NULL handle" in L.orbx_last_error()      # a good slice, no handle
    S.pos = None
    assert L.orbx_search_in_neighbors(None, ctypes.byref(S), 0, None, 0, ctypes.byref(R)) == ERR_ARG and b"NULL slice array" in L.orbx_last_error()
    for name, s, text in bad:      # inconsistent slices are reported as such before the handle is looked at
        S, _ = orbx.fuse_marshal(s, keep)
        assert L.orbx_search_in_neighbors(None, ctypes.byref(S), 0, None, 0, ctypes.byref(R)) == ERR_ARG, name
        assert text.encode() in L.orbx_last_error(), (name, L.orbx_last_error())
        assert L.orbx_fuse_apply(None, ctypes.byref(S), 0, None, None, None, None, 0, ctypes.byref(R)) == ERR_ARG, name
    big = dict(base["searchable"][0])
    S, _ = orbx.fuse_marshal(base, keep)
    tab = ctypes.cast(S.searchable, ctypes.POINTER(orbx.FuseKeyFrame))
    tab[0].nlevels = 13
    assert L.orbx_search_in_neighbors(None, ctypes.byref(S), 0, None, 0, ctypes.byref(R)) == ERR_CAPACITY and b"levels" in L.orbx_last_error()
    tab[0].nlevels = 8
    tab[0].num_features = 70000
    assert L.orbx_search_in_neighbors(None, ctypes.byref(S), 0, None, 0, ctypes.byref(R)) == ERR_CAPACITY and b"65535" in L.orbx_last_error()
    assert big["slot"] == 0


@pytest.mark.skipif(not os.access(REF / "include" / "KeyFrame.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "SearchInNeighbors_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "SearchInNeighbors_hip.cc").read_text()
    for piece in ("orbx_search_in_neighbors(", "Replace(", "AddObservation(", "AddMapPoint(", "shim_error.h"):
        assert piece in text, piece
    assert "SearchInNeighbors_hip" not in (ROOT / "oracle" / "Makefile").read_text()


# ---------------------------------------------------------------------------------------------------------------------
# gpu
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matcher(orbx):
    m = orbx.ORBmatcher(0.6, True, max_features=256)
    yield m
    m.close()


@pytest.mark.gpu
def test_fuse_apply_on_hand_made_cases(orbx, matcher):
    for case in hand_cases(orbx):
        name, sl, kf, lst, bi, bd, act = case
        fr.assert_equal_results(matcher.FuseApply(sl, kf, lst, act, bi, bd), _apply_ref(case), name)


def _decision_list_case(orbx, n, seed):
    """n entries, every one a decision: keyframe 0 has n features holding weak points or nothing, the list is n points of keyframe 1"""
    rng = np.random.default_rng(seed)
    kfp0 = [(n + i if rng.random() < 0.6 else -1) for i in range(n)]
    held = [p for p in kfp0 if p >= 0]
    other = [(p, 2, i, 0) for i, p in enumerate(held) if rng.random() < 0.5] + [(i, 3, i, int(rng.random() < 0.3)) for i in range(n) if rng.random() < 0.5]
    sl = fs.hand_slice(orbx, {0: kfp0, 1: list(range(n))}, 2 * n, other_obs=other, stereo={0: set(range(0, n, 3))}, seed=seed)
    # points n.. that keyframe 0 does not hold are unobserved: fine (they are never listed)
    return sl, 0, list(range(n)), rng.permutation(n).tolist(), rng.integers(0, 51, n).tolist(), [1] * n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 300])
def test_fuse_apply_lists_around_a_wave(orbx, matcher, n):
    sl, kf, lst, bi, bd, act = _decision_list_case(orbx, n, n)
    want = fr.fuse_apply(sl, kf, lst, act, bi, bd)
    assert want["nfused"][0] == n and len(want["log"]) == n
    fr.assert_equal_results(matcher.FuseApply(sl, kf, lst, act, bi, bd), want)


@pytest.mark.gpu
@pytest.mark.parametrize("nobs,nbad", [(70, 0), (150, 9), (600, 0)])
def test_fuse_apply_long_observation_lists(orbx, matcher, nobs, nbad):
    """a point with more observations than a wave (and than the descriptors kept in LDS): the merge, the re-check and the median run past 64 / 256 / 512"""
    NK = 2 + 2 * nobs
    other = [(0, 2 + 2 * i, i, i % 5 == 0) for i in range(nobs)] + [(1, 3 + 2 * i, i, 0) for i in range(nobs - 1)] + [(1, 2, 7, 0)]      # keyframe 2 observes both
    kf_bad = np.zeros(NK, np.uint8)
    kf_bad[4:4 + 2 * nbad:2] = 1
    sl = fs.hand_slice(orbx, {0: [1, -1], 1: [0]}, 2, other_obs=other, num_keyframes=NK, kf_bad=kf_bad, ranks=np.random.default_rng(nobs).permutation(NK), seed=nobs)
    want = fr.fuse_apply(sl, 0, [0], [1], [0], [10])
    assert want["log"][0, 4] == RH and want["conflict_erases"] == 1 and want["obs_offset"][1] == 2 * nobs + 1
    fr.assert_equal_results(matcher.FuseApply(sl, 0, [0], [1], [0], [10]), want)


@pytest.mark.gpu
def test_fuse_apply_empty_keyframe_and_empty_list(orbx, matcher):
    sl = fs.hand_slice(orbx, {0: [], 1: [0, 1]}, 2)
    fr.assert_equal_results(matcher.FuseApply(sl, 0, [0, 1], [0, 0], [-1, -1], [256, 256]), fr.fuse_apply(sl, 0, [0, 1], [0, 0], [-1, -1], [256, 256]), "0 features")
    r = matcher.FuseApply(sl, 1, [], [], [], [])
    fr.assert_equal_results(r, fr.fuse_apply(sl, 1, [], [], [], []), "empty list")
    assert len(r["log"]) == 0 and r["nfused"].tolist() == [0]
    # ... and the chain on a keyframe without features: no target has anything to match, the reverse pass lists nothing it could place
    r = matcher.SearchInNeighbors(sl, 0, [1], full=True)
    fr.assert_equal_results(r, fr.search_in_neighbors(sl, 0, [1]), "chain, 0 features")
    assert r["candidates"].tolist() == [0, 1]


def _assert_full(got, want):
    """the prepare and search results of every call, floats by bit pattern"""
    for c in range(len(want["list"])):
        assert (got["active"][c] == want["active"][c]).all(), c
        on = want["active"][c] > 0
        for k in ("u", "v", "ur", "radius"):
            assert (np.asarray(got[k][c], np.float32)[on].view(np.uint32) == np.asarray(want[k][c], np.float32)[on].view(np.uint32)).all(), (c, k)
        assert (got["level"][c][on] == want["level"][c][on]).all(), c
        assert (got["best_idx"][c] == want["best_idx"][c]).all() and (got["best_dist"][c] == want["best_dist"][c]).all(), c


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", _chain_shapes())
def test_chain_equals_restatement(orbx, matcher, cfg):
    sl, cur, tg, want = _chain(orbx, cfg)
    got = matcher.SearchInNeighbors(sl, cur, tg, full=True)
    _assert_full(got, want)
    fr.assert_equal_results(got, want)
    plain = matcher.SearchInNeighbors(sl, cur, tg)      # without the per-call arrays: the same chain on one reused region
    fr.assert_equal_results(plain, want)
    ms, launches, apply_ms = matcher.search_in_neighbors_last_timing()
    assert launches == 2 + 3 * (len(tg) + 1) + 2 + 1 and ms > 0 and apply_ms == 0


@pytest.mark.gpu
def test_chain_equals_single_calls_through_the_host(orbx, matcher):
    """T + 1 synchronous single calls with the state fed back between them: the device's own search (FuseSearch) on the restatement's prepare values, FuseApply, and
    the next slice from the result"""
    cfg = _chain_shapes()[0]
    sl, cur, tg, want = _chain(orbx, cfg)
    chain = matcher.SearchInNeighbors(sl, cur, tg)
    state, logs, nfused = sl, [], []
    replaced = np.full(len(sl["bad"]), -1, np.int32)      # (GetReplaced() is no input of a call: a fresh slice starts without it)
    lst = [int(p) for p in np.asarray(sl["searchable"][0]["kf_point"])]
    for c, t in enumerate(list(tg) + [cur]):
        st = fr.State(state)
        if c == len(tg):
            lst = fr.gather(st, tg)
            assert lst == chain["candidates"].tolist()
        si = st.sidx[t]
        prep = fr.prepare(st, si, lst)
        k = state["searchable"][si]
        pts = dict(prep, desc=np.array([state["desc"][max(p, 0)] for p in lst], np.uint8).reshape(-1, 32))
        bi, bd = matcher.FuseSearch(dict(kps=k["kps"], desc=k["desc"], u_right=k["u_right"], inv_level_sigma2=k["inv_level_sigma2"], width=640, height=480), pts, True)
        r = matcher.FuseApply(state, t, lst, prep["active"], bi, bd)
        rows = fr.log_rows(r["log"])
        rows[:, 0] = c
        logs.append(rows)
        nfused.append(int(r["nfused"][0]))
        replaced = np.where(r["replaced"] >= 0, r["replaced"], replaced)
        state = orbx.fuse_next_slice(state, r)
    assert (np.concatenate(logs) == fr.log_rows(chain["log"])).all() and nfused == chain["nfused"].tolist()
    good = chain["point_bad"] == 0      # (Observations() of a replaced point is not modelled: the chain keeps the old count, a fresh slice derives 0)
    for k in ("point_bad", "visible", "found", "desc", "obs_offset", "obs_kf", "obs_idx", "obs_stereo"):
        assert (np.asarray(r[k]) == np.asarray(chain[k])).all(), k
    assert (replaced == chain["replaced"]).all()
    assert (r["point_obs"][good] == chain["point_obs"][good]).all()
    for a, b in zip(r["kf_point"], chain["kf_point"]):
        assert (a == b).all()


@pytest.mark.gpu
def test_capacity_and_errors(orbx, matcher):
    sl, cur, tg, want = _chain(orbx, _chain_shapes()[0])
    L = _bind(orbx)
    for kw in (dict(log_capacity=len(want["log"]) - 1), dict(candidates_capacity=len(want["candidates"]) - 1), dict(obs_capacity=len(want["obs_kf"]) - 1)):
        call = matcher.search_in_neighbors_prepare(sl, cur, tg, **kw)
        o = [x for x in call.keep if isinstance(x, dict) and "log" in x][0]
        for v in o.values():
            v.view(np.uint8)[...] = 0xA5
        assert call.raw() == ERR_CAPACITY and b"capacities" in L.orbx_last_error(), kw
        assert all((v.view(np.uint8) == 0xA5).all() for v in o.values()), kw      # nothing was written
        fr.assert_equal_results(matcher.SearchInNeighbors(sl, cur, tg), want)      # the handle remains usable
    # exact capacities suffice
    fr.assert_equal_results(matcher.SearchInNeighbors(sl, cur, tg, log_capacity=len(want["log"]), candidates_capacity=len(want["candidates"]), obs_capacity=len(want["obs_kf"])), want)
    # a target that is the current keyframe, or not searchable
    for bad_targets in ([cur], [len(sl["kf_rank"]) - 1], [99]):
        with pytest.raises(orbx.OrbxError) as e:
            matcher.SearchInNeighbors(sl, cur, bad_targets)
        assert e.value.code == ERR_ARG
    with pytest.raises(orbx.OrbxError) as e:
        matcher.FuseApply(sl, cur, [0], [1], [100000], [10])
    assert e.value.code == ERR_ARG
    fr.assert_equal_results(matcher.SearchInNeighbors(sl, cur, tg), want)


@pytest.mark.gpu
def test_handle_grows_and_returns(orbx):
    """a fresh handle: a small call, a larger one (every buffer grows), the small one again - each equal to the restatement, and the matcher's other calls still work"""
    m = orbx.ORBmatcher(0.6, True, max_features=256)
    small, big = _chain(orbx, _chain_shapes()[1]), _chain(orbx, _chain_shapes()[3])
    case = hand_cases(orbx)[0]
    for sl, cur, tg, want in (small, big, small):
        fr.assert_equal_results(m.SearchInNeighbors(sl, cur, tg), want)
        fr.assert_equal_results(m.FuseApply(case[1], case[2], case[3], case[6], case[4], case[5]), _apply_ref(case))
    m.close()
