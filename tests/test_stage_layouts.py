"""The staged layouts of the single calls (csrc/orbx_stage.h planned by every host-array entry point) at the shapes where a layout can go wrong:
optional arrays present and absent on one handle, a buffer that grows between two small calls, sizes on the 256-byte padding boundary, a
capacity above the count, regions of no bytes.  Every result is compared with the reference its module's own test uses."""
import numpy as np
import pytest

import covis_ref as cr
import covis_scenes as cs
import essential_graph_ref as eg
import kfdb_ref as kr
import mappoint_ref as mr
import oracle_lib
import sim3_ref as sr
import test_covisibility as tcov
import test_essential_graph as teg
import test_frustum as tfr
import test_kfdb as tkf
import test_mappoint_refresh as tmp
import test_new_map_points as tnp
import test_projection as tpr
import test_sim3_solver as ts3
import triangulate_ref as tr

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------------
# optional arrays: the same call with and without them on ONE handle, alternating three times
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_mappoint_ops_with_and_without_desc_valid(orbx):
    rng = np.random.default_rng(21)
    pts = []
    for n in (1, 3, 64, 65, 130):
        q = mr.synth_point(rng, n)
        q["valid"] = (rng.random(n) < 0.6).astype(np.uint8)
        q["valid"][n - 1] = 1
        pts.append(q)
    masked = mr.pack(pts)
    free = dict(masked, desc_valid=None)
    want_masked, want_free = mr.restate(masked), mr.restate(free)
    assert not mr.same_bits(want_masked, want_free)      # the mask decides something
    ops = orbx.MapPointOps(64, 512)
    for _ in range(3):
        assert mr.same_bits(tmp.run(ops, masked), want_masked)
        assert mr.same_bits(tmp.run(ops, free), want_free)
    ops.close()


def _search_by_projection(orbx, mt, frame, pts, th, occupied, has_obs):
    """ORBmatcher.SearchByProjection with frame.occupied / points.has_observations NULL on request (the class always passes both)"""
    import ctypes
    k = np.ascontiguousarray(frame["kps"], orbx.KEYPOINT_DTYPE)
    n, m = len(k), len(pts["proj_x"])
    f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731
    u8 = lambda a: np.ascontiguousarray(a, np.uint8)         # noqa: E731
    d, ur, sf = u8(frame["desc"]), f32(frame["u_right"]), f32(frame["scale_factors"])
    occ, obs = u8(frame["occupied"]), u8(pts["has_obs"])
    px, py, pxr, vc = f32(pts["proj_x"]), f32(pts["proj_y"]), f32(pts["proj_xr"]), f32(pts["view_cos"])
    lvl, inv, md = np.ascontiguousarray(pts["level"], np.int32), u8(pts["in_view"]), u8(pts["desc"])
    cn, cm = np.array([n], np.int32), np.array([m], np.int32)
    gw, gh = np.float32(64) / np.float32(frame["width"]), np.float32(48) / np.float32(frame["height"])
    F = orbx.ProjectionFrame(k.ctypes.data, d.ctypes.data, ur.ctypes.data, occ.ctypes.data if occupied else None, cn.ctypes.data, n, 1, 0.0, 0.0, float(gw), float(gh))
    P = orbx.ProjectionPoints(px.ctypes.data, py.ctypes.data, pxr.ctypes.data, lvl.ctypes.data, vc.ctypes.data, inv.ctypes.data, obs.ctypes.data if has_obs else None,
                              md.ctypes.data, cm.ctypes.data, m)
    out, nm = np.full(n, -1, np.int32), ctypes.c_int32()
    rc = mt._L.orbx_search_by_projection(mt._h, ctypes.byref(F), ctypes.byref(P), sf.ctypes.data_as(ctypes.c_void_p), len(sf), ctypes.c_float(th), ctypes.c_float(mt.nnratio),
                                         out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nm))
    orbx._check(rc)
    return nm.value, out


def test_search_by_projection_with_and_without_flags(orbx, oracle):
    """NULL occupied = no feature occupied, NULL has_observations = every point has some (include/orbx.h)"""
    fr, pts = tpr.make_case(7, n=300, m=260)
    frame = dict(fr, kps=tpr._struct_kps(orbx, fr["kps7"]))
    none_fr, all_pts = dict(fr, occupied=np.zeros(300, np.uint8)), dict(pts, has_obs=np.ones(260, np.uint8))
    want = {(True, True): oracle_lib.search_by_projection(oracle, fr, pts, 3.0, 0.8), (False, False): oracle_lib.search_by_projection(oracle, none_fr, all_pts, 3.0, 0.8),
            (True, False): oracle_lib.search_by_projection(oracle, fr, all_pts, 3.0, 0.8)}
    assert not (want[(True, True)][1] == want[(False, False)][1]).all()
    mt = orbx.ORBmatcher(0.8, True, max_features=512)
    # the class's own path first (both arrays), as the module's test calls it
    n0, a0 = mt.SearchByProjection(frame, pts, 3.0)
    assert n0 == want[(True, True)][0] and (a0 == want[(True, True)][1]).all()
    for _ in range(3):
        for key in ((True, True), (False, False), (True, False)):
            got_n, got = _search_by_projection(orbx, mt, frame, pts, 3.0, *key)
            assert got_n == want[key][0] and (got == want[key][1]).all(), key
    mt.close()


def test_triangulate_matches_with_and_without_raw_and_stereo(orbx):
    p, _ = tnp._pair("short_stereo_63")
    full = dict(p)
    for o in ("o1", "o2"):      # explicit raw keys, half a pixel off the undistorted ones (the stereo path unprojects them)
        k = p[o]["kps"]
        full[o] = dict(p[o], raw=np.stack([k["x"] + np.float32(0.5), k["y"] - np.float32(0.25)], 1).astype(np.float32))
    bare = dict(p, o1=dict(p["o1"], raw=None, u_right=None, depth=None), o2=dict(p["o2"], raw=None, u_right=None, depth=None))
    noraw = dict(p, o1=dict(p["o1"], raw=None), o2=dict(p["o2"], raw=None))
    cases = [(c, tr.triangulate(c["g1"], c["g2"], c["o1"], c["o2"], c["idx1"], c["idx2"])) for c in (full, bare, noraw)]
    assert ((cases[0][1]["status"] == tr.STEREO1) | (cases[0][1]["status"] == tr.STEREO2)).any() and not (cases[0][1]["status"] == cases[1][1]["status"]).all()
    assert not np.array_equal(cases[0][1]["x3d"], cases[2][1]["x3d"])      # the raw keys decide something too
    mt = orbx.ORBmatcher(0.6, False, max_features=128)
    for _ in range(3):
        for c, want in cases:
            tnp._check_geometry(mt.TriangulateMatches([c]), want)
    tnp._check_geometry(mt.TriangulateMatches([full, bare, noraw]), {k: np.concatenate([w[k] for _, w in cases]) for k in ("status", "x3d", "near", "dist1")})
    mt.close()


def test_covisibility_connections_culling_connections(orbx):
    """culling stages four arrays more than the connections do"""
    a, b = cs.tie_scene(), cs.cascade_scene()
    want_a, want_b = cr.update_connections(a), cr.keyframe_culling(b)
    cov = orbx.Covisibility()
    for _ in range(3):
        tcov._same(cov.UpdateConnections(a), want_a, tcov.CONN_FIELDS, "connections")
        tcov._same(cov.KeyFrameCulling(b), want_b, tcov.CULL_FIELDS, "culling")
    tcov._same(cov.UpdateConnections(a), want_a, tcov.CONN_FIELDS, "connections")
    cov.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# growth: a small call, one at least four times larger, the small one again
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sim3_solve(h, names):
    cs_ = [ts3._scene(n) for n in names]
    mi, fs = ts3._row(names[0])[5], ts3._row(names[0])[6]
    out = h.Solve(cs_, sets=[c["sets"] for c in cs_], min_inliers=mi, fix_scale=fs, full=True)
    for r in out:
        r.masks = np.array([r.inliers(it) for it in range(r.iterations)], bool).reshape(r.iterations, r.n)
    return out


def _sim3_check(name, d):
    """counts and masks against the restatement's inlier check of the device's own models, the events against its scan (tests/test_sim3_solver.py)"""
    c, mi = ts3._scene(name), ts3._row(name)[5]
    if d.iterations:
        count, inl = sr.check_inliers(ts3._con(d), c["K1"], c["K2"], d.t12m, d.t21m)
        assert (d.count == count).all() and (d.masks == inl).all()
    ev, first, best = sr.scan_events(d.count, mi)
    assert (d.is_event == ev).all() and d.first_event == first and d.best_iteration == best and d.no_more == (d.n < mi or first < 0)


def _sim3_bits(r):
    return [np.ascontiguousarray(getattr(r, k)).tobytes() for k in ("r12", "t12", "s12", "count", "is_event", "inliers_first", "x3dc1", "x3dc2", "p1im1", "p2im2", "max_err1", "max_err2",
                                                                      "nmat", "quat", "t12m", "t21m", "masks")] + [r.first_event, r.best_iteration, r.no_more]


def test_sim3_solver_grows_and_returns():
    h = ts3._orbx().Sim3Solver(max_candidates=2, max_matches=1024, max_iterations=300)
    small = _sim3_solve(h, ["general_21"])[0]          # 21 matches, 7 iterations
    large = _sim3_solve(h, ["general_1000"])[0]        # 1000 matches, 300 iterations: both mapped buffers grow
    again = _sim3_solve(h, ["general_21"])[0]
    _sim3_check("general_21", small)
    _sim3_check("general_1000", large)
    assert _sim3_bits(small) == _sim3_bits(again)
    h.close()


def test_mappoint_ops_grows_and_returns(orbx):
    small, large = mr.synth_batch([1, 2, 65], seed=31), mr.concat(mr.synth_batch([3, 64, 256, 300, 600] * 3, seed=32), tmp.window())
    assert len(large["desc"]) >= 4 * len(small["desc"])
    want_small, want_large = mr.restate(small), mr.restate(large)
    ops = orbx.MapPointOps(1024, 16384)
    first = tmp.run(ops, small)
    assert mr.same_bits(first, want_small)
    assert mr.same_bits(tmp.run(ops, large), want_large)
    third = tmp.run(ops, small)
    assert mr.same_bits(third, want_small)
    for k in first:
        assert np.ascontiguousarray(first[k]).tobytes() == np.ascontiguousarray(third[k]).tobytes(), k
    ops.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# sizes on the padding boundary: n * 4 = 252 / 256 / 260 bytes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_is_in_frustum_63_64_65_points(orbx):
    """isInFrustum is a function of the point alone: the calls with 63, 64 and 65 points agree with the rows of one call with 3000 (far from every
    padding boundary).  The 3000-point call is compared with the compiled reference, the one tests/test_frustum.py uses, where that is built; where it
    is not (test_frustum.py skips there), only the prefix comparison runs, on normals made here: a boundary check, not a check against a reference."""
    T, Ts, sk, P = tfr._setup(orbx, 5, n=3000)
    ref = oracle_lib.ref_is_in_frustum(T, Ts, sk, P, 0.5) if oracle_lib.slam_lib() is not None else None
    mt = orbx.ORBmatcher(0.8, True, max_features=3000)
    if ref is None:      # normals and distance ranges of the points as the module's test takes them from the reference: made here
        rng = np.random.default_rng(6)
        nrm = rng.normal(size=(3000, 3)).astype(np.float32)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
        pts = dict(pos=P, normal=nrm, max_distance=np.full(3000, 40.0, np.float32), min_distance=np.full(3000, 0.05, np.float32))
        lsf = float(np.float32(np.log(np.float32(1.2))))
    else:
        pts, lsf = dict(pos=P, normal=ref["normal"], max_distance=ref["max_distance"], min_distance=ref["min_distance"]), ref["log_scale_factor"]
    args = (T, (500.0, 500.0, 320.0, 240.0, 40.0), (0.0, 640.0, 0.0, 480.0), lsf, 8)
    whole = mt.isInFrustum(*args, pts, 0.5)
    assert 0 < whole["in_view"][:63].sum() < 63
    if ref is not None:
        ok = ref["in_view"] > 0
        assert (whole["in_view"] == ref["in_view"]).all() and (whole["level"][ok] == ref["level"][ok]).all()
        for k in ("proj_x", "proj_y", "proj_xr", "view_cos"):
            assert (whole[k][ok].view(np.uint32) == ref[k][ok].view(np.uint32)).all(), k
    for n in (63, 64, 65, 63):
        got = mt.isInFrustum(*args, {k: v[:n] for k, v in pts.items()}, 0.5)
        ok = whole["in_view"][:n] > 0
        assert len(got["in_view"]) == n and (got["in_view"] == whole["in_view"][:n]).all() and (got["level"][ok] == whole["level"][:n][ok]).all()
        for k in ("proj_x", "proj_y", "proj_xr", "view_cos"):
            assert (got[k][ok].view(np.uint32) == whole[k][:n][ok].view(np.uint32)).all(), (n, k)
    mt.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# capacity above the count; regions of no bytes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_create_new_map_points_one_feature_capacity_nine(orbx, oracle):
    """KF1 holds one feature in a set of capacity 9: every array of KF1 is staged with one element on the host and room for nine on the device"""
    sc, want = tnp._chain("one"), tnp._chain_want("one")
    mt = orbx.ORBmatcher(0.6, False, max_features=64)
    got = mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"], capacity1=9)
    tnp._check_chain(got, want, 1, 1)
    assert mt.new_points_last_timing()[1] == 5
    exact = mt.CreateNewMapPoints(sc["kf1"], sc["neighbours"])
    assert exact["count"] == got["count"] and np.array_equal(exact["created"], got["created"])
    mt.close()


def test_essential_graph_without_points(orbx):
    """two keyframes, the edges between them and no map points: the point arrays and the off-diagonal index take no bytes"""
    G = teg._scene("n2_free")[0]
    assert G.N == 2 and len(G.points) == 0
    h = orbx.EssentialGraphOptimizer(max_keyframes=4, max_edges=8, max_points=4)
    lin = h.linearize(G, fix_scale=G.fix_scale)
    assert (lin["meas"].view(np.uint64) == eg.measurements(G).view(np.uint64)).all()
    want = eg.optimize(G, M=lin["meas"])
    for _ in range(2):
        d = h.OptimizeEssentialGraph(G, fix_scale=G.fix_scale, full=True)
        assert d.iterations == want["iterations"] and (d.est.view(np.uint64) == want["est"].view(np.uint64)).all()
        Tiw, inv, pts = eg.write_back(G, d.est)
        assert (d.Tiw.view(np.uint32) == Tiw.view(np.uint32)).all() and (d.inv.view(np.uint64) == inv.view(np.uint64)).all() and d.points.shape == pts.shape
    h.close()


def test_sim3_solver_candidate_without_iterations():
    """two candidates, the second below min_inliers: it stages matches, but no set and no iteration"""
    h = ts3._orbx().Sim3Solver(max_candidates=2, max_matches=64, max_iterations=8)
    both = _sim3_solve(h, ["general_21", "general_19"])
    assert h.last_timing()[1] == 4
    assert [b.n for b in both] == [21, 19] and both[0].iterations == 7 and both[1].iterations == 0 and both[1].no_more and both[1].first_event == -1
    _sim3_check("general_21", both[0])
    _sim3_check("general_19", both[1])
    alone = _sim3_solve(h, ["general_21"])[0]
    assert _sim3_bits(alone) == _sim3_bits(both[0])
    flipped = _sim3_solve(h, ["general_19", "general_21"])      # the empty regions in front
    assert _sim3_bits(flipped[1]) == _sim3_bits(both[0]) and flipped[0].iterations == 0 and flipped[0].no_more
    h.close()


def test_kfdb_query_with_an_empty_word_list(orbx):
    """a relocalisation query without words between two with words: its slice of the staged words and values has no bytes"""
    bows = [([1, 5, 9, 20], [0.25] * 4), ([1, 5, 9, 30], [0.25] * 4), ([5, 9, 20, 40], [0.25] * 4), ([50, 60, 70, 80], [0.25] * 4)]
    db, ref = orbx.KeyFrameDatabase(n_words=100, max_keyframes=8, max_entries=64, max_queries=4, max_query_words=16), kr.KeyFrameDatabaseRef(100)
    for i, (w, v) in enumerate(bows):
        db.add(i, (w, v))
        ref.add(i, w, v)
    db.set_covisibles(0, [1, 2])
    ref.set_covisibles(0, [1, 2])
    qs = [dict(mode=kr.RELOC, words=[1, 5, 9, 20], values=[0.25] * 4), dict(mode=kr.RELOC, words=[], values=[]), dict(mode=kr.RELOC, words=[50, 60], values=[0.5, 0.5])]
    for _ in range(2):
        want = ref.query_batch(qs)
        got = db.query(qs)
        for q, (g, w) in enumerate(zip(got, want)):
            tkf._same(g, w, "query %d" % q)
        assert got[1]["n_sharing"] == 0 and len(got[1]["candidates"]) == 0 and [int(i) for i in got[0]["candidates"]] == [0]
    db.close()
