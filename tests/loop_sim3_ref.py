"""The refine step of LoopClosing::ComputeSim3 (reference src/LoopClosing.cc:435-480), ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1314-1523) and the pair
gather of Optimizer::OptimizeSim3 (src/Optimizer.cc:1429-1520) restated on plain arrays.

The numeric steps are callables, so the same glue serves two purposes (tests/test_loop_sim3.py):
  * with the project's CPU oracles (oracle_lib.fuse_best, optsim3_ref.optimize_sim3) it is the CPU reference of the chain;
  * with the existing device entry points (ORBmatcher.FuseSearch, Sim3Optimizer.OptimizeSim3) it is "the composition of today's entry points with the glue on
    the host", which the chain must equal bit for bit.
A map point is its keyframe slot.  A keyframe is the dict ORBmatcher._loop_keyframe takes: kps (structured), desc, Rcw, tcw, cam, scale_factors,
log_scale_factor, inv_level_sigma2, width, height, valid, pos, max_distance, min_distance, point_desc (+ bow_match on a candidate)."""
import math

import numpy as np

import optsim3_ref as osr

F32, F64 = np.float32, np.float64
TH_HIGH = 100
MAX_PAIRS = 1024            # ORBX_SIM3_OPT_MAX_PAIRS
MIN_INLIERS = 20            # src/LoopClosing.cc:463
FAILED, SUCCESS, OVERFLOW = 0, 1, 2


def transforms(R12, t12, s12):
    """src/ORBmatcher.cc:1333-1335 in float, the quotient and the products of sR21 in double: sR12, t12, sR21, t21"""
    R, t, s = np.asarray(R12, F32).reshape(3, 3), np.asarray(t12, F32).reshape(3), F32(s12)
    sR12 = s * R
    inv = F64(1.0) / F64(s)
    sR21 = (inv * R.T.astype(F64)).astype(F32)
    t21 = ((-sR21[:, 0]) * t[0] + (-sR21[:, 1]) * t[1]) + (-sR21[:, 2]) * t[2]
    return sR12.astype(F32), t, sR21, t21.astype(F32)


def bounds_of(kf):
    """(float) of the KeyFrame's int mnMinX, mnMaxX, mnMinY, mnMaxY"""
    f = lambda v: F32(int(F32(v)))      # noqa: E731
    return f(kf.get("min_x", 0.0)), f(kf.get("max_x", kf["width"])), f(kf.get("min_y", 0.0)), f(kf.get("max_y", kf["height"]))


def project(src, dst, cam, M, tv, already, th):
    """One direction of SearchBySim3 (:1367-1411): the slots of `src` carried into the camera of `dst` by (M, tv).  cam: KF1's intrinsics (both directions).
    Per slot u, v, level, radius and active = the slot reaches GetFeaturesInArea (zeros where it does not)."""
    R, t = np.asarray(src["Rcw"], F32).reshape(3, 3), np.asarray(src["tcw"], F32).reshape(3)
    P = np.asarray(src["pos"], F32).reshape(-1, 3)
    fx, fy, cx, cy = [F32(v) for v in cam[:4]]
    minx, maxx, miny, maxy = bounds_of(dst)
    sf = np.asarray(dst["scale_factors"], F32)
    nlevels = len(sf)
    maxD, minD = np.asarray(src["max_distance"], F32), np.asarray(src["min_distance"], F32)
    m = len(P)
    ok = (np.asarray(src["valid"]) != 0) & (np.asarray(already) == 0)                                   # :1371-1375
    a, b = np.zeros((m, 3), F32), np.zeros((m, 3), F32)
    with np.errstate(all="ignore"):
        for r in range(3):
            a[:, r] = ((R[r, 0] * P[:, 0] + R[r, 1] * P[:, 1]) + R[r, 2] * P[:, 2]) + t[r]              # :1378
        for r in range(3):
            b[:, r] = ((M[r, 0] * a[:, 0] + M[r, 1] * a[:, 1]) + M[r, 2] * a[:, 2]) + tv[r]              # :1379
        ok = ok & ~(b[:, 2] < 0)                                                                       # :1382
        invz = (F64(1.0) / b[:, 2].astype(F64)).astype(F32)                                             # :1386
        x, y = b[:, 0] * invz, b[:, 1] * invz
        u, v = fx * x + cx, fy * y + cy
        ok = ok & (u >= minx) & (u < maxx) & (v >= miny) & (v < maxy)                                   # KeyFrame::IsInImage
        b64 = b.astype(F64)
        dist = np.sqrt(b64[:, 0] * b64[:, 0] + b64[:, 1] * b64[:, 1] + b64[:, 2] * b64[:, 2]).astype(F32)   # cv::norm, :1399
        ok = ok & ~((dist < F32(0.8) * minD) | (dist > F32(1.2) * maxD))                                # :1402
        ratio = maxD / dist
    out = dict(u=np.zeros(m, F32), v=np.zeros(m, F32), ur=np.zeros(m, F32), level=np.zeros(m, np.int32), radius=np.zeros(m, F32), active=ok.astype(np.uint8))
    lsf = float(F32(dst["log_scale_factor"]))
    for i in np.flatnonzero(ok):
        lvl = min(max(int(math.ceil(math.log(float(ratio[i])) / lsf)), 0), nlevels - 1)               # MapPoint::PredictScale(dist3D, pKF)
        out["u"][i], out["v"][i], out["level"][i] = u[i], v[i], lvl
        out["radius"][i] = F32(th) * sf[lvl]                                                           # :1411
    return out


def fuse_kf(kf):
    """the keyframe as FuseSearch / oracle_lib.fuse_best take it"""
    out = {k: kf[k] for k in ("kps", "desc", "inv_level_sigma2", "width", "height") }
    out.update({k: kf[k] for k in ("min_x", "min_y", "max_x", "max_y") if k in kf})
    out["u_right"] = np.full(len(kf["kps"]), -1.0, F32)
    return out


def search_by_sim3(kf1, kf2, pre12, R12, t12, s12, th, fuse_best):
    """SearchBySim3 with vpMatches12 = pre12 (KF2 slots or -1) going in.  -> dict(matches12, n_found, match1, match2, query1, query2)"""
    n1, n2 = len(kf1["kps"]), len(kf2["kps"])
    pre = np.asarray(pre12, np.int32)
    alr1, alr2 = pre >= 0, np.zeros(n2, bool)
    alr2[pre[(pre >= 0) & (pre < n2)]] = True                                                          # :1347-1357
    sR12, t, sR21, t21 = transforms(R12, t12, s12)
    q1 = project(kf1, kf2, kf1["cam"], sR21, t21, alr1, th)
    q2 = project(kf2, kf1, kf1["cam"], sR12, t, alr2, th)
    vn = []
    for q, src, dst in ((q1, kf1, kf2), (q2, kf2, kf1)):
        bi, bd = fuse_best(fuse_kf(dst), dict(q, desc=np.asarray(src["point_desc"], np.uint8)))
        vn.append(np.where((q["active"] > 0) & (np.asarray(bd) <= TH_HIGH), np.asarray(bi), -1).astype(np.int32))
    m12, found = pre.copy(), 0
    for i1 in range(n1):                                                                               # :1507-1521
        idx2 = vn[0][i1]
        if idx2 >= 0 and vn[1][idx2] == i1:
            m12[i1] = idx2
            found += 1
    return dict(matches12=m12, n_found=found, match1=vn[0], match2=vn[1], query1=q1, query2=q2)


def gather(kf1, kf2, m12, R12, t12, s12, limit=None):
    """The loop of src/Optimizer.cc:1429-1520: (problem dict of Sim3Optimizer, the KF1 feature of each pair)"""
    v1, v2 = np.asarray(kf1["valid"]) != 0, np.asarray(kf2["valid"]) != 0
    i1 = np.array([i for i in range(len(m12)) if m12[i] >= 0 and v1[i] and v2[m12[i]]], np.int64)
    if limit is not None:
        i1 = i1[:limit]
    i2 = np.asarray(m12, np.int64)[i1]
    k1, k2 = kf1["kps"], kf2["kps"]
    is1, is2 = np.asarray(kf1["inv_level_sigma2"], F32), np.asarray(kf2["inv_level_sigma2"], F32)
    p = dict(Rcw1=kf1["Rcw"], tcw1=kf1["tcw"], Rcw2=kf2["Rcw"], tcw2=kf2["tcw"], K1=tuple(kf1["cam"][:4]), K2=tuple(kf2["cam"][:4]),
             world1=np.asarray(kf1["pos"], F32).reshape(-1, 3)[i1], world2=np.asarray(kf2["pos"], F32).reshape(-1, 3)[i2],
             obs1=np.stack([k1["x"][i1], k1["y"][i1]], 1).astype(F32).reshape(-1, 2), obs2=np.stack([k2["x"][i2], k2["y"][i2]], 1).astype(F32).reshape(-1, 2),
             inv_sigma2_1=is1[np.clip(k1["octave"][i1], 0, len(is1) - 1)], inv_sigma2_2=is2[np.clip(k2["octave"][i2], 0, len(is2) - 1)],
             R12=np.asarray(R12, F32).astype(F64).reshape(3, 3), t12=np.asarray(t12, F32).astype(F64).reshape(3), s12=float(F32(s12)))
    return p, i1


def scw_of(quat, t, s, Rcw2, tcw2):
    """mg2oScw = gScm * gSmw (:469-471) with sim3.h's operations in float64, and Converter::toCvMat of it: (4,4) float32"""
    gSmw = osr.sim3_from_Rts(np.asarray(Rcw2, F32).astype(F64).reshape(3, 3), np.asarray(tcw2, F32).astype(F64).reshape(3), 1.0)
    S = osr.sim3_mul((list(quat), list(t), float(s)), gSmw)
    R = np.asarray(osr.quat_to_R(S[0]), F64).reshape(3, 3)
    T = np.eye(4, dtype=F32)
    T[:3, :3] = (F64(S[2]) * R).astype(F32)
    T[:3, 3] = np.asarray(S[1], F64).astype(F32)
    return T


def refine(kf1, kf2, hyp, th, th2, fix_scale, fuse_best, optimize):
    """:437-474 for one event.  optimize(problem, th2, fix_scale) -> object / dict with n_inliers, n_bad, quat, t, s, removed_first, removed_final."""
    get = lambda r, k: r[k] if isinstance(r, dict) else getattr(r, k)      # noqa: E731
    bow, inl = np.asarray(kf2["bow_match"], np.int32), np.asarray(hyp["inliers"]) != 0
    pre = np.where(inl, bow, -1).astype(np.int32)                                                      # :437-443
    s = search_by_sim3(kf1, kf2, pre, hyp["R12"], hyp["t12"], hyp["s12"], th, fuse_best)
    m12 = s["matches12"].copy()
    p, i1 = gather(kf1, kf2, m12, hyp["R12"], hyp["t12"], hyp["s12"])
    n_pairs = len(i1)
    over = n_pairs > MAX_PAIRS
    if over:
        p, _ = gather(kf1, kf2, m12, hyp["R12"], hyp["t12"], hyp["s12"], limit=0)                      # no optimisation: the estimate as passed in
    r = optimize(p, th2, fix_scale)
    n_in, n_bad = (0, 0) if over else (int(get(r, "n_inliers")), int(get(r, "n_bad")))
    if not over and n_pairs:
        rem = np.asarray(get(r, "removed_first"), bool) | np.asarray(get(r, "removed_final"), bool)
        m12[i1[rem]] = -1                                                                              # src/Optimizer.cc:1541 / :1578
    quat, t, sc = np.asarray(get(r, "quat"), F64), np.asarray(get(r, "t"), F64), float(get(r, "s"))
    status = OVERFLOW if over else (SUCCESS if n_in >= MIN_INLIERS else FAILED)
    return dict(status=status, n_found=s["n_found"], n_pairs=n_pairs, n_inliers=n_in, n_bad=n_bad, quat=quat, t=t, s=sc, scw=scw_of(quat, t, sc, kf2["Rcw"], kf2["tcw"]),
                matches12=m12, search=s, pair_i1=i1, opt=r)


def walk(statuses):
    """What the loop of :403-482 does with the events in the order given: (winner or -1, an overflow was met before any winner)"""
    for k, st in enumerate(statuses):
        if st == SUCCESS:
            return k, False
        if st == OVERFLOW:
            return -1, True
    return -1, False


def run(kf1, cands, hyps, th, th2, fix_scale, fuse_best, optimize):
    """Every event, as orbx_loop_refine_sim3 reports them: dict of arrays over H + the winner's matches12 + winner / hypothesis / candidate / overflow"""
    per = [refine(kf1, cands[h["candidate"]], h, th, th2, fix_scale, fuse_best, optimize) for h in hyps]
    out = {k: np.array([p[k] for p in per]) for k in ("status", "n_found", "n_pairs", "n_inliers", "n_bad", "quat", "t", "s", "scw")}
    win, over = walk(out["status"].tolist())
    out.update(winner=win, hypothesis=win, candidate=hyps[win]["candidate"] if win >= 0 else -1, overflow=over,
               matches12=per[win]["matches12"] if win >= 0 else np.full(len(kf1["kps"]), -1, np.int32), per=per)
    return out


def cpu_optimize(problem, th2, fix_scale):
    """optsim3_ref on a problem dict, in the shape `refine` reads"""
    P = osr.Problem(problem, th2, fix_scale)
    r = osr.optimize_sim3(P)
    return dict(n_inliers=r["n_inliers"], n_bad=r["n_bad"], quat=np.array(r["S"][0], F64), t=np.array(r["S"][1], F64), s=float(r["S"][2]),
                removed_first=r["removed_first"], removed_final=r["removed_final"], full=r, problem=P)
