"""The refine loop of Tracking::Relocalization (reference src/Tracking.cc:2135-2223) and ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th,
ORBdist) (src/ORBmatcher.cc:1731-1863) restated on plain arrays.

The numeric steps are callables, so the same glue serves two purposes (tests/test_relocalize_refine.py):
  * with the project's CPU oracles (oracle_lib.pose_optimization / area_search_greedy) it is the CPU reference of the chain;
  * with the existing device entry points (PoseOptimizer.PoseOptimization, ORBmatcher.AreaSearchGreedy) it is "the composition of the existing calls with the
    glue on the host", which the chain must equal bit for bit.
A map point is its keyframe slot.  frame: dict(kps7, desc, u_right, cam, scale_factors, log_scale_factor, width, height); cand: dict(valid, pos, max_distance,
min_distance, desc, kf_angle, bow_match)."""
import math

import numpy as np

HISTO_LENGTH = 30
# the exits of the refine loop, in the order of the source
EXIT_POSE1_FEW, EXIT_POSE1_OK, EXIT_SEARCH1_FEW, EXIT_POSE2_OK, EXIT_POSE2_FEW, EXIT_SEARCH2_FEW, EXIT_POSE3_OK, EXIT_POSE3_FEW = range(8)
SUCCESS = (EXIT_POSE1_OK, EXIT_POSE2_OK, EXIT_POSE3_OK)


# ---- src/ORBmatcher.cc:1735-1790 in the reference's float / double steps ----
def project(frame, cand, Tcw, found, th):
    """Per slot: u, v, radius, min_level, max_level and active = the slot reaches GetFeaturesInArea (zeros where it does not)."""
    f = np.float32
    T = np.asarray(Tcw, np.float32).reshape(-1)[:12].reshape(3, 4)
    fx, fy, cx, cy = [f(v) for v in frame["cam"][:4]]
    minx, miny = f(frame.get("min_x", 0.0)), f(frame.get("min_y", 0.0))
    maxx, maxy = f(frame.get("max_x", frame["width"])), f(frame.get("max_y", frame["height"]))
    sf = np.asarray(frame["scale_factors"], np.float32)
    nlevels = len(sf)
    P = np.asarray(cand["pos"], np.float32).reshape(-1, 3)
    maxD, minD = np.asarray(cand["max_distance"], np.float32), np.asarray(cand["min_distance"], np.float32)
    m = len(P)
    ok = np.asarray(cand["valid"]) != 0                                          # pMP && !pMP->isBad(), :1752-1754
    if found is not None:
        ok = ok & (np.asarray(found) == 0)                                       # !sAlreadyFound.count(pMP)
    Pc = np.zeros((m, 3), np.float32)
    Ow = np.zeros(3, np.float32)
    for r in range(3):
        Pc[:, r] = ((T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]) + T[r, 3]      # Rcw*x3Dw+tcw, :1758
        Ow[r] = ((-T[0, r]) * T[0, 3] + (-T[1, r]) * T[1, 3]) + (-T[2, r]) * T[2, 3]            # -Rcw.t()*tcw, :1737
    with np.errstate(all="ignore"):
        invz = (np.float64(1.0) / Pc[:, 2].astype(np.float64)).astype(np.float32)               # const float invzc = 1.0/x3Dc.at<float>(2), :1762
        u, v = fx * Pc[:, 0] * invz + cx, fy * Pc[:, 1] * invz + cy                             # :1764-1765
        ok = ok & (u >= minx) & (u <= maxx) & (v >= miny) & (v <= maxy)                         # :1767-1770
        PO = P - Ow[None, :]
        PO64 = PO.astype(np.float64)
        dist = np.sqrt(PO64[:, 0] * PO64[:, 0] + PO64[:, 1] * PO64[:, 1] + PO64[:, 2] * PO64[:, 2]).astype(np.float32)      # cv::norm, :1774
        ok = ok & ~((dist < f(0.8) * minD) | (dist > f(1.2) * maxD))                            # :1776-1781
        ratio = maxD / dist                                                                     # MapPoint::PredictScale, src/MapPoint.cc:571-586
    out = dict(u=np.zeros(m, np.float32), v=np.zeros(m, np.float32), radius=np.zeros(m, np.float32), min_level=np.zeros(m, np.int32), max_level=np.zeros(m, np.int32),
               active=ok.astype(np.uint8))
    lsf = float(np.float32(frame["log_scale_factor"]))
    for i in np.flatnonzero(ok):
        lvl = min(max(int(math.ceil(math.log(float(ratio[i])) / lsf)), 0), nlevels - 1)
        out["u"][i], out["v"][i] = u[i], v[i]
        out["radius"][i] = f(th) * sf[lvl]                                                      # :1788
        out["min_level"][i], out["max_level"][i] = lvl - 1, lvl + 1                             # :1791
    return out


# ---- :1824-1860 ----
def three_maxima(counts):
    """ORBmatcher::ComputeThreeMaxima (:1866-1908) on the bins' sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):                                # :1899-1907
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def histogram_keep(kf_angle, frame_angle, assigned):
    """Which of the slots that took a feature (assigned[i] >= 0) keep it behind the rotation histogram.  Returns keep[slots] (bool)."""
    assigned = np.asarray(assigned)
    factor = np.float32(HISTO_LENGTH) / np.float32(360.0)
    bins = np.full(len(assigned), -1, np.int64)
    for i in np.flatnonzero(assigned >= 0):
        rot = np.float32(kf_angle[i]) - np.float32(frame_angle[assigned[i]])                    # :1826
        if rot < 0.0:
            rot = np.float32(rot + np.float32(360.0))
        x = float(np.float32(rot * factor))
        b = int(math.floor(abs(x) + 0.5) * (1 if x >= 0 else -1))                               # round(): halves away from zero
        if b == HISTO_LENGTH:
            b = 0
        bins[i] = b
    inds = three_maxima(np.bincount(bins[bins >= 0], minlength=HISTO_LENGTH))
    return (assigned >= 0) & np.isin(bins, [i for i in inds if i >= 0])


def search_by_projection(project_fn, area_search, frame, cand, mvp, found, Tcw, th, orb_dist, check_orientation):
    """:1731-1863 on mvp (in place).  project_fn(Tcw, found, th) -> the queries; area_search(queries, blocked, orb_dist) -> assigned[slots].  Returns nmatches."""
    q = project_fn(Tcw, found, th)
    asg = np.asarray(area_search(q, (mvp >= 0).astype(np.uint8), orb_dist))                     # :1791-1822
    keep = asg >= 0
    if check_orientation:
        keep = histogram_keep(np.asarray(cand["kf_angle"], np.float32), np.asarray(frame["kps7"], np.float32)[:, 3], asg)
    slots = np.flatnonzero(keep)
    mvp[asg[slots]] = slots
    return int(len(slots))


# ---- src/Tracking.cc:2135-2223 ----
def refine(n, cand, Tcw, inliers, pose_opt, search):
    """One returned pose through the refine loop.  pose_opt(mvp, Tcw) -> dict(pose (4, 4), outlier[n] over the features (valid where mvp >= 0), inliers, stats[8]);
    search(mvp, found, Tcw, th, orb_dist) -> nadditional, writing mvp.  Returns the fields of orbx_relocalize_refine for this hypothesis + map_point / outlier."""
    bow = np.asarray(cand["bow_match"], np.int32)
    npts = len(cand["valid"])
    mask = np.asarray(inliers) != 0
    mvp = np.where(mask, bow, -1).astype(np.int32)                                              # :2143-2152
    found = np.zeros(npts, np.uint8)
    found[mvp[mvp >= 0]] = 1
    outl = np.zeros(n, np.uint8)
    res = dict(ngood=np.zeros(3, np.int32), nadditional=np.zeros(2, np.int32), n_correspondences=np.zeros(3, np.int32), stats=np.zeros((3, 8), np.float64))
    T = np.eye(4, dtype=np.float32)
    T[:3, :] = np.asarray(Tcw, np.float32).reshape(-1)[:12].reshape(3, 4)
    state = dict(T=T)

    def run_pose(k):
        has = mvp >= 0
        r = pose_opt(mvp, state["T"])
        outl[has] = np.asarray(r["outlier"], np.uint8)[has]
        state["T"] = np.asarray(r["pose"], np.float32).reshape(4, 4)
        res["ngood"][k], res["n_correspondences"][k], res["stats"][k] = int(r["inliers"]), int(has.sum()), np.asarray(r["stats"], np.float64)
        return int(r["inliers"])

    def drop():
        mvp[(mvp >= 0) & (outl != 0)] = -1

    def done(stage):
        res.update(stage=stage, success=int(stage in SUCCESS), pose=state["T"], map_point=mvp, outlier=outl)
        return res

    nGood = run_pose(0)                                                                         # :2156
    if nGood < 10:                                                                              # :2159
        return done(EXIT_POSE1_FEW)
    drop()                                                                                      # :2162-2164
    if nGood >= 50:                                                                             # :2169 / :2218
        return done(EXIT_POSE1_OK)
    nadd = search(mvp, found, state["T"], 10.0, 100)                                            # :2171
    res["nadditional"][0] = nadd
    if nadd + nGood < 50:                                                                       # :2179
        return done(EXIT_SEARCH1_FEW)
    nGood = run_pose(1)                                                                         # :2182 (the outliers stay)
    if nGood >= 50:
        return done(EXIT_POSE2_OK)
    if nGood <= 30:                                                                             # :2188
        return done(EXIT_POSE2_FEW)
    found[:] = 0                                                                                # :2191-2194
    found[mvp[mvp >= 0]] = 1
    nadd = search(mvp, found, state["T"], 3.0, 64)                                              # :2195
    res["nadditional"][1] = nadd
    if nGood + nadd < 50:                                                                       # :2203
        return done(EXIT_SEARCH2_FEW)
    nGood = run_pose(2)                                                                         # :2205
    drop()                                                                                      # :2207-2209
    return done(EXIT_POSE3_OK if nGood >= 50 else EXIT_POSE3_FEW)


def pose_problem(frame, cand, mvp, Tcw, inv_level_sigma2):
    """The PoseOptimization problem of the features that hold a point, in ascending feature order (the form of track_ref.motion_model)."""
    idx = np.flatnonzero(mvp >= 0)
    k7 = np.asarray(frame["kps7"], np.float32)
    obs = np.stack([k7[idx, 0], k7[idx, 1], np.asarray(frame["u_right"], np.float32)[idx]], 1).astype(np.float32)
    octave = np.clip(k7[idx, 5].astype(np.int64), 0, len(inv_level_sigma2) - 1)
    return idx, dict(pose=np.asarray(Tcw, np.float32), cam=frame["cam"], Xw=np.asarray(cand["pos"], np.float32).reshape(-1, 3)[mvp[idx]].reshape(-1, 3), obs=obs,
                     inv_sigma2=np.asarray(inv_level_sigma2, np.float32)[octave])


def run(frame, cands, hyps, sequence, inv_level_sigma2, pose_opt_problem, area_search_fn, check_orientation, project_fn=project):
    """Every hypothesis through refine() and the walk over `sequence`: the result dict of ORBmatcher.RelocalizeRefine.
    pose_opt_problem(problem) -> dict(pose, outlier[edges], inliers, stats); area_search_fn(frame_dict, queries, max_dist) -> (nm, assigned, dists)."""
    n = len(frame["kps7"])
    per = []
    for h in hyps:
        cand = cands[h["candidate"]]

        def pose_opt(mvp, T, cand=cand):
            idx, prob = pose_problem(frame, cand, mvp, T, inv_level_sigma2)
            r = pose_opt_problem(prob)
            o = np.zeros(n, np.uint8)
            o[idx] = np.asarray(r["outlier"], np.uint8)[:len(idx)]
            return dict(pose=r["pose"], outlier=o, inliers=r["inliers"], stats=r["stats"])

        def area(q, blocked, orb_dist, cand=cand):
            fd = dict(kps=frame.get("kps", frame["kps7"]), desc=frame["desc"], blocked=blocked, width=frame["width"], height=frame["height"])
            for k in ("min_x", "min_y", "max_x", "max_y"):
                if k in frame:
                    fd[k] = frame[k]
            return area_search_fn(fd, dict(q, desc=cand["desc"]), orb_dist)[1]

        def search(mvp, found, T, th, orb_dist, cand=cand):
            return search_by_projection(lambda Tc, fnd, t: project_fn(frame, cand, Tc, fnd, t), area, frame, cand, mvp, found, T, th, orb_dist, check_orientation)
        per.append(refine(n, cand, h["Tcw"], h["inliers"], pose_opt, search))
    winner = next((s for s, hi in enumerate(sequence) if per[hi]["success"]), -1)
    hc = int(sequence[winner if winner >= 0 else len(sequence) - 1])
    out = {k: np.stack([p[k] for p in per]) for k in ("ngood", "nadditional", "n_correspondences", "stats", "pose")}
    out.update(stage=np.array([p["stage"] for p in per], np.int32), success=np.array([p["success"] for p in per], np.int32), map_point=per[hc]["map_point"],
               outlier=per[hc]["outlier"], winner=winner, hypothesis=hc, candidate=int(hyps[hc]["candidate"]), per=per)
    return out
