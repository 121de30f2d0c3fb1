"""Tracking::TrackWithMotionModel (reference src/Tracking.cc:1370-1421) and Tracking::TrackLocalMap (:1454-1489) restated on plain arrays.

The numeric steps are callables, so the same glue serves two purposes (tests/test_track_chain.py):
  * with the project's CPU oracles (oracle_lib.search_by_projection_last / search_by_projection / pose_optimization and the Frame::isInFrustum
    restatement below) it is the CPU reference of the chains;
  * with the existing device entry points (ORBmatcher.SearchByProjectionLast / SearchLocalPoints, PoseOptimizer.PoseOptimization) it is "the
    composition of the existing calls with the glue on the host", which the chains must equal bit for bit.
A frame is the dict of the projection tests (kps7 = x, y, size, angle, response, octave, class_id per feature; u_right; ...)."""
import math

import numpy as np


# ---- the loops, vectorised (the test holds them against a line-by-line translation) ----
def discard(mvp, outlier, last_has_obs, nmatches):
    """:1403-1421.  mvp[i] = last-frame feature whose point mvpMapPoints[i] holds or -1; outlier[i] = mvbOutlier[i].
    Returns (mvp after, discarded flags, nmatches after the decrements, nmatchesMap)."""
    mvp = np.asarray(mvp)
    has = mvp >= 0
    disc = has & (np.asarray(outlier) != 0)
    kept = has & ~disc
    obs = np.ones(len(mvp), bool) if last_has_obs is None else np.asarray(last_has_obs)[np.maximum(mvp, 0)] != 0
    return np.where(kept, mvp, -1).astype(np.int32), disc.astype(np.uint8), int(nmatches - disc.sum()), int((kept & obs).sum())


def statistics(has_point, outlier, observed, sensor_stereo):
    """:1464-1489.  has_point[i] = mvpMapPoints[i] != NULL, observed[i] = its Observations() > 0.
    Returns (found, cleared, inliers_map = mnMatchesInliers with !mbOnlyTracking, inliers_all = with mbOnlyTracking)."""
    has, out = np.asarray(has_point) != 0, np.asarray(outlier) != 0
    inl = has & ~out
    cleared = has & out & bool(sensor_stereo)
    return inl.astype(np.uint8), cleared.astype(np.uint8), int((inl & (np.asarray(observed) != 0)).sum()), int(inl.sum())


def _obs_of(fr, idx):
    k7 = np.asarray(fr["kps7"], np.float32)
    return np.stack([k7[idx, 0], k7[idx, 1], np.asarray(fr["u_right"], np.float32)[idx]], 1).astype(np.float32)


def motion_model(search, pose_opt, fr, last, th, inv_level_sigma2):
    """search(th) -> (nmatches, assigned[n] with -2 = pruned); pose_opt(dict(pose, cam, Xw, obs, inv_sigma2)) -> dict(pose, outlier, inliers, stats)."""
    n = len(fr["kps7"])
    nm, a = search(th)                                                        # :1382
    wide = 0
    if nm < 20:                                                               # :1386-1390
        nm, a = search(2 * th)
        wide = 1
    a = np.asarray(a, np.int32)
    mvp = np.where(a >= 0, a, -1).astype(np.int32)
    idx = np.flatnonzero(mvp >= 0)
    res = dict(search_matches=a, nmatches_search=int(nm), wide=wide, n_correspondences=len(idx))
    if nm < 20:                                                               # :1393
        res.update(ran_pose=0, pose=np.asarray(fr["Tcw"], np.float32).reshape(4, 4), matches=mvp, discarded=np.zeros(n, np.uint8), nmatches=int(nm), nmatches_map=0,
                   pose_inliers=0, stats=np.zeros(8))
        return res
    octave = np.asarray(fr["kps7"], np.float32)[idx, 5].astype(np.int64)
    prob = dict(pose=np.asarray(fr["Tcw"], np.float32), cam=fr["cam"], Xw=np.asarray(last["pos"], np.float32)[mvp[idx]].reshape(-1, 3), obs=_obs_of(fr, idx),
                inv_sigma2=np.asarray(inv_level_sigma2, np.float32)[octave])
    r = pose_opt(prob)                                                        # :1398
    outl = np.zeros(n, np.uint8)
    outl[idx] = r["outlier"]
    matches, disc, nmatches, nmap = discard(mvp, outl, last.get("has_obs"), nm)
    res.update(ran_pose=1, pose=np.asarray(r["pose"], np.float32).reshape(4, 4), matches=matches, discarded=disc, nmatches=nmatches, nmatches_map=nmap,
               pose_inliers=int(r["inliers"]), stats=np.asarray(r["stats"], np.float64), problem=prob)
    return res


def local_map(search_local, pose_opt, fr, Tcw, cam, points, held, held_pos, inv_level_sigma2, sensor_stereo):
    """search_local() -> (nmatches, assigned[n], frustum dict); the rest as above.  fr["occupied"][i] = the held point has observations."""
    n = len(fr["kps7"])
    nm, a, fv = search_local()                                                # :1454
    a = np.asarray(a, np.int32)
    held = np.asarray(held) != 0
    has = (a >= 0) | held
    idx = np.flatnonzero(has)
    pos = np.asarray(points["pos"], np.float32).reshape(-1, 3)
    Xw = np.asarray(held_pos, np.float32).reshape(-1, 3).copy()
    Xw[a >= 0] = pos[a[a >= 0]]
    octave = np.asarray(fr["kps7"], np.float32)[idx, 5].astype(np.int64)
    prob = dict(pose=np.asarray(Tcw, np.float32), cam=cam, Xw=Xw[idx], obs=_obs_of(fr, idx), inv_sigma2=np.asarray(inv_level_sigma2, np.float32)[octave])
    r = pose_opt(prob)                                                        # :1459
    outl = np.zeros(n, np.uint8)
    outl[idx] = r["outlier"]
    pobs = np.ones(len(pos), np.uint8) if points.get("has_obs") is None else np.asarray(points["has_obs"], np.uint8)
    occ = np.zeros(n, np.uint8) if fr.get("occupied") is None else np.asarray(fr["occupied"], np.uint8)
    observed = np.where(a >= 0, pobs[np.maximum(a, 0)] if len(pobs) else 0, occ)
    found, cleared, imap, iall = statistics(has, outl, observed, sensor_stereo)
    return dict(assigned=a, nmatches=int(nm), frustum=fv, n_correspondences=len(idx), pose=np.asarray(r["pose"], np.float32).reshape(4, 4), outlier=outl, found=found,
                cleared=cleared, pose_inliers=int(r["inliers"]), inliers_map=imap, inliers_all=iall, stats=np.asarray(r["stats"], np.float64), problem=prob)


# ---- Frame::isInFrustum + MapPoint::PredictScale (src/Frame.cc:608-742, src/MapPoint.cc:571-586) in the reference's float / double steps ----
def is_in_frustum(Tcw, cam, bounds, log_scale_factor, nlevels, points, cos_limit=0.5):
    f = np.float32
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    fx, fy, cx, cy, mbf = [f(v) for v in cam]
    minx, maxx, miny, maxy = [f(v) for v in bounds]
    P, Pn = np.asarray(points["pos"], np.float32).reshape(-1, 3), np.asarray(points["normal"], np.float32).reshape(-1, 3)
    maxD, minD = np.asarray(points["max_distance"], np.float32), np.asarray(points["min_distance"], np.float32)
    m = len(P)
    Pc = np.zeros((m, 3), np.float32)
    Ow = np.zeros(3, np.float32)
    for r in range(3):
        Pc[:, r] = ((T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]) + T[r, 3]
        Ow[r] = ((-T[0, r]) * T[0, 3] + (-T[1, r]) * T[1, 3]) + (-T[2, r]) * T[2, 3]
    out = dict(in_view=np.zeros(m, np.uint8), proj_x=np.zeros(m, np.float32), proj_y=np.zeros(m, np.float32), proj_xr=np.zeros(m, np.float32),
               level=np.zeros(m, np.int32), view_cos=np.zeros(m, np.float32))
    with np.errstate(all="ignore"):
        invz = f(1.0) / Pc[:, 2]
        u, v = fx * Pc[:, 0] * invz + cx, fy * Pc[:, 1] * invz + cy
        PO = P - Ow[None, :]
        dist = np.sqrt((PO.astype(np.float64) ** 2)[:, 0] + (PO.astype(np.float64) ** 2)[:, 1] + (PO.astype(np.float64) ** 2)[:, 2]).astype(np.float32)
        dot = PO[:, 0].astype(np.float64) * Pn[:, 0] + PO[:, 1].astype(np.float64) * Pn[:, 1] + PO[:, 2].astype(np.float64) * Pn[:, 2]
        vc = (dot / dist.astype(np.float64)).astype(np.float32)
        ok = ~(Pc[:, 2] < 0) & ~((u < minx) | (u > maxx)) & ~((v < miny) | (v > maxy)) & ~((dist < f(0.8) * minD) | (dist > f(1.2) * maxD)) & ~(vc < f(cos_limit))
        ratio = maxD / dist
    for i in np.flatnonzero(ok):
        lvl = int(math.ceil(math.log(float(ratio[i])) / float(np.float32(log_scale_factor))))
        out["level"][i] = min(max(lvl, 0), nlevels - 1)
    out["in_view"][:] = ok
    for k, val in (("proj_x", u), ("proj_y", v), ("proj_xr", u - mbf * invz), ("view_cos", vc)):
        out[k][ok] = val[ok]
    return out
