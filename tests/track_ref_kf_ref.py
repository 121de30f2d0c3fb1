"""Tracking::TrackReferenceKeyFrame (reference src/Tracking.cc:1189-1238) and the head of Tracking::Relocalization (:2063-2095, with the collection
loop of the PnPsolver constructor, src/PnPsolver.cc:136-158) restated on plain arrays.

As in tests/track_ref.py the numeric steps are callables, so the same glue is
  * the CPU reference of the two chains, with oracle_lib.search_by_bow / pose_optimization, and
  * "the existing entry points composed on the host", with ORBmatcher.SearchByBoW / PoseOptimizer.PoseOptimization,
which orbx_track_reference_keyframe / orbx_reloc_match_candidates must equal bit for bit (tests/test_track_reference_keyframe.py).

A keyframe is dict(kps7, desc, groups, valid, pos, has_obs), a frame dict(kps7 (mvKeys), kps7_un (mvKeysUn), desc, groups, u_right, Tcw, cam); kps7 =
x, y, size, angle, response, octave, class_id per feature."""
import numpy as np


def discard(mvp, outlier, kf_has_obs, nmatches):
    """:1215-1236.  mvp[i] = keyframe slot whose point mvpMapPoints[i] holds or -1.  -> (mvp after, discarded, nmatches after, nmatchesMap)"""
    mvp = np.asarray(mvp)
    has = mvp >= 0
    disc = has & (np.asarray(outlier) != 0)
    kept = has & ~disc
    obs = np.ones(len(mvp), bool) if kf_has_obs is None else np.asarray(kf_has_obs)[np.maximum(mvp, 0)] != 0
    return np.where(kept, mvp, -1).astype(np.int32), disc.astype(np.uint8), int(nmatches - disc.sum()), int((kept & obs).sum())


def reference_keyframe(search, pose_opt, kf, fr, inv_level_sigma2):
    """search() -> (nmatches, matches[n]: keyframe slot per frame feature or -1); pose_opt(dict(pose, cam, Xw, obs, inv_sigma2)) -> dict(pose, outlier,
    inliers, stats).  fr["Tcw"] = the pose handed to SetPose (:1206)."""
    k7u = np.asarray(fr["kps7_un"], np.float32)
    n = len(k7u)
    nm, a = search()                                                          # :1195
    a = np.asarray(a, np.int32)
    idx = np.flatnonzero(a >= 0)
    res = dict(search_matches=a, nmatches_search=int(nm), n_correspondences=len(idx))
    if nm < 15:                                                               # :1201
        res.update(ran_pose=0, pose=np.asarray(fr["Tcw"], np.float32).reshape(4, 4), matches=a.copy(), discarded=np.zeros(n, np.uint8), nmatches=int(nm), nmatches_map=0,
                   pose_inliers=0, stats=np.zeros(8))
        return res
    obs = np.stack([k7u[idx, 0], k7u[idx, 1], np.asarray(fr["u_right"], np.float32)[idx]], 1).astype(np.float32)
    prob = dict(pose=np.asarray(fr["Tcw"], np.float32), cam=fr["cam"], Xw=np.asarray(kf["pos"], np.float32).reshape(-1, 3)[a[idx]].reshape(-1, 3), obs=obs,
                inv_sigma2=np.asarray(inv_level_sigma2, np.float32)[k7u[idx, 5].astype(np.int64)])
    r = pose_opt(prob)                                                        # :1209
    outl = np.zeros(n, np.uint8)
    outl[idx] = r["outlier"]
    matches, disc, nmatches, nmap = discard(a, outl, kf.get("has_obs"), nm)
    res.update(ran_pose=1, pose=np.asarray(r["pose"], np.float32).reshape(4, 4), matches=matches, discarded=disc, nmatches=nmatches, nmatches_map=nmap,
               pose_inliers=int(r["inliers"]), stats=np.asarray(r["stats"], np.float64), problem=prob)
    return res


def pnp_collect(row, kps7_un, level_sigma2, pos):
    """src/PnPsolver.cc:136-158 over one vvpMapPointMatches row (keyframe slot or -1; SearchByBoW only hands out non-bad points).
    -> (mvKeyPointIndices, mvP2D, mvSigma2, mvP3Dw)"""
    row, k7u = np.asarray(row), np.asarray(kps7_un, np.float32)
    idx = np.flatnonzero(row >= 0)
    return (idx.astype(np.int32), k7u[idx, :2].astype(np.float32).reshape(-1, 2), np.asarray(level_sigma2, np.float32)[k7u[idx, 5].astype(np.int64)],
            np.asarray(pos, np.float32).reshape(-1, 3)[row[idx]].reshape(-1, 3))


def reloc_match(search, fr, kfs, level_sigma2):
    """search(kf) -> (nmatches, row).  -> dict(matches (K, N), nmatches, discarded, n, key_index / p2d / sigma2 / p3dw: lists of K arrays)"""
    n, K = len(fr["kps7_un"]), len(kfs)
    out = dict(matches=np.full((K, n), -1, np.int32), nmatches=np.zeros(K, np.int32), discarded=np.zeros(K, np.uint8), n=np.zeros(K, np.int32),
               key_index=[np.zeros(0, np.int32)] * K, p2d=[np.zeros((0, 2), np.float32)] * K, sigma2=[np.zeros(0, np.float32)] * K, p3dw=[np.zeros((0, 3), np.float32)] * K)
    for k, kf in enumerate(kfs):
        if kf.get("bad"):                                                     # :2066
            out["discarded"][k] = 1
            continue
        nm, row = search(kf)                                                  # :2073
        out["matches"][k], out["nmatches"][k] = row, nm
        if nm < 15:                                                           # :2075
            out["discarded"][k] = 1
            continue
        out["key_index"][k], out["p2d"][k], out["sigma2"][k], out["p3dw"][k] = pnp_collect(row, fr["kps7_un"], level_sigma2, kf["pos"])
        out["n"][k] = len(out["key_index"][k])
    return out
