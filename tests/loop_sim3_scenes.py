"""Scenes of tests/test_loop_sim3.py: a current keyframe KF1 and K loop candidates that see (part of) the same structure through maps of their own, each
related to KF1's by a similarity X1c = s R12 X2c + t12, with SearchByBoW's matches and the events a Sim3Solver would return.

Slots of KF1: `real` points (candidate c sees the first shared[c] of them), `twins` (KF1-only copies of the first real points: the point next to them takes
the same KF2 feature, and the mutual check of SearchBySim3 drops one of the two), `decoys` (valid points nobody else sees; a wrong BoW match pairs a KF1 decoy
with a KF2 decoy: a pair whose chi2 is far beyond any threshold) and `extras` (features without a map point).  Every slot order is shuffled.
A map point carries its own feature's descriptor and the distances MapPoint's constructor computes from its keyframe (src/MapPoint.cc:70-92), so a scene
can be handed to the compiled reference as it is.  Camera, image size and scale tables are those of oracle/refslam_wrap.cc."""
import math

import numpy as np

from test_fuse import INV_SIGMA2, SF
from test_matcher import _rand_desc

F32, F64 = np.float32, np.float64
CAM = (500.0, 500.0, 320.0, 240.0)
WIDTH, HEIGHT = 640, 480
LOG_SF = float(np.log(F32(1.2)))


def _rot(axis, ang):
    axis = np.asarray(axis, F64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def mappoint_distances(Rcw, tcw, pos, octave):
    """mfMaxDistance, mfMinDistance as MapPoint(Pos, pMap, pFrame, idxF) leaves them: dist = cv::norm(Pos - Ow) narrowed to float, times the level's scale factor"""
    R, t, P = np.asarray(Rcw, F32).reshape(3, 3), np.asarray(tcw, F32).reshape(3), np.asarray(pos, F32).reshape(-1, 3)
    Ow = np.array([((-R[0, r]) * t[0] + (-R[1, r]) * t[1]) + (-R[2, r]) * t[2] for r in range(3)], F32)
    PC = (P - Ow[None, :]).astype(F64)
    dist = np.sqrt(PC[:, 0] * PC[:, 0] + PC[:, 1] * PC[:, 1] + PC[:, 2] * PC[:, 2]).astype(F32)
    mx = dist * SF[octave]
    return mx.astype(F32), (mx / SF[-1]).astype(F32)


def _project(X):
    return np.stack([CAM[0] * X[:, 0] / X[:, 2] + CAM[2], CAM[1] * X[:, 1] / X[:, 2] + CAM[3]], 1)


def _keyframe(orbx, R, t, Xc, octave, desc, valid, noise, g):
    """A keyframe whose slot i holds the camera point Xc[i] (valid[i]) seen at `octave[i]` with descriptor desc[i]; invalid slots are features at random places"""
    n = len(Xc)
    R32, t32 = R.astype(F32), t.astype(F32)
    world = ((Xc - t) @ R).astype(F32)                     # R^T (Xc - t)
    uv = np.where(valid[:, None], _project(np.where(valid[:, None], Xc, [0, 0, 1.0])) + g.normal(size=(n, 2)) * (noise * SF[octave])[:, None],
                  np.stack([g.uniform(0, WIDTH, n), g.uniform(0, HEIGHT, n)], 1))
    k = np.zeros(n, orbx.KEYPOINT_DTYPE)
    k["x"], k["y"], k["size"], k["octave"], k["class_id"], k["response"] = uv[:, 0], uv[:, 1], 31, octave, -1, 40
    world[~valid] = 0
    mx, mn = mappoint_distances(R32, t32, world, octave)
    return dict(kps=k, desc=desc, point_desc=desc, Rcw=R32, tcw=t32, cam=CAM, scale_factors=SF, log_scale_factor=LOG_SF, inv_level_sigma2=INV_SIGMA2, width=WIDTH, height=HEIGHT,
                valid=valid.astype(np.uint8), pos=world, max_distance=mx, min_distance=mn)


def _shuffle(kf, perm):
    out = dict(kf)
    for k in ("kps", "desc", "point_desc", "valid", "pos", "max_distance", "min_distance"):
        out[k] = np.ascontiguousarray(kf[k][perm])
    return out


def _flip(desc, g, most):
    d = desc.copy()
    for i in range(len(d)):
        for b in g.integers(0, 256, int(g.integers(0, most + 1))):
            d[i, b >> 3] ^= 1 << (b & 7)
    return d


def _front(g, n):
    z = g.uniform(3.0, 8.0, n)
    return np.stack([g.uniform(-0.4, 0.4, n) * z, g.uniform(-0.27, 0.27, n) * z, z], 1)


def build(orbx, seed, shared, scales=None, bow=30, twins=0, decoys=12, extras=20, noise=0.3):
    """-> (kf1, cands, truth): cands[c] carries bow_match [N1] (the first bow[c] shared points of candidate c, true matches) and `slot2` [N1] (the KF2 slot of the
    same point or -1: for the tests, not for the chain); kf1 carries `kind` [N1] (0 real, 1 twin, 2 decoy, 3 extra) and `point` [N1] (index of the real point);
    truth[c] = (R12, t12, s)."""
    g = np.random.default_rng(seed)
    K, nr = len(shared), max(shared)
    scales = [1.0] * K if scales is None else scales
    bow = [bow] * K if np.isscalar(bow) else bow
    X1 = _front(g, nr)
    oct1 = g.integers(1, 6, nr)
    base = _rand_desc(g, nr)
    Rc1, tc1 = _rot(g.normal(size=3), 0.4), g.normal(size=3)
    # KF1: real | twins | decoys | extras
    n1 = nr + twins + decoys + extras
    Xc = np.concatenate([X1, X1[:twins] + 1e-3, _front(g, decoys), np.zeros((extras, 3))])
    octs = np.concatenate([oct1, oct1[:twins], g.integers(1, 6, decoys), g.integers(0, 8, extras)])
    d1 = _flip(base, g, 6)
    tw = d1[:twins].copy()
    tw[:, 0] ^= 1
    desc = np.concatenate([d1, tw, _rand_desc(g, decoys + extras)]) if twins + decoys + extras else d1
    valid = np.arange(n1) < nr + twins + decoys
    kf1 = _keyframe(orbx, Rc1, tc1, Xc, octs, desc, valid, noise, g)
    kind = np.concatenate([np.zeros(nr, int), np.ones(twins, int), np.full(decoys, 2), np.full(extras, 3)])
    point = np.concatenate([np.arange(nr), np.arange(twins), np.full(decoys + extras, -1)])
    perm1 = g.permutation(n1)
    inv1 = np.argsort(perm1)
    kf1 = _shuffle(kf1, perm1)
    kf1["kind"], kf1["point"] = kind[perm1], point[perm1]
    cands, truth = [], []
    for c in range(K):
        ns, s = shared[c], float(scales[c])
        R12, t12 = _rot(g.normal(size=3), float(g.uniform(0.02, 0.08))), g.normal(size=3) * 0.08
        Rc2, tc2 = _rot(g.normal(size=3), 0.7), g.normal(size=3)
        X2 = (X1[:ns] - t12) @ R12 / s                     # R12^T (X1c - t12) / s
        dist1, dist2 = np.linalg.norm(X1[:ns], axis=1), np.linalg.norm(X2, axis=1)
        lvl2 = np.clip(np.ceil(np.log(dist1 * SF[oct1[:ns]] / dist2) / math.log(1.2)), 0, 7).astype(int)
        oct2 = np.clip(lvl2 - (g.random(ns) < 0.3), 0, 7)
        n2 = ns + decoys + extras
        Xc2 = np.concatenate([X2, _front(g, decoys), np.zeros((extras, 3))])
        octs2 = np.concatenate([oct2, g.integers(1, 6, decoys), g.integers(0, 8, extras)])
        desc2 = np.concatenate([_flip(base[:ns], g, 6), _rand_desc(g, decoys + extras)]) if decoys + extras else _flip(base[:ns], g, 6)
        kf2 = _keyframe(orbx, Rc2, tc2, Xc2, octs2, desc2, np.arange(n2) < ns + decoys, noise, g)
        perm2 = g.permutation(n2)
        inv2 = np.argsort(perm2)
        kf2 = _shuffle(kf2, perm2)
        slot2 = np.full(n1, -1, np.int32)
        slot2[inv1[:ns]] = inv2[:ns]
        bm = np.full(n1, -1, np.int32)
        nb = min(bow[c], ns)
        bm[inv1[:nb]] = inv2[:nb]
        kf2["bow_match"], kf2["slot2"] = bm, slot2
        kf2["decoy_pairs"] = [(int(inv1[nr + twins + j]), int(inv2[ns + j])) for j in range(decoys)]      # (KF1 decoy slot, KF2 decoy slot)
        cands.append(kf2)
        truth.append((R12, t12, s))
    return kf1, cands, truth


def hypothesis(kf1, cands, truth, c, seed, kind="good", seeds=None, wrong=0, fix=False):
    """An event of candidate c: the truth moved a little ("good") or far ("bad"), the mask over `seeds` of its true BoW matches (None = all) and `wrong` decoy
    pairs, which are added to the candidate's bow_match."""
    g = np.random.default_rng(seed)
    R12, t12, s = truth[c]
    if kind == "good":
        R, t, sc = _rot(g.normal(size=3), 0.003) @ R12, t12 + 0.005 * g.normal(size=3), s * 1.002
    else:
        R, t, sc = _rot(g.normal(size=3), 0.5) @ R12, t12 + 1.0, s
    if fix:
        sc = 1.0
    bm = cands[c]["bow_match"]
    have = np.flatnonzero(bm >= 0)
    have = have[[i for i, f in enumerate(have) if kf1["kind"][f] == 0]]
    mask = np.zeros(len(bm), np.uint8)
    mask[have if seeds is None else have[:seeds]] = 1
    for a, b in cands[c]["decoy_pairs"][:wrong]:
        bm[a] = b
        mask[a] = 1
    return dict(candidate=c, R12=R.astype(F32), t12=t.astype(F32), s12=F32(sc), inliers=mask)


def from_fuse_scene(orbx, seed, s=1.0, npre=0):
    """Two keyframes out of test_fuse._scene: KF1 = its source keyframe (pose I, every feature holds the point it created), KF2 = its target keyframe in a map
    of its own that is KF1's scaled by 1 / s, so that X1c = s R12 X2c + t12 with R12 = Rt^T, t12 = -Rt^T tt.  A target feature holds the point whose projection
    lies nearest (within 6 px), any other a point on its own viewing ray.  -> (kf1, kf2 (with bow_match: npre true pairs), (R12, t12, s))"""
    from test_fuse import _scene
    kf, Tt, sk, Ts, P, cdesc, g = _scene(orbx, seed)
    nc, n = len(P), len(kf["kps"])
    Rt, tt = Tt[:3, :3].astype(F64), Tt[:3, 3].astype(F64)
    base = dict(cam=CAM, scale_factors=SF, log_scale_factor=LOG_SF, inv_level_sigma2=INV_SIGMA2, width=WIDTH, height=HEIGHT)
    eye, zero = np.eye(3, dtype=F32), np.zeros(3, F32)
    mx, mn = mappoint_distances(eye, zero, P, sk["octave"])
    kf1 = dict(base, kps=sk, desc=cdesc, point_desc=cdesc, Rcw=eye, tcw=zero, valid=np.ones(nc, np.uint8), pos=P.astype(F32), max_distance=mx, min_distance=mn)
    Pc = P.astype(F64) @ Rt.T + tt
    front = Pc[:, 2] > 0.1
    uv = np.where(front[:, None], _project(np.where(front[:, None], Pc, [0, 0, 1.0])), -1e6)
    k2 = kf["kps"]
    X2c = np.zeros((n, 3))
    owner = np.full(n, -1)
    for i in range(n):
        d = np.abs(uv - [k2["x"][i], k2["y"][i]]).max(1)
        j = int(np.argmin(d))
        if d[j] < 6.0:
            X2c[i], owner[i] = Pc[j], j
        else:
            z = g.uniform(2.5, 9.0)
            X2c[i] = [(k2["x"][i] - CAM[2]) / CAM[0] * z, (k2["y"][i] - CAM[3]) / CAM[1] * z, z]
    R2, t2 = Rt.astype(F32), (tt / s).astype(F32)
    pos2 = ((X2c / s - tt / s) @ Rt).astype(F32)
    mx2, mn2 = mappoint_distances(R2, t2, pos2, k2["octave"])
    bm = np.full(nc, -1, np.int32)
    seen = set()
    for i in np.flatnonzero(owner >= 0):
        if len(seen) < npre and owner[i] not in seen:
            bm[owner[i]] = i
            seen.add(int(owner[i]))
    kf2 = dict(base, kps=k2, desc=kf["desc"], point_desc=kf["desc"], Rcw=R2, tcw=t2, valid=np.ones(n, np.uint8), pos=pos2, max_distance=mx2, min_distance=mn2, bow_match=bm)
    return kf1, kf2, (Rt.T, -Rt.T @ tt, s)
