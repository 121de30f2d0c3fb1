"""Scenes of tests/test_search_in_neighbors.py and tools/latency_search_in_neighbors.py: map slices as fuse_slice() dicts.

hand_slice   a slice whose geometry does not matter (orbx_fuse_apply takes the search results from the caller): the keyframes' kf_point and the other
             keyframes' observations are given literally.
chain_scene  a current keyframe, T targets and a few further observers looking at M world points.  Per world point one of
               shared     the old point is held by the current keyframe and by some targets; the other targets have an empty feature there (forward ADD)
               duplicate  the current keyframe holds a freshly triangulated two-observation duplicate, the targets hold the old point with more observations
                          (the duplicate is replaced by the holder in the first target that sees it, and is bad for the targets behind it: the calls are
                          coupled); for half of them the old point is also observed by the duplicate's second observer (the conflict erase)
               weak       the current keyframe holds the point, every target holds a weak point of its own there with fewer or equally many observations
                          (the holder is replaced)
               badheld    the targets' features there hold a point that is bad (nothing changes, nFused counts)
               reverse    only the targets hold the point, the current keyframe has an empty feature there (ADD in the reverse pass)
"""
import math

import numpy as np

SF = np.array([1.0, 1.2, 1.44, 1.728, 2.0736, 2.48832, 2.985984, 3.5831808], np.float32)
INV_SIGMA2 = (np.float32(1.0) / (SF * SF)).astype(np.float32)
LOG_SF = np.float32(math.log(float(np.float32(1.2))))      # logf(1.2f)
CAM = (500.0, 500.0, 320.0, 240.0, 40.0)
BOUNDS = (0.0, 0.0, 640.0, 480.0)


def _kp_dtype():
    return np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def _flip(rng, d, nmax=10):
    d = d.copy()
    for b in rng.integers(0, 256, int(rng.integers(0, nmax + 1))):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _pose(rng):
    a = rng.normal(0, 0.02, 3)
    ca, sa = np.cos(a), np.sin(a)
    Rx = np.array([[1, 0, 0], [0, ca[0], -sa[0]], [0, sa[0], ca[0]]])
    Ry = np.array([[ca[1], 0, sa[1]], [0, 1, 0], [-sa[1], 0, ca[1]]])
    Rz = np.array([[ca[2], -sa[2], 0], [sa[2], ca[2], 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = rng.normal(0, 0.15, 3)
    return T.astype(np.float32)


def _keyframe(slot, kps, desc, ur, kfp, Tcw=None):
    T = np.eye(4, dtype=np.float32) if Tcw is None else np.asarray(Tcw, np.float32)
    ow = (-(T[:3, :3].T.astype(np.float64) @ T[:3, 3].astype(np.float64))).astype(np.float32)
    return dict(slot=slot, kps=kps, desc=np.asarray(desc, np.uint8).reshape(-1, 32), u_right=np.asarray(ur, np.float32), kf_point=np.asarray(kfp, np.int32), Tcw=T, ow=ow, cam=CAM,
                bounds=BOUNDS, scale_factors=SF, inv_level_sigma2=INV_SIGMA2, log_scale_factor=LOG_SF)


def _points(P, rng, pos=None, rawmax=None, desc=None, bad=None):
    pos = np.tile(np.array([0, 0, 5], np.float32), (P, 1)) if pos is None else np.asarray(pos, np.float32).reshape(P, 3)
    nrm = (pos.astype(np.float64) / np.maximum(np.linalg.norm(pos.astype(np.float64), axis=1), 1e-9)[:, None]).astype(np.float32) if P else np.zeros((0, 3), np.float32)
    rawmax = np.full(P, 8.0, np.float32) if rawmax is None else np.asarray(rawmax, np.float32)
    return dict(pos=pos, normal=nrm, raw_max_dist=rawmax, max_dist=(np.float32(1.2) * rawmax).astype(np.float32),
                min_dist=(np.float32(0.8) * (rawmax / SF[-1])).astype(np.float32), desc=rng.integers(0, 256, (P, 32)).astype(np.uint8) if desc is None else np.asarray(desc, np.uint8),
                bad=np.zeros(P, np.uint8) if bad is None else np.asarray(bad, np.uint8), visible=rng.integers(1, 50, P).astype(np.int32), found=rng.integers(1, 30, P).astype(np.int32))


def hand_slice(orbx, kf_points, P, other_obs=(), stereo=None, ranks=None, kf_bad=None, bad=None, num_keyframes=None, seed=0):
    """kf_points: {slot: [point id or -1 per feature]} of the searchable keyframes; other_obs: (point, slot, feature, stereo) of the others;
    stereo: {slot: set of stereo features}.  Descriptors are random, one per feature."""
    rng = np.random.default_rng(seed)
    searchable = []
    for slot, kfp in kf_points.items():
        n = len(kfp)
        kps = np.zeros(n, _kp_dtype())
        kps["x"], kps["y"], kps["size"], kps["class_id"] = rng.uniform(20, 600, n), rng.uniform(20, 440, n), 31, -1
        ur = np.full(n, -1.0, np.float32)
        for f in (stereo or {}).get(slot, ()):
            ur[f] = kps["x"][f] - 8.0
        searchable.append(_keyframe(slot, kps, rng.integers(0, 256, (n, 32)).astype(np.uint8), ur, kfp))
    oo = [(p, kf, f, st, rng.integers(0, 256, 32).astype(np.uint8)) for p, kf, f, st in other_obs]
    return orbx.fuse_slice(searchable, _points(P, rng, bad=bad), oo, num_keyframes=num_keyframes, ranks=ranks, kf_bad=kf_bad)


def chain_scene(orbx, seed, T=3, M=150, mode="mixed", repeat=False, bad_observer=False, noise_features=15, present=0.8, info=None, mix=(0.25, 0.3, 0.2, 0.1, 0.15)):
    """-> (slice, current slot, target slots).  mode: mono / stereo / mixed (u_right of the features).  info: a dict that receives cat (the kind of every
    world point), old (its old point) and feature ((searchable keyframe, world point) -> feature).  mix: the shares of shared / duplicate / weak / badheld / reverse
    world points; present: the chance that a target sees a world point."""
    rng = np.random.default_rng(seed)
    S, NO = T + 1, 3                                            # searchable keyframes 0 (current), 1..T; other observers T+1..T+3
    NK = S + NO
    poses = [_pose(rng) for _ in range(S)]
    X = np.stack([rng.uniform(-2.3, 2.3, M), rng.uniform(-1.7, 1.7, M), rng.uniform(4, 9, M)], 1).astype(np.float32)
    base = rng.integers(0, 256, (M, 32)).astype(np.uint8)
    oct0 = rng.integers(0, 6, M)
    rawmax0 = (np.linalg.norm(X.astype(np.float64), axis=1) * SF[oct0]).astype(np.float32)
    cat = rng.choice(5, M, p=list(mix))      # shared, duplicate, weak, badheld, reverse
    ppos, praw, pdesc, pbad = [], [], [], []

    def new_point(j, bad=0):
        ppos.append(X[j] + rng.normal(0, 0.003, 3).astype(np.float32)); praw.append(rawmax0[j]); pdesc.append(_flip(rng, base[j], 6)); pbad.append(bad)
        return len(ppos) - 1
    old = [new_point(j) for j in range(M)]
    feats = [[] for _ in range(S)]                              # per searchable keyframe: (world point, holder)
    other = []                                                  # (point, slot, feature, stereo, descriptor)
    ocount = [0] * NO

    def observe_other(p, j, o):
        other.append((p, S + o, ocount[o], int(rng.random() < 0.3) if mode != "mono" else 0, _flip(rng, base[j])))
        ocount[o] += 1
    for j in range(M):
        c = cat[j]
        tsee = [t for t in range(1, S) if rng.random() < present]
        if c == 0:
            feats[0].append((j, old[j]))
            for t in range(1, S):
                feats[t].append((j, old[j] if t in tsee else -1))
            observe_other(old[j], j, 0)
        elif c == 1:
            d = new_point(j)
            feats[0].append((j, d))
            observe_other(d, j, 1)
            for t in tsee:
                feats[t].append((j, old[j]))
            observe_other(old[j], j, 0)
            if rng.random() < 0.5:
                observe_other(old[j], j, 1)                      # the old point and its duplicate are both observed by observer 1
            if len(tsee) < 2:
                observe_other(old[j], j, 2)
        elif c == 2:
            feats[0].append((j, old[j]))
            observe_other(old[j], j, 0)
            if rng.random() < 0.5:
                observe_other(old[j], j, 2)
            for t in tsee:
                w = new_point(j)
                feats[t].append((j, w))
                if rng.random() < 0.5:
                    observe_other(w, j, 1)
        elif c == 3:
            feats[0].append((j, old[j]))
            observe_other(old[j], j, 0)
            for t in tsee:
                feats[t].append((j, new_point(j, bad=1)))
        else:
            feats[0].append((j, -1))
            for t in tsee:
                feats[t].append((j, old[j]))
            observe_other(old[j], j, 2)
    searchable = []
    for s in range(S):
        T4 = poses[s]
        order = rng.permutation(len(feats[s]))
        n = len(order) + noise_features
        kps = np.zeros(n, _kp_dtype())
        kps["size"], kps["class_id"], kps["response"] = 31, -1, 40
        desc, ur, kfp = np.zeros((n, 32), np.uint8), np.full(n, -1.0, np.float32), np.full(n, -1, np.int32)
        ow = -(T4[:3, :3].T.astype(np.float64) @ T4[:3, 3].astype(np.float64))
        for f, e in enumerate(order):
            j, holder = feats[s][e]
            Pc = T4[:3, :3].astype(np.float64) @ X[j].astype(np.float64) + T4[:3, 3].astype(np.float64)
            lvl = int(np.clip(np.ceil(np.log(float(rawmax0[j]) / np.linalg.norm(X[j].astype(np.float64) - ow)) / np.log(1.2)), 0, 7))
            kps["x"][f] = Pc[0] / Pc[2] * 500 + 320 + rng.normal(0, 0.5) * SF[lvl]
            kps["y"][f] = Pc[1] / Pc[2] * 500 + 240 + rng.normal(0, 0.5) * SF[lvl]
            kps["octave"][f] = max(lvl - int(rng.integers(0, 2)), 0)
            desc[f] = _flip(rng, base[j])
            if mode == "stereo" or (mode == "mixed" and rng.random() < 0.4):
                ur[f] = kps["x"][f] - 40.0 / Pc[2] + rng.normal(0, 0.3)
            kfp[f] = holder
            if info is not None:
                info.setdefault("feature", {})[(s, int(j))] = f
        m = len(order)
        kps["x"][m:], kps["y"][m:], kps["octave"][m:] = rng.uniform(0, 640, noise_features), rng.uniform(0, 480, noise_features), rng.integers(0, 8, noise_features)
        desc[m:] = rng.integers(0, 256, (noise_features, 32))
        searchable.append(_keyframe(s, kps, desc, ur, kfp, T4))
    if info is not None:
        info.update(cat=cat, old=old)
    P = len(ppos)
    pts = _points(P, rng, pos=np.array(ppos, np.float32), rawmax=np.array(praw, np.float32), desc=np.array(pdesc, np.uint8), bad=np.array(pbad, np.uint8))
    kf_bad = np.zeros(NK, np.uint8)
    if bad_observer:
        kf_bad[S] = 1
    sl = orbx.fuse_slice(searchable, pts, other, num_keyframes=NK, ranks=rng.permutation(NK) * 7 + 3, kf_bad=kf_bad)
    targets = list(range(1, S))
    if repeat and T > 2:
        targets.append(2)
    return sl, 0, targets
