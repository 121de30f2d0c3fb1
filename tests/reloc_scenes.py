"""Synthetic relocalisation scenes for the refine chain (tests/test_relocalize_refine.py, tools/latency_relocalize.py): ONE frame and several candidate
keyframes whose slots hold the frame's world points, built so that a hypothesis takes a chosen exit of Tracking::Relocalization's refine loop.

A candidate is described by how many of the frame's real features it covers in each role:
  g  good seeds        BoW match + PnP inlier, the slot holds the feature's true world point
  b  wrong seeds       BoW match + PnP inlier of a CLUTTER feature; the slot holds the world point of a real feature that is left free.  An outlier of pose 1;
                       the slot stays in sFound for search 1 and is found - at its real feature - by search 2
  f  as b, but the slot's point is displaced so that it reprojects 2.75 px * scale beside the real feature: inside search 2's window (3 px * scale), an
     outlier of pose 3 (chi2 7.56 > 5.991)
  e  extra points      no BoW match; found by search 1, inliers of pose 2
  d  decoys            as e, displaced by 6 px * scale: found by search 1 (window 10 px * scale), outliers of pose 2 (which stay, :2188)
  w  wild rotation     as e with the keyframe's angle turned by 180 degrees: assigned by search 1, removed by the rotation histogram
  o  BoW only          as e with a BoW match that PnP did not count as an inlier (mask 0): not in sFound
The remaining slots are invalid, behind the camera, outside the image, out of the distance range, or in view with a descriptor that matches nothing."""
import numpy as np

import track_scenes as ts

CAM, W, H, SCALES, INV_SIGMA2, LOG_SCALE = ts.CAM, ts.W, ts.H, ts.SCALES, ts.INV_SIGMA2, ts.LOG_SCALE

# one candidate per exit of the refine loop (reloc_ref.EXIT_*), in exit order
EXIT_SPECS = (dict(g=6), dict(g=60), dict(g=20, e=10, o=2), dict(g=20, e=40, w=3), dict(g=14, e=6, d=40), dict(g=20, e=20, d=14), dict(g=20, e=18, d=15, b=15),
              dict(g=20, e=18, d=15, f=15))


def build(seed, specs, sensor="mixed", n_features=400, n_real=250, n_slots=300):
    """-> (frame, cands, hyps): hypothesis i = candidate i's designed hypothesis (specs[i])."""
    rng = np.random.default_rng(seed)
    Tt = ts.pose(rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3))
    n, m = n_features, n_real
    clutter = n - m
    u, v, z = rng.uniform(40, W - 40, m), rng.uniform(40, H - 40, m), rng.uniform(2.0, 8.0, m)
    octave = rng.integers(0, 6, m)
    sc = SCALES[octave].astype(np.float64)
    noise = rng.normal(0, 0.3, (m, 2)) * sc[:, None]
    k7 = np.zeros((n, 7), np.float32)
    k7[:m, 0], k7[:m, 1], k7[:m, 5] = u + noise[:, 0], v + noise[:, 1], octave
    k7[m:, 0], k7[m:, 1], k7[m:, 5] = rng.uniform(5, W - 5, clutter), rng.uniform(5, H - 5, clutter), rng.integers(0, 8, clutter)
    k7[:, 2], k7[:, 3], k7[:, 6] = 31, rng.uniform(0, 360, n), -1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ur = np.concatenate([ts._u_right(rng, sensor, k7[:m, 0].astype(np.float64), z, m), ts._u_right(rng, sensor, k7[m:, 0].astype(np.float64), rng.uniform(2, 8, clutter), clutter)])
    Ow = -Tt[:3, :3].T @ Tt[:3, 3]
    cands, hyps = [], []
    for ci, spec in enumerate(specs):
        g, b, f, e, d, w, o = [int(spec.get(k, 0)) for k in "gbfedwo"]
        real = rng.permutation(m)
        roles = np.split(real[:g + b + f + e + d + w + o], np.cumsum([g, b, f, e, d, w]))
        wrong_feat = m + rng.permutation(clutter)[:b + f]                        # the clutter features the wrong seeds sit on
        slots = rng.permutation(n_slots)
        valid = np.zeros(n_slots, np.uint8)
        pos = rng.normal(0, 3, (n_slots, 3))
        maxd, mind = np.full(n_slots, 10.0), np.full(n_slots, 1.0)
        cdesc = rng.integers(0, 256, (n_slots, 32), dtype=np.uint8)
        ang = rng.uniform(0, 360, n_slots)
        bow, mask = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
        si = 0
        for role, feats in zip("gbfedwo", roles):
            for k in feats:
                s = slots[si]
                si += 1
                du = dv = 0.0
                if role == "d":
                    a = rng.uniform(0, 2 * np.pi)
                    du, dv = 6.0 * sc[k] * np.cos(a), 6.0 * sc[k] * np.sin(a)
                if role == "f":                                                  # beside the feature itself (its noise included): 2.75 px * scale along one axis
                    du, dv = [(2.75 * sc[k], 0.0), (-2.75 * sc[k], 0.0), (0.0, 2.75 * sc[k]), (0.0, -2.75 * sc[k])][int(rng.integers(0, 4))]
                    du, dv = du + noise[k, 0], dv + noise[k, 1]
                X = ts._backproject(Tt, np.array([u[k] + du]), np.array([v[k] + dv]), np.array([z[k]]))[0]
                valid[s], pos[s] = 1, X
                maxd[s] = np.linalg.norm(X - Ow) * sc[k] * 0.95                  # PredictScale gives the feature's octave
                mind[s] = maxd[s] / SCALES[7]
                cdesc[s] = ts._flip(rng, desc[k:k + 1], 20)[0]
                ang[s] = (k7[k, 3] + rng.uniform(-3, 3) + (180.0 if role == "w" else 0.0)) % 360
                if role in "go":
                    bow[k], mask[k] = s, 1 if role == "g" else 0
        for i, j in enumerate(wrong_feat):                                       # b, f: the BoW match of a clutter feature (their slots follow the g slots)
            bow[j], mask[j] = slots[g + i], 1
        rest = slots[si:]
        kinds = rng.integers(0, 5, len(rest))                                    # 0 invalid | 1 behind | 2 outside the image | 3 too far | 4 in view, no match
        for s, kind in zip(rest, kinds):
            uu, vv, zz = rng.uniform(40, W - 40), rng.uniform(40, H - 40), rng.uniform(2.0, 8.0)
            if kind == 1:
                zz = -zz
            if kind == 2:
                uu = W + rng.uniform(5, 200)
            X = ts._backproject(Tt, np.array([uu]), np.array([vv]), np.array([zz]))[0]
            pos[s], valid[s] = X, 0 if kind == 0 else 1
            maxd[s] = np.linalg.norm(X - Ow) * (0.5 if kind == 3 else 1.3)
            mind[s] = maxd[s] / SCALES[7]
        cands.append(dict(valid=valid, pos=pos.astype(np.float32), max_distance=maxd.astype(np.float32), min_distance=mind.astype(np.float32), desc=cdesc,
                          kf_angle=ang.astype(np.float32), bow_match=bow))
        Th = ts.pose(rng.normal(0, 0.001, 3), rng.normal(0, 0.005, 3)) @ Tt
        hyps.append(dict(candidate=ci, Tcw=Th.astype(np.float32), inliers=mask))
    frame = dict(kps7=k7, desc=desc, u_right=ur, scale_factors=SCALES, log_scale_factor=LOG_SCALE, width=W, height=H, cam=CAM)
    return frame, cands, hyps


def exits_scene(seed=1, sensor="mixed"):
    return build(seed, EXIT_SPECS, sensor)


def boundary_scene(seed=7, counts=(40, 255, 256, 257, 513)):
    """Hypotheses with exactly `counts` correspondences in pose 1 (good seeds): the boundaries of the pose kernel's instantiations."""
    return build(seed, [dict(g=c) for c in counts], "mixed", n_features=600, n_real=520, n_slots=520)
