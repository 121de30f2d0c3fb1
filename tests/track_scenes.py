"""Synthetic frames for the tracking chains (tests/test_track_chain.py, tools/latency_track_chain.py): a last frame / a local map whose points
are seen again in the current frame with noise, clutter features, a share of WRONG correspondences (the right descriptor, but a world position
that reprojects 10 - 40 px away: real outliers for PoseOptimization), points without observations, mono / stereo / mixed uRight."""
import math

import numpy as np

import track_ref

CAM = (517.3, 516.5, 318.6, 255.3, 40.0)
W, H = 640, 480
SCALES = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
INV_SIGMA2 = (np.float32(1.0) / (SCALES * SCALES)).astype(np.float32)
LOG_SCALE = float(np.float32(math.log(np.float32(1.2))))


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(r, t):
    T = np.eye(4)
    T[:3, :3] = rot(*r)
    T[:3, 3] = t
    return T


def struct_kps(orbx, k7):
    k = np.zeros(len(k7), orbx.KEYPOINT_DTYPE)
    for j, c in enumerate(("x", "y", "size", "angle", "response")):
        k[c] = k7[:, j]
    k["octave"], k["class_id"] = k7[:, 5].astype(np.int32), k7[:, 6].astype(np.int32)
    return k


def _flip(rng, desc, maxbits):
    out = desc.copy()
    for i in range(len(out)):
        for b in rng.integers(0, 256, rng.integers(0, maxbits)):
            out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _backproject(T, u, v, z):
    fx, fy, cx, cy, _ = CAM
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    return (T[:3, :3].T @ (Xc - T[:3, 3]).T).T


def _wrong(rng, u, v, octave, radius_per_level, share):
    """Reprojection targets 10 - 40 px away from the feature for a share of the points - as far as the search window of the point's level still
    reaches the feature (0.85 of the radius)."""
    reach = 0.85 * radius_per_level[octave]
    w = (rng.random(len(u)) < share) & (reach > 11.0)
    d = rng.uniform(10.0, np.minimum(40.0, np.maximum(reach, 10.5)))
    a = rng.uniform(0, 2 * np.pi, len(u))
    return np.where(w, u + d * np.cos(a), u), np.where(w, v + d * np.sin(a), v), w


def _u_right(rng, sensor, u, z, n):
    bf = CAM[4]
    ur = u - bf / z + rng.normal(0, 0.3, n)
    if sensor == "mono":
        return np.full(n, -1.0, np.float32)
    if sensor == "mixed":
        ur = np.where(rng.random(n) < 0.5, ur, -1.0)
    return ur.astype(np.float32)


def motion_scene(seed, n_last=400, clutter=300, sensor="mixed", wrong=0.12, off_px=0.0, th=15.0, obs_frac=0.8, invalid=0.1, behind=0, clean=False, max_octave=6):
    """TrackWithMotionModel: (fr, last) in the dicts of oracle_lib.search_by_projection_last, fr["Tcw"] = the PREDICTED pose (the true one turned
    about y so that every projection moves by about off_px).  clean: every last-frame point is valid, observed and correctly placed (each one is
    matched: the number of correspondences is n_last).  behind: that many extra valid last-frame points behind the camera, which the search skips -
    they raise the host's upper bound on the correspondences, not their number."""
    rng = np.random.default_rng(seed)
    fx = CAM[0]
    Tt = pose(rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3))                       # the current frame's true pose
    Tl = pose(rng.normal(0, 0.01, 3), [0, 0, 0])
    twc = -Tt[:3, :3].T @ Tt[:3, 3]
    Tl[:3, 3] = -Tl[:3, :3] @ twc + np.array([0.03, 0.0, 0.0])                     # sideways: neither forward nor backward against mb
    Tp = pose([0.0, off_px / fx, 0.0], [0, 0, 0]) @ Tt if off_px else pose(rng.normal(0, 0.0005, 3), rng.normal(0, 0.002, 3)) @ Tt
    u, v, z = rng.uniform(40, W - 40, n_last), rng.uniform(40, H - 40, n_last), rng.uniform(2.0, 8.0, n_last)
    octave = rng.integers(0, max_octave, n_last)
    if clean:
        wrong, invalid, obs_frac = 0.0, 0.0, 1.0
    uw, vw, is_wrong = _wrong(rng, u, v, octave, th * SCALES.astype(np.float64), wrong)
    Xw = _backproject(Tt, uw, vw, z)
    noise = rng.normal(0, 0.4, (n_last, 2)) * SCALES[octave][:, None]
    n = n_last + clutter
    k7 = np.zeros((n, 7), np.float32)
    k7[:n_last, 0], k7[:n_last, 1] = u + noise[:, 0], v + noise[:, 1]
    k7[:n_last, 5] = octave
    lang = rng.uniform(0, 360, n_last)
    k7[:n_last, 3] = (lang + np.clip(rng.normal(0, 2.0, n_last), -5.0, 5.0)) % 360      # (within the histogram's bin 0: |rot| < 6)
    if not clean:                                                                   # inconsistent rotations: assigned, then pruned by the histogram (-2)
        wild = rng.random(n_last) < 0.06
        k7[:n_last, 3][wild] = rng.uniform(0, 360, int(wild.sum()))
    k7[n_last:, 0], k7[n_last:, 1] = rng.uniform(5, W - 5, clutter), rng.uniform(5, H - 5, clutter)
    k7[n_last:, 3], k7[n_last:, 5] = rng.uniform(0, 360, clutter), rng.integers(0, 8, clutter)
    k7[:, 2], k7[:, 6] = 31, -1
    ldesc = rng.integers(0, 256, (n_last, 32), dtype=np.uint8)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc[:n_last] = _flip(rng, ldesc, 30)
    ur = np.concatenate([_u_right(rng, sensor, k7[:n_last, 0].astype(np.float64), z, n_last), _u_right(rng, sensor, k7[n_last:, 0].astype(np.float64), rng.uniform(2, 8, clutter), clutter)])
    perm = np.arange(n) if clean else rng.permutation(n)                            # (clean scenes keep feature i = last-frame point i: clutter appended behind changes no order)
    k7, desc, ur = k7[perm], desc[perm], ur[perm]
    lk = np.zeros((n_last + behind, 7), np.float32)
    lk[:n_last, 0], lk[:n_last, 1], lk[:n_last, 3], lk[:n_last, 5] = u, v, lang, octave
    lk[:, 2], lk[:, 6] = 31, -1
    valid = np.ones(n_last + behind, np.uint8)
    valid[:n_last][rng.random(n_last) < invalid] = 0
    valid[:n_last][rng.random(n_last) < invalid / 3] = 2
    has_obs = np.ones(n_last + behind, np.uint8)
    has_obs[:n_last] = rng.random(n_last) < obs_frac
    if behind:
        Xb = _backproject(Tt, rng.uniform(40, W - 40, behind), rng.uniform(40, H - 40, behind), -rng.uniform(2.0, 8.0, behind))
        Xw = np.concatenate([Xw, Xb])
        ldesc = np.concatenate([ldesc, rng.integers(0, 256, (behind, 32), dtype=np.uint8)])
    fr = dict(kps7=k7, desc=desc, u_right=ur, occupied=np.zeros(n, np.uint8), scale_factors=SCALES, width=W, height=H, Tcw=Tp.astype(np.float32), cam=CAM)
    last = dict(Tcw=Tl.astype(np.float32), valid=valid, pos=Xw.astype(np.float32), desc=ldesc, has_obs=has_obs, kps7=lk)
    return fr, last, dict(mono=sensor == "mono", th=th, wrong=is_wrong, truth=Tt)


def trim_valid(fr, last, count_of, target, tries=60):
    """Clears valid flags of `last` from the back until count_of(last) == target (the restatement decides): the scenes with an exact number of
    matches or correspondences."""
    order = np.flatnonzero(last["valid"] == 1)
    k = min(len(order), target)
    for _ in range(tries):
        v = last["valid"].copy()
        v[order[k:]] = 0
        c = count_of(dict(last, valid=v))
        if c == target:
            return dict(last, valid=v)
        k = max(0, min(len(order), k + (target - c)))
    raise AssertionError("no prefix of the valid points gives %d" % target)


def local_scene(seed, m=500, n_held=150, clutter=300, sensor="mixed", wrong=0.12, th=3.0, obs_frac=0.85, held_obs_frac=0.85):
    """TrackLocalMap: a frame at pose T (slightly off the truth) that already holds n_held points (TrackWithMotionModel's matches) and m local map
    points to be searched; features = noisy re-observations + clutter.  Returns (fr, sc): fr as in the projection tests + held / held_pos, sc = the
    points (pos, normal, max_distance, min_distance, desc, has_obs), Tcw, cam."""
    rng = np.random.default_rng(seed)
    Tt = pose(rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3))
    Tp = pose(rng.normal(0, 0.0005, 3), rng.normal(0, 0.002, 3)) @ Tt
    Ts = pose(rng.normal(0, 0.03, 3), rng.normal(0, 0.15, 3)) @ Tt                 # the keyframe the points were created from
    Ows = -Ts[:3, :3].T @ Ts[:3, 3]
    tot = m + n_held
    u, v, z = rng.uniform(40, W - 40, tot), rng.uniform(40, H - 40, tot), rng.uniform(2.0, 8.0, tot)
    src_oct = rng.integers(0, 6, tot)
    Xtrue = _backproject(Tt, u, v, z)
    d = Xtrue - Ows[None, :]
    dist = np.linalg.norm(d, axis=1)
    pts = dict(pos=Xtrue.astype(np.float32), normal=(d / dist[:, None]).astype(np.float32), max_distance=(dist * SCALES[src_oct] * 1.04).astype(np.float32))
    pts["min_distance"] = (pts["max_distance"] / SCALES[7]).astype(np.float32)
    fv = track_ref.is_in_frustum(Tp.astype(np.float32), CAM, (0.0, float(W), 0.0, float(H)), LOG_SCALE, 8, pts)
    level = fv["level"]                                                            # the level the reference will predict: the feature is found there
    radius = 2.5 * th * SCALES.astype(np.float64)                                  # ORBmatcher::RadiusByViewingCos: 2.5 or 4.0
    is_held = np.arange(tot) >= m
    uw, vw, is_wrong = _wrong(rng, u, v, level, radius, wrong)
    hw = is_held & (rng.random(tot) < wrong)                                       # a held point needs no window: any offset makes an outlier
    ang, dd = rng.uniform(0, 2 * np.pi, tot), rng.uniform(10, 40, tot)
    uw, vw = np.where(hw, u + dd * np.cos(ang), uw), np.where(hw, v + dd * np.sin(ang), vw)
    Xw = _backproject(Tt, uw, vw, z).astype(np.float32)
    noise = rng.normal(0, 0.4, (tot, 2)) * SCALES[level][:, None]
    n = tot + clutter
    k7 = np.zeros((n, 7), np.float32)
    k7[:tot, 0], k7[:tot, 1], k7[:tot, 5] = u + noise[:, 0], v + noise[:, 1], level
    k7[tot:, 0], k7[tot:, 1], k7[tot:, 5] = rng.uniform(5, W - 5, clutter), rng.uniform(5, H - 5, clutter), rng.integers(0, 8, clutter)
    k7[:, 2], k7[:, 3], k7[:, 6] = 31, rng.uniform(0, 360, n), -1
    pdesc = rng.integers(0, 256, (tot, 32), dtype=np.uint8)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc[:tot] = _flip(rng, pdesc, 30)
    ur = np.concatenate([_u_right(rng, sensor, k7[:tot, 0].astype(np.float64), z, tot), _u_right(rng, sensor, k7[tot:, 0].astype(np.float64), rng.uniform(2, 8, clutter), clutter)])
    held = np.zeros(n, np.uint8)
    held[m:tot] = 1
    held_pos = np.zeros((n, 3), np.float32)
    held_pos[m:tot] = Xw[m:]
    occupied = np.zeros(n, np.uint8)
    occupied[m:tot] = rng.random(n_held) < held_obs_frac
    perm = rng.permutation(n)
    fr = dict(kps7=k7[perm], desc=desc[perm], u_right=ur[perm], occupied=occupied[perm], scale_factors=SCALES, width=W, height=H, held=held[perm], held_pos=held_pos[perm])
    sc = dict(pos=Xw[:m], normal=pts["normal"][:m], max_distance=pts["max_distance"][:m], min_distance=pts["min_distance"][:m], desc=pdesc[:m],
              has_obs=(rng.random(m) < obs_frac).astype(np.uint8), Tcw=Tp.astype(np.float32), cam=CAM, th=th, stereo=sensor == "stereo")
    return fr, sc
