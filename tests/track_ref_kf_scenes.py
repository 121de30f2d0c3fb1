"""Synthetic scenes for Tracking::TrackReferenceKeyFrame and the head of Tracking::Relocalization (tests/test_track_reference_keyframe.py,
tools/latency_track_ref.py): keyframes whose slots hold world points that the frame sees again - a descriptor up to 29 bits away, the same vocabulary
node, a consistent rotation -, plus what makes the branches of the two functions: slots without a (good) map point, points without observations,
WRONG world positions (reprojecting 10 - 40 px away: outliers of PoseOptimization), rotations that the histogram prunes, features that are not filed
in the FeatureVector, clutter on both sides, mono / stereo / mixed uRight, and mvKeys that differ from mvKeysUn.

A keyframe is dict(kps7, desc, groups, valid, pos, has_obs), a frame dict(kps7 (mvKeys), kps7_un (mvKeysUn), desc, groups, u_right, Tcw, cam)."""
import numpy as np

import track_scenes as ts

CAM, W, H, SCALES, INV_SIGMA2 = ts.CAM, ts.W, ts.H, ts.SCALES, ts.INV_SIGMA2
LEVEL_SIGMA2 = (SCALES * SCALES).astype(np.float32)
N_GROUPS = 40


def _distort(k7_un):
    """mvKeys from mvKeysUn: a smooth radial shift of up to ~3 px (the search reads angles only; the pose problem must read mvKeysUn)"""
    k = k7_un.copy()
    dx, dy = (k[:, 0] - CAM[2]) / W, (k[:, 1] - CAM[3]) / H
    r2 = dx * dx + dy * dy
    k[:, 0], k[:, 1] = k[:, 0] + 6.0 * dx * r2, k[:, 1] + 6.0 * dy * r2
    return k.astype(np.float32)


def _frame(rng, n_real, clutter, sensor):
    """The frame's own arrays in construction order: n_real features that see a world point (returned with their truth), then clutter."""
    Tt = ts.pose(rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3))
    u, v, z = rng.uniform(40, W - 40, n_real), rng.uniform(40, H - 40, n_real), rng.uniform(2.0, 8.0, n_real)
    octave = rng.integers(0, 6, n_real)
    noise = rng.normal(0, 0.4, (n_real, 2)) * SCALES[octave][:, None]
    n = n_real + clutter
    k7 = np.zeros((n, 7), np.float32)
    k7[:n_real, 0], k7[:n_real, 1], k7[:n_real, 5] = u + noise[:, 0], v + noise[:, 1], octave
    k7[n_real:, 0], k7[n_real:, 1], k7[n_real:, 5] = rng.uniform(5, W - 5, clutter), rng.uniform(5, H - 5, clutter), rng.integers(0, 8, clutter)
    k7[:, 2], k7[:, 3], k7[:, 6] = 31, rng.uniform(0, 360, n), -1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    groups = rng.integers(0, N_GROUPS, n).astype(np.int32)
    ur = np.concatenate([ts._u_right(rng, sensor, k7[:n_real, 0].astype(np.float64), z, n_real),
                         ts._u_right(rng, sensor, k7[n_real:, 0].astype(np.float64), rng.uniform(2, 8, clutter), clutter)])
    return Tt, (u, v, z, octave), k7, desc, groups, ur


def _keyframe(rng, Tt, truth, k7, desc, groups, seen, n_slots, wrong, invalid, obs_frac, wild, clean):
    """A keyframe with n_slots slots of which the first len(seen) hold the world points of the frame features `seen` (then permuted unless clean)."""
    u, v, z, octave = [t[seen] for t in truth]
    m, extra = len(seen), n_slots - len(seen)
    uw, vw, is_wrong = ts._wrong(rng, u, v, octave, 40.0 * np.ones(8), wrong)
    pos = np.concatenate([ts._backproject(Tt, uw, vw, z), ts._backproject(Tt, rng.uniform(40, W - 40, extra), rng.uniform(40, H - 40, extra), rng.uniform(2, 8, extra))])
    kk = np.zeros((n_slots, 7), np.float32)
    kk[:, 0], kk[:, 1], kk[:, 2], kk[:, 6] = rng.uniform(5, W - 5, n_slots), rng.uniform(5, H - 5, n_slots), 31, -1
    kk[:m, 5], kk[m:, 5] = octave, rng.integers(0, 8, extra)
    kk[:m, 3] = (k7[seen, 3] + np.clip(rng.normal(0, 2.0, m), -5.0, 5.0)) % 360      # (within the histogram's bin 0: |rot| < 6)
    kk[m:, 3] = rng.uniform(0, 360, extra)
    kd = rng.integers(0, 256, (n_slots, 32), dtype=np.uint8)
    kd[:m] = ts._flip(rng, desc[seen], 30)
    kg = rng.integers(0, N_GROUPS, n_slots).astype(np.int32)
    kg[:m] = groups[seen]
    valid, has_obs = np.ones(n_slots, np.uint8), np.ones(n_slots, np.uint8)
    if not clean:
        turn = rng.random(m) < wild                                                   # inconsistent rotations: matched, then pruned by the histogram
        kk[:m, 3][turn] = rng.uniform(0, 360, int(turn.sum()))
        valid[rng.random(n_slots) < invalid] = 0
        has_obs[:] = rng.random(n_slots) < obs_frac
        kg[rng.random(n_slots) < 0.02] = -1                                           # not filed in the FeatureVector
    perm = np.arange(n_slots) if clean else rng.permutation(n_slots)
    kf = dict(kps7=kk[perm], desc=kd[perm], groups=kg[perm], valid=valid[perm], pos=pos[perm].astype(np.float32), has_obs=has_obs[perm])
    return kf, is_wrong


def ref_scene(seed, n_seen=400, kf_extra=100, clutter=300, sensor="mixed", wrong=0.12, invalid=0.1, obs_frac=0.8, wild=0.06, clean=False):
    """TrackReferenceKeyFrame: (kf, fr, meta).  fr["Tcw"] = the last frame's pose, slightly off the truth.  clean: every keyframe slot is valid, observed,
    correctly placed and consistently rotated, and nothing is permuted: each of the n_seen points is matched, so the number of correspondences is n_seen,
    while kf_extra (valid slots that match nothing) and clutter only raise the host's bound min(N, valid slots)."""
    rng = np.random.default_rng(seed)
    Tt, truth, k7u, desc, groups, ur = _frame(rng, n_seen, clutter, sensor)
    kf, is_wrong = _keyframe(rng, Tt, truth, k7u, desc, groups, np.arange(n_seen), n_seen + kf_extra, wrong, invalid, obs_frac, wild, clean)
    n = n_seen + clutter
    if not clean:
        groups = groups.copy()
        groups[rng.random(n) < 0.02] = -1
    perm = np.arange(n) if clean else rng.permutation(n)
    Tp = ts.pose(rng.normal(0, 0.003, 3), rng.normal(0, 0.01, 3)) @ Tt
    k7u = k7u[perm]
    fr = dict(kps7=_distort(k7u), kps7_un=k7u, desc=desc[perm], groups=groups[perm], u_right=ur[perm], Tcw=Tp.astype(np.float32), cam=CAM)
    return kf, fr, dict(truth=Tt, wrong=is_wrong)


def reloc_scene(seed, n_frame=600, n_real=400, kfs=((500, 200),) * 3, sensor="mono"):
    """Relocalization's head: (fr, [kf]) - ONE frame with n_real features that see world points, and per entry (n_slots, n_seen) of `kfs` a candidate
    keyframe that holds n_seen of them (a random subset) among n_slots slots."""
    rng = np.random.default_rng(seed)
    n_real = min(n_real, n_frame)
    Tt, truth, k7u, desc, groups, ur = _frame(rng, n_real, n_frame - n_real, sensor)
    cands = []
    for n_slots, n_seen in kfs:
        seen = np.sort(rng.permutation(n_real)[:min(n_seen, n_slots, n_real)])
        cands.append(_keyframe(rng, Tt, truth, k7u, desc, groups, seen, n_slots, 0.1, 0.1, 0.8, 0.06, False)[0])
    groups = groups.copy()
    groups[rng.random(n_frame) < 0.02] = -1
    perm = rng.permutation(n_frame)
    k7u = k7u[perm]
    fr = dict(kps7=_distort(k7u), kps7_un=k7u, desc=desc[perm], groups=groups[perm], u_right=ur[perm], Tcw=Tt.astype(np.float32), cam=CAM)
    return fr, cands


def trim_valid(kf, count_of, target):
    """Clears valid flags of the keyframe from the back until count_of(kf) == target (the restatement decides)."""
    return ts.trim_valid(None, kf, count_of, target)
