"""Sim3Solver (reference src/Sim3Solver.cc) restated in numpy, and the scenes of tests/test_sim3_solver.py.

The float32 form does every operation in the order include/orbx.h lists above orbx_sim3_solver_create (numpy's float32 / float64 element-wise
operations are IEEE operations, one rounding each), vectorised over the iterations of a candidate.  Every stage takes the stage before it as an
argument, so that a test can feed it the DEVICE's own upstream output.  The float64 form takes the eigenvector from numpy.linalg.eigh.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
SWEEPS = 8      # ORBX_SIM3_JACOBI_SWEEPS of include/orbx.h


# ---------------------------------------------------------------------------------------------------------------------------------------
# constructor (:48-140), FromCameraToImage (:526-545)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _transform(R, t, X):
    R, t, X = np.asarray(R, F32).reshape(3, 3), np.asarray(t, F32).reshape(3), np.asarray(X, F32).reshape(-1, 3)
    return np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)


def _to_image(X, K):
    fx, fy, cx, cy = [F32(v) for v in K]
    with np.errstate(all="ignore"):
        invz = F32(1) / X[:, 2]
        return np.stack([fx * (X[:, 0] * invz) + cx, fy * (X[:, 1] * invz) + cy], 1)


def max_error(sigma2):
    """std::vector<size_t>::push_back(9.210 * sigmaSquare), read back as a float"""
    return (F64(9.210) * np.asarray(sigma2, F32).astype(F64)).astype(np.uint64).astype(F32)


def constructor(c):
    x1, x2 = _transform(c["Rcw1"], c["tcw1"], c["world1"]), _transform(c["Rcw2"], c["tcw2"], c["world2"])
    return dict(x3dc1=x1, x3dc2=x2, p1im1=_to_image(x1, c["K1"]), p2im2=_to_image(x2, c["K2"]), max_err1=max_error(c["sigma2_1"]), max_err2=max_error(c["sigma2_2"]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# ComputeSim3 (:309-448)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _centroid(P):
    s = (P[:, :, 0] + P[:, :, 1]) + P[:, :, 2]
    C = (s.astype(F64) / 3.0).astype(F32)
    return P - C[:, :, None], C


def model_inputs(x1, x2, sets):
    """-> Pr1, Pr2 (it,3,3) [it, row, point], O1, O2 (it,3), nmat (it,4,4), all float32"""
    sets = np.asarray(sets).reshape(-1, 3)
    P1, P2 = np.transpose(x1[sets], (0, 2, 1)), np.transpose(x2[sets], (0, 2, 1))
    Pr1, O1 = _centroid(P1)
    Pr2, O2 = _centroid(P2)
    M = np.zeros((len(sets), 3, 3), F32)
    for i in range(3):
        for j in range(3):
            M[:, i, j] = (Pr2[:, i, 0] * Pr1[:, j, 0] + Pr2[:, i, 1] * Pr1[:, j, 1]) + Pr2[:, i, 2] * Pr1[:, j, 2]
    m = lambda i, j: M[:, i, j]
    N11, N12, N13, N14 = (m(0, 0) + m(1, 1)) + m(2, 2), m(1, 2) - m(2, 1), m(2, 0) - m(0, 2), m(0, 1) - m(1, 0)
    N22, N23, N24 = (m(0, 0) - m(1, 1)) - m(2, 2), m(0, 1) + m(1, 0), m(2, 0) + m(0, 2)
    N33, N34, N44 = (-m(0, 0) + m(1, 1)) - m(2, 2), m(1, 2) + m(2, 1), (-m(0, 0) - m(1, 1)) + m(2, 2)
    N = np.stack([N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44], 1).astype(F32).reshape(-1, 4, 4)
    return Pr1, Pr2, O1, O2, N


def jacobi_eig4(N, sweeps=SWEEPS):
    """jacobi_eig4 of csrc/orbx_sim3.hip operation by operation: cyclic two-sided Jacobi in float64 on the float32 N (it,4,4); the column of V under
    the largest diagonal entry (the first of equal ones), narrowed to float32"""
    a = np.asarray(N, F32).astype(F64).copy()
    v = np.broadcast_to(np.eye(4), a.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(3):
                for q in range(p + 1, 4):
                    alpha, beta, gamma = a[:, p, p], a[:, q, q], a[:, p, q]
                    nz = gamma != 0.0
                    zeta = (beta - alpha) / (2.0 * gamma)
                    t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    cr = 1.0 / np.sqrt(1.0 + t * t)
                    c, s = np.where(nz, cr, 1.0)[:, None], np.where(nz, cr * t, 0.0)[:, None]
                    ap, aq, vp, vq = a[:, :, p].copy(), a[:, :, q].copy(), v[:, :, p].copy(), v[:, :, q].copy()
                    a[:, :, p], a[:, :, q] = c * ap - s * aq, s * ap + c * aq
                    v[:, :, p], v[:, :, q] = c * vp - s * vq, s * vp + c * vq
                    ap, aq = a[:, p, :].copy(), a[:, q, :].copy()
                    a[:, p, :], a[:, q, :] = c * ap - s * aq, s * ap + c * aq
    best, e = a[:, 0, 0].copy(), v[:, :, 0].copy()
    for k in range(1, 4):
        take = a[:, k, k] > best
        best = np.where(take, a[:, k, k], best)
        e = np.where(take[:, None], v[:, :, k], e)
    return e.astype(F32)


def eigh_quat(N):
    """float64: the eigenvector of the largest eigenvalue of the float32 N by numpy.linalg.eigh, and the relative gap (l1 - l2) / |l1| to the next"""
    w, V = np.linalg.eigh(np.asarray(N, F32).astype(F64))
    with np.errstate(all="ignore"):
        gap = (w[:, 3] - w[:, 2]) / np.abs(w[:, 3])
    return V[:, :, 3], np.where(np.isfinite(gap), gap, 0.0)


def rodrigues(vec):
    """cv::Rodrigues, vector -> matrix, in float64: (it,3) -> (it,3,3)"""
    r = np.asarray(vec).astype(F64)
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    theta = np.sqrt((rx * rx + ry * ry) + rz * rz)
    with np.errstate(all="ignore"):
        c, s = np.cos(theta), np.sin(theta)
        c1, it = 1.0 - c, 1.0 / theta
        rx, ry, rz = rx * it, ry * it, rz * it
        z = np.zeros_like(rx)
        rrt = np.stack([rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz], 1)
        rxm = np.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], 1)
        eye = np.eye(3).reshape(1, 9)
        R = (c[:, None] * eye + c1[:, None] * rrt) + s[:, None] * rxm
    R = np.where((theta < np.finfo(F64).eps)[:, None], eye, R)
    return R.reshape(-1, 3, 3)


def rotation_from_quat(q):
    """:372-386 in float64 on the float32 quaternion -> R (it,3,3) float64 (the caller narrows)"""
    q = np.asarray(q, F32).astype(F64)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        ang = np.arctan2(nrm, q[:, 0])
        scale = (2.0 * ang) / nrm
        vec = (scale[:, None] * q[:, 1:]).astype(F32)
    return rodrigues(vec)


def model_from_rotation(R, Pr1, Pr2, O1, O2, fix_scale):
    """:390-447 in float32 from the float32 R -> s12 (it), t12 (it,3), t12m, t21m (it,4,4)"""
    R = np.asarray(R, F32)
    n = len(R)
    with np.errstate(all="ignore"):
        P3 = np.zeros((n, 3, 3), F32)
        for i in range(3):
            for j in range(3):
                P3[:, i, j] = (R[:, i, 0] * Pr2[:, 0, j] + R[:, i, 1] * Pr2[:, 1, j]) + R[:, i, 2] * Pr2[:, 2, j]
        if fix_scale:
            s = np.ones(n, F32)
        else:
            nom, den = np.zeros(n, F64), np.zeros(n, F64)
            for i in range(3):
                for j in range(3):
                    nom = nom + Pr1[:, i, j].astype(F64) * P3[:, i, j].astype(F64)
                    den = den + (P3[:, i, j] * P3[:, i, j]).astype(F64)
            s = (nom / den).astype(F32)
        sR = s[:, None, None] * R
        inv = 1.0 / s.astype(F64)
        sRinv = (inv[:, None, None] * np.transpose(R, (0, 2, 1)).astype(F64)).astype(F32)
        t = np.stack([O1[:, i] - ((sR[:, i, 0] * O2[:, 0] + sR[:, i, 1] * O2[:, 1]) + sR[:, i, 2] * O2[:, 2]) for i in range(3)], 1)
        ns = -sRinv
        tinv = np.stack([(ns[:, i, 0] * t[:, 0] + ns[:, i, 1] * t[:, 1]) + ns[:, i, 2] * t[:, 2] for i in range(3)], 1)
    T12, T21 = np.zeros((n, 4, 4), F32), np.zeros((n, 4, 4), F32)
    T12[:, :3, :3], T12[:, :3, 3], T12[:, 3, 3] = sR, t, 1
    T21[:, :3, :3], T21[:, :3, 3], T21[:, 3, 3] = sRinv, tinv, 1
    return s, t, T12, T21


def compute_sim3(x1, x2, sets, fix_scale, sweeps=SWEEPS):
    """the float32 form, all stages chained"""
    Pr1, Pr2, O1, O2, N = model_inputs(x1, x2, sets)
    q = jacobi_eig4(N, sweeps)
    R = rotation_from_quat(q).astype(F32)
    s, t, T12, T21 = model_from_rotation(R, Pr1, Pr2, O1, O2, fix_scale)
    return dict(nmat=N, quat=q, r12=R, s12=s, t12=t, t12m=T12, t21m=T21)


def compute_sim3_f64(x1, x2, sets, fix_scale):
    """the float64 form: the same formulas in float64 on the float32 camera points, the eigenvector from numpy.linalg.eigh -> r12, t12, s12, t12m,
    t21m (float64) and the relative eigenvalue gap of every set"""
    sets = np.asarray(sets).reshape(-1, 3)
    P1, P2 = np.transpose(x1[sets], (0, 2, 1)).astype(F64), np.transpose(x2[sets], (0, 2, 1)).astype(F64)
    O1, O2 = P1.sum(2) / 3.0, P2.sum(2) / 3.0
    Pr1, Pr2 = P1 - O1[:, :, None], P2 - O2[:, :, None]
    M = Pr2 @ np.transpose(Pr1, (0, 2, 1))
    m = lambda i, j: M[:, i, j]
    N = np.stack([m(0, 0) + m(1, 1) + m(2, 2), m(1, 2) - m(2, 1), m(2, 0) - m(0, 2), m(0, 1) - m(1, 0),
                  m(1, 2) - m(2, 1), m(0, 0) - m(1, 1) - m(2, 2), m(0, 1) + m(1, 0), m(2, 0) + m(0, 2),
                  m(2, 0) - m(0, 2), m(0, 1) + m(1, 0), -m(0, 0) + m(1, 1) - m(2, 2), m(1, 2) + m(2, 1),
                  m(0, 1) - m(1, 0), m(2, 0) + m(0, 2), m(1, 2) + m(2, 1), -m(0, 0) - m(1, 1) + m(2, 2)], 1).reshape(-1, 4, 4)
    w, V = np.linalg.eigh(N)
    q = V[:, :, 3]
    with np.errstate(all="ignore"):
        gap = (w[:, 3] - w[:, 2]) / np.abs(w[:, 3])
        nrm = np.linalg.norm(q[:, 1:], axis=1)
        ang = np.arctan2(nrm, q[:, 0])
        R = rodrigues((2.0 * ang / nrm)[:, None] * q[:, 1:])
        P3 = R @ Pr2
        s = np.ones(len(sets)) if fix_scale else (Pr1 * P3).sum((1, 2)) / (P3 * P3).sum((1, 2))
        t = O1 - s[:, None] * (R @ O2[:, :, None])[:, :, 0]
        T12, T21 = np.zeros((len(sets), 4, 4)), np.zeros((len(sets), 4, 4))
        T12[:, :3, :3], T12[:, :3, 3], T12[:, 3, 3] = s[:, None, None] * R, t, 1
        sRinv = np.transpose(R, (0, 2, 1)) / s[:, None, None]
        T21[:, :3, :3], T21[:, :3, 3], T21[:, 3, 3] = sRinv, -(sRinv @ t[:, :, None])[:, :, 0], 1
    return dict(r12=R, t12=t, s12=s, t12m=T12, t21m=T21, gap=np.where(np.isfinite(gap), gap, 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# CheckInliers / Project (:451-523)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _project(T, X, K):
    T = np.asarray(T, F32).reshape(-1, 4, 4)
    fx, fy, cx, cy = [F32(v) for v in K]
    x, y, z = X[None, :, 0], X[None, :, 1], X[None, :, 2]
    with np.errstate(all="ignore"):
        P = [((T[:, r, 0, None] * x + T[:, r, 1, None] * y) + T[:, r, 2, None] * z) + T[:, r, 3, None] for r in range(3)]
        invz = F32(1) / P[2]
        return fx * (P[0] * invz) + cx, fy * (P[1] * invz) + cy


def check_inliers(con, K1, K2, T12, T21):
    """con: the constructor's arrays (or the device's) -> count (m) int32, inliers (m,n) bool"""
    u21, v21 = _project(T12, con["x3dc2"], K1)
    u12, v12 = _project(T21, con["x3dc1"], K2)
    with np.errstate(all="ignore"):
        d1x, d1y = con["p1im1"][None, :, 0] - u21, con["p1im1"][None, :, 1] - v21
        d2x, d2y = u12 - con["p2im2"][None, :, 0], v12 - con["p2im2"][None, :, 1]
        e1 = (d1x.astype(F64) * d1x.astype(F64) + d1y.astype(F64) * d1y.astype(F64)).astype(F32)
        e2 = (d2x.astype(F64) * d2x.astype(F64) + d2y.astype(F64) * d2y.astype(F64)).astype(F32)
        inl = (e1 < con["max_err1"][None, :]) & (e2 < con["max_err2"][None, :])
    return inl.sum(1).astype(np.int32), inl


# ---------------------------------------------------------------------------------------------------------------------------------------
# SetRansacParameters (:143-196), iterate (:199-285), the loop of LoopClosing::ComputeSim3 (src/LoopClosing.cc:403-482)
# ---------------------------------------------------------------------------------------------------------------------------------------
def ransac_iterations(prob, min_inliers, max_iterations, n):
    if min_inliers == n:
        k = 1
    else:
        eps = float(F32(min_inliers) / F32(n))
        k = int(math.ceil(math.log(1 - prob) / math.log(1 - math.pow(eps, 3))))
    return max(1, min(k, max_iterations))


def sets_example():
    """a scripted randint and what the draw, overwrite-with-back, pop scheme (:228-249) makes of it for n = 6"""
    script = [0, 0, 0, 5, 4, 3, 2, 2, 1]
    # [0..5]: draw slot 0 -> 0, list [5,1,2,3,4]; slot 0 -> 5, list [4,1,2,3]; slot 0 -> 4
    # draw slot 5 -> 5, list [0,1,2,3,4]; slot 4 -> 4, list [0,1,2,3]; slot 3 -> 3
    # draw slot 2 -> 2, list [0,1,5,3,4]; slot 2 -> 5, list [0,1,4,3]; slot 1 -> 1
    return script, [[0, 5, 4], [5, 4, 3], [2, 5, 1]]


def scan_events(count, min_inliers):
    """a straight loop over all iterations -> is_event (it) bool, first_event, best_iteration"""
    best, best_it, first, ev = 0, -1, -1, []
    for it, c in enumerate(count):
        e = False
        if c >= best:
            best, best_it = int(c), it
            e = c > min_inliers
        ev.append(bool(e))
        if e and first < 0:
            first = it
    return np.array(ev, bool), first, best_it


class Solver:
    """iterate / find / the getters of the reference, as a state machine over per-iteration outputs (count, inliers (it,n), r12, t12, s12)"""

    def __init__(self, count, inliers, r12, t12, s12, n, min_inliers, indices1=None, mN1=None):
        self.count, self.inliers, self.r12, self.t12, self.s12 = count, inliers, r12, t12, s12
        self.n, self.min_inliers, self.max_its = n, min_inliers, len(count)
        self.indices1 = np.arange(n) if indices1 is None else np.asarray(indices1)
        self.mN1 = n if mN1 is None else mN1
        self.mnIterations, self.mnBestInliers, self.best = 0, 0, -1

    def T12(self, it):
        T = np.eye(4, dtype=F32)
        T[:3, :3] = F32(self.s12[it]) * np.asarray(self.r12[it], F32)
        T[:3, 3] = self.t12[it]
        return T

    def iterate(self, nIterations):
        vb = np.zeros(self.mN1, bool)
        if self.n < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.mnIterations < self.max_its and cur < nIterations:
            cur += 1
            it = self.mnIterations
            self.mnIterations += 1
            if self.count[it] >= self.mnBestInliers:
                self.mnBestInliers, self.best = int(self.count[it]), it
                if self.count[it] > self.min_inliers:
                    vb[self.indices1[np.asarray(self.inliers[it], bool)]] = True
                    return self.T12(it), False, vb, int(self.count[it])
        return None, self.mnIterations >= self.max_its, vb, 0

    def GetEstimatedRotation(self):
        return self.r12[self.best]

    def GetEstimatedTranslation(self):
        return self.t12[self.best]

    def GetEstimatedScale(self):
        return self.s12[self.best]


def round_robin(solvers, accept, per_visit=5, max_visits=10000):
    """LoopClosing.cc:403-482 up to the point where Scm is non-empty: candidates in turn, `per_visit` iterations each, a candidate is discarded on
    bNoMore, the loop ends when accept(candidate, nInliers) says so (the place of SearchBySim3 / OptimizeSim3 >= 20) or nobody is left.
    -> [(candidate, bNoMore, nInliers, inlier indices, T12 bits or None, (R, t, s) bits or None)]"""
    discarded, left, match, log = [False] * len(solvers), len(solvers), False, []
    while left > 0 and not match and len(log) < max_visits:
        for i, S in enumerate(solvers):
            if discarded[i]:
                continue
            T, no_more, vb, k = S.iterate(per_visit)
            if no_more:
                discarded[i] = True
                left -= 1
            est = None
            if T is not None:
                est = (np.asarray(S.GetEstimatedRotation(), F32).tobytes(), np.asarray(S.GetEstimatedTranslation(), F32).tobytes(), F32(S.GetEstimatedScale()).tobytes())
            log.append((i, bool(no_more), int(k), tuple(np.flatnonzero(vb).tolist()), None if T is None else np.asarray(T, F32).tobytes(), est))
            if T is not None and accept(i, k):
                match = True
                break
    return log


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    return rodrigues((axis * angle)[None])[0]


def scene(n, seed, angle=0.3, scale=1.7, noise=0.01, outliers=0.3, kind="general"):
    """Two maps of the same n points related by a similarity: map 2 = (map 1 expressed through S12^-1), each seen by its keyframe.
    X1c = s * R * X2c + t holds for the camera coordinates up to `noise` (position noise on map 2) except for the gross outliers.
    kind: "general"; "behind" moves a tenth of the points behind camera 2; "z0" puts world points of map 1 exactly on camera 1's z = 0 plane."""
    g = np.random.default_rng(seed)
    K1, K2 = (520.0, 525.0, 320.0, 240.0), (500.0, 505.0, 315.0, 245.0)
    Rcw1, tcw1 = _rot([0.2, 1.0, 0.1], 0.2), np.array([0.1, -0.2, 0.3])
    Rcw2, tcw2 = _rot([1.0, 0.3, -0.2], -0.15), np.array([-0.3, 0.1, 0.2])
    R12, t12 = _rot([0.3, -0.5, 0.8], angle), np.array([0.4, -0.1, 0.25])
    X1c = np.stack([g.uniform(-2, 2, n), g.uniform(-1.5, 1.5, n), g.uniform(3, 9, n)], 1)
    X2c = (X1c - t12) @ R12 / scale                      # R12^T (X1c - t) / s
    X2c = X2c + g.normal(0, noise, X2c.shape)
    nout = int(round(outliers * n))
    out = g.permutation(n)[:nout]
    X2c[out] = np.stack([g.uniform(-1, 1, nout), g.uniform(-1, 1, nout), g.uniform(2, 5, nout)], 1)
    if kind == "behind":
        X2c[g.permutation(n)[:max(1, n // 10)], 2] *= -1.0
    w1 = (X1c - tcw1) @ Rcw1                             # Rcw^T (Xc - tcw)
    w2 = (X2c - tcw2) @ Rcw2
    c = dict(Rcw1=Rcw1.astype(F32), tcw1=tcw1.astype(F32), Rcw2=Rcw2.astype(F32), tcw2=tcw2.astype(F32), K1=K1, K2=K2, world1=w1.astype(F32), world2=w2.astype(F32))
    if kind == "z0":
        # identity pose for keyframe 1 and world z = 0 exactly: the constructor's invz is 1 / 0
        c["Rcw1"], c["tcw1"] = np.eye(3, dtype=F32), np.zeros(3, F32)
        c["world1"] = X1c.astype(F32)
        c["world1"][:max(1, n // 16), 2] = 0.0
    # mvLevelSigma2 of scale factor 1.2: products with 9.210 have fractional parts (1.44 * 9.21 = 13.26 -> 13)
    lv = 1.2 ** (2 * g.integers(0, 8, (2, n)))
    c["sigma2_1"], c["sigma2_2"] = lv[0].astype(F32), lv[1].astype(F32)
    c["truth"] = dict(R=R12, t=t12, s=scale, outlier=np.isin(np.arange(n), out))
    # mvnIndices1: the kept pairs are every other slot of vpMatched12, and a few more slots behind
    c["indices1"], c["mN1"] = 2 * np.arange(n) + 1, 2 * n + 3
    return c


def draw_sets(n, iterations, seed):
    g = np.random.default_rng(seed)
    out = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(3):
            r = int(g.integers(0, len(avail)))
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def solve(c, sets, min_inliers, fix_scale, form="f32"):
    """the whole restated chain on a scene -> dict with the per-iteration arrays and the events"""
    con = constructor(c)
    n = len(con["x3dc1"])
    sets = np.asarray(sets, np.int32).reshape(-1, 3)
    if n < min_inliers:
        sets = sets[:0]
    if form == "f32":
        m = compute_sim3(con["x3dc1"], con["x3dc2"], sets, fix_scale)
    else:
        m = compute_sim3_f64(con["x3dc1"], con["x3dc2"], sets, fix_scale)
    count, inl = check_inliers(con, c["K1"], c["K2"], np.asarray(m["t12m"], F32), np.asarray(m["t21m"], F32)) if len(sets) else (np.zeros(0, np.int32), np.zeros((0, n), bool))
    ev, first, best = scan_events(count, min_inliers)
    m.update(con)
    m.update(count=count, inliers=inl, is_event=ev, first_event=first, best_iteration=best, no_more=bool(n < min_inliers or first < 0), sets=sets)
    return m


def similarity_error(R, t, s, truth):
    """(rotation angle in degrees, |t - t_true|, |s / s_true - 1|)"""
    dR = np.asarray(R, F64) @ truth["R"].T
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1.0) / 2.0))))
    return ang, float(np.linalg.norm(np.asarray(t, F64) - truth["t"])), abs(float(s) / truth["s"] - 1.0)
