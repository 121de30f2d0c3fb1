"""Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1364-1590 with the vendored g2o) restated in numpy float64, operation by operation in
the order csrc/orbx_optimize_sim3.hip computes: the exponential, product, inverse, map and log of g2o/types/sim3.h, the two projection edges
of types_seven_dof_expmap.h, g2o's central differences (base_binary_edge.hpp:147-200), the Huber quadratic form, the Levenberg driver
(optimization_algorithm_levenberg.cpp:61-164), the two rounds and the tests on the errors as the last trial left them.

A Sim3 is (q, t, s): q = [x, y, z, w] like Eigen's coeffs(), python floats.  Everything per pair is vectorised over the pairs; an elementwise numpy
operation rounds like the scalar one, so the per-pair values are those of a scalar loop.  Sums over the edges are taken in the order of the
device's block sums (block_sum; g2o's loop over the edges has another order, and so has every host build of it that vectorises)."""
import math

import numpy as np

DELTA = 1e-9
SCALAR = 1.0 / (2.0 * DELTA)
EPS = 0.00001
DBL_MAX = float(np.finfo(np.float64).max)


def cam_points(R, t, Xw):
    """P3Dc = R * P3Dw + t in FLOAT, (R[0]*x + R[1]*y) + R[2]*z, then + t: the arithmetic of k_sim3_prepare"""
    R, t, X = np.asarray(R, np.float32).reshape(3, 3), np.asarray(t, np.float32).reshape(3), np.asarray(Xw, np.float32).reshape(-1, 3)
    out = np.zeros_like(X)
    for r in range(3):
        out[:, r] = ((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r]
    return out


def quat_from_R(R):
    """Eigen::Quaterniond(Matrix3d)"""
    R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    q = [0.0] * 4
    t = (R[0] + R[4]) + R[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
        return q
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    m = lambda a, b: R[3 * a + b]      # noqa: E731
    t = math.sqrt(((m(i, i) - m(j, j)) - m(k, k)) + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m(k, j) - m(j, k)) * t
    q[j] = (m(j, i) + m(i, j)) * t
    q[k] = (m(k, i) + m(i, k)) * t
    return q


def quat_to_R(q):
    """Quaterniond::toRotationMatrix"""
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def rotate(q, v):
    """Quaterniond * Vector3d; v = three scalars or three arrays"""
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    return [(v[0] + q[3] * uv[0]) + (q[1] * uv[2] - q[2] * uv[1]),
            (v[1] + q[3] * uv[1]) + (q[2] * uv[0] - q[0] * uv[2]),
            (v[2] + q[3] * uv[2]) + (q[0] * uv[1] - q[1] * uv[0])]


def sim3_map(S, v):
    q, t, s = S
    r = rotate(q, v)
    return [s * r[0] + t[0], s * r[1] + t[1], s * r[2] + t[2]]


def sim3_mul(a, b):
    p, r = a[0], b[0]
    q = [((p[3] * r[0] + p[0] * r[3]) + p[1] * r[2]) - p[2] * r[1],
         ((p[3] * r[1] + p[1] * r[3]) + p[2] * r[0]) - p[0] * r[2],
         ((p[3] * r[2] + p[2] * r[3]) + p[0] * r[1]) - p[1] * r[0],
         ((p[3] * r[3] - p[0] * r[0]) - p[1] * r[1]) - p[2] * r[2]]
    rt = rotate(p, b[1])
    return (q, [a[2] * rt[0] + a[1][0], a[2] * rt[1] + a[1][1], a[2] * rt[2] + a[1][2]], a[2] * b[2])


def sim3_inverse(a):
    q, t, s = a
    qc = [-q[0], -q[1], -q[2], q[3]]
    f = -1.0 / s
    return (qc, rotate(qc, [f * t[0], f * t[1], f * t[2]]), 1.0 / s)


def _skew(w):
    return [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]


def _mat3(a, b):
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


_I3 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def sim3_exp(u):
    """Sim3(const Vector7d &), sim3.h:70-142; -> (S, branch) with branch = (|sigma| < eps, theta < eps)"""
    u = [float(v) for v in u]
    w, sigma = u[0:3], u[6]
    theta = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    Om = _skew(w)
    Om2 = _mat3(Om, Om)
    s = math.exp(sigma)
    small = theta < EPS
    if small:
        R = [(_I3[k] + Om[k]) + Om2[k] for k in range(9)]
    else:
        ca, cb = math.sin(theta) / theta, (1.0 - math.cos(theta)) / (theta * theta)
        R = [(_I3[k] + ca * Om[k]) + cb * Om2[k] for k in range(9)]
    if abs(sigma) < EPS:
        C = 1.0
        if small:
            A, B = 1.0 / 2.0, 1.0 / 6.0
        else:
            theta2 = theta * theta
            A = (1.0 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1.0) / sigma
        sigma2 = sigma * sigma
        if small:
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
        else:
            a, b, theta2 = s * math.sin(theta), s * math.cos(theta), theta * theta
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2
    W = [(A * Om[k] + B * Om2[k]) + C * _I3[k] for k in range(9)]
    t = [(W[3 * i] * u[3] + W[3 * i + 1] * u[4]) + W[3 * i + 2] * u[5] for i in range(3)]
    return (quat_from_R(R), t, s), (abs(sigma) < EPS, small)


def sim3_log(S):
    """Sim3::log(), sim3.h:148-230; -> (Vector7d, branch) with branch = (|sigma| < eps, d > 1 - eps)"""
    q, t, s = S
    sigma = math.log(s)
    R = quat_to_R(q)
    d = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    near = d > 1 - EPS
    if abs(sigma) < EPS:
        C = 1.0
        if near:
            omega = 0.5 * dR
            A, B = 1.0 / 2.0, 1.0 / 6.0
        else:
            theta = math.acos(d)
            theta2 = theta * theta
            omega = theta / (2 * math.sqrt(1 - d * d)) * dR
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        if near:
            sigma2 = sigma * sigma
            omega = 0.5 * dR
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        else:
            theta = math.acos(d)
            omega = theta / (2 * math.sqrt(1 - d * d)) * dR
            theta2 = theta * theta
            a, b = s * math.sin(theta), s * math.cos(theta)
            c = theta2 + sigma * sigma
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
    Om = np.array(_skew(omega)).reshape(3, 3)
    W = A * Om + B * Om @ Om + C * np.eye(3)
    ups = np.linalg.solve(W, np.asarray(t, np.float64))
    return np.concatenate([omega, ups, [sigma]]), (abs(sigma) < EPS, near)


def sim3_from_Rts(R, t, s):
    """g2o::Sim3(Quaterniond(R), t, s)"""
    return (quat_from_R(R), [float(v) for v in np.asarray(t, np.float64).reshape(3)], float(s))


def edge_error(S, X, obs, K):
    """obs - cam_map(project(S.map(X))) over the pairs: X (n,3), obs (n,2) float64, K = (fx, fy, cx, cy) -> (n,2)"""
    p = sim3_map(S, [X[:, 0], X[:, 1], X[:, 2]])
    with np.errstate(all="ignore"):
        return np.stack([obs[:, 0] - ((p[0] / p[2]) * K[0] + K[2]), obs[:, 1] - ((p[1] / p[2]) * K[1] + K[3])], 1)


def chi2_of(e, w):
    return w * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])


def huber(delta, e2):
    """RobustKernelHuber::robustify -> rho[0], rho[1]"""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(e2)
        inside = e2 <= dsqr
        return np.where(inside, e2, (2.0 * sq) * delta - dsqr), np.where(inside, 1.0, delta / sq)


_LANE = np.arange(64)
_BUTTERFLY = (_LANE ^ 1, _LANE ^ 2, (_LANE & ~7) | (7 - (_LANE & 7)), (_LANE & ~15) | (15 - (_LANE & 15)))


def block_sum(terms, act):
    """Sum over the edges in the device's fixed order.  terms (n, 2, ...): per pair the e12 and the e21 term; act (n) bool.  Thread t of 256 adds the
    terms of its pairs t, t + 256, ... (e12, then e21) to 0; a wave adds neighbouring lanes, pairs of lanes, the mirrored half row of 8 and the
    mirrored row of 16 (DPP butterflies), then its four rows as (r0 + r1) + (r2 + r3); the four waves add up as (w0 + w1) + (w2 + w3)."""
    terms = np.asarray(terms, np.float64)
    n = terms.shape[0]
    T = np.zeros((256,) + terms.shape[2:])
    for j in range((n + 255) // 256):
        idx = np.arange(256 * j, min(n, 256 * j + 256))
        on = act[idx]
        for e in range(2):
            T[idx[on] - 256 * j] = T[idx[on] - 256 * j] + terms[idx[on], e]
    v = T.reshape((4, 64) + terms.shape[2:])
    for perm in _BUTTERFLY:
        v = v + v[:, perm]
    w = (v[:, 0] + v[:, 16]) + (v[:, 32] + v[:, 48])
    return (w[0] + w[1]) + (w[2] + w[3])


class Problem:
    """The per-pair data of a problem dict (the keys of Sim3Optimizer._problem): float inputs, widened where the reference widens them.
    x3dc1 / x3dc2 may be replaced (the device's own, or perturbed ones)."""

    def __init__(self, p, th2=10.0, fix_scale=False, x3dc1=None, x3dc2=None):
        f4, f8 = np.float32, np.float64
        self.x3dc1 = cam_points(p["Rcw1"], p["tcw1"], p["world1"]) if x3dc1 is None else np.asarray(x3dc1)
        self.x3dc2 = cam_points(p["Rcw2"], p["tcw2"], p["world2"]) if x3dc2 is None else np.asarray(x3dc2)
        self.X1, self.X2 = self.x3dc1.astype(f8).reshape(-1, 3), self.x3dc2.astype(f8).reshape(-1, 3)
        self.o1, self.o2 = np.asarray(p["obs1"], f4).reshape(-1, 2).astype(f8), np.asarray(p["obs2"], f4).reshape(-1, 2).astype(f8)
        self.w1, self.w2 = np.asarray(p["inv_sigma2_1"], f4).reshape(-1).astype(f8), np.asarray(p["inv_sigma2_2"], f4).reshape(-1).astype(f8)
        self.K1, self.K2 = [float(f4(v)) for v in p["K1"]], [float(f4(v)) for v in p["K2"]]
        self.n = len(self.X1)
        self.th2 = float(f4(th2))
        self.delta = float(np.sqrt(f4(th2)))      # sqrt(th2) as a float root, widened
        self.fix_scale = bool(fix_scale)
        self.S0 = sim3_from_Rts(p["R12"], p["t12"], p["s12"])


def errors_at(P, S):
    return edge_error(S, P.X2, P.o1, P.K1), edge_error(sim3_inverse(S), P.X1, P.o2, P.K2)


def oplus(S, u, fix_scale):
    u = [float(v) for v in u]
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u)[0], S)


def linearize(P, S, active=None):
    """One linearisation at S -> dict(errors (2n,2), chi2 (2n), jac (2n,2,7), H (7,7), b (7), chi (robust)); edge 2 i = e12, 2 i + 1 = e21;
    zeros for the pairs outside `active`"""
    n = P.n
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    e12, e21 = errors_at(P, S)
    J = np.zeros((n, 2, 2, 7))
    for d in range(7):
        u = [0.0] * 7
        u[d] = DELTA
        Sp = oplus(S, u, P.fix_scale)
        u[d] = -DELTA
        Sm = oplus(S, u, P.fix_scale)
        J[:, 0, :, d] = SCALAR * (edge_error(Sp, P.X2, P.o1, P.K1) - edge_error(Sm, P.X2, P.o1, P.K1))
        J[:, 1, :, d] = SCALAR * (edge_error(sim3_inverse(Sp), P.X1, P.o2, P.K2) - edge_error(sim3_inverse(Sm), P.X1, P.o2, P.K2))
    E = np.stack([e12, e21], 1)                      # (n, 2 edges, 2 rows)
    w = np.stack([P.w1, P.w2], 1)                    # (n, 2)
    chi = w * (E[..., 0] * E[..., 0] + E[..., 1] * E[..., 1])
    rho0, rho1 = huber(P.delta, chi)
    a = act[:, None]
    E, chi, J = np.where(a[..., None], E, 0.0), np.where(a, chi, 0.0), np.where(a[..., None, None], J, 0.0)
    rho0, rho1 = np.where(a, rho0, 0.0), np.where(a, rho1, 0.0)
    W = rho1 * w
    c0, c1 = (-(w * E[..., 0])) * rho1, (-(w * E[..., 1])) * rho1
    J0, J1 = J[:, :, 0, :], J[:, :, 1, :]            # (n, 2, 7)
    WJ0, WJ1 = W[..., None] * J0, W[..., None] * J1
    Ht = J0[..., :, None] * WJ0[..., None, :] + J1[..., :, None] * WJ1[..., None, :]      # J0[i] * (W * J0[j]) + J1[i] * (W * J1[j])
    bt = J0 * c0[..., None] + J1 * c1[..., None]
    H, b = block_sum(Ht, act), block_sum(bt, act)
    H = np.triu(H) + np.triu(H, 1).T                 # the device sums the upper triangle
    return dict(errors=E.reshape(2 * n, 2), chi2=chi.reshape(2 * n), jac=J.reshape(2 * n, 2, 7), H=H, b=b, chi=float(block_sum(rho0, act)))


def ldlt_solve(H, b, lam):
    """(H + lam I) x = b by LDL^T without pivoting -> (ok, x); not ok on a non-positive or non-finite factor"""
    A = [[float(H[i, j]) for j in range(7)] for i in range(7)]
    for i in range(7):
        A[i][i] += lam
    Dg, ok = [0.0] * 7, True
    with np.errstate(all="ignore"):
        for j in range(7):
            LD = [0.0] * 7
            dj = np.float64(A[j][j])
            for k in range(j):
                LD[k] = A[j][k] * Dg[k]
                dj = dj - A[j][k] * LD[k]
            ok = ok and bool(dj > 0.0) and bool(np.isfinite(dj))
            Dg[j] = dj
            for i in range(j + 1, 7):
                lij = np.float64(A[i][j])
                for k in range(j):
                    lij = lij - A[i][k] * LD[k]
                A[i][j] = lij / dj
        x = [0.0] * 7
        for i in range(7):
            s = np.float64(b[i])
            for k in range(i):
                s = s - A[i][k] * x[k]
            x[i] = s
        for i in range(7):
            x[i] = x[i] / Dg[i]
        for i in range(6, -1, -1):
            s = x[i]
            for k in range(i + 1, 7):
                s = s - A[k][i] * x[k]
            x[i] = s
    return ok, [float(v) for v in x]


def robust_chi(P, e12, e21, act):
    r12, _ = huber(P.delta, chi2_of(e12, P.w1))
    r21, _ = huber(P.delta, chi2_of(e21, P.w2))
    return float(block_sum(np.stack([r12, r21], 1), act))


def optimize(P, S, act, err, iterations):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg over the active pairs.  err = [e12, e21] (n,2) each: _error of the
    edges, updated in place for the active pairs by every error pass -> (S, Levenberg iterations run, final robust chi2, why it ended: "iterations",
    "trials" (10 trials), "rho0" (rho == 0) or "three" (three iterations without progress))"""
    if not act.any():
        return S, 0, 0.0, "iterations"
    x = [0.0] * 7
    lam = ni = 0.0
    n_bad = 0
    done, cur, why = 0, 0.0, "iterations"
    am = act[:, None]
    for it in range(iterations):
        lin = linearize(P, S, act)
        E = lin["errors"].reshape(P.n, 2, 2)
        err[0][:], err[1][:] = np.where(am, E[:, 0], err[0]), np.where(am, E[:, 1], err[1])
        cur = ini = lin["chi"]
        H, b = lin["H"], lin["b"]
        if it == 0:
            lam, ni, n_bad = 1e-5 * max(0.0, max(abs(float(H[q, q])) for q in range(7))), 2.0, 0
        qmax, stop = 0, False
        while True:
            save = S
            ok, xx = ldlt_solve(H, b, lam)
            if ok:
                x = xx
            if P.fix_scale:
                x[6] = 0.0
            S = oplus(S, x, P.fix_scale)
            e12, e21 = errors_at(P, S)
            err[0][:], err[1][:] = np.where(am, e12, err[0]), np.where(am, e21, err[1])
            temp = robust_chi(P, e12, e21, act)
            if not ok:
                temp = DBL_MAX
            scale = 0.0
            for j in range(7):
                scale = scale + x[j] * (lam * x[j] + float(b[j]))
            scale = scale + 1e-3
            with np.errstate(all="ignore"):
                rho = float((np.float64(cur) - np.float64(temp)) / np.float64(scale))
            if rho > 0.0 and math.isfinite(temp):
                t2r = 2.0 * rho - 1.0
                alpha = min(1.0 - (t2r * t2r) * t2r, 2.0 / 3.0)
                lam = lam * max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = temp
            else:
                lam = lam * ni
                ni = ni * 2.0
                S = save
            qmax += 1
            if not (rho < 0.0 and qmax < 10):
                break
        done += 1
        if qmax == 10 or rho == 0.0:
            stop, why = True, ("trials" if qmax == 10 else "rho0")
        else:
            n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
            stop = n_bad >= 3
            why = "three" if stop else why
        if stop:
            break
    return S, done, cur, why


def optimize_sim3(P):
    """-> dict(n_inliers, S (q, t, s), removed_first, removed_final, n_bad, chi2_round1 / chi2_round2 (n,2), -1 = not in the graph, stats (2,2),
    returned_zero, why = how each round's optimize() ended)"""
    n = P.n
    act = np.ones(n, bool)
    err = [np.zeros((n, 2)), np.zeros((n, 2))]
    out = dict(removed_first=np.zeros(n, bool), removed_final=np.zeros(n, bool), chi2_round1=-np.ones((n, 2)), chi2_round2=-np.ones((n, 2)),
               stats=np.zeros((2, 2)), n_bad=0, n_inliers=0, S=P.S0, returned_zero=True, why=["", ""])
    if n == 0:
        return out
    S, it1, chi1, out["why"][0] = optimize(P, P.S0, act, err, 5)
    out["stats"][0] = (it1, chi1)
    c12, c21 = chi2_of(err[0], P.w1), chi2_of(err[1], P.w2)
    out["chi2_round1"] = np.stack([c12, c21], 1)
    bad = (c12 > P.th2) | (c21 > P.th2)
    out["removed_first"], out["n_bad"] = bad, int(bad.sum())
    act = act & ~bad
    if n - out["n_bad"] < 10:
        return out
    S, it2, chi2, out["why"][1] = optimize(P, S, act, err, 10 if out["n_bad"] > 0 else 5)
    out["stats"][1] = (it2, chi2)
    c12, c21 = chi2_of(err[0], P.w1), chi2_of(err[1], P.w2)
    out["chi2_round2"] = np.where(act[:, None], np.stack([c12, c21], 1), -1.0)
    bad2 = act & ((c12 > P.th2) | (c21 > P.th2))
    out["removed_final"] = bad2
    out["n_inliers"] = int((act & ~bad2).sum())
    out["S"], out["returned_zero"] = S, False
    return out


def near_threshold(res, th2, rel=1e-6):
    """(n) bool: pairs one of whose tested chi2 values lies within a relative `rel` of th2"""
    c = np.concatenate([res["chi2_round1"], res["chi2_round2"]], 1)
    return (np.abs(c - th2) <= rel * th2).any(1)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def _rot(axis, ang):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def make_scene(n, seed, outliers=0.0, noise=0.5, fix_scale=False, k2=None, behind=0.0, start=1.0):
    """Two keyframes whose maps differ by a similarity: points X1 of map 1 in front of camera 1, the same points in map 2's frame X2 with
    X1c = s R X2c + t; observations with `noise` px of Gaussian noise, scaled by the octave's sigma; a share `outliers` of the pairs gets a wrong
    observation in image 2; a share `behind` of the pairs has its camera-2 point behind camera 2.  The initial estimate is the truth moved by `start`
    times (0.02 rad, 0.03 m, 2 % of scale).  -> problem dict (+ "truth" = (R, t, s), "outlier" (n) bool)"""
    g = np.random.default_rng(seed)
    f4 = np.float32
    K1 = (458.654, 457.296, 367.215, 248.375)
    K2 = K1 if k2 is None else k2
    s = 1.0 if fix_scale else float(g.uniform(0.7, 1.4))
    R12 = _rot(g.normal(size=3), float(g.uniform(0.05, 0.3)))
    t12 = g.normal(size=3) * 0.3
    Rc1, tc1 = _rot(g.normal(size=3), 0.4), g.normal(size=3)
    Rc2, tc2 = _rot(g.normal(size=3), 0.7), g.normal(size=3)
    X2c = np.stack([g.uniform(-1.5, 1.5, n), g.uniform(-1.0, 1.0, n), g.uniform(3.0, 8.0, n)], 1)
    nb = int(round(behind * n))
    if nb:
        X2c[g.choice(n, nb, replace=False), 2] *= -1.0
    X1c = s * X2c @ R12.T + t12
    w1 = (X1c - tc1) @ Rc1                      # Rc1^T (X1c - tc1)
    w2 = (X2c - tc2) @ Rc2
    oct1, oct2 = g.integers(0, 8, n), g.integers(0, 8, n)
    sig1, sig2 = 1.2 ** oct1, 1.2 ** oct2
    pr = lambda X, K: np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)      # noqa: E731
    obs1 = pr(X1c, K1) + g.normal(size=(n, 2)) * (noise * sig1)[:, None]
    obs2 = pr(X2c, K2) + g.normal(size=(n, 2)) * (noise * sig2)[:, None]
    out = np.zeros(n, bool)
    no = int(round(outliers * n))
    if no:
        out[g.choice(n, no, replace=False)] = True
        obs2[out] += g.uniform(15, 40, (no, 2)) * g.choice([-1.0, 1.0], (no, 2))
    dR = _rot(g.normal(size=3), 0.02 * start)
    Rs, ts, ss = dR @ R12, t12 + 0.03 * start * g.normal(size=3), (1.0 if fix_scale else s * (1.0 + 0.02 * start))
    return dict(Rcw1=Rc1.astype(f4), tcw1=tc1.astype(f4), Rcw2=Rc2.astype(f4), tcw2=tc2.astype(f4), K1=K1, K2=K2, world1=w1.astype(f4), world2=w2.astype(f4),
                obs1=obs1.astype(f4), obs2=obs2.astype(f4), inv_sigma2_1=(1.0 / sig1 ** 2).astype(f4), inv_sigma2_2=(1.0 / sig2 ** 2).astype(f4),
                R12=Rs.astype(f4).astype(np.float64), t12=ts.astype(f4).astype(np.float64), s12=float(f4(ss)), truth=(R12, t12, s), outlier=out)
