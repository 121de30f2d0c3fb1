"""numpy float64 restatement of PnPsolver (reference src/PnPsolver.cc), written from the algorithm with line references only.

Two linear-algebra back ends serve the places where the reference calls OpenCV (cvSVD, cvSolve(CV_SVD), cvInvert(CV_SVD)):
  "numpy"   numpy.linalg: what the stages of the device are judged against;
  "jacobi"  the device's own cyclic Jacobi iterations (csrc/orbx_pnp.hip) restated operation by operation: what the sweep counts
            were chosen with, and what test_jacobi_sweeps_settled runs.
Everything else - the sums in the reference's order, qr_solve, the mixed-precision CheckInliers, SetRansacParameters, the draw, Refine and
iterate - is restated literally and shared by both.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TINY, ORTH, RANK = 2.0 ** -60, 2.0 ** -49, 2.0 ** -104
SWEEPS12, SWEEPS_SMALL = 12, 8      # ORBX_PNP_JACOBI_SWEEPS, ORBX_PNP_SMALL_SWEEPS of include/orbx.h
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


# ---------------------------------------------------------------------------------------------------------------------------------------
# SetRansacParameters (:181-230), the draw (:274-290)
# ---------------------------------------------------------------------------------------------------------------------------------------
def ransac_parameters(prob=0.99, min_inliers=8, max_its=300, min_set=4, eps=0.4, n=0):
    """-> (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)"""
    eps = F32(eps)
    m = int(F32(n) * eps)      # int N * float: a float product, truncated
    m = max(m, min_inliers, min_set)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = F32(m) / F32(n)
    if eps < q:
        eps = q
    if m == n:
        its = 1
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.ceil(np.log(1 - F64(prob)) / np.log(1 - np.power(F64(eps), 3)))
        its = int(x) if np.isfinite(x) and -2 ** 31 <= x < 2 ** 31 else -2 ** 31      # what the x86 conversion makes of NaN / out of range
    return m, max(1, min(its, max_its)), eps


def draw_sets(n, iterations, randint, k=4):
    """`iterations` sets of k distinct indices: randint(0, len(available) - 1) (inclusive), the drawn slot overwritten with the back, the back popped"""
    out = np.zeros((iterations, k), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(k):
            r = int(randint(0, len(avail) - 1))
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def rng_sets(n, iterations, seed, k=4):
    g = np.random.default_rng(seed)
    return draw_sets(n, iterations, lambda lo, hi: g.integers(lo, hi + 1), k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the device's Jacobi iterations, operation by operation
# ---------------------------------------------------------------------------------------------------------------------------------------
def _cst(alpha, beta, gamma, small):
    if abs(gamma) <= small:
        return 1.0, 0.0, 0.0
    zeta = (beta - alpha) / (2.0 * gamma)
    t = math.copysign(1.0, zeta) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
    c = 1.0 / math.sqrt(1.0 + t * t)
    return c, c * t, t


def jacobi_eig(A, sweeps):
    """cyclic two-sided Jacobi on the symmetric matrix: off-diagonal entries of rows / columns p, q rotated, the diagonal moved by t * gamma, the
    rotated entry set to zero -> (diagonal, V with eigenvectors in its columns)"""
    A = np.array(A, F64)
    n = len(A)
    V = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            rotated = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    alpha, beta, gamma = float(A[p, p]), float(A[q, q]), float(A[p, q])
                    if gamma == 0.0:
                        continue      # already annihilated: the identity
                    c, s, t = _cst(alpha, beta, gamma, TINY * (abs(alpha) + abs(beta)))
                    rotated = rotated or t != 0.0
                    ap, aq = A[:, p].copy(), A[:, q].copy()
                    newp, newq = c * ap - s * aq, s * ap + c * aq
                    A[:, p] = newp
                    A[p, :] = newp
                    A[:, q] = newq
                    A[q, :] = newq
                    A[p, p] = alpha - t * gamma      # the classical diagonal update; the matrix stays exactly symmetric
                    A[q, q] = beta + t * gamma
                    A[p, q] = 0.0
                    A[q, p] = 0.0
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p] = c * vp - s * vq
                    V[:, q] = s * vp + c * vq
            if not rotated:
                break      # every off-diagonal entry is exactly zero: the later sweeps are identities
    return np.diag(A).copy(), V


def order_desc(d):
    """rank of every |d[k]| in descending order, the first of equal ones first"""
    a = np.abs(d)
    order = list(range(len(d)))
    for k in range(len(d)):
        rank = sum(1 for j in range(len(d)) if a[j] > a[k] or (a[j] == a[k] and j < k))
        order[rank] = k
    return order


def onesided_jacobi(a, sweeps):
    """Hestenes: a <- a V with orthogonal columns -> (a V, V)"""
    a = np.array(a, F64)
    m, k = a.shape
    v = np.eye(k)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(k - 1):
                for q in range(p + 1, k):
                    alpha = beta = gamma = 0.0
                    for i in range(m):
                        alpha = alpha + a[i, p] * a[i, p]
                        beta = beta + a[i, q] * a[i, q]
                        gamma = gamma + a[i, p] * a[i, q]
                    c, s, _ = _cst(float(alpha), float(beta), float(gamma), ORTH * math.sqrt(alpha * beta) if alpha * beta >= 0 else float("nan"))
                    ap, aq = a[:, p].copy(), a[:, q].copy()
                    a[:, p] = c * ap - s * aq
                    a[:, q] = s * ap + c * aq
                    vp, vq = v[:, p].copy(), v[:, q].copy()
                    v[:, p] = c * vp - s * vq
                    v[:, q] = s * vp + c * vq
    return a, v


def jacobi_ls(a, b, sweeps):
    """x = V Sigma^-2 (a V)^T b for the right-hand sides in the columns of b, negligible singular values dropped"""
    B, v = onesided_jacobi(a, sweeps)
    m, k = B.shape
    b = np.array(b, F64).reshape(m, -1)
    s2 = np.zeros(k)
    for j in range(k):
        s = 0.0
        for i in range(m):
            s = s + B[i, j] * B[i, j]
        s2[j] = s
    smax = 0.0
    for j in range(k):
        smax = s2[j] if s2[j] > smax else smax
    x = np.zeros((k, b.shape[1]))
    with np.errstate(all="ignore"):
        for nb in range(b.shape[1]):
            w = np.zeros(k)
            for j in range(k):
                s = 0.0
                for i in range(m):
                    s = s + B[i, j] * b[i, nb]
                w[j] = s / s2[j] if s2[j] > smax * RANK else 0.0
            for r in range(k):
                s = 0.0
                for j in range(k):
                    s = s + v[r, j] * w[j]
                x[r, nb] = s
    return x


class Backend:
    def __init__(self, kind="numpy", sweeps12=SWEEPS12, sweeps_small=SWEEPS_SMALL):
        self.kind, self.sweeps12, self.sweeps_small = kind, sweeps12, sweeps_small

    def svd_sym(self, A):
        """cvSVD(A, W, U, 0, CV_SVD_U_T) of a symmetric positive semidefinite A -> (W descending, Ut with the vectors in its rows)"""
        A = np.asarray(A, F64)
        if self.kind == "numpy":
            w, v = np.linalg.eigh(A)
            return np.abs(w[::-1]), v[:, ::-1].T.copy()
        d, V = jacobi_eig(A, self.sweeps12 if len(A) == 12 else self.sweeps_small)
        o = order_desc(d)
        return np.abs(d[o]), V[:, o].T.copy()

    def solve(self, A, b):
        """cvSolve(A, b, x, CV_SVD)"""
        if self.kind == "numpy":
            return np.linalg.lstsq(np.asarray(A, F64), np.asarray(b, F64), rcond=None)[0]
        return jacobi_ls(A, b, self.sweeps_small)[:, 0]

    def invert(self, A):
        """cvInvert(A, Ainv, CV_SVD)"""
        if self.kind == "numpy":
            return np.linalg.pinv(np.asarray(A, F64))
        return jacobi_ls(A, np.eye(len(A)), self.sweeps_small)

    def rotation(self, abt):
        """U V^T of cvSVD(ABt, D, U, V) (:864-869)"""
        if self.kind == "numpy":
            u, _, vt = np.linalg.svd(np.asarray(abt, F64))
            return u @ vt
        B, v = onesided_jacobi(abt, self.sweeps_small)
        U = np.zeros((3, 3))
        with np.errstate(all="ignore"):
            for k in range(3):
                sig = math.sqrt((B[0, k] * B[0, k] + B[1, k] * B[1, k]) + B[2, k] * B[2, k])
                U[:, k] = B[:, k] / sig
        R = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                R[i, j] = (U[i, 0] * v[j, 0] + U[i, 1] * v[j, 1]) + U[i, 2] * v[j, 2]
        return R


NUMPY, JACOBI = Backend("numpy"), Backend("jacobi")


# ---------------------------------------------------------------------------------------------------------------------------------------
# EPnP (:507-1385), stage by stage
# ---------------------------------------------------------------------------------------------------------------------------------------
def centroid(pws):
    s = np.zeros(3)
    for p in pws:
        s = s + p
    return s / float(len(pws))


def pw0tpw0(pws, c0):
    s = np.zeros((3, 3))
    for p in pws:
        d = p - c0
        s = s + d[:, None] * d[None, :]
    return s


def control_points(c0, dc, uct, m):
    """:555-561"""
    cws = np.zeros((4, 3))
    cws[0] = c0
    with np.errstate(invalid="ignore"):
        for i in range(1, 4):
            k = math.sqrt(dc[i - 1] / float(m)) if dc[i - 1] >= 0 else float("nan")
            cws[i] = c0 + k * uct[i - 1]
    return cws


def cc_matrix(cws):
    """:589-591"""
    return np.array([[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)], F64)


def alphas_of(cws, ci, pws):
    """:595-615; -> (m, 4)"""
    d = np.asarray(pws, F64) - cws[0]
    a = np.zeros((len(d), 4))
    for j in range(3):
        a[:, 1 + j] = (ci[j, 0] * d[:, 0] + ci[j, 1] * d[:, 1]) + ci[j, 2] * d[:, 2]
    a[:, 0] = ((1.0 - a[:, 1]) - a[:, 2]) - a[:, 3]
    return a


def mtm_of(alphas, us, K):
    """fill_M (:627-645) and M^T M (:707), the rows of a point added pair by pair in point order"""
    fu, fv, uc, vc = [float(v) for v in K]
    acc = np.zeros((12, 12))
    for a, (u, v) in zip(alphas, np.asarray(us, F64)):
        m1, m2 = np.zeros(12), np.zeros(12)
        for i in range(4):
            m1[3 * i], m1[3 * i + 2] = a[i] * fu, a[i] * (uc - u)
            m2[3 * i + 1], m2[3 * i + 2] = a[i] * fv, a[i] * (vc - v)
        acc = (acc + m1[:, None] * m1[None, :]) + m2[:, None] * m2[None, :]
    return acc


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def L_6x10(ut):
    """:1042-1101"""
    v = [ut[11], ut[10], ut[9], ut[8]]
    L = np.zeros((6, 10))
    for r, (a, b) in enumerate(PAIRS):
        dv = [v[i][3 * a:3 * a + 3] - v[i][3 * b:3 * b + 3] for i in range(4)]
        L[r] = [_dot(dv[0], dv[0]), 2.0 * _dot(dv[0], dv[1]), _dot(dv[1], dv[1]), 2.0 * _dot(dv[0], dv[2]), 2.0 * _dot(dv[1], dv[2]),
                _dot(dv[2], dv[2]), 2.0 * _dot(dv[0], dv[3]), 2.0 * _dot(dv[1], dv[3]), 2.0 * _dot(dv[2], dv[3]), _dot(dv[3], dv[3])]
    return L


def rho_of(cws):
    """:1104-1113"""
    return np.array([_dot(cws[a] - cws[b], cws[a] - cws[b]) for a, b in PAIRS])


def find_betas(which, L, rho, be=NUMPY):
    """find_betas_approx_1 / _2 / _3 (:937-1039), which = 0, 1, 2"""
    betas = np.zeros(4)
    with np.errstate(all="ignore"):
        if which == 0:
            b4 = be.solve(L[:, [0, 1, 3, 6]], rho)
            if b4[0] < 0:
                betas[0] = math.sqrt(-b4[0])
                betas[1:] = [-b4[1] / betas[0], -b4[2] / betas[0], -b4[3] / betas[0]]
            else:
                betas[0] = math.sqrt(b4[0]) if b4[0] >= 0 else float("nan")
                betas[1:] = [b4[1] / betas[0], b4[2] / betas[0], b4[3] / betas[0]]
        else:
            b = be.solve(L[:, [0, 1, 2]] if which == 1 else L[:, [0, 1, 2, 3, 4]], rho)
            if b[0] < 0:
                betas[0] = math.sqrt(-b[0])
                betas[1] = math.sqrt(-b[2]) if b[2] < 0 else 0.0
            else:
                betas[0] = math.sqrt(b[0]) if b[0] >= 0 else float("nan")
                betas[1] = math.sqrt(b[2]) if b[2] > 0 else 0.0
            if b[1] < 0:
                betas[0] = -betas[0]
            if which == 2:
                betas[2] = b[3] / betas[0]
    return betas


def qr_solve(A, b):
    """:1251-1385 for an nr x nc system, operation by operation -> X, or None on the reference's "A is singular" return"""
    A = np.array(A, F64)
    b = np.array(b, F64)
    nr, nc = A.shape
    A1, A2 = np.zeros(nc), np.zeros(nc)
    with np.errstate(all="ignore"):
        for k in range(nc):
            eta = abs(A[k, k])
            for i in range(k + 1, nr):      # the pointer is advanced behind the comparison: rows k .. nr - 2 are looked at
                elt = abs(A[i - 1, k])
                if eta < elt:
                    eta = elt
            if eta == 0:
                return None
            inv_eta = 1. / eta
            s = 0.0
            for i in range(k, nr):
                A[i, k] = A[i, k] * inv_eta
                s = s + A[i, k] * A[i, k]
            sigma = math.sqrt(s) if s >= 0 else float("nan")
            if A[k, k] < 0:
                sigma = -sigma
            A[k, k] = A[k, k] + sigma
            A1[k] = sigma * A[k, k]
            A2[k] = -eta * sigma
            for j in range(k + 1, nc):
                s = 0.0
                for i in range(k, nr):
                    s = s + A[i, k] * A[i, j]
                tau = s / A1[k]
                for i in range(k, nr):
                    A[i, j] = A[i, j] - tau * A[i, k]
        for j in range(nc):
            tau = 0.0
            for i in range(j, nr):
                tau = tau + A[i, j] * b[i]
            tau = tau / A1[j]
            for i in range(j, nr):
                b[i] = b[i] - tau * A[i, j]
        X = np.zeros(nc)
        X[nc - 1] = b[nc - 1] / A2[nc - 1]
        for i in range(nc - 2, -1, -1):
            s = 0.0
            for j in range(i + 1, nc):
                s = s + A[i, j] * X[j]
            X[i] = (b[i] - s) / A2[i]
    return X


def gn_system(L, rho, betas):
    """compute_A_and_b_gauss_newton (:1184-1209)"""
    A, b = np.zeros((6, 4)), np.zeros(6)
    B = betas
    with np.errstate(all="ignore"):
        for i in range(6):
            r = L[i]
            A[i, 0] = (((2 * r[0]) * B[0] + r[1] * B[1]) + r[3] * B[2]) + r[6] * B[3]
            A[i, 1] = ((r[1] * B[0] + (2 * r[2]) * B[1]) + r[4] * B[2]) + r[7] * B[3]
            A[i, 2] = ((r[3] * B[0] + r[4] * B[1]) + (2 * r[5]) * B[2]) + r[8] * B[3]
            A[i, 3] = ((r[6] * B[0] + r[7] * B[1]) + r[8] * B[2]) + (2 * r[9]) * B[3]
            b[i] = rho[i] - ((((((((((r[0] * B[0]) * B[0] + (r[1] * B[0]) * B[1]) + (r[2] * B[1]) * B[1]) + (r[3] * B[0]) * B[2]) + (r[4] * B[1]) * B[2]) +
                                  (r[5] * B[2]) * B[2]) + (r[6] * B[0]) * B[3]) + (r[7] * B[1]) * B[3]) + (r[8] * B[2]) * B[3]) + (r[9] * B[3]) * B[3])
    return A, b


def gauss_newton(L, rho, betas):
    """:1213-1247; a singular step adds nothing (the reference adds an uninitialised increment)"""
    betas = np.array(betas, F64)
    for _ in range(5):
        A, b = gn_system(L, rho, betas)
        x = qr_solve(A, b)
        if x is not None:
            betas = betas + x
    return betas


def ccs_of(betas, ut):
    """compute_ccs (:649-665) -> (4, 3)"""
    c = np.zeros(12)
    with np.errstate(all="ignore"):
        for i in range(4):
            c = c + betas[i] * ut[11 - i]
    return c.reshape(4, 3)


def pcs_of(alphas, ccs):
    """compute_pcs (:669-681) -> (m, 3)"""
    a = alphas
    with np.errstate(all="ignore"):
        return ((a[:, 0:1] * ccs[0][None, :] + a[:, 1:2] * ccs[1][None, :]) + a[:, 2:3] * ccs[2][None, :]) + a[:, 3:4] * ccs[3][None, :]


def abt_of(pcs, pws, pc0, pw0):
    s = np.zeros((3, 3))
    with np.errstate(all="ignore"):
        for pc, pw in zip(pcs, pws):
            s = s + (pc - pc0)[:, None] * (pw - pw0)[None, :]
    return s


def finish_R_t(R, pc0, pw0):
    """:872-885"""
    R = np.array(R, F64)
    with np.errstate(all="ignore"):
        det = (((((R[0, 0] * R[1, 1]) * R[2, 2] + (R[0, 1] * R[1, 2]) * R[2, 0]) + (R[0, 2] * R[1, 0]) * R[2, 1]) - (R[0, 2] * R[1, 1]) * R[2, 0]) -
               (R[0, 1] * R[1, 0]) * R[2, 2]) - (R[0, 0] * R[1, 2]) * R[2, 1]
        if det < 0:
            R[2] = -R[2]
        t = np.array([pc0[i] - _dot(R[i], pw0) for i in range(3)])
    return R, t


def reprojection_error(R, t, pws, us, K):
    """:790-813"""
    fu, fv, uc, vc = [float(v) for v in K]
    s = 0.0
    with np.errstate(all="ignore"):
        for pw, (u, v) in zip(np.asarray(pws, F64), np.asarray(us, F64)):
            Xc, Yc = _dot(R[0], pw) + t[0], _dot(R[1], pw) + t[1]
            inv = 1.0 / (_dot(R[2], pw) + t[2])
            ue, ve = uc + (fu * Xc) * inv, vc + (fv * Yc) * inv
            s = s + math.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))
    return s / float(len(pws))


def R_and_t(ut, betas, alphas, pws, us, K, c0, be=NUMPY):
    """compute_R_and_t (:917-932) -> (R, t, error, dict of the pieces)"""
    ccs = ccs_of(betas, ut)
    pcs = pcs_of(alphas, ccs)
    if pcs[0, 2] < 0.0:      # solve_for_sign (:897-914)
        ccs, pcs = -ccs, -pcs
    pc0 = np.zeros(3)
    for pc in pcs:
        pc0 = pc0 + pc
    pc0 = pc0 / float(len(pcs))
    abt = abt_of(pcs, np.asarray(pws, F64), pc0, c0)
    R, t = finish_R_t(be.rotation(abt), pc0, c0)
    return R, t, reprojection_error(R, t, pws, us, K), dict(ccs=ccs, pc0=pc0, abt=abt)


def choose(errs):
    """:750-752 -> N (1, 2 or 3)"""
    N = 1
    if errs[1] < errs[0]:
        N = 2
    if errs[2] < errs[N - 1]:
        N = 3
    return N


def compute_pose(pws, us, K, be=NUMPY):
    """compute_pose (:684-759) on float positions pws (m, 3) and keypoints us (m, 2) -> dict of every stage"""
    pws, us = np.asarray(pws, F32).astype(F64), np.asarray(us, F32).astype(F64)
    m = len(pws)
    o = {}
    c0 = centroid(pws)
    o["pca"] = pw0tpw0(pws, c0)
    o["dc"], o["uct"] = be.svd_sym(o["pca"])
    o["cws"] = control_points(c0, o["dc"], o["uct"], m)
    o["ci"] = be.invert(cc_matrix(o["cws"]))
    o["alphas"] = alphas_of(o["cws"], o["ci"], pws)
    o["mtm"] = mtm_of(o["alphas"], us, K)
    o["d"], o["ut"] = be.svd_sym(o["mtm"])
    o["L"], o["rho"] = L_6x10(o["ut"]), rho_of(o["cws"])
    o["b0"], o["b1"], o["Rs"], o["ts"], o["errs"] = np.zeros((3, 4)), np.zeros((3, 4)), np.zeros((3, 3, 3)), np.zeros((3, 3)), np.zeros(3)
    for a in range(3):
        o["b0"][a] = find_betas(a, o["L"], o["rho"], be)
        o["b1"][a] = gauss_newton(o["L"], o["rho"], o["b0"][a])
        o["Rs"][a], o["ts"][a], o["errs"][a], _ = R_and_t(o["ut"], o["b1"][a], o["alphas"], pws, us, K, c0, be)
    o["choice"] = choose(o["errs"])
    o["R"], o["t"], o["err"] = o["Rs"][o["choice"] - 1], o["ts"][o["choice"] - 1], o["errs"][o["choice"] - 1]
    return o


# ---------------------------------------------------------------------------------------------------------------------------------------
# CheckInliers (:421-458), Refine (:366-418), iterate (:240-363)
# ---------------------------------------------------------------------------------------------------------------------------------------
def max_error(sigma2, th2=5.991):
    return np.asarray(sigma2, F32) * F32(th2)


def check_inliers(R, t, K, p2d, p3d, maxerr):
    """-> (count, mask); the member types of include/PnPsolver.h: mRi, mti, fu .. vc double; Xc, Yc, invZc, distX, distY, error2 float; ue, ve double"""
    fu, fv, uc, vc = [F64(F32(v)) for v in K]
    R, t = np.asarray(R, F64), np.asarray(t, F64)
    P = np.asarray(p3d, F32).astype(F64)
    p2 = np.asarray(p2d, F32)
    with np.errstate(all="ignore"):
        Xc = (((R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1]) + R[0, 2] * P[:, 2]) + t[0]).astype(F32)
        Yc = (((R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1]) + R[1, 2] * P[:, 2]) + t[1]).astype(F32)
        invZc = (1.0 / (((R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1]) + R[2, 2] * P[:, 2]) + t[2])).astype(F32)
        ue = uc + (fu * Xc.astype(F64)) * invZc.astype(F64)
        ve = vc + (fv * Yc.astype(F64)) * invZc.astype(F64)
        distX = (p2[:, 0].astype(F64) - ue).astype(F32)
        distY = (p2[:, 1].astype(F64) - ve).astype(F32)
        error2 = distX * distX + distY * distY
        mask = error2 < np.asarray(maxerr, F32)
    return int(mask.sum()), mask


def tcw_of(R, t):
    """:310-316 / :407-413: Rcw, tcw narrowed to float inside a 4x4 identity"""
    T = np.eye(4, dtype=F32)
    T[:3, :3] = np.asarray(R, F64).astype(F32)
    T[:3, 3] = np.asarray(t, F64).astype(F32)
    return T


def refine(mask, c, K, maxerr, be=NUMPY):
    """Refine (:366-418) on the running-best mask -> (R, t, count, mask)"""
    idx = np.flatnonzero(mask)
    o = compute_pose(c["p3d"][idx], c["p2d"][idx], K, be)
    cnt, m = check_inliers(o["R"], o["t"], K, c["p2d"], c["p3d"], maxerr)
    return o["R"], o["t"], cnt, m


class Iterate:
    """The stateful loop of iterate (:240-363), sequential and literal.  model(i) -> (Tcw, count, mask) of iteration i;
    refine_fn(mask) -> (Tcw, count, mask) of Refine on the running best."""

    def __init__(self, n, min_inliers, max_its, model, refine_fn):
        self.N, self.min_inliers, self.max_its, self.model, self.refine_fn = n, min_inliers, max_its, model, refine_fn
        self.mnIterations, self.mnBestInliers, self.best_mask, self.best_T = 0, 0, None, None
        self.refine_calls = 0

    def iterate(self, nIterations):
        """-> (Tcw or None, bNoMore, vbInliers or None, nInliers)"""
        if self.N < self.min_inliers:
            return None, True, None, 0
        cur = 0
        while self.mnIterations < self.max_its or cur < nIterations:
            cur += 1
            it = self.mnIterations
            self.mnIterations += 1
            T, count, mask = self.model(it)
            if count >= self.min_inliers:
                if count > self.mnBestInliers:
                    self.best_mask, self.mnBestInliers, self.best_T = mask, count, T
                self.refine_calls += 1
                rT, rcount, rmask = self.refine_fn(self.best_mask)
                if rcount > self.min_inliers:
                    return rT, False, rmask, rcount
        if self.mnIterations >= self.max_its:
            if self.mnBestInliers >= self.min_inliers:
                return self.best_T, True, self.best_mask, self.mnBestInliers
            return None, True, None, 0
        return None, False, None, 0

    def find(self):
        return self.iterate(self.max_its)


def records_of(counts, min_inliers):
    """-> (record_of[i] = index of the latest record at or before i or -1, the records' iterations): the running best changes only on
    count >= min_inliers and count > best"""
    best, recs, rec_of = 0, [], []
    for i, c in enumerate(counts):
        if c >= min_inliers and c > best:
            best = int(c)
            recs.append(i)
        rec_of.append(len(recs) - 1)
    return np.array(rec_of, np.int64), np.array(recs, np.int64)


class Replay:
    """The same surface from the "records + events" formulation the device computes: per iteration only the count, per record the refined
    result, computed ONCE per record.  counts(i) / record data are looked up, nothing is carried but mnIterations."""

    def __init__(self, n, min_inliers, max_its, counts, model_T, model_mask, refined):
        """counts[i]; model_T(i), model_mask(i); refined(r) -> (Tcw, count, mask) of record r"""
        self.N, self.min_inliers, self.max_its = n, min_inliers, max_its
        self.counts, self.model_T, self.model_mask, self.refined = counts, model_T, model_mask, refined
        self.mnIterations = 0

    def iterate(self, nIterations):
        if self.N < self.min_inliers:
            return None, True, None, 0
        cur = 0
        while self.mnIterations < self.max_its or cur < nIterations:
            cur += 1
            it = self.mnIterations
            self.mnIterations += 1
            counts = self.counts(it + 1)
            if counts[it] >= self.min_inliers:
                rec_of, _ = records_of(counts[:it + 1], self.min_inliers)
                rT, rcount, rmask = self.refined(int(rec_of[it]))
                if rcount > self.min_inliers:
                    return rT, False, rmask, rcount
        if self.mnIterations >= self.max_its:
            counts = self.counts(self.mnIterations)
            _, recs = records_of(counts[:self.mnIterations], self.min_inliers)
            if len(recs):
                b = int(recs[-1])
                return self.model_T(b), True, self.model_mask(b), int(counts[b])
            return None, True, None, 0
        return None, False, None, 0

    def find(self):
        return self.iterate(self.max_its)


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
K_TEST = (500.0, 500.0, 320.0, 240.0)
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], F32)


def rodrigues(v):
    th = float(np.linalg.norm(v))
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(v, F64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def scene(n, seed, outliers=0.0, noise=True, K=K_TEST, behind=False, decoy=0):
    """n matches: points 2-10 m in front of a camera at a random pose, keypoints with octave-dependent pixel noise (sigma = 0.5 * 1.2^octave),
    a share of gross outliers (keypoints redrawn over the image).  behind: match 0's point is moved behind the camera.  decoy: the last `decoy`
    matches see their points from a SECOND pose, without noise: a consistent minority that a set drawn inside it fits exactly."""
    g = np.random.default_rng(seed)
    R = rodrigues(g.normal(size=3) * 0.4)
    t = g.normal(size=3) * 0.5
    fu, fv, uc, vc = K
    uv = np.stack([g.uniform(20, 620, n), g.uniform(20, 460, n)], 1)
    z = g.uniform(2.0, 10.0, n)
    pc = np.stack([(uv[:, 0] - uc) / fu * z, (uv[:, 1] - vc) / fv * z, z], 1)
    pw = (pc - t) @ R      # R^T (pc - t)
    octave = g.integers(0, 8, n)
    p2d = uv.copy()
    if noise:
        p2d += g.normal(size=(n, 2)) * (0.5 * 1.2 ** octave)[:, None]
    nout = int(round(outliers * n))
    out_idx = g.permutation(n)[:nout]
    p2d[out_idx] = np.stack([g.uniform(0, 640, nout), g.uniform(0, 480, nout)], 1)
    if behind and n:
        pw[0] = (np.array([0.1, 0.1, -3.0]) - t) @ R
    if decoy:
        R2, t2 = rodrigues(g.normal(size=3) * 0.1) @ R, t + g.normal(size=3) * 0.3
        q = pw[n - decoy:] @ R2.T + t2
        p2d[n - decoy:] = np.stack([uc + fu * q[:, 0] / q[:, 2], vc + fv * q[:, 1] / q[:, 2]], 1)
        out_idx = out_idx[out_idx < n - decoy]
    is_out = np.zeros(n, bool)
    is_out[out_idx] = True
    return dict(K=K, p2d=p2d.astype(F32), p3d=pw.astype(F32), sigma2=SIGMA2[octave], R=R, t=t, outlier=is_out)


def rot_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, F64).T @ np.asarray(Rb, F64)) - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))


def ulp_perturbed(x, g):
    """every entry moved by one ulp, up or down at random"""
    x = np.asarray(x, F64)
    return np.nextafter(x, np.where(g.integers(0, 2, x.shape) == 1, np.inf, -np.inf))
