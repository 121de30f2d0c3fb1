"""Expected values of monocular initialisation (orbx_initialize / orbx_init_score_models / orbx_init_check_rt), independent of the code under test.

A numpy restatement of Initializer (reference src/Initializer.cc) from its stated semantics - NOT the reference and not compiled from it:
    float32 where the reference computes in float, one operation per numpy call, so nothing is fused or promoted; Mat::dot and cv::norm
    accumulate in float64 from 0; 1.0 / x is a float64 quotient narrowed to float32; Mat / double divides in float64; sequential float32
    sums where the reference loops (Normalize, the scores: numpy's cumsum adds in order); 3-term matrix products left to right in float32;
    null vectors and 3x3 SVDs from numpy.linalg.svd in float64, narrowed to float32 where the reference holds a float matrix; Mat::inv by
    cofactors in float64 (inv3), narrowed to float32; cv::determinant by cofactors in float64.
Stage-wise: normalize, compute_h21, compute_f21 (rank2), denormalise_h / _f, check_homography, check_fundamental, decompose_e, decompose_h,
check_rt (status, `near`), reconstruct_f_select, reconstruct_h_select, initialize.  `near` marks the CheckRT decisions that sit on a
threshold (COS_EPS / REL_EPS of tests/triangulate_ref.py): a different last bit may flip them legitimately.

Also: the device's two Jacobi iterations restated in float64 (jacobi_null9: 9 columns, the four disjoint pairs of a round-robin round at a
time, 16-lane butterfly sums; jacobi_svd3) for the choice of their sweep counts, initializer_sets' hand-worked example, the scene
generators and the screening of scenes (margins)."""
import numpy as np

from triangulate_ref import COS_EPS, REL_EPS, jacobi_null as jacobi_null4

F32, F64 = np.float32, np.float64
NOT_INLIER, NONFINITE, BEHIND1, BEHIND2, REPROJ1, REPROJ2, GOOD, GOOD_LOW_PARALLAX = range(8)
NAMES = ("NOT_INLIER", "NONFINITE", "BEHIND1", "BEHIND2", "REPROJ1", "REPROJ2", "GOOD", "GOOD_LOW_PARALLAX")
K_DEFAULT = (500.0, 500.0, 320.0, 240.0)
TH_H = F32(5.991)
TH_F = F32(3.841)
COS_GATE = 0.99998


# ---------------------------------------------------------------------------------------------------------------------------------------
# small algebra
# ---------------------------------------------------------------------------------------------------------------------------------------
def mm3(a, b):
    """(..., 3, 3) x (..., 3, k): a0*b0 + a1*b1 + a2*b2 left to right in the element type"""
    s = a[..., :, 0:1] * b[..., 0:1, :]
    s = s + a[..., :, 1:2] * b[..., 1:2, :]
    s = s + a[..., :, 2:3] * b[..., 2:3, :]
    return s


def inv3(m):
    """Mat::inv of (..., 3, 3): cofactors over the determinant, in float64"""
    m = np.asarray(m, F64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., i, j] for i in range(3) for j in range(3)]
    c00, c01, c02 = m11 * m22 - m12 * m21, m02 * m21 - m01 * m22, m01 * m12 - m02 * m11
    c10, c11, c12 = m12 * m20 - m10 * m22, m00 * m22 - m02 * m20, m02 * m10 - m00 * m12
    c20, c21, c22 = m10 * m21 - m11 * m20, m01 * m20 - m00 * m21, m00 * m11 - m01 * m10
    det = m00 * c00 + m01 * c10 + m02 * c20
    out = np.stack([c00, c01, c02, c10, c11, c12, c20, c21, c22], -1) / det[..., None]
    return out.reshape(m.shape)


def det3(m):
    m = np.asarray(m, F64)
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]) + m[..., 0, 1] * (m[..., 1, 2] * m[..., 2, 0] - m[..., 1, 0] * m[..., 2, 2]) +
            m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def kmat(K):
    fx, fy, cx, cy = [F32(v) for v in K]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F32)


def seqsum(x, axis=-1):
    """sequential float32 sum from 0 (numpy's cumsum adds in order)"""
    x = np.asarray(x, F32)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), F32)
    return np.take(np.cumsum(x, axis=axis, dtype=F32), -1, axis=axis)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Normalize, the two minimal solvers, denormalisation
# ---------------------------------------------------------------------------------------------------------------------------------------
def compact(matches12):
    """mvMatches12: (N, 2) pairs (i1, i2) in i1 order"""
    m = np.asarray(matches12, np.int64)
    i1 = np.nonzero(m >= 0)[0]
    return np.stack([i1, m[i1]], 1)


def normalize(xy):
    """Normalize over ALL keypoints of a frame -> (normalised (n, 2) float32, T (3, 3) float32)"""
    xy = np.asarray(xy, F32)
    n = F32(len(xy))
    mean = seqsum(xy, 0) / n
    vn = xy - mean[None, :]
    dev = seqsum(np.abs(vn), 0) / n
    s = (1.0 / dev.astype(F64)).astype(F32)
    pn = vn * s[None, :]
    T = np.eye(3, dtype=F32)
    T[0, 0], T[1, 1] = s[0], s[1]
    T[0, 2], T[1, 2] = (-mean[0]) * s[0], (-mean[1]) * s[1]
    return pn.astype(F32), T


def build_ah(p1, p2):
    """(M, 8, 2) normalised pairs -> the (M, 16, 9) float32 DLT matrix of ComputeH21"""
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    r0 = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
    r1 = np.stack([u1, v1, o, z, z, z, (-u2) * u1, (-u2) * v1, -u2], -1)
    return np.stack([r0, r1], -2).reshape(p1.shape[:-2] + (16, 9)).astype(F32)


def build_af(p1, p2):
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(F32)


def null9(A):
    """(M, r, 9) float32 -> vt.row(8) of the float64 SVD (M, 9) float64, and the relative gap (s8 - s9) / s1 (s9 = 0 for 8 rows)"""
    u, s, vt = np.linalg.svd(A.astype(F64), full_matrices=True)
    s9 = s[..., 8] if s.shape[-1] > 8 else np.zeros(s.shape[:-1])
    return vt[..., 8, :], (s[..., 7] - s9) / s[..., 0]


def compute_h21(p1, p2):
    nv, gap = null9(build_ah(p1, p2))
    return nv.astype(F32).reshape(nv.shape[:-1] + (3, 3)), gap


def rank2(fpre, prod64=False, svd=None):
    """the second SVD of ComputeF21: u * diag(w with w[2] = 0) * vt in float32 (prod64: everything in float64, for the error yardstick)"""
    fpre = np.asarray(fpre, F32)
    u, w, vt = np.linalg.svd(fpre.astype(F64)) if svd is None else svd(fpre)
    w = w.copy()
    w[..., 2] = 0
    T = F64 if prod64 else F32
    u, w, vt = u.astype(T), w.astype(T), vt.astype(T)
    d = np.zeros(fpre.shape, T)
    for i in range(3):
        d[..., i, i] = w[..., i]
    return mm3(mm3(u, d), vt)


def compute_f21(p1, p2):
    nv, gap = null9(build_af(p1, p2))
    fpre = nv.astype(F32).reshape(nv.shape[:-1] + (3, 3))
    return rank2(fpre), fpre, gap


def denormalise_h(hn, T1, T2):
    """H21 = T2inv * Hn * T1 in float32; H12 = H21.inv() -> both (M, 3, 3) float32"""
    t2inv = inv3(T2).astype(F32)
    h21 = mm3(mm3(t2inv, np.asarray(hn, F32)), T1)
    return h21, inv3(h21).astype(F32)


def denormalise_f(fn, T1, T2):
    return mm3(mm3(np.ascontiguousarray(T2.T), np.asarray(fn, F32)), T1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# scores
# ---------------------------------------------------------------------------------------------------------------------------------------
def _inv_sigma2(sigma):
    s = F32(sigma)
    return F32(1.0 / F64(s * s))


def _score(chi1, chi2, th, th_score):
    in1, in2 = ~(chi1 > th), ~(chi2 > th)
    t1 = np.where(in1, th_score - chi1, F32(0)).astype(F32)
    t2 = np.where(in2, th_score - chi2, F32(0)).astype(F32)
    terms = np.stack([t1, t2], -1).reshape(chi1.shape[:-1] + (-1,))      # match 0 term 1, match 0 term 2, match 1 term 1 ...
    return seqsum(terms, -1), in1 & in2


def check_homography(h21, h12, pts, sigma):
    """h21, h12 (M, 3, 3) float32; pts (N, 4) float32 = u1, v1, u2, v2 of the matches -> score (M) float32, inliers (M, N) bool, chi (M, N, 2)"""
    h, hi = np.asarray(h21, F32).reshape(-1, 9), np.asarray(h12, F32).reshape(-1, 9)
    u1, v1, u2, v2 = [np.asarray(pts, F32)[None, :, k] for k in range(4)]
    H = [h[:, k:k + 1] for k in range(9)]
    I = [hi[:, k:k + 1] for k in range(9)]
    isq = _inv_sigma2(sigma)
    with np.errstate(all="ignore"):
        w = (1.0 / (I[6] * u2 + I[7] * v2 + I[8]).astype(F64)).astype(F32)
        a = (I[0] * u2 + I[1] * v2 + I[2]) * w
        b = (I[3] * u2 + I[4] * v2 + I[5]) * w
        d1 = (u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)
        chi1 = d1 * isq
        w = (1.0 / (H[6] * u1 + H[7] * v1 + H[8]).astype(F64)).astype(F32)
        a = (H[0] * u1 + H[1] * v1 + H[2]) * w
        b = (H[3] * u1 + H[4] * v1 + H[5]) * w
        d2 = (u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)
        chi2 = d2 * isq
        score, inl = _score(chi1, chi2, TH_H, TH_H)
    return score, inl, np.stack([chi1, chi2], -1)


def check_fundamental(f21, pts, sigma):
    f = np.asarray(f21, F32).reshape(-1, 9)
    u1, v1, u2, v2 = [np.asarray(pts, F32)[None, :, k] for k in range(4)]
    Fm = [f[:, k:k + 1] for k in range(9)]
    isq = _inv_sigma2(sigma)
    with np.errstate(all="ignore"):
        a2 = Fm[0] * u1 + Fm[1] * v1 + Fm[2]
        b2 = Fm[3] * u1 + Fm[4] * v1 + Fm[5]
        c2 = Fm[6] * u1 + Fm[7] * v1 + Fm[8]
        num2 = a2 * u2 + b2 * v2 + c2
        d1 = num2 * num2 / (a2 * a2 + b2 * b2)
        chi1 = d1 * isq
        a1 = Fm[0] * u2 + Fm[3] * v2 + Fm[6]
        b1 = Fm[1] * u2 + Fm[4] * v2 + Fm[7]
        c1 = Fm[2] * u2 + Fm[5] * v2 + Fm[8]
        num1 = a1 * u1 + b1 * v1 + c1
        d2 = num1 * num1 / (a1 * a1 + b1 * b1)
        chi2 = d2 * isq
        score, inl = _score(chi1, chi2, TH_F, TH_H)
    return score, inl, np.stack([chi1, chi2], -1)


def first_argmax(scores):
    """the iteration FindHomography / FindFundamental keep: currentScore > score, strict, from score = 0 (iteration 0 when nothing beats 0)"""
    return int(np.argmax(np.asarray(scores)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# motion hypotheses
# ---------------------------------------------------------------------------------------------------------------------------------------
def _svd3(A, svd=None):
    return np.linalg.svd(np.asarray(A, F32).astype(F64)) if svd is None else svd(np.asarray(A, F32))


def decompose_e(f21, K, prod64=False, svd=None):
    """ReconstructF's four motions in its order: (R1, t), (R2, t), (R1, -t), (R2, -t) -> R (4, 3, 3), t (4, 3)"""
    Km = kmat(K)
    E = mm3(mm3(np.ascontiguousarray(Km.T), np.asarray(f21, F32).reshape(3, 3)), Km)
    u, w, vt = _svd3(E, svd)
    T = F64 if prod64 else F32
    u, vt = u.astype(T), vt.astype(T)
    t = u[:, 2]
    t = (t.astype(F64) / np.sqrt(np.sum(t.astype(F64) * t.astype(F64)))).astype(T)
    W = np.zeros((3, 3), T)
    W[0, 1], W[1, 0], W[2, 2] = -1, 1, 1
    R1 = mm3(mm3(u, W), vt)
    if det3(R1) < 0:
        R1 = -R1
    R2 = mm3(mm3(u, np.ascontiguousarray(W.T)), vt)
    if det3(R2) < 0:
        R2 = -R2
    return np.stack([R1, R2, R1, R2]), np.stack([t, t, -t, -t])


def decompose_h(h21, K, prod64=False, svd=None):
    """ReconstructH's eight motions in its order -> valid, R (8, 3, 3), t (8, 3) (zeros when the singular values are too close)"""
    Km = kmat(K)
    T = F64 if prod64 else F32
    invK = inv3(Km).astype(F32)
    A = mm3(mm3(invK, np.asarray(h21, F32).reshape(3, 3)), Km)
    U, w, Vt = _svd3(A, svd)
    U, w, Vt = U.astype(T), w.astype(T), Vt.astype(T)
    s = T(det3(U) * det3(Vt))
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        if F64(d1 / d2) < 1.00001 or F64(d2 / d3) < 1.00001 or not np.isfinite(F64(d1 / d2)) or not np.isfinite(F64(d2 / d3)):
            return False, np.zeros((8, 3, 3), T), np.zeros((8, 3), T)
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [aux_st, -aux_st, -aux_st, aux_st]
    aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
    sU = s * U
    Rs, ts = [], []
    for fam in range(2):
        for i in range(4):
            Rp = np.eye(3, dtype=T)
            if fam == 0:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[i], st[i], ct
                tp = np.array([x1[i], 0, -x3[i]], T) * (d1 - d3)
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[i], -1, sp[i], -cp
                tp = np.array([x1[i], 0, x3[i]], T) * (d1 + d3)
            Rs.append(mm3(mm3(sU, Rp), Vt))
            t = mm3(U, tp.astype(T)[:, None])[:, 0]
            n = np.sqrt(np.sum(t.astype(F64) * t.astype(F64)))
            ts.append((t.astype(F64) / n).astype(T))
    return True, np.stack(Rs), np.stack(ts)


# ---------------------------------------------------------------------------------------------------------------------------------------
# CheckRT
# ---------------------------------------------------------------------------------------------------------------------------------------
def parallax_deg(c):
    """acos(cos) * 180 / CV_PI: float acos, float product, float64 quotient narrowed to float32"""
    a = np.arccos(np.asarray(c, F32)).astype(F32)
    return (F64(a * F32(180)) / np.pi).astype(F32) if np.ndim(a) else F32(F64(a * F32(180)) / np.pi)


def triangulation_rows(R, t, K, pts):
    """the (N, 4, 4) float32 A of Triangulate with P1 = K [I | 0], P2 = K [R | t]"""
    Km = kmat(K)
    P1 = np.zeros((3, 4), F32)
    P1[:, :3] = Km
    P2 = mm3(Km, np.concatenate([np.asarray(R, F32), np.asarray(t, F32)[:, None]], 1))
    u1, v1, u2, v2 = [np.asarray(pts, F32)[:, k:k + 1] for k in range(4)]
    A = np.empty((len(u1), 4, 4), F32)
    A[:, 0] = u1 * P1[2][None, :] - P1[0][None, :]
    A[:, 1] = v1 * P1[2][None, :] - P1[1][None, :]
    A[:, 2] = u2 * P2[2][None, :] - P2[0][None, :]
    A[:, 3] = v2 * P2[2][None, :] - P2[1][None, :]
    return A


def check_rt(R, t, K, pts, pairs, inliers, th2, n1, null_vector=None):
    """CheckRT of one motion.  pts (N, 4), pairs (N, 2), inliers (N) bool -> dict(status (N) uint8, p3d (N, 3) float32 per MATCH (the
    triangulated point wherever one was computed), cos (N) float32, near (N) bool, good int, vb_good (n1) bool, vp3d (n1, 3) float32,
    cos_sel float32 (1.0 when nothing is good: acos(1) = 0), parallax float32 in degrees, dist1 (N) float64)"""
    R, t = np.asarray(R, F32).reshape(3, 3), np.asarray(t, F32).reshape(3)
    fx, fy, cx, cy = [F32(v) for v in K]
    pts = np.asarray(pts, F32)
    N = len(pts)
    inl = np.asarray(inliers, bool)
    th2 = F32(th2)
    with np.errstate(all="ignore"):
        A = triangulation_rows(R, t, K, pts)
        nv = np.linalg.svd(A.astype(F64))[2][:, 3, :] if null_vector is None else null_vector(A)
        p = (nv[:, :3] / nv[:, 3:4]).astype(F32)
        O2 = mm3(-np.ascontiguousarray(R.T), t[:, None])[:, 0]
        finite = np.isfinite(p).all(1)
        pd = p.astype(F64)
        dist1 = np.sqrt(pd[:, 0] * pd[:, 0] + pd[:, 1] * pd[:, 1] + pd[:, 2] * pd[:, 2]).astype(F32)
        n2 = (p - O2[None, :]).astype(F32)
        n2d = n2.astype(F64)
        dist2 = np.sqrt(n2d[:, 0] * n2d[:, 0] + n2d[:, 1] * n2d[:, 1] + n2d[:, 2] * n2d[:, 2]).astype(F32)
        dot = pd[:, 0] * n2d[:, 0] + pd[:, 1] * n2d[:, 1] + pd[:, 2] * n2d[:, 2]
        cosp = (dot / (dist1 * dist2).astype(F64)).astype(F32)
        low = cosp.astype(F64) < COS_GATE
        p2 = (mm3(R[None], p[:, :, None])[:, :, 0] + t[None, :]).astype(F32)
        iz1 = (1.0 / p[:, 2].astype(F64)).astype(F32)
        ex, ey = (fx * p[:, 0] * iz1 + cx) - pts[:, 0], (fy * p[:, 1] * iz1 + cy) - pts[:, 1]
        e1 = ex * ex + ey * ey
        iz2 = (1.0 / p2[:, 2].astype(F64)).astype(F32)
        ex, ey = (fx * p2[:, 0] * iz2 + cx) - pts[:, 2], (fy * p2[:, 1] * iz2 + cy) - pts[:, 3]
        e2 = ex * ex + ey * ey
        status = np.full(N, NOT_INLIER, np.uint8)
        near = np.zeros(N, bool)
        alive = inl.copy()
        d1 = dist1.astype(F64)
        near_gate = np.abs(cosp.astype(F64) - COS_GATE) <= COS_EPS

        def stage(fail, code, close):
            nonlocal alive, near
            near |= alive & close
            status[alive & fail] = code
            alive = alive & ~fail

        stage(~finite, NONFINITE, np.zeros(N, bool))
        stage((p[:, 2] <= 0) & low, BEHIND1, (np.abs(pd[:, 2]) <= REL_EPS * d1) | ((p[:, 2] <= 0) & near_gate))
        stage((p2[:, 2] <= 0) & low, BEHIND2, (np.abs(p2[:, 2].astype(F64)) <= REL_EPS * dist2.astype(F64)) | ((p2[:, 2] <= 0) & near_gate))
        stage(e1 > th2, REPROJ1, np.abs(e1.astype(F64) - F64(th2)) <= REL_EPS * F64(th2))
        stage(e2 > th2, REPROJ2, np.abs(e2.astype(F64) - F64(th2)) <= REL_EPS * F64(th2))
        near |= alive & near_gate
        status[alive & low] = GOOD
        status[alive & ~low] = GOOD_LOW_PARALLAX
    good = alive
    vb = np.zeros(n1, bool)
    vp = np.zeros((n1, 3), F32)
    i1 = np.asarray(pairs)[:, 0]
    vb[i1[good & low]] = True
    vp[i1[good]] = p[good]
    cs = np.sort(cosp[good])
    cos_sel = cs[min(50, len(cs) - 1)] if len(cs) else F32(1.0)
    computed = inl & finite
    return dict(status=status, p3d=np.where(computed[:, None], p, F32(0)).astype(F32), cos=cosp, near=near, good=int(good.sum()), vb_good=vb, vp3d=vp, cos_sel=F32(cos_sel),
                parallax=parallax_deg(F32(cos_sel)), dist1=d1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------------------------------
def reconstruct_f_select(good, parallax, n_inliers, min_parallax=1.0, min_triangulated=50):
    """-> (success, hypothesis 0..3 or -1).  The `else if` chain: only the FIRST hypothesis that reaches maxGood is asked for its parallax."""
    good = [int(g) for g in good]
    mx = max(good)
    n_min = max(int(0.9 * n_inliers), int(min_triangulated))
    nsimilar = sum(1 for g in good if g > 0.7 * mx)
    if mx < n_min or nsimilar > 1:
        return False, -1
    k = good.index(mx)
    return (True, k) if F32(parallax[k]) > F32(min_parallax) else (False, -1)


def reconstruct_h_select(good, parallax, n_inliers, min_parallax=1.0, min_triangulated=50):
    best = second = 0
    idx, bp = -1, F32(-1)
    for i, g in enumerate(int(g) for g in good):
        if g > best:
            second, best, idx, bp = best, g, i, F32(parallax[i])
        elif g > second:
            second = g
    ok = second < 0.75 * best and bp >= F32(min_parallax) and best > min_triangulated and best > 0.9 * n_inliers
    return (True, idx) if ok else (False, -1)


def select(rh, hyp_valid, hyp_good, hyp_parallax, n_inl_h, n_inl_f, min_parallax=1.0, min_triangulated=50):
    """Initialize's branch on RH and the two selections over the twelve hypotheses (4 of DecomposeE, then 8 of ReconstructH)
    -> (success, model, hypothesis 0..11 or -1)"""
    if F32(rh) > F32(0.40):
        if not all(hyp_valid[4:]):
            return False, 0, -1
        ok, k = reconstruct_h_select(hyp_good[4:], hyp_parallax[4:], n_inl_h, min_parallax, min_triangulated)
        return ok, 0, (4 + k if ok else -1)
    ok, k = reconstruct_f_select(hyp_good[:4], hyp_parallax[:4], n_inl_f, min_parallax, min_triangulated)
    return ok, 1, (k if ok else -1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the whole of Initialize
# ---------------------------------------------------------------------------------------------------------------------------------------
def initializer_sets_example():
    """hand-worked: N = 10, one iteration, randint always returning its lower bound 0.  available = [0..9]: draw index 0 -> 0, the back (9)
    takes its place -> [9,1..8]; draw 0 -> 9, back 8 -> [8,1..7]; then 8, 7, 6, 5, 4, 3.  With randint always the upper bound the back itself
    is drawn each time: 9, 8, 7, 6, 5, 4, 3, 2."""
    return [0, 9, 8, 7, 6, 5, 4, 3], [9, 8, 7, 6, 5, 4, 3, 2]


def initialize(keys1, keys2, matches12, K, sets, sigma=1.0, min_parallax=1.0, min_triangulated=50):
    """-> dict with every stage's values (the names of orbx_init_result)"""
    keys1, keys2 = np.asarray(keys1, F32), np.asarray(keys2, F32)
    pairs = compact(matches12)
    N, n1 = len(pairs), len(keys1)
    sets = np.asarray(sets, np.int64).reshape(-1, 8)
    pts = np.concatenate([keys1[pairs[:, 0]], keys2[pairs[:, 1]]], 1)
    pn1, T1 = normalize(keys1)
    pn2, T2 = normalize(keys2)
    p1, p2 = pn1[pairs[sets, 0]], pn2[pairs[sets, 1]]
    hn, gap_h = compute_h21(p1, p2)
    fn, fpre, gap_f = compute_f21(p1, p2)
    h21, h12 = denormalise_h(hn, T1, T2)
    f21 = denormalise_f(fn, T1, T2)
    sh_all, inl_h_all, chi_h = check_homography(h21, h12, pts, sigma)
    sf_all, inl_f_all, chi_f = check_fundamental(f21, pts, sigma)
    bh, bf = first_argmax(sh_all), first_argmax(sf_all)
    sh, sf = sh_all[bh], sf_all[bf]
    with np.errstate(all="ignore"):
        rh = F32(sh / F32(sh + sf))
    inl_h, inl_f = inl_h_all[bh], inl_f_all[bf]
    Re, te = decompose_e(f21[bf], K)
    valid_h, Rh, th = decompose_h(h21[bh], K)
    hyp_r, hyp_t = np.concatenate([Re, Rh]).astype(F32), np.concatenate([te, th]).astype(F32)
    hyp_valid = np.array([1] * 4 + [int(valid_h)] * 8, np.uint8)
    th2 = F32(4.0 * F64(F32(sigma) * F32(sigma)))
    crt = []
    for k in range(12):
        if hyp_valid[k]:
            crt.append(check_rt(hyp_r[k], hyp_t[k], K, pts, pairs, inl_f if k < 4 else inl_h, th2, n1))
        else:
            crt.append(dict(status=np.zeros(N, np.uint8), p3d=np.zeros((N, 3), F32), cos=np.zeros(N, F32), near=np.zeros(N, bool), good=0, vb_good=np.zeros(n1, bool),
                            vp3d=np.zeros((n1, 3), F32), cos_sel=F32(1), parallax=F32(0), dist1=np.ones(N)))
    good = [c["good"] for c in crt]
    par = [c["parallax"] for c in crt]
    ok, model, hyp = select(rh, hyp_valid, good, par, int(inl_h.sum()), int(inl_f.sum()), min_parallax, min_triangulated)
    out = dict(n_matches=N, pairs=pairs, pts=pts, t1=T1, t2=T2, hn=hn, fpre=fpre, fn=fn, gap_h=gap_h, gap_f=gap_f, h21=h21, h12=h12, f21=f21, score_h=sh_all, score_f=sf_all,
               chi_h=chi_h, chi_f=chi_f, best_h=bh, best_f=bf, sh=sh, sf=sf, rh=rh, inliers_h=inl_h, inliers_f=inl_f, hyp_r=hyp_r, hyp_t=hyp_t, hyp_valid=hyp_valid,
               hyp_good=np.array(good, np.int32), hyp_cos_parallax=np.array([c["cos_sel"] for c in crt], F32), hyp_parallax_deg=np.array(par, F32), check_rt=crt,
               success=bool(ok), model=model, hyp=hyp, th2=th2)
    if ok:
        out.update(r21=hyp_r[hyp], t21=hyp_t[hyp], p3d=crt[hyp]["vp3d"], triangulated=crt[hyp]["vb_good"])
    else:
        out.update(r21=np.zeros((3, 3), F32), t21=np.zeros(3, F32), p3d=np.zeros((n1, 3), F32), triangulated=np.zeros(n1, bool))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the device's Jacobi iterations, restated in float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def round_robin_pairs(r):
    """the four disjoint column pairs of round r = 0..8 over 9 columns (the tenth player of the circle method is the bye)"""
    out = []
    for k in range(1, 5):
        a, b = (r + k) % 9, (r + 9 - k) % 9
        out.append((min(a, b), max(a, b)))
    return out


def _butterfly16(x):
    """sum over the last axis (16 entries) the way sixteen lanes do it with xor shuffles 8, 4, 2, 1: every lane ends with the same bits"""
    idx = np.arange(16)
    for o in (8, 4, 2, 1):
        x = x + x[..., idx ^ o]
    return x[..., 0]


def _rotation(alpha, beta, gamma):
    with np.errstate(all="ignore"):
        zeta = (beta - alpha) / (2.0 * gamma)
        t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
        c = 1.0 / np.sqrt(1.0 + t * t)
        s = c * t
    skip = gamma == 0.0
    return np.where(skip, 1.0, c), np.where(skip, 0.0, s)


def jacobi_null9(A, sweeps):
    """(M, r <= 16, 9) float32 -> (M, 9) float64: one-sided Jacobi on the 9 columns (rows padded with zeros to 16), V alongside, round-robin
    rounds of four concurrent pairs; the column of V under the smallest column norm (the first of equals)"""
    A = np.asarray(A, F32)
    M, r = A.shape[0], A.shape[1]
    a = np.zeros((M, 9, 16))
    a[:, :, :r] = np.swapaxes(A.astype(F64), 1, 2)
    v = np.tile(np.eye(9), (M, 1, 1))      # [m, column, row]
    for _ in range(sweeps):
        for rnd in range(9):
            for p, q in round_robin_pairs(rnd):
                ap, aq, vp, vq = a[:, p].copy(), a[:, q].copy(), v[:, p].copy(), v[:, q].copy()
                c, s = _rotation(_butterfly16(ap * ap), _butterfly16(aq * aq), _butterfly16(ap * aq))
                c, s = c[:, None], s[:, None]
                a[:, p], a[:, q] = c * ap - s * aq, s * ap + c * aq
                v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
    n2 = np.zeros((M, 9))
    for i in range(16):
        n2 = n2 + a[:, :, i] * a[:, :, i]
    return v[np.arange(M), np.argmin(n2, axis=1)]


def jacobi_svd3(A, sweeps):
    """(M, 3, 3) float32 -> U (M, 3, 3), w (M, 3), Vt (M, 3, 3) float64: one-sided Jacobi on the columns, cyclic (0,1) (0,2) (1,2); singular
    values = column norms, sorted descending (stable); U's columns = the rotated columns over their norms"""
    a = np.ascontiguousarray(np.swapaxes(np.asarray(A, F32).astype(F64), -1, -2)).reshape(-1, 3, 3)      # [m, column, row]
    M = len(a)
    v = np.tile(np.eye(3), (M, 1, 1))
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            ap, aq, vp, vq = a[:, p].copy(), a[:, q].copy(), v[:, p].copy(), v[:, q].copy()
            alpha = ap[:, 0] * ap[:, 0] + ap[:, 1] * ap[:, 1] + ap[:, 2] * ap[:, 2]
            beta = aq[:, 0] * aq[:, 0] + aq[:, 1] * aq[:, 1] + aq[:, 2] * aq[:, 2]
            gamma = ap[:, 0] * aq[:, 0] + ap[:, 1] * aq[:, 1] + ap[:, 2] * aq[:, 2]
            c, s = _rotation(alpha, beta, gamma)
            c, s = c[:, None], s[:, None]
            a[:, p], a[:, q] = c * ap - s * aq, s * ap + c * aq
            v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
    w = np.sqrt(a[:, :, 0] * a[:, :, 0] + a[:, :, 1] * a[:, :, 1] + a[:, :, 2] * a[:, :, 2])
    order = np.argsort(-w, axis=1, kind="stable")
    rows = np.arange(M)[:, None]
    w, a, v = w[rows, order], a[rows, order], v[rows, order]
    with np.errstate(all="ignore"):
        u = a / w[:, :, None]
    return np.swapaxes(u, 1, 2), w, v      # U[m, row, column]; Vt[m, k, :] = column k of V


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


SCENE_KINDS = ("general", "planar", "planar_tilted", "forward", "rotation_only", "outliers_20", "few_inliers", "h_degenerate")


def scene(kind, n, seed, noise=0.5, K=K_DEFAULT):
    """two views of n points: keys1 (n1, 2), keys2 (n2, 2) float32, matches12 (n1) int32 with -1 gaps (n1 = n + n // 3 + 2, n2 = n1 + 5:
    unmatched keypoints in both frames, frame 2 in shuffled order), the motion R (3, 3), t (3) with x2 = R x1 + t"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    u = rng.uniform(40, 600, n)
    v = rng.uniform(40, 440, n)
    x, y = (u - cx) / fx, (v - cy) / fy
    R = _rot(*rng.normal(0, 0.02, 3))
    t = np.array([1.0, 0.1, 0.06])
    if kind in ("general", "outliers_20", "few_inliers"):
        z = rng.uniform(4, 9, n)
    elif kind == "planar":
        z = np.full(n, 5.0)
    elif kind == "planar_tilted":
        z = 5.0 / (1.0 + 0.35 * x + 0.2 * y)      # the plane 0.35 X + 0.2 Y + Z = 5
    elif kind == "forward":
        z = rng.uniform(4, 9, n)
        t = np.array([0.03, 0.02, 0.8])
    elif kind == "rotation_only":
        z = rng.uniform(4, 9, n)
        R = _rot(0.01, 0.06, -0.02)
        t = np.zeros(3)
    elif kind == "h_degenerate":
        z = np.full(n, 5.0)
        R = np.eye(3)
        t = np.array([0.0, 0.0, 1.0])      # H = K (I + t n^T / d) K^-1 with t along n: singular values 1, 1, 1.2
    else:
        raise ValueError(kind)
    X = np.stack([x * z, y * z, z], 1)
    X2 = X @ R.T + t[None, :]
    p1 = np.stack([u, v], 1) + rng.normal(0, noise, (n, 2))
    p2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1) + rng.normal(0, noise, (n, 2))
    wrong = {"outliers_20": 0.2, "few_inliers": 0.5}.get(kind, 0.0)
    if wrong:
        bad = rng.permutation(n)[:int(round(wrong * n))]
        p2[bad] = np.stack([rng.uniform(20, 620, len(bad)), rng.uniform(20, 460, len(bad))], 1)
    n1, n2 = n + n // 3 + 2, n + n // 3 + 7
    slots1 = np.sort(rng.permutation(n1)[:n])
    slots2 = rng.permutation(n2)[:n]
    keys1 = np.stack([rng.uniform(20, 620, n1), rng.uniform(20, 460, n1)], 1)
    keys2 = np.stack([rng.uniform(20, 620, n2), rng.uniform(20, 460, n2)], 1)
    keys1[slots1], keys2[slots2] = p1, p2
    m = np.full(n1, -1, np.int32)
    m[slots1] = slots2
    return dict(kind=kind, keys1=keys1.astype(F32), keys2=keys2.astype(F32), matches12=m, R=R, t=t, K=tuple(K), X=X, slots1=slots1)


def draw_sets(n, iterations, seed):
    """mvSets by the swap-with-the-back scheme, from numpy's generator"""
    rng = np.random.default_rng(seed)
    out = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            r = int(rng.integers(0, len(avail)))
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def rotation_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, F64) @ np.asarray(Rb, F64).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def direction_angle_deg(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    c = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def reprojection_px(res, sc):
    """largest reprojection error of the triangulated points in both views under the recovered motion"""
    tri = np.asarray(res["triangulated"], bool)
    if not tri.any():
        return 0.0
    fx, fy, cx, cy = sc["K"]
    P = np.asarray(res["p3d"], F64)[tri]
    R, t = np.asarray(res["r21"], F64).reshape(3, 3), np.asarray(res["t21"], F64).reshape(3)
    P2 = P @ R.T + t[None, :]
    k1 = sc["keys1"][tri].astype(F64)
    k2 = sc["keys2"][sc["matches12"][tri]].astype(F64)
    e1 = np.hypot(fx * P[:, 0] / P[:, 2] + cx - k1[:, 0], fy * P[:, 1] / P[:, 2] + cy - k1[:, 1])
    e2 = np.hypot(fx * P2[:, 0] / P2[:, 2] + cx - k2[:, 0], fy * P2[:, 1] / P2[:, 2] + cy - k2[:, 1])
    return float(max(e1.max(), e2.max()))


def margins(r, min_parallax=1.0, min_triangulated=50):
    """how far a restated run is from every decision a last bit could flip (test_scenes_are_screened)"""
    def lead(s):
        u = np.unique(s)[::-1]
        return float("inf") if len(u) < 2 or u[0] <= 0 else float((u[0] - u[1]) / u[0])
    use_h = r["rh"] > F32(0.40)
    fam = slice(4, 12) if use_h else slice(0, 4)
    good = r["hyp_good"][fam].astype(F64)
    n_inl = float(r["inliers_h"].sum() if use_h else r["inliers_f"].sum())
    best = good.max()
    counts = []
    if use_h and r["hyp_valid"][4]:
        second = np.sort(good)[-2]
        counts += [abs(second - 0.75 * best), abs(best - min_triangulated), abs(best - 0.9 * n_inl)]
    elif not use_h:
        counts += [abs(best - max(int(0.9 * n_inl), min_triangulated))] + [abs(g - 0.7 * best) for g in good if g != best]
        counts += [0.0] * (int((good == best).sum()) - 1 if best > 0 else 0)      # a tie for maxGood is decided by order: not decidable as a set
    k = int(np.argmax(good))
    par = float(r["hyp_parallax_deg"][fam][k])
    near = np.mean([c["near"].mean() if len(c["near"]) else 0.0 for c in r["check_rt"]])
    return dict(lead_h=lead(r["score_h"]), lead_f=lead(r["score_f"]), rh=float(abs(F64(r["rh"]) - 0.40)), counts=float(min(counts)) if counts else float("inf"),
                parallax=abs(par - min_parallax) / min_parallax if best > 0 else float("inf"), near=float(near), gap_h=float(r["gap_h"].min()), gap_f=float(r["gap_f"].min()))
