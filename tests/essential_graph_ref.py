"""Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1017-1339 with the vendored g2o) restated in numpy float64, operation by operation
in the order csrc/orbx_essential_graph.hip computes: the measurements, EdgeSim3's error log(C * v1 * v2^-1) with the four branches of Sim3::log
(sim3.h:148-230; W u = t by the adjugate, which stands in for W.lu().solve(t)), g2o's central differences through oplus, the block assembly in
edge order, the block-sparse LDL^T on the pattern of L with both substitutions, the Levenberg driver of optsim3_ref.optimize with lambda_init in
place of tau * maxDiagonal, and the pose / map-point write-back.  exp, sin, cos, log and acos are the kernels' own series (EgMath), restated too.

A set of Sim3s is an (n, 8) array [qx, qy, qz, qw, tx, ty, tz, s]; inside, (q, t, s) with lists of arrays, so that optsim3_ref's sim3_* functions
(elementwise arithmetic) run vectorised over the edges: an elementwise numpy operation rounds like the scalar one."""
import math

import numpy as np

from optsim3_ref import DBL_MAX, DELTA, EPS, SCALAR, _I3, _mat3, _rot, _skew, quat_from_R, quat_to_R, sim3_inverse, sim3_map, sim3_mul

THREADS = 256
MAX_TRIALS = 10


# ---- the elementary functions as the kernels pin them (EgMath): argument reductions and Horner series of IEEE operations, bit for bit -------------
_EXP_C = (1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889, 0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10)
_SIN_C = (1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15, -8.22063524662433e-18)
_COS_C = (1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07, 2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14, -1.5619206968586225e-16, 4.110317623312165e-19)
_LOG_C = (2.0, 0.6666666666666666, 0.4, 0.2857142857142857, 0.2222222222222222, 0.18181818181818182, 0.15384615384615385, 0.13333333333333333, 0.11764705882352941, 0.10526315789473684, 0.09523809523809523, 0.08695652173913043, 0.08)
_ASIN_C = (1.0, 0.16666666666666666, 0.075, 0.044642857142857144, 0.030381944444444444, 0.022372159090909092, 0.017352764423076924, 0.01396484375, 0.011551800896139705, 0.009761609529194078, 0.008390335809616815, 0.0073125258735988454, 0.006447210311889649, 0.005740037670841924, 0.005153309682319905, 0.004660143486915096, 0.004240907093679363, 0.003880964558837669, 0.0035692053938259347, 0.003297059503473485, 0.0030578216492580306, 0.002846178401108942, 0.00265787063820729, 0.0024894486782468836, 0.002338091892111975, 0.0022014739737101384, 0.0020776610325181676, 0.0019650336162772837)
_INV_LN2, _LN2_HI, _LN2_LO = 1.44269504088896338700e+00, 6.93147180369123816490e-01, 1.90821492927058770002e-10
_INV_PIO2, _PIO2_HI, _PIO2_LO = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050650619224932e-11


def _horner(c, x):
    p = c[-1]
    for n in range(len(c) - 2, -1, -1):
        p = p * x + c[n]
    return p


def eg_exp(x):
    x = np.asarray(x, np.float64)
    k = np.rint(x * _INV_LN2)
    r = (x - k * _LN2_HI) - k * _LN2_LO
    return np.ldexp(_horner(_EXP_C, r), k.astype(np.int64).astype(np.int32))


def eg_sincos(t):
    t = np.asarray(t, np.float64)
    k = np.rint(t * _INV_PIO2)
    r = (t - k * _PIO2_HI) - k * _PIO2_LO
    r2 = r * r
    s, c = r * _horner(_SIN_C, r2), _horner(_COS_C, r2)
    q = k.astype(np.int64) & 3
    return np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c))), np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))


def eg_log(x):
    m, e = np.frexp(np.asarray(x, np.float64))
    low = m < 0.70710678118654752440
    m, e = np.where(low, m * 2.0, m), (e - low).astype(np.float64)
    f = (m - 1.0) / (m + 1.0)
    r = f * _horner(_LOG_C, f * f)
    return e * _LN2_HI + (e * _LN2_LO + r)


def eg_acos(d):
    d = np.asarray(d, np.float64)
    hi, lo = d > 0.5, d < -0.5
    z2 = np.where(hi, (1.0 - d) * 0.5, np.where(lo, (1.0 + d) * 0.5, d * d))
    z = np.where(hi | lo, np.sqrt(z2), d)
    a = z * _horner(_ASIN_C, z2)
    return np.where(hi, a + a, np.where(lo, 3.141592653589793 - (a + a), 1.5707963267948966 - a))


def sim3_exp(u):
    """optsim3_ref.sim3_exp (Sim3(const Vector7d &), sim3.h:70-142) with the pinned exp, sin and cos; -> (S, branch)"""
    u = [float(v) for v in u]
    w, sigma = u[0:3], u[6]
    theta = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    Om = _skew(w)
    Om2 = _mat3(Om, Om)
    s = float(eg_exp(sigma))
    sn, cs = [float(v) for v in eg_sincos(theta)]
    small = theta < EPS
    if small:
        R = [(_I3[k] + Om[k]) + Om2[k] for k in range(9)]
    else:
        ca, cb = sn / theta, (1.0 - cs) / (theta * theta)
        R = [(_I3[k] + ca * Om[k]) + cb * Om2[k] for k in range(9)]
    if abs(sigma) < EPS:
        C = 1.0
        if small:
            A, B = 1.0 / 2.0, 1.0 / 6.0
        else:
            theta2 = theta * theta
            A = (1.0 - cs) / theta2
            B = (theta - sn) / (theta2 * theta)
    else:
        C = (s - 1.0) / sigma
        sigma2 = sigma * sigma
        if small:
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
        else:
            a, b, theta2 = s * sn, s * cs, theta * theta
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2
    W = [(A * Om[k] + B * Om2[k]) + C * _I3[k] for k in range(9)]
    t = [(W[3 * i] * u[3] + W[3 * i + 1] * u[4]) + W[3 * i + 2] * u[5] for i in range(3)]
    return (quat_from_R(R), t, s), (abs(sigma) < EPS, small)


def unpack(V):
    V = np.asarray(V, np.float64).reshape(-1, 8)
    return ([V[:, 0], V[:, 1], V[:, 2], V[:, 3]], [V[:, 4], V[:, 5], V[:, 6]], V[:, 7])


def pack(S, n):
    q, t, s = S
    return np.stack([np.broadcast_to(np.asarray(a, np.float64), (n,)) for a in list(q) + list(t) + [s]], 1).copy()


def take(S, idx):
    q, t, s = S
    return ([a[idx] for a in q], [a[idx] for a in t], s[idx])


def one(V, i):
    """row i as a scalar Sim3 of python floats"""
    r = [float(v) for v in np.asarray(V)[i]]
    return (r[0:4], r[4:7], r[7])


def sim3_log_v(S):
    """Sim3::log() over a set -> (n, 7), branch flags (|sigma| < eps, d > 1 - eps)"""
    q, t, s = S
    with np.errstate(all="ignore"):
        sigma = eg_log(s)
        R = quat_to_R(q)
        d = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
        dR = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
        near, small = d > 1.0 - EPS, np.abs(sigma) < EPS
        theta = eg_acos(d)
        sn, cs = eg_sincos(theta)
        f = theta / (2.0 * np.sqrt(1.0 - d * d))
        om = [np.where(near, 0.5 * dR[k], f * dR[k]) for k in range(3)]
        theta2, sigma2 = theta * theta, sigma * sigma
        A_sf, B_sf = (1.0 - cs) / theta2, (theta - sn) / (theta2 * theta)
        C_l = (s - 1.0) / sigma
        A_ln, B_ln = ((sigma - 1.0) * s + 1.0) / sigma2, (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
        a, b, c = s * sn, s * cs, theta2 + sigma2
        A_lf = (a * sigma + (1.0 - b) * theta) / (theta * c)
        B_lf = ((C_l - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2
        A = np.where(small, np.where(near, 1.0 / 2.0, A_sf), np.where(near, A_ln, A_lf))
        B = np.where(small, np.where(near, 1.0 / 6.0, B_sf), np.where(near, B_ln, B_lf))
        C = np.where(small, 1.0, C_l)
        Om = _skew(om)
        Om2 = _mat3(Om, Om)
        I3 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        W = [(A * Om[k] + B * Om2[k]) + C * I3[k] for k in range(9)]
        a00, a01, a02 = W[4] * W[8] - W[5] * W[7], W[2] * W[7] - W[1] * W[8], W[1] * W[5] - W[2] * W[4]
        a10, a11, a12 = W[5] * W[6] - W[3] * W[8], W[0] * W[8] - W[2] * W[6], W[2] * W[3] - W[0] * W[5]
        a20, a21, a22 = W[3] * W[7] - W[4] * W[6], W[1] * W[6] - W[0] * W[7], W[0] * W[4] - W[1] * W[3]
        det = (W[0] * a00 + W[1] * a10) + W[2] * a20
        u = [((a00 * t[0] + a01 * t[1]) + a02 * t[2]) / det, ((a10 * t[0] + a11 * t[1]) + a12 * t[2]) / det, ((a20 * t[0] + a21 * t[1]) + a22 * t[2]) / det]
    n = np.shape(sigma)[0]
    return np.stack([np.broadcast_to(v, (n,)) for v in om + u + [sigma]], 1), (small, near)


def edge_error(C, v1, v2):
    """EdgeSim3::computeError over the edges: log((C * v1) * v2^-1) -> (E, 7)"""
    return sim3_log_v(sim3_mul(sim3_mul(C, v1), sim3_inverse(v2)))[0]


def oplus(S, u, fix_scale):
    u = [float(v) for v in u]
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u)[0], S)


class Graph:
    """est, meas (N, 8); fixed; edges (E, 3) int = (i, j, kind); fix_scale; optionally points (M, 3) float32 and ref (M) int32"""

    def __init__(self, est, meas, fixed, edges, fix_scale=False, points=None, ref=None):
        self.est = np.ascontiguousarray(est, np.float64).reshape(-1, 8)
        self.meas = self.est.copy() if meas is None else np.ascontiguousarray(meas, np.float64).reshape(-1, 8)
        self.N, self.fixed, self.fix_scale = len(self.est), int(fixed), bool(fix_scale)
        self.edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
        self.E = len(self.edges)
        self.points = np.zeros((0, 3), np.float32) if points is None else np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.ref = np.zeros(0, np.int32) if ref is None else np.ascontiguousarray(ref, np.int32).reshape(-1)

    def with_poses(self, est, meas):
        return Graph(est, meas, self.fixed, self.edges, self.fix_scale, self.points, self.ref)


def measurements(G):
    """Sji = Sjw * Swi per edge, from est (kind 0) or meas (kind 1) -> (E, 8)"""
    if G.E == 0:
        return np.zeros((0, 8))
    i, j, kind = G.edges[:, 0], G.edges[:, 1], G.edges[:, 2]
    src = np.where((kind == 0)[:, None], G.est[i], G.meas[i]), np.where((kind == 0)[:, None], G.est[j], G.meas[j])
    return pack(sim3_mul(unpack(src[1]), sim3_inverse(unpack(src[0]))), G.E)


# ---- symbolic ---------------------------------------------------------------------------------------------------------------------------
def symbolic(G, order=None):
    """Block symbolic elimination in `order` (vertex indices of the free keyframes; default: ascending) -> dict(pos (N), order, nf, nOff, colPtr,
    rowIdx (the blocks of L below the diagonal, by column), fill = blocks of L's lower triangle with the diagonal, aPtr / aItem (per block the
    contributing edges in edge order, edge << 2 | code), targets (per column, the blocks its pairs (a >= b) update))"""
    N = G.N
    order = [v for v in range(N) if v != G.fixed] if order is None else [int(v) for v in order]
    assert sorted(order) == [v for v in range(N) if v != G.fixed]
    nf = len(order)
    pos = -np.ones(N, np.int64)
    pos[order] = np.arange(nf)
    col = [set() for _ in range(nf)]
    pe = pos[G.edges[:, :2]] if G.E else np.zeros((0, 2), np.int64)
    for pi, pj in pe:
        if pi >= 0 and pj >= 0:
            col[min(pi, pj)].add(int(max(pi, pj)))
    for q in range(nf):
        rows = sorted(col[q])
        if len(rows) > 1:
            col[rows[0]].update(rows[1:])
        col[q] = rows
    colPtr = np.zeros(nf + 1, np.int64)
    colPtr[1:] = np.cumsum([len(c) for c in col])
    rowIdx = np.array([r for c in col for r in c], np.int64)
    nOff = len(rowIdx)
    index = {}
    for q in range(nf):
        for k, p in enumerate(col[q]):
            index[(p, q)] = nf + int(colPtr[q]) + k
    lists = [[] for _ in range(nf + nOff)]
    for e, (pi, pj) in enumerate(pe):
        if pi >= 0:
            lists[pi].append(e << 2 | 0)
        if pj >= 0:
            lists[pj].append(e << 2 | 1)
        if pi >= 0 and pj >= 0:
            lists[index[(pi, pj)] if pi > pj else index[(pj, pi)]].append(e << 2 | (2 if pi > pj else 3))
    aPtr = np.zeros(nf + nOff + 1, np.int64)
    aPtr[1:] = np.cumsum([len(c) for c in lists])
    aItem = np.array([v for c in lists for v in c], np.int64)
    targets = []
    for q in range(nf):
        rows = col[q]
        ia, ib = np.tril_indices(len(rows))
        targets.append((ia, ib, np.array([rows[a] if a == b else index[(rows[a], rows[b])] for a, b in zip(ia, ib)], np.int64)))
    return dict(pos=pos, order=np.array(order, np.int64), nf=nf, nOff=nOff, colPtr=colPtr, rowIdx=rowIdx, fill=nf + nOff, aPtr=aPtr, aItem=aItem, targets=targets)


# ---- one linearisation ------------------------------------------------------------------------------------------------------------------
def _rows_sum(A, B):
    """sum over the seven error rows, in row order, of A[:, k, r] * B[:, k, c] -> (E, 7, 7)"""
    t = A[:, 0, :, None] * B[:, 0, None, :]
    for k in range(1, 7):
        t = t + A[:, k, :, None] * B[:, k, None, :]
    return t


def errors_at(G, M, V):
    V = np.asarray(V, np.float64).reshape(-1, 8)
    return edge_error(unpack(M), unpack(V[G.edges[:, 0]]), unpack(V[G.edges[:, 1]]))


def strided_tree_sum(v):
    """thread t of 256 adds v[t], v[t + 256], ... to 0; then a binary tree over the partial sums"""
    v = np.asarray(v, np.float64).reshape(-1)
    T = np.zeros(THREADS)
    for j in range(0, len(v), THREADS):
        c = v[j:j + THREADS]
        T[:len(c)] = T[:len(c)] + c
    s = THREADS // 2
    while s > 0:
        T[:s] = T[:s] + T[s:2 * s]
        s //= 2
    return float(T[0])


def chi2_of(err):
    c = err[:, 0] * err[:, 0]
    for k in range(1, 7):
        c = c + err[:, k] * err[:, k]
    return c


def linearize(G, V, M=None, sym=None):
    """One linearisation at the estimates V (N, 8) with the measurements M (default: restated) -> dict(meas, errors (E,7), chi2, jac (E,2,7,7), Hb
    (blocks on the pattern of L), bp (nf,7), h_diag (N,7,7), h_off (E,7,7), b (N,7))"""
    V = np.asarray(V, np.float64).reshape(-1, 8)
    M = measurements(G) if M is None else np.asarray(M, np.float64).reshape(-1, 8)
    sym = symbolic(G) if sym is None else sym
    E, nf, pos = G.E, sym["nf"], sym["pos"]
    C, Vi, Vj = unpack(M), unpack(V[G.edges[:, 0]]), unpack(V[G.edges[:, 1]])
    err = edge_error(C, Vi, Vj)
    J = np.zeros((E, 2, 7, 7))
    for v in range(2):
        for d in range(7):
            e = []
            for val in (DELTA, -DELTA):
                u = [0.0] * 7
                u[d] = val
                e.append(edge_error(C, oplus(Vi, u, G.fix_scale), Vj) if v == 0 else edge_error(C, Vi, oplus(Vj, u, G.fix_scale)))
            J[:, v, :, d] = SCALAR * (e[0] - e[1])
        J[pos[G.edges[:, v]] < 0, v] = 0.0
    J0, J1 = J[:, 0], J[:, 1]
    terms = [_rows_sum(J0, J0), _rows_sum(J1, J1), _rows_sum(J0, J1), _rows_sum(J1, J0)]
    bterms = []
    for A in (J0, J1):
        t = A[:, 0, :] * (-err[:, 0:1])
        for k in range(1, 7):
            t = t + A[:, k, :] * (-err[:, k:k + 1])
        bterms.append(t)
    nL = nf + sym["nOff"]
    Hb, bp = np.zeros((nL, 7, 7)), np.zeros((nf, 7))
    aPtr, aItem = sym["aPtr"], sym["aItem"]
    blk = np.repeat(np.arange(nL), np.diff(aPtr))
    rank = np.arange(len(aItem)) - aPtr[blk]
    edge, code = aItem >> 2, aItem & 3
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        for c in range(4):
            sel = (rank == r) & (code == c)
            Hb[blk[sel]] = Hb[blk[sel]] + terms[c][edge[sel]]
            if c < 2:
                bp[blk[sel]] = bp[blk[sel]] + bterms[c][edge[sel]]
    h_diag, b, h_off = np.zeros((G.N, 7, 7)), np.zeros((G.N, 7)), np.zeros((E, 7, 7))
    h_diag[sym["order"]], b[sym["order"]] = Hb[:nf], bp
    index = {}
    for q in range(nf):
        for k in range(int(sym["colPtr"][q]), int(sym["colPtr"][q + 1])):
            index[(int(sym["rowIdx"][k]), q)] = nf + k
    for e in range(E):
        pi, pj = int(pos[G.edges[e, 0]]), int(pos[G.edges[e, 1]])
        if pi >= 0 and pj >= 0:
            h_off[e] = Hb[index[(pi, pj)]] if pi > pj else Hb[index[(pj, pi)]].T
    return dict(meas=M, errors=err, chi2=strided_tree_sum(chi2_of(err)), jac=J, Hb=Hb, bp=bp, h_diag=h_diag, h_off=h_off, b=b, sym=sym)


# ---- the block-sparse solve -------------------------------------------------------------------------------------------------------------
def _ldlt7(A):
    """scalar LDL^T of one 7x7 block without pivoting -> (unit lower L in A's lower triangle, d, ok)"""
    A = [[np.float64(A[i][j]) for j in range(7)] for i in range(7)]
    Dg, ok = [np.float64(0.0)] * 7, True
    for q in range(7):
        LD = [0.0] * 7
        dq = A[q][q]
        for k in range(q):
            LD[k] = A[q][k] * Dg[k]
            dq = dq - A[q][k] * LD[k]
        ok = ok and bool(dq > 0.0) and bool(np.isfinite(dq))
        Dg[q] = dq
        for i in range(q + 1, 7):
            l = A[i][q]
            for k in range(q):
                l = l - A[i][k] * LD[k]
            A[i][q] = l / dq
    return np.array(A, np.float64), np.array(Dg, np.float64), ok


def sparse_solve(sym, Hb, bp, lam):
    """(H + lam I) x = b by the block LDL^T of k_eg_solve -> (ok, x (nf, 7) in elimination order)"""
    nf, colPtr, rowIdx = sym["nf"], sym["colPtr"], sym["rowIdx"]
    L = np.array(Hb, np.float64)
    di = np.arange(7)
    L[:nf, di, di] = L[:nf, di, di] + lam
    y, dv, ok = np.array(bp, np.float64), np.zeros((nf, 7)), True
    with np.errstate(all="ignore"):
        for j in range(nf):
            cs, ce = int(colPtr[j]), int(colPtr[j + 1])
            A, Dg, okj = _ldlt7(L[j])
            ok = ok and okj
            z = [np.float64(0.0)] * 7
            for i in range(7):
                s = y[j, i]
                for k in range(i):
                    s = s - A[i, k] * z[k]
                z[i] = s
            L[j], dv[j], y[j] = A, Dg, z
            if ce == cs:
                continue
            blocks = L[nf + cs:nf + ce]
            w = np.zeros_like(blocks)
            for c in range(7):
                s = blocks[:, :, c]
                for k in range(c):
                    s = s - w[:, :, k] * A[c, k]
                w[:, :, c] = s
            Lb = w / Dg[None, None, :]
            L[nf + cs:nf + ce] = Lb
            ia, ib, tg = sym["targets"][j]
            acc = L[tg]
            for k in range(7):
                acc = acc - w[ia][:, :, k, None] * Lb[ib][:, None, :, k]
            L[tg] = acc
            rows = rowIdx[cs:ce]
            acc = y[rows]
            for k in range(7):
                acc = acc - Lb[:, :, k] * z[k]
            y[rows] = acc
        y = y / dv
        x = np.zeros((nf, 7))
        for j in range(nf - 1, -1, -1):
            cs, ce = int(colPtr[j]), int(colPtr[j + 1])
            acc = y[j].copy()
            for a in range(cs, ce):
                la, xa = L[nf + a], x[rowIdx[a]]
                for k in range(7):
                    acc = acc - la[k, :] * xa[k]
            A = L[j]
            for i in range(6, -1, -1):
                s = acc[i]
                for k in range(i + 1, 7):
                    s = s - A[k, i] * x[j, k]
                x[j, i] = s
    return ok, x


def dense_system(sym, Hb, bp):
    """the same system as a dense symmetric matrix (elimination order) -> H (7 nf, 7 nf), b"""
    nf = sym["nf"]
    H = np.zeros((7 * nf, 7 * nf))
    for p in range(nf):
        H[7 * p:7 * p + 7, 7 * p:7 * p + 7] = np.tril(Hb[p]) + np.tril(Hb[p], -1).T
    for q in range(nf):
        for k in range(int(sym["colPtr"][q]), int(sym["colPtr"][q + 1])):
            p = int(sym["rowIdx"][k])
            H[7 * p:7 * p + 7, 7 * q:7 * q + 7] = Hb[nf + k]
            H[7 * q:7 * q + 7, 7 * p:7 * p + 7] = Hb[nf + k].T
    return H, np.asarray(bp).reshape(-1)


def scale_sum(x, b, lam):
    x, b = np.asarray(x).reshape(-1), np.asarray(b).reshape(-1)
    return strided_tree_sum(x * (lam * x + b))


def apply_update(G, sym, V, x):
    """oplus of every free vertex: Sim3(x) * estimate, x[6] = 0 under fix_scale"""
    out = np.array(V, np.float64)
    for p, v in enumerate(sym["order"]):
        out[v] = pack(oplus(one(V, v), x[p], G.fix_scale), 1)[0]
    return out


# ---- the Levenberg driver ---------------------------------------------------------------------------------------------------------------
def optimize(G, iterations=20, lambda_init=1e-16, M=None, V0=None):
    """-> dict(est (N,8), chi2 (initial, final), iterations, ended, log = [(trials, chi2, lambda, rho)] per iteration, accepts = per iteration the
    accept / reject flags of its trials, gains = per trial chi2 - trial chi2 (what rho's sign decides; None on a failed solve), progress = per iteration
    that did not end the run (ini - cur) * 1e3 - ini (what the three-strikes rule decides), sym)"""
    sym = symbolic(G)
    V = np.array(G.est if V0 is None else V0, np.float64)
    out = dict(est=V, chi2=(0.0, 0.0), iterations=0, ended="iterations", log=[], accepts=[], gains=[], progress=[], sym=sym)
    if G.E == 0:
        return out
    M = measurements(G) if M is None else M
    cur = chi0 = strided_tree_sum(chi2_of(errors_at(G, M, V)))
    lam, ni, n_bad = float(lambda_init), 2.0, 0
    x = np.zeros((sym["nf"], 7))
    for it in range(iterations):
        lin = linearize(G, V, M, sym)
        ini = cur
        qmax, acc = 0, []
        while True:
            ok, xx = sparse_solve(sym, lin["Hb"], lin["bp"], lam)
            if ok:
                x = xx
                if G.fix_scale:
                    x[:, 6] = 0.0
            T = apply_update(G, sym, V, x)
            temp = strided_tree_sum(chi2_of(errors_at(G, M, T))) if ok else DBL_MAX
            scale = scale_sum(x, lin["bp"], lam) + 1e-3
            with np.errstate(all="ignore"):
                rho = float((np.float64(cur) - np.float64(temp)) / np.float64(scale))
            out["gains"].append(cur - temp if ok else None)
            if rho > 0.0 and math.isfinite(temp):
                t2r = 2.0 * rho - 1.0
                lam = lam * max(1.0 / 3.0, min(1.0 - (t2r * t2r) * t2r, 2.0 / 3.0))
                ni, cur, V = 2.0, temp, T
                acc.append(True)
            else:
                lam, ni = lam * ni, ni * 2.0
                acc.append(False)
            qmax += 1
            if not (rho < 0.0 and qmax < MAX_TRIALS):
                break
        out["log"].append((qmax, cur, lam, rho))
        out["accepts"].append(acc)
        out["iterations"] += 1
        if qmax == MAX_TRIALS or rho == 0.0:
            out["ended"] = "trials" if qmax == MAX_TRIALS else "rho0"
            break
        out["progress"].append((ini - cur) * 1e3 - ini)
        n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
        if n_bad >= 3:
            out["ended"] = "three"
            break
    out["est"], out["chi2"] = V, (chi0, cur)
    return out


# ---- write-back -------------------------------------------------------------------------------------------------------------------------
def write_back(G, V):
    """-> Tiw (N, 3, 4) float32 = [R | t / s], inv (N, 8) = vCorrectedSwc, points (M, 3) float32"""
    V = np.asarray(V, np.float64).reshape(-1, 8)
    S = unpack(V)
    R = quat_to_R(S[0])
    f = 1.0 / S[2]
    Tiw = np.zeros((G.N, 3, 4), np.float32)
    Tiw[:, :, :3] = np.moveaxis(R, 2, 0).astype(np.float32)
    for r in range(3):
        Tiw[:, r, 3] = (S[1][r] * f).astype(np.float32)
    inv = pack(sim3_inverse(S), G.N)
    ident = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    has = G.ref >= 0
    idx = np.where(has, G.ref, 0)
    Srw = np.where(has[:, None], G.est[idx], ident)
    Swr = np.where(has[:, None], inv[idx], ident)
    p = G.points.astype(np.float64)
    a = sim3_map(unpack(Srw), [p[:, 0], p[:, 1], p[:, 2]])
    b = sim3_map(unpack(Swr), a)
    pts = np.stack(b, 1).astype(np.float32) if len(p) else np.zeros((0, 3), np.float32)
    return Tiw, inv, pts


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def _sim3_of(R, t, s):
    return np.array(quat_from_R(R) + [float(v) for v in t] + [float(s)])


def make_scene(N, seed, fix_scale=False, K=None, band=3, loop_nb=2, old_loop=False, duplicate=False, isolated=False, fixed=0, points=0, scale_drift=(0.03, 0.02)):
    """A closed trajectory of N keyframes with accumulated drift (per step: rotation sigma 0.03 rad, translation sigma 0.08, log-scale 0.03 +- 0.02, no
    scale drift under fix_scale).  The keyframes are on a circle looking along it; the last returns to the first (the loop keyframe, vertex `fixed`
    when N allows).  The last K keyframes are corrected as CorrectLoop does: est = drifted pose * (drifted current)^-1 * true current; meas keeps the
    drifted pose.  Edges: kind 0 from the corrected keyframes to the loop keyframe and its `loop_nb` neighbours; parents (i, i - 1), covisibles
    (i, i - d), d = 2..band, kind 1; optionally an older kind-1 loop edge in the middle (old_loop = True; an integer above 1 spreads that many over the
    trajectory), a LoopConnections edge on a spanning-tree pair and a repeated parent edge, one isolated vertex (no edge at all).  scale_drift = mean
    and sigma of the log-scale drift per step.  -> Graph, truth (N, 8)"""
    g = np.random.default_rng(seed)
    K = max(1, min(N - 1, N // 8 if K is None else K))
    truth, drift = [], []
    Sd = None
    for i in range(N):
        ang = 2.0 * math.pi * i / max(N, 3)
        Rwc = _rot([0.0, 0.0, 1.0], ang)
        twc = np.array([math.cos(ang), math.sin(ang), 0.0]) * (0.15 * N + 1.0)
        Rcw, tcw = Rwc.T, -Rwc.T @ twc
        truth.append((Rcw, tcw, 1.0))
        if i == 0:
            Sd = (Rcw, tcw, 1.0)
        else:
            Rp, tp, _ = truth[i - 1]
            Rrel, trel = Rcw @ Rp.T, tcw - Rcw @ Rp.T @ tp
            dR = _rot(g.normal(size=3), float(g.normal() * 0.03))
            dt = g.normal(size=3) * 0.08
            ds = 1.0 if fix_scale else math.exp(scale_drift[0] + scale_drift[1] * float(g.normal()))
            Re, te, se = dR @ Rrel, trel + dt, ds                      # the drifted relative motion, a similarity
            Sd = (Re @ Sd[0], se * (Re @ Sd[1]) + te, se * Sd[2])
        drift.append(Sd)
    meas = np.stack([_sim3_of(*d) for d in drift])
    est = meas.copy()
    cur = N - 1
    tru = np.stack([_sim3_of(*t) for t in truth])
    if N > 2:
        # corrected current pose: the true one (the loop's Sim3 measurement); the K - 1 before it follow rigidly: Siw_corr = Sic * Scw_corr
        Scw_corr, Swc = one(tru, cur), sim3_inverse(one(meas, cur))
        for i in range(N - K, N):
            est[i] = pack(sim3_mul(sim3_mul(one(meas, i), Swc), Scw_corr), 1)[0]
    elif N == 2:
        est[1] = tru[1] if fixed == 0 else est[1]
    edges = []
    iso = N // 2 + 1 if isolated else -1
    for i in range(N - K, N):
        for j in range(0, min(loop_nb + 1, N - K)):
            if i != j and iso not in (i, j):
                edges.append((i, j, 0))
    for i in range(1, N):
        for d in range(1, band + 1):
            j = i - d
            if j < 0 or iso in (i, j):
                continue
            if d > 1 and i >= N - K and j <= loop_nb:
                continue
            edges.append((i, j, 1))
    if old_loop and N >= 40:
        c = int(old_loop)
        if c == 1:
            edges.append((2 * N // 3, N // 4, 1))
        else:
            for k in range(c):
                i = (N - 2 * K) * (k + 1) // (c + 1)
                edges.append((i + (N - 2 * K) // (2 * c + 2), max(i - (N - 2 * K) // (2 * c + 2), 0), 1))
    if duplicate and N >= 4 and K >= 2:      # a LoopConnections edge on a spanning-tree pair inside the corrected set, and a parent edge twice
        edges.append((N - 1, N - 2, 0))
        edges.append((3, 2, 1))
    pts = ref = None
    if points:
        ref = g.integers(-1, N, points).astype(np.int32)
        ref[0] = -1
        pts = g.normal(size=(points, 3)).astype(np.float32) * 3.0
    return Graph(est, meas, min(fixed, N - 1), np.array(edges, np.int32).reshape(-1, 3), fix_scale, pts, ref), tru


def relative(V, i, j):
    """Sij = Siw * Sjw^-1 as (R, t, s)"""
    S = sim3_mul(one(V, i), sim3_inverse(one(V, j)))
    return quat_to_R(S[0]), np.array(S[1]), S[2]
