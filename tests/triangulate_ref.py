"""Expected values of the new-map-point geometry (orbx_triangulate_matches / orbx_create_new_map_points), independent of the code under test.

A numpy restatement of the per-match body of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:423-596) and of
KeyFrame::UnprojectStereo (src/KeyFrame.cc:805-827) from their stated semantics - NOT the reference and not compiled from it:
    float32 where the reference computes in float; Mat::dot and cv::norm accumulate in float64 from 0; invz = float32(1.0 / float64(z));
    the 3-term matrix products go left to right in float32; one operation per numpy call (over all matches at once), so nothing is fused
    or promoted.  The null vector of the float32 A comes from numpy.linalg.svd in float64 (x3d) and, for the error yardstick, in float32
    (x3d32).  UnprojectStereo reads the RAW keypoint; the second keyframe's stereo reprojection uses the FIRST keyframe's mbf.
`near` marks the matches that sit on a threshold (module constants COS_EPS / REL_EPS): a different last bit may flip them legitimately.

Also: the same one-sided Jacobi the device runs, restated in float64 (jacobi_null), the scene generators of tests/test_new_map_points.py and
the sequential chain over neighbours built from existing pieces (oracle_lib.search_for_triangulation + triangulate + mask update)."""
import numpy as np

F32, F64 = np.float32, np.float64
NONE, TRIANGULATED, STEREO1, STEREO2, LOW_PARALLAX, W_ZERO, DEPTH_INVALID, BEHIND1, BEHIND2, REPROJ1, REPROJ2, DIST_ZERO, SCALE = range(13)
NAMES = ("NONE", "TRIANGULATED", "STEREO1", "STEREO2", "LOW_PARALLAX", "W_ZERO", "DEPTH_INVALID", "BEHIND1", "BEHIND2", "REPROJ1", "REPROJ2", "DIST_ZERO", "SCALE")
COS_EPS = 1e-5      # a cosine comparison whose two sides are this close
REL_EPS = 1e-3      # any other comparison, relative

SF = np.array([1.0, 1.2, 1.44, 1.728, 2.0736, 2.48832, 2.985984, 3.5831808], F32)
SIGMA2 = (SF * SF).astype(F32)


def make_geom(T, fx=500.0, fy=500.0, cx=320.0, cy=240.0, mbf=40.0, scale_factor=1.2, sf=SF, sigma2=SIGMA2):
    """pose and calibration of one keyframe from a 4x4 (or 3x4) Tcw, the way KeyFrame keeps them: invfx = 1/fx in float, mb = mbf/fx,
    Ow = -Rwc*tcw as a float 3-term product"""
    T = np.asarray(T, F64)[:3, :4].astype(F32)
    R, t = T[:, :3], T[:, 3]
    Rwc = R.T
    ow = -(F32(Rwc[:, 0] * t[0]) + F32(Rwc[:, 1] * t[1]) + F32(Rwc[:, 2] * t[2]))
    return dict(tcw=np.ascontiguousarray(T), center=ow.astype(F32), fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy), invfx=F32(F32(1.0) / F32(fx)), invfy=F32(F32(1.0) / F32(fy)),
                mb=F32(F32(mbf) / F32(fx)), mbf=F32(mbf), scale_factor=F32(scale_factor), scale_factors=np.asarray(sf, F32), level_sigma2=np.asarray(sigma2, F32))


def _dot3(a, b):
    """Mat::dot of (M,3) float32 rows: products and sums in float64, from 0"""
    s = a[:, 0].astype(F64) * b[:, 0].astype(F64)
    s = s + a[:, 1].astype(F64) * b[:, 1].astype(F64)
    s = s + a[:, 2].astype(F64) * b[:, 2].astype(F64)
    return s


def _norm3(a):
    return np.sqrt(_dot3(a, a))


def _rwc_times(T, x, y, z):
    """Rwc * (x, y, z) with Rwc = Rcw^T: 3-term float32 products left to right -> (M,3)"""
    out = []
    for i in range(3):
        s = T[0, i] * x
        s = s + T[1, i] * y
        s = s + T[2, i] * z
        out.append(s.astype(F32))
    return np.stack(out, 1)


def _row_dot_plus(T, r, X):
    """float32(Rcw.row(r).dot(x3Dt) + tcw(r)): float64 dot plus a float"""
    row = np.broadcast_to(T[r, :3], X.shape)
    return (_dot3(row, X) + F64(T[r, 3])).astype(F32)


def _unproject(g, o, idx):
    z = o["depth"][idx].astype(F32)
    raw = o["raw"] if o.get("raw") is not None else np.stack([o["kps"]["x"], o["kps"]["y"]], 1)
    u, v = raw[idx, 0].astype(F32), raw[idx, 1].astype(F32)
    x = (u - g["cx"]) * z
    x = x * g["invfx"]
    y = (v - g["cy"]) * z
    y = y * g["invfy"]
    X = _rwc_times(g["tcw"], x, y, z) + g["center"][None, :]
    return X.astype(F32), z > 0


def build_A(g1, g2, xn1x, xn1y, xn2x, xn2y):
    T1, T2 = g1["tcw"], g2["tcw"]
    A = np.empty((len(xn1x), 4, 4), F32)
    A[:, 0] = xn1x[:, None] * T1[2][None, :] - T1[0][None, :]
    A[:, 1] = xn1y[:, None] * T1[2][None, :] - T1[1][None, :]
    A[:, 2] = xn2x[:, None] * T2[2][None, :] - T2[0][None, :]
    A[:, 3] = xn2y[:, None] * T2[2][None, :] - T2[1][None, :]
    return A


def jacobi_null(A, sweeps):
    """the device's null vector: one-sided (Hestenes) Jacobi in float64 on the columns of the float32 A (M,4,4), cyclic over the six pairs,
    `sweeps` times; the column of V under the smallest column norm (the first of equals) -> (M,4) float64"""
    a = np.ascontiguousarray(np.swapaxes(A.astype(F64), 1, 2))      # [m, column, row]
    M = len(a)
    v = np.tile(np.eye(4), (M, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(3):
                for q in range(p + 1, 4):
                    alpha = beta = gamma = np.zeros(M)
                    for r in range(4):
                        alpha = alpha + a[:, p, r] * a[:, p, r]
                        beta = beta + a[:, q, r] * a[:, q, r]
                        gamma = gamma + a[:, p, r] * a[:, q, r]
                    zeta = (beta - alpha) / (2.0 * gamma)
                    t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = c * t
                    skip = gamma == 0.0
                    c, s = np.where(skip, 1.0, c)[:, None], np.where(skip, 0.0, s)[:, None]
                    ap, aq, vp, vq = a[:, p].copy(), a[:, q].copy(), v[:, p].copy(), v[:, q].copy()
                    a[:, p], a[:, q] = c * ap - s * aq, s * ap + c * aq
                    v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
    n2 = np.zeros((M, 4))
    for r in range(4):
        n2 = n2 + a[:, :, r] * a[:, :, r]
    k = np.argmin(n2, axis=1)                                        # first minimum
    return v[np.arange(M), k]


def triangulate(g1, g2, o1, o2, idx1, idx2, null_vector=None):
    """o*: dict(kps (structured mvKeysUn), raw (n,2) or None, u_right, depth (or None = monocular)).  Returns dict(status (M) uint8, x3d (M,3)
    float32 (0 where no point was computed), x3d32 (the float32-SVD point), near (M) bool, dist1 (M) float64).
    null_vector: callable A -> (M,4) float64 replacing the float64 SVD (used to restate the device's Jacobi)."""
    idx1, idx2 = np.asarray(idx1, np.int64), np.asarray(idx2, np.int64)
    M = len(idx1)
    out = dict(status=np.zeros(M, np.uint8), x3d=np.zeros((M, 3), F32), x3d32=np.zeros((M, 3), F32), near=np.zeros(M, bool), dist1=np.ones(M, F64))
    if M == 0:
        return out
    with np.errstate(all="ignore"):
        k1, k2 = o1["kps"][idx1], o2["kps"][idx2]
        x1p, y1p, x2p, y2p = k1["x"].astype(F32), k1["y"].astype(F32), k2["x"].astype(F32), k2["y"].astype(F32)
        oc1 = np.clip(k1["octave"], 0, len(g1["scale_factors"]) - 1)
        oc2 = np.clip(k2["octave"], 0, len(g2["scale_factors"]) - 1)
        ur1 = o1["u_right"][idx1].astype(F32) if o1.get("u_right") is not None else np.full(M, -1, F32)
        ur2 = o2["u_right"][idx2].astype(F32) if o2.get("u_right") is not None else np.full(M, -1, F32)
        dp1 = o1["depth"][idx1].astype(F32) if o1.get("depth") is not None else np.full(M, -1, F32)
        dp2 = o2["depth"][idx2].astype(F32) if o2.get("depth") is not None else np.full(M, -1, F32)
        st1, st2 = ur1 >= 0, ur2 >= 0
        one = np.ones(M, F32)
        xn1x = (x1p - g1["cx"]) * g1["invfx"]
        xn1y = (y1p - g1["cy"]) * g1["invfy"]
        xn2x = (x2p - g2["cx"]) * g2["invfx"]
        xn2y = (y2p - g2["cy"]) * g2["invfy"]
        ray1, ray2 = _rwc_times(g1["tcw"], xn1x, xn1y, one), _rwc_times(g2["tcw"], xn2x, xn2y, one)
        cosr = (_dot3(ray1, ray2) / (_norm3(ray1) * _norm3(ray2))).astype(F32)
        cs = cosr + F32(1)
        half1, half2 = F32(g1["mb"] / F32(2)), F32(g2["mb"] / F32(2))
        c1 = np.cos(F32(2) * np.arctan2(np.full(M, half1, F32), dp1)).astype(F32)
        c2 = np.cos(F32(2) * np.arctan2(np.full(M, half2, F32), dp2)).astype(F32)
        cs1 = np.where(st1, c1, cs).astype(F32)
        cs2 = np.where(~st1 & st2, c2, cs).astype(F32)
        cst = np.minimum(cs1, cs2)
        anyst = st1 | st2
        tri = (cosr < cst) & (cosr > 0) & (anyst | (cosr.astype(F64) < 0.9998))
        s1 = ~tri & st1 & (cs1 < cs2)
        s2 = ~tri & ~s1 & st2 & (cs2 < cs1)
        near = (np.abs(cosr.astype(F64) - cst.astype(F64)) <= COS_EPS) | (np.abs(cosr.astype(F64)) <= COS_EPS) | (~anyst & (np.abs(cosr.astype(F64) - 0.9998) <= COS_EPS))
        near |= ~tri & anyst & (np.abs(cs1.astype(F64) - cs2.astype(F64)) <= COS_EPS)
        # triangulation path
        A = build_A(g1, g2, xn1x, xn1y, xn2x, xn2y)
        A = np.where(tri[:, None, None], A, np.eye(4, dtype=F32)[None])
        nv = np.linalg.svd(A.astype(F64))[2][:, 3, :] if null_vector is None else null_vector(A)
        nv32 = np.linalg.svd(A)[2][:, 3, :]
        wzero = tri & (nv[:, 3] == 0.0)
        Xt = (nv[:, :3] / nv[:, 3:4]).astype(F32)
        Xt32 = (nv32[:, :3] / nv32[:, 3:4]).astype(F32)
        # stereo paths
        Xs1, ok1 = _unproject(g1, o1, idx1) if o1.get("depth") is not None else (np.zeros((M, 3), F32), np.zeros(M, bool))
        Xs2, ok2 = _unproject(g2, o2, idx2) if o2.get("depth") is not None else (np.zeros((M, 3), F32), np.zeros(M, bool))
        status = np.full(M, LOW_PARALLAX, np.uint8)
        status[tri], status[s1], status[s2] = TRIANGULATED, STEREO1, STEREO2
        status[wzero] = W_ZERO
        status[(s1 & ~ok1) | (s2 & ~ok2)] = DEPTH_INVALID
        have = (status >= TRIANGULATED) & (status <= STEREO2)
        X = np.where(tri[:, None], Xt, np.where(s1[:, None], Xs1, Xs2)).astype(F32)
        X = np.where(have[:, None], X, F32(0)).astype(F32)
        X32 = np.where(tri[:, None], Xt32, X).astype(F32)
        path = status.copy()
        T1, T2 = g1["tcw"], g2["tcw"]
        z1, z2 = _row_dot_plus(T1, 2, X), _row_dot_plus(T2, 2, X)
        d1v, d2v = (X - g1["center"][None, :]).astype(F32), (X - g2["center"][None, :]).astype(F32)
        dist1, dist2 = _norm3(d1v).astype(F32), _norm3(d2v).astype(F32)
        alive = have.copy()

        def stage(fail, code, close):
            nonlocal alive, near
            near |= alive & close
            status[alive & fail] = code
            alive = alive & ~fail

        stage(z1 <= 0, BEHIND1, np.abs(z1.astype(F64)) <= REL_EPS * dist1.astype(F64))
        stage(z2 <= 0, BEHIND2, np.abs(z2.astype(F64)) <= REL_EPS * dist2.astype(F64))

        def reproj(g, T, z, kx, ky, ur, st, sig):
            x, y = _row_dot_plus(T, 0, X), _row_dot_plus(T, 1, X)
            invz = (1.0 / z.astype(F64)).astype(F32)
            u = g["fx"] * x
            u = u * invz
            u = u + g["cx"]
            v = g["fy"] * y
            v = v * invz
            v = v + g["cy"]
            ex, ey = u - kx, v - ky
            e2 = ex * ex + ey * ey
            u_r = u - g1["mbf"] * invz                      # the current keyframe's mbf in both tests
            er = u_r - ur
            e3 = e2 + er * er
            err = np.where(st, e3, e2).astype(F64)
            th = np.where(st, 7.8, 5.991) * sig.astype(F64)
            return err > th, np.abs(err - th) <= REL_EPS * th

        f, c = reproj(g1, T1, z1, x1p, y1p, ur1, st1, g1["level_sigma2"][oc1])
        stage(f, REPROJ1, c)
        f, c = reproj(g2, T2, z2, x2p, y2p, ur2, st2, g2["level_sigma2"][oc2])
        stage(f, REPROJ2, c)
        stage((dist1 == 0) | (dist2 == 0), DIST_ZERO, np.zeros(M, bool))
        rd = dist2 / dist1
        ro = g1["scale_factors"][oc1] / g2["scale_factors"][oc2]
        rf = F32(F32(1.5) * g1["scale_factor"])
        lo, hi = rd * rf, ro * rf
        stage((lo < ro) | (rd > hi), SCALE, (np.abs(lo.astype(F64) - ro) <= REL_EPS * ro) | (np.abs(rd.astype(F64) - hi) <= REL_EPS * hi))
        status[alive] = path[alive]
    out.update(status=status, x3d=X, x3d32=X32, near=near, dist1=dist1.astype(F64))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


BASELINES = {"side": (0.4, 0.05, 0.02), "forward": (0.05, 0.02, 0.6), "short": (0.05, 0.0, 0.0), "axis": (0.0, 0.0, 0.5), "far": (0.004, 0.0, 0.0), "tiny": (0.01, 0.0, 0.0)}


def pose(rng, baseline):
    T = np.eye(4)
    T[:3, :3] = _rot(*rng.normal(0, 0.03, 3))
    T[:3, 3] = BASELINES[baseline] if isinstance(baseline, str) else baseline
    return T


def observe(orbx, rng, T, P, g, stereo_frac, noise, octave, gross=0.0):
    """one keyframe's observations of the world points P: noisy mvKeysUn, raw keys a fraction of a pixel off (the distortion the reference
    removes), mvuRight / mvDepth for a share of the features.  gross: share of the keypoints moved 30-60 px in a random direction (far
    beyond every chi2 bound, where Gaussian noise of a pixel puts many matches ON a bound)"""
    n = len(P)
    Pc = P @ T[:3, :3].T + T[:3, 3]
    z = np.where(np.abs(Pc[:, 2]) < 1e-6, 1e-6, Pc[:, 2])
    uv = Pc[:, :2] / z[:, None] * 500 + np.array([320, 240]) + rng.normal(0, noise, (n, 2))
    if gross > 0:
        off, ang, r = rng.random(n) < gross, rng.uniform(0, 2 * np.pi, n), rng.uniform(30, 60, n)
        uv = uv + np.where(off[:, None], np.stack([r * np.cos(ang), r * np.sin(ang)], 1), 0.0)
    k = np.zeros(n, orbx.KEYPOINT_DTYPE)
    k["x"], k["y"], k["size"], k["response"], k["octave"], k["class_id"] = uv[:, 0], uv[:, 1], 31, 50, octave, -1
    raw = (uv + rng.normal(0, 0.3, (n, 2))).astype(F32)
    st = (rng.random(n) < stereo_frac) & (z > 0)
    depth = np.where(st, z, -1.0).astype(F32)
    ur = np.where(st, uv[:, 0] - float(g["mbf"]) / z + rng.normal(0, noise, n), -1.0).astype(F32)
    ur = np.where(st, np.maximum(ur, 0), ur).astype(F32)
    return dict(kps=k, raw=raw, u_right=ur if stereo_frac > 0 else None, depth=depth if stereo_frac > 0 else None)


def pair_scene(orbx, seed, n=300, baseline="side", stereo_frac=0.0, noise=0.6, depth=(3.0, 10.0), wrong=0.15, mbf=40.0, noise2=None):
    """two keyframes seeing n random points, the match list (true correspondences, a share `wrong` re-paired at random: points behind a
    camera, large reprojection errors), octaves equal in both views except for a share that jumps (the scale test)"""
    rng = np.random.default_rng(seed)
    T1, T2 = np.eye(4), pose(rng, baseline)
    g1, g2 = make_geom(T1, mbf=mbf), make_geom(T2, mbf=mbf)
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(depth[0], depth[1], n)], 1)
    oc1 = rng.integers(0, 8, n)
    oc2 = np.where(rng.random(n) < 0.1, rng.integers(0, 8, n), oc1)
    o1 = observe(orbx, rng, T1, P, g1, stereo_frac, noise, oc1)
    perm = rng.permutation(n)
    o2 = observe(orbx, rng, T2, P[perm], g2, stereo_frac, noise if noise2 is None else noise2, oc2[perm])
    inv = np.argsort(perm)
    idx1 = np.arange(n)
    idx2 = inv.copy()
    w = rng.random(n) < wrong
    idx2[w] = rng.integers(0, n, int(w.sum()))
    keep = rng.random(n) < 0.9
    return dict(g1=g1, g2=g2, o1=o1, o2=o2, idx1=idx1[keep].astype(np.int32), idx2=idx2[keep].astype(np.int32), T1=T1, T2=T2)


def restate_pairs(pairs, **kw):
    """triangulate() over a list of pair scenes, concatenated like orbx_triangulate_matches returns them"""
    rs = [triangulate(p["g1"], p["g2"], p["o1"], p["o2"], p["idx1"], p["idx2"], **kw) for p in pairs]
    return {k: np.concatenate([r[k] for r in rs]) for k in rs[0]}


def f12_epipole(T1, T2, K=None):
    """LocalMapping::ComputeF12 and the epipole of ORBmatcher::SearchForTriangulation (KF1's centre in KF2), as tests/test_triangulation.py builds them"""
    K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], F64) if K is None else K
    R12 = T1[:3, :3] @ T2[:3, :3].T
    t12 = -R12 @ T2[:3, 3] + T1[:3, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = (np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)).astype(F32)
    Cw = -T1[:3, :3].T @ T1[:3, 3]
    C2 = T2[:3, :3] @ Cw + T2[:3, 3]
    epi = np.array([500 * C2[0] / C2[2] + 320, 500 * C2[1] / C2[2] + 240], F32) if abs(C2[2]) > 1e-9 else np.array([1e6, 1e6], F32)
    return F12, epi


def chain_scene(orbx, seed, n=300, K=3, stereo_frac=0.0, baselines=None, n2=None, noise=0.05, gross=0.15):
    """KF1 and K neighbours seeing the same points: descriptors repeat (competition for the same KF2 feature), node ids mostly agree, 30 % of
    KF1's features already hold a MapPoint.  n2: features per neighbour (list; 0 = an empty neighbour).  Keypoints are either within a
    twentieth of a pixel or grossly off, so that hardly a match sits on a threshold (its outcome would change the later searches)."""
    rng = np.random.default_rng(seed)
    names = ["side", "forward", "tiny"]
    baselines = baselines or [names[k % 3] for k in range(K)]
    n2 = n2 or [n] * K
    cap2 = max(max(n2), 1)
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(3, 10, n)], 1)
    base = rng.integers(0, 256, (max(n // 3, 1), 32), dtype=np.uint8)
    d1 = base[rng.integers(0, len(base), n)]
    oc = rng.integers(0, 8, n)
    T1 = np.eye(4)
    g1 = make_geom(T1)
    o1 = observe(orbx, rng, T1, P, g1, stereo_frac, noise, oc)
    groups1 = (rng.integers(0, 9, n) * 5).astype(np.int32)
    ang = rng.uniform(0, 360, n).astype(F32)
    o1["kps"]["angle"] = ang
    kf1 = dict(o1, desc=d1, groups=groups1, has_mp=(rng.random(n) < 0.3).astype(np.uint8), g=g1, T=T1)
    nbs = []
    for k in range(K):
        m = n2[k]
        scale = 1.0 + 0.5 * (k // 3)
        T2 = pose(rng, tuple(scale * np.array(BASELINES[baselines[k]])))
        g2 = make_geom(T2)
        sel = rng.permutation(n)[:m]
        o2 = observe(orbx, rng, T2, P[sel], g2, stereo_frac, noise, oc[sel], gross)
        d2 = d1[sel].copy()
        for i in range(m):
            for b in rng.integers(0, 256, 6)[: rng.integers(0, 7)]:
                d2[i, b >> 3] ^= 1 << (b & 7)
        o2["kps"]["angle"] = (ang[sel] + rng.normal(0, 4, m).astype(F32)) % 360
        gr = groups1[sel].copy()
        gr[rng.random(m) < 0.1] = 0
        F12, epi = f12_epipole(T1, T2)
        nbs.append(dict(o2, desc=d2, groups=gr.astype(np.int32), has_mp=(rng.random(m) < 0.3).astype(np.uint8), g=g2, T=T2, F12=F12, epipole=epi))
    return dict(kf1=kf1, neighbours=nbs, cap2=cap2)


def _search_dict(kf):
    ur = kf["u_right"] if kf.get("u_right") is not None else np.full(len(kf["kps"]), -1, F32)
    return dict(kps=kf["kps"], desc=kf["desc"], groups=kf["groups"], has_mp=kf["has_mp"], u_right=ur)


def expected_chain(oracle_lib, orc, sc, check_ori=False, sequential=True, stop_after=None):
    """the chain from existing pieces: per neighbour the CPU restatement of SearchForTriangulation on the current mask, triangulate() on its
    matches, the mask update.  sequential=False: every search on the INITIAL mask (what parallel pairs would compute)."""
    kf1 = sc["kf1"]
    n1 = len(kf1["kps"])
    has_mp = kf1["has_mp"].copy()
    K = len(sc["neighbours"])
    out = dict(nmatches=np.zeros(K, np.int32), matches=np.full((K, max(n1, 1)), -1, np.int32), status=np.zeros((K, max(n1, 1)), np.uint8),
               x3d=np.zeros((K, max(n1, 1), 3), F32), near=np.zeros((K, max(n1, 1)), bool), created=[])
    for k, nb in enumerate(sc["neighbours"]):
        if stop_after is not None and k >= stop_after:
            break
        a = _search_dict(kf1)
        a["has_mp"] = has_mp.copy() if sequential else kf1["has_mp"].copy()
        if n1 and len(nb["kps"]):
            nm, mt = oracle_lib.search_for_triangulation(orc, a, _search_dict(nb), nb["F12"], nb["epipole"], nb["g"]["scale_factors"], nb["g"]["level_sigma2"], False, check_ori)
        else:
            nm, mt = 0, np.full(n1, -1, np.int32)
        out["nmatches"][k] = nm
        out["matches"][k, :n1] = mt
        i1 = np.nonzero(mt >= 0)[0]
        r = triangulate(kf1["g"], nb["g"], kf1, nb, i1, mt[i1])
        out["status"][k, i1], out["x3d"][k, i1], out["near"][k, i1] = r["status"], r["x3d"], r["near"]
        acc = i1[(r["status"] >= TRIANGULATED) & (r["status"] <= STEREO2)]
        has_mp[acc] = 1
        for i in acc:
            out["created"].append((k, int(i), int(mt[i]), int(out["status"][k, i])) + tuple(out["x3d"][k, i]))
    return out
