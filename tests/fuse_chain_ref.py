"""Steps 2 and 3 of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:666-713) restated literally on the arrays of orbx_fuse_slice
(fuse_slice's dict): plain sequential loops, with ORBmatcher::Fuse (src/ORBmatcher.cc:1020-1174), MapPoint::Replace / AddObservation /
ComputeDistinctiveDescriptors (src/MapPoint.cc:154-166, 244-307, 359-439) and the candidate gather each written as the reference writes them.
std::map<KeyFrame*, size_t> is a list of (keyframe, feature, stereo, descriptor) kept in ascending RANK.  Floats: np.float32 scalars, one operation per
expression, so nothing is fused or promoted; Mat::dot and cv::norm accumulate in float64 (oracle/cvshim), the viewing gate compares doubles."""
import math

import numpy as np

TH_LOW = 50
ADDED, REPLACED_BY_HOLDER, REPLACED_HOLDER, HOLDER_BAD = 0, 1, 2, 3
GRID_COLS, GRID_ROWS = 64, 48
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
f32 = np.float32


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


class State:
    """The mutable part of the map slice"""
    def __init__(self, sl):
        self.sl = sl
        self.rank = [int(r) for r in np.asarray(sl["kf_rank"]).reshape(-1)]
        self.kf_bad = [int(b) for b in np.asarray(sl["kf_bad"]).reshape(-1)]
        self.sidx = {int(k["slot"]): i for i, k in enumerate(sl["searchable"])}
        self.kf_point = [[int(p) for p in np.asarray(k["kf_point"]).reshape(-1)] for k in sl["searchable"]]
        P = len(np.asarray(sl["bad"]).reshape(-1))
        self.P = P
        self.bad = [int(b) for b in np.asarray(sl["bad"]).reshape(-1)]
        self.visible = [int(v) for v in np.asarray(sl["visible"]).reshape(-1)]
        self.found = [int(v) for v in np.asarray(sl["found"]).reshape(-1)]
        self.desc = [np.array(d, np.uint8) for d in np.asarray(sl["desc"], np.uint8).reshape(-1, 32)]
        self.replaced = [-1] * P
        off = np.asarray(sl["obs_offset"]).reshape(-1)
        od = np.asarray(sl["obs_desc"], np.uint8).reshape(-1, 32)
        okf, oidx, ost = (np.asarray(sl[k]).reshape(-1) for k in ("obs_kf", "obs_idx", "obs_stereo"))
        self.obs = [[(int(okf[o]), int(oidx[o]), int(ost[o] != 0), od[o]) for o in range(off[p], off[p + 1])] for p in range(P)]
        self.nobs = [sum(2 if o[2] else 1 for o in ob) for ob in self.obs]
        self.conflict_erases = 0

    def in_keyframe(self, p, kf):
        return any(o[0] == kf for o in self.obs[p])


def add_observation(st, p, kf, idx):
    """MapPoint::AddObservation + KeyFrame::AddMapPoint"""
    if st.in_keyframe(p, kf):
        return
    k = st.sl["searchable"][st.sidx[kf]]
    stereo = 1 if np.asarray(k["u_right"], np.float32).reshape(-1)[idx] >= 0 else 0
    ob = st.obs[p]
    at = 0
    while at < len(ob) and st.rank[ob[at][0]] < st.rank[kf]:
        at += 1
    ob.insert(at, (kf, idx, stereo, np.asarray(k["desc"], np.uint8).reshape(-1, 32)[idx]))
    st.nobs[p] += 2 if stereo else 1
    st.kf_point[st.sidx[kf]][idx] = p


def compute_distinctive_descriptors(st, p):
    descs = [o[3] for o in st.obs[p] if not st.kf_bad[o[0]]]
    N = len(descs)
    if N == 0:
        return
    best_median, best = 2 ** 31 - 1, 0
    for i in range(N):
        d = sorted(hamming(descs[i], descs[j]) for j in range(N))
        median = d[int(0.5 * (N - 1))]
        if median < best_median:
            best_median, best = median, i
    st.desc[p] = np.array(descs[best], np.uint8)


def replace(st, a, b):
    """a->Replace(b)"""
    if a == b:
        return
    obs = st.obs[a]
    st.obs[a] = []
    st.bad[a] = 1
    nvisible, nfound = st.visible[a], st.found[a]
    st.replaced[a] = b
    for kf, idx, stereo, d in obs:      # ascending rank: the order of the map
        if not st.in_keyframe(b, kf):
            if kf in st.sidx:
                st.kf_point[st.sidx[kf]][idx] = b      # ReplaceMapPointMatch
            ob = st.obs[b]
            at = 0
            while at < len(ob) and st.rank[ob[at][0]] < st.rank[kf]:
                at += 1
            ob.insert(at, (kf, idx, stereo, d))
            st.nobs[b] += 2 if stereo else 1
        else:
            if kf in st.sidx:
                st.kf_point[st.sidx[kf]][idx] = -1     # EraseMapPointMatch
            st.conflict_erases += 1
    st.found[b] += nfound
    st.visible[b] += nvisible
    compute_distinctive_descriptors(st, b)


def prepare(st, si, lst):
    """:1040-1086 per list entry on the current state -> dict(active, u, v, ur, level, radius)"""
    sl, k = st.sl, st.sl["searchable"][si]
    n = len(lst)
    out = dict(active=np.zeros(n, np.uint8), u=np.zeros(n, f32), v=np.zeros(n, f32), ur=np.zeros(n, f32), level=np.zeros(n, np.int32), radius=np.zeros(n, f32))
    T = np.asarray(k["Tcw"], f32).reshape(-1, 4)[:3]
    Ow = np.asarray(k["ow"], f32).reshape(3)
    fx, fy, cx, cy, bf = (f32(c) for c in k["cam"])
    minx, miny, maxx, maxy = (int(f32(b)) for b in k["bounds"])      # KeyFrame keeps the bounds as int
    sf = np.asarray(k["scale_factors"], f32).reshape(-1)
    logsf, nlev, th = f32(k["log_scale_factor"]), len(sf), f32(sl.get("th", 3.0))
    pos, nrm = np.asarray(sl["pos"], f32).reshape(-1, 3), np.asarray(sl["normal"], f32).reshape(-1, 3)
    mind, maxd, rawmax = (np.asarray(sl[q], f32).reshape(-1) for q in ("min_dist", "max_dist", "raw_max_dist"))
    for i, p in enumerate(lst):
        p = int(p)
        if p < 0 or st.bad[p] or st.in_keyframe(p, int(k["slot"])):
            continue
        Pw = pos[p]
        Pc = []
        for r in range(3):
            t = T[r, 0] * Pw[0]
            t = t + T[r, 1] * Pw[1]
            t = t + T[r, 2] * Pw[2]
            Pc.append(f32(t + T[r, 3]))
        if Pc[2] < f32(0.0):
            continue
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            invz = f32(1.0) / Pc[2]
            x, y = Pc[0] * invz, Pc[1] * invz
            u, v = fx * x + cx, fy * y + cy
        if not (u >= f32(minx) and u < f32(maxx) and v >= f32(miny) and v < f32(maxy)):
            continue
        ur = u - bf * invz
        PO = [Pw[c] - Ow[c] for c in range(3)]
        dist3D = f32(math.sqrt(float(PO[0]) * float(PO[0]) + float(PO[1]) * float(PO[1]) + float(PO[2]) * float(PO[2])))
        if dist3D < mind[p] or dist3D > maxd[p]:
            continue
        if float(PO[0]) * float(nrm[p, 0]) + float(PO[1]) * float(nrm[p, 1]) + float(PO[2]) * float(nrm[p, 2]) < 0.5 * float(dist3D):
            continue
        ratio = rawmax[p] / dist3D
        nScale = int(math.ceil(math.log(float(ratio)) / float(logsf)))      # MapPoint::PredictScale
        nScale = 0 if nScale < 0 else (nlev - 1 if nScale >= nlev else nScale)
        out["active"][i], out["u"][i], out["v"][i], out["ur"][i], out["level"][i], out["radius"][i] = 1, u, v, ur, nScale, th * sf[nScale]
    return out


def roundf(x):
    x = np.asarray(x, np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def search(st, si, lst, prep):
    """:1088-1148: GetFeaturesInArea, the level and chi-square gates, the first minimum in the cell-major order -> (best_idx, best_dist)"""
    k = st.sl["searchable"][si]
    n = len(lst)
    bi, bd = np.full(n, -1, np.int32), np.full(n, 256, np.int32)
    kp = k["kps"]
    N = len(kp)
    if N == 0:
        return bi, bd
    kx, ky, octv = np.asarray(kp["x"], f32), np.asarray(kp["y"], f32), np.asarray(kp["octave"], np.int64)
    ur = np.asarray(k["u_right"], f32).reshape(-1)
    dk = np.asarray(k["desc"], np.uint8).reshape(-1, 32)
    s2 = np.asarray(k["inv_level_sigma2"], f32).reshape(-1)
    minx, miny, maxx, maxy = (f32(b) for b in k["bounds"])
    gw, gh = f32(64) / (maxx - minx), f32(48) / (maxy - miny)
    wx, wy = f32(int(minx)), f32(int(miny))
    cxs, cys = roundf((kx - minx) * gw), roundf((ky - miny) * gh)      # the cell AssignFeaturesToGrid filed the feature in
    for i in range(n):
        if not prep["active"][i]:
            continue
        x, y, r, xr, lvl = prep["u"][i], prep["v"][i], prep["radius"][i], prep["ur"][i], int(prep["level"][i])
        cx0, cx1 = max(0, int(math.floor((x - wx - r) * gw))), min(GRID_COLS - 1, int(math.ceil((x - wx + r) * gw)))
        cy0, cy1 = max(0, int(math.floor((y - wy - r) * gh))), min(GRID_ROWS - 1, int(math.ceil((y - wy + r) * gh)))
        if cx0 >= GRID_COLS or cx1 < 0 or cy0 >= GRID_ROWS or cy1 < 0:
            continue
        ok = (cxs >= cx0) & (cxs <= cx1) & (cys >= cy0) & (cys <= cy1) & (np.abs(kx - x) < r) & (np.abs(ky - y) < r) & (octv >= lvl - 1) & (octv <= lvl)
        ex, ey, er = x - kx, y - ky, xr - ur
        e3, e2 = (ex * ex + ey * ey) + er * er, ex * ex + ey * ey
        chi = np.where(ur >= 0, (e3 * s2[octv]).astype(np.float64) > 7.8, (e2 * s2[octv]).astype(np.float64) > 5.99)
        ok &= ~chi
        best = None
        d = st.desc[int(lst[i])]
        for idx in np.nonzero(ok)[0]:
            key = (hamming(d, dk[idx]), int(cxs[idx]), int(cys[idx]), int(idx))
            if best is None or key < best:
                best = key
        if best is not None:
            bi[i], bd[i] = best[3], best[0]
    return bi, bd


def apply(st, si, lst, active, best_idx, best_dist, call, log):
    """:1150-1171 in list order, with the re-check of :1045 at the entry's turn -> nFused"""
    k = st.sl["searchable"][si]
    kf = int(k["slot"])
    nfused = 0
    for i, p in enumerate(lst):
        p = int(p)
        if p < 0 or st.bad[p] or st.in_keyframe(p, kf) or not active[i]:
            continue
        if best_dist[i] <= TH_LOW:
            bi = int(best_idx[i])
            q = st.kf_point[si][bi]
            if q >= 0:
                if not st.bad[q]:
                    if st.nobs[q] > st.nobs[p]:
                        log.append((call, i, p, bi, REPLACED_BY_HOLDER, q))
                        replace(st, p, q)
                    else:
                        log.append((call, i, p, bi, REPLACED_HOLDER, q))
                        replace(st, q, p)
                else:
                    log.append((call, i, p, bi, HOLDER_BAD, q))
            else:
                log.append((call, i, p, bi, ADDED, -1))
                add_observation(st, p, kf, bi)
            nfused += 1
    return nfused


def fuse(st, si, lst, call, log, keep=None):
    """One ORBmatcher::Fuse call of searchable keyframe si on the list"""
    prep = prepare(st, si, lst)
    bi, bd = search(st, si, lst, prep)
    if keep is not None:
        keep.append(dict(prep, best_idx=bi, best_dist=bd, list=np.array(lst, np.int32)))
    return apply(st, si, lst, prep["active"], bi, bd, call, log)


def gather(st, targets):
    """:690-711"""
    cand, seen = [], set()
    for t in targets:
        for p in st.kf_point[st.sidx[int(t)]]:
            if p < 0 or st.bad[p] or p in seen:
                continue
            seen.add(p)
            cand.append(p)
    return cand


def export(st, log, nfused, cand, calls=None):
    P = st.P
    off = np.zeros(P + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in st.obs])
    flat = [o for ob in st.obs for o in ob]
    out = dict(log=np.array(log, np.int32).reshape(-1, 6), nfused=np.array(nfused, np.int32), candidates=np.array(cand, np.int32),
               kf_point=[np.array(k, np.int32) for k in st.kf_point], point_bad=np.array(st.bad, np.uint8), replaced=np.array(st.replaced, np.int32),
               point_obs=np.array(st.nobs, np.int32), visible=np.array(st.visible, np.int32), found=np.array(st.found, np.int32),
               desc=np.array(st.desc, np.uint8).reshape(-1, 32), obs_offset=off, obs_kf=np.array([o[0] for o in flat], np.int32),
               obs_idx=np.array([o[1] for o in flat], np.int32), obs_stereo=np.array([o[2] for o in flat], np.uint8), conflict_erases=st.conflict_erases)
    if calls is not None:
        for key in ("active", "u", "v", "ur", "level", "radius", "best_idx", "best_dist", "list"):
            out[key] = [c[key] for c in calls]
    return out


def search_in_neighbors(sl, current, targets):
    st = State(sl)
    cur = st.sidx[int(current)]
    lst = list(st.kf_point[cur])      # vpMapPointMatches, captured once (:671)
    log, nfused, calls = [], [], []
    for c, t in enumerate(targets):
        nfused.append(fuse(st, st.sidx[int(t)], lst, c, log, calls))
    cand = gather(st, targets)
    nfused.append(fuse(st, cur, cand, len(targets), log, calls))
    return export(st, log, nfused, cand, calls)


def fuse_apply(sl, kf, lst, active, best_idx, best_dist):
    st = State(sl)
    log = []
    n = apply(st, st.sidx[int(kf)], [int(p) for p in lst], active, best_idx, best_dist, 0, log)
    return export(st, log, [n], [])


def log_rows(log):
    """a result's structured log (FUSE_DECISION_DTYPE) as the (n, 6) int32 rows of this module"""
    log = np.asarray(log)
    if log.dtype.names:
        return np.stack([log[k] for k in ("call", "position", "point", "feature", "kind", "other")], 1).astype(np.int32).reshape(-1, 6)
    return log.astype(np.int32).reshape(-1, 6)


STATE_KEYS = ("nfused", "candidates", "point_bad", "replaced", "point_obs", "visible", "found", "desc", "obs_offset", "obs_kf", "obs_idx", "obs_stereo")


def assert_equal_results(got, want, what=""):
    """every field of a result, no tolerance"""
    assert (log_rows(got["log"]) == log_rows(want["log"])).all() and len(got["log"]) == len(want["log"]), what + " log"
    for k in STATE_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a == b).all(), "%s %s" % (what, k)
    assert len(got["kf_point"]) == len(want["kf_point"])
    for i, (a, b) in enumerate(zip(got["kf_point"], want["kf_point"])):
        assert (np.asarray(a) == np.asarray(b)).all(), "%s kf_point of searchable keyframe %d" % (what, i)
