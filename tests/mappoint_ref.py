"""Expected values of the batched MapPoint refresh (orbx_mappoint_refresh), independent of the code under test.

A numpy restatement of MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:359-439) and MapPoint::UpdateNormalAndDepth
(:477-521) from their stated semantics - NOT the reference and not compiled from it:
    descriptor: N valid descriptors in list order, row i = Hamming distances to all N (self-distance 0 included), median = the element at
                sorted position (N-1)//2, winner = the lowest i with the smallest median, returned as its position in the full list;
                N == 0 -> (-1, INT_MAX);
    normal:     per observer in list order v = pos - Ow (float32), s = sqrt(v0^2 + v1^2 + v2^2) accumulated in float64 from 0,
                u = float32(float64(v) / s), normal = normal + u in float32 ONE OBSERVER AFTER THE OTHER (a Python loop: a float sum of three or
                more terms depends on the order); then normal = float32(float64(normal) / float64(n));
    depth:      dist = float32(sqrt(float64 sum of (pos - refOw)^2)), max = dist * ref_scale, min = max / top_scale (float32 operations).
One operation per numpy call, so nothing is fused or promoted.

Also the batch generators: from an lba_synth window (keyframe centres from the poses, a point's observers from the window's edges in
increasing keyframe index) and with prescribed observation counts.  Descriptors: one random 256-bit string per point with a few random bits
flipped per observation, so that row medians tie often.  A batch is a dict of the arrays orbx_mappoint_batch names."""
import numpy as np

F32, F64 = np.float32, np.float64
INT_MAX = 2**31 - 1
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
KEYS = ("obs_offset", "desc", "desc_valid", "cam_center", "pos", "ref_center", "ref_scale", "top_scale")


def scale_factors(nlevels=8, factor=1.2):
    """mvScaleFactor as the extractor builds it: s[i] = s[i-1] * scaleFactor in float"""
    s = [F32(1.0)]
    for _ in range(1, nlevels):
        s.append(F32(s[-1] * F32(factor)))
    return np.array(s, F32)


def distance_matrix(desc):
    """all-pairs Hamming distances of (N,32) uint8 descriptors"""
    d = np.ascontiguousarray(desc, np.uint8)
    return POP[d[:, None, :] ^ d[None, :, :]].sum(2)


def distinctive(desc, valid=None):
    """(best_obs, best_median) of one point: desc (n,32) uint8, valid (n) or None"""
    n = len(desc)
    idx = [i for i in range(n) if valid is None or valid[i]]
    N = len(idx)
    if N == 0:
        return -1, INT_MAX
    D = distance_matrix(np.asarray(desc)[idx])
    k = (N - 1) // 2
    med = np.partition(D, k, axis=1)[:, k]      # the k-th order statistic of every row
    i = int(np.argmin(med))                     # first minimum = lowest index
    return idx[i], int(med[i])


def unit(pos, ow):
    v = [F32(pos[c]) - F32(ow[c]) for c in range(3)]
    s = F64(0.0)
    for c in range(3):
        sq = F64(v[c]) * F64(v[c])
        s = s + sq
    s = np.sqrt(s)
    return [F32(F64(v[c]) / s) for c in range(3)]


def normal_depth(pos, cams, ref_center, ref_scale, top_scale):
    """(normal (3), max_dist, min_dist) of one point with len(cams) >= 1 observers, cams in list order"""
    acc = [F32(0.0), F32(0.0), F32(0.0)]
    for ow in cams:
        u = unit(pos, ow)
        for c in range(3):
            acc[c] = F32(acc[c] + u[c])
    n = F64(len(cams))
    normal = np.array([F32(F64(acc[c]) / n) for c in range(3)], F32)
    v = [F32(pos[c]) - F32(ref_center[c]) for c in range(3)]
    s = F64(0.0)
    for c in range(3):
        sq = F64(v[c]) * F64(v[c])
        s = s + sq
    dist = F32(np.sqrt(s))
    mx = F32(dist * F32(ref_scale))
    mn = F32(mx / F32(top_scale))
    return normal, mx, mn


def restate(b):
    """the whole batch -> dict like MapPointOps.refresh returns; rows of points without observations stay 0 (updated == 0)"""
    off = b["obs_offset"]
    M = len(off) - 1
    o = dict(best_obs=np.zeros(M, np.int32), best_median=np.zeros(M, np.int32), normal=np.zeros((M, 3), F32), max_dist=np.zeros(M, F32),
             min_dist=np.zeros(M, F32), updated=np.zeros(M, np.uint8))
    for p in range(M):
        a, e = int(off[p]), int(off[p + 1])
        if e == a:
            continue
        o["updated"][p] = 1
        o["best_obs"][p], o["best_median"][p] = distinctive(b["desc"][a:e], None if b["desc_valid"] is None else b["desc_valid"][a:e])
        o["normal"][p], o["max_dist"][p], o["min_dist"][p] = normal_depth(b["pos"][p], b["cam_center"][a:e], b["ref_center"][p], b["ref_scale"][p], b["top_scale"][p])
    return o


def same_bits(got, want, rows=None):
    """every output equal: ints by value, floats by bit pattern.  rows: boolean mask of the points compared (default: those `want` updated)"""
    if not np.array_equal(got["updated"], want["updated"]):
        return False
    m = want["updated"] != 0 if rows is None else rows
    ok = np.array_equal(got["best_obs"][m], want["best_obs"][m]) and np.array_equal(got["best_median"][m], want["best_median"][m])
    for k in ("normal", "max_dist", "min_dist"):
        ok = ok and np.array_equal(np.ascontiguousarray(got[k][m], F32).view(np.uint32), np.ascontiguousarray(want[k][m], F32).view(np.uint32))
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------------
def flipped_descriptors(rng, n, flips):
    """n descriptors: one random 256-bit string, `flips` random bits flipped in each copy"""
    base = rng.integers(0, 2, 256, dtype=np.uint8)
    bits = np.tile(base, (n, 1))
    for i in range(n):
        bits[i, rng.choice(256, flips, replace=False)] ^= 1
    return np.packbits(bits, axis=1)


def pack(points):
    """list of dict(desc (n,32), valid (n) or None, cams (n,3), pos, ref_center, ref_scale, top_scale) -> batch"""
    off = np.zeros(len(points) + 1, np.int32)
    off[1:] = np.cumsum([len(q["desc"]) for q in points])
    any_valid = any(q.get("valid") is not None for q in points)
    def cat(xs, shape, dt):
        return np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(shape) for x in xs] + [np.zeros(0, dt).reshape(shape)]), dt)
    b = dict(obs_offset=off,
             desc=cat([q["desc"] for q in points], (-1, 32), np.uint8),
             desc_valid=cat([np.ones(len(q["desc"]), np.uint8) if q.get("valid") is None else q["valid"] for q in points], (-1,), np.uint8) if any_valid else None,
             cam_center=cat([q["cams"] for q in points], (-1, 3), F32),
             pos=np.array([q["pos"] for q in points], F32).reshape(-1, 3), ref_center=np.array([q["ref_center"] for q in points], F32).reshape(-1, 3),
             ref_scale=np.array([q["ref_scale"] for q in points], F32), top_scale=np.array([q["top_scale"] for q in points], F32))
    return b


def unpack(b):
    off = b["obs_offset"]
    out = []
    for p in range(len(off) - 1):
        a, e = int(off[p]), int(off[p + 1])
        out.append(dict(desc=b["desc"][a:e], valid=None if b["desc_valid"] is None else b["desc_valid"][a:e], cams=b["cam_center"][a:e], pos=b["pos"][p],
                        ref_center=b["ref_center"][p], ref_scale=b["ref_scale"][p], top_scale=b["top_scale"][p]))
    return out


def concat(*batches):
    return pack(sum((unpack(b) for b in batches), []))


def reverse(b):
    """the same points with every observation list reversed"""
    pts = unpack(b)
    for q in pts:
        q["desc"], q["cams"] = q["desc"][::-1], q["cams"][::-1]
        q["valid"] = None if q["valid"] is None else q["valid"][::-1]
    return pack(pts)


def synth_point(rng, n, flips=6, desc=None):
    """a point near the origin seen from n centres 3..7 m away; the reference keyframe is one of the observers, its level uniform in 0..7"""
    sf = scale_factors()
    pos = rng.uniform(-1.0, 1.0, 3).astype(F32)
    d = rng.normal(size=(max(n, 1), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cams = (d * rng.uniform(3.0, 7.0, (max(n, 1), 1))).astype(F32)
    ref = cams[int(rng.integers(0, max(n, 1)))]
    assert np.linalg.norm(cams.astype(F64) - pos.astype(F64), axis=1).min() >= 0.1
    return dict(desc=flipped_descriptors(rng, n, flips) if desc is None else np.asarray(desc, np.uint8).reshape(n, 32), valid=None, cams=cams[:n], pos=pos, ref_center=ref,
                ref_scale=sf[int(rng.integers(0, 8))], top_scale=sf[7])


def synth_batch(ns, seed, flips=6):
    rng = np.random.default_rng(seed)
    return pack([synth_point(rng, int(n), flips) for n in ns])


def window_batch(w, seed, flips=6):
    """from an lba_synth.make_window dict: every point with its observers in increasing keyframe index"""
    rng = np.random.default_rng(seed)
    sf = scale_factors()
    T = np.asarray(w["poses"], F64).reshape(-1, 4, 4)
    centres = np.array([-(t[:3, :3].T @ t[:3, 3]) for t in T]).astype(F32)      # Ow = -Rcw^T tcw
    pts = []
    for p in range(w["P"]):
        ks = np.sort(w["edge_kf"][w["edge_point"] == p])
        n = len(ks)
        pos = np.asarray(w["points"][p], F32)
        cams = centres[ks] if n else np.zeros((0, 3), F32)
        if n:
            assert np.linalg.norm(cams.astype(F64) - pos.astype(F64), axis=1).min() >= 0.1
        pts.append(dict(desc=flipped_descriptors(rng, n, flips), valid=None, cams=cams, pos=pos, ref_center=cams[0] if n else np.zeros(3, F32),
                        ref_scale=sf[int(rng.integers(0, 8))], top_scale=sf[7]))
    return pack(pts)
