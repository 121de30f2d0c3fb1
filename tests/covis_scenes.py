"""Scenes of tests/test_covisibility.py and tools/latency_covis.py: slices of a map as the arrays of orbx_covis_slice (dicts, the keys of
covis_slice in the package).  Everything is seeded; a scene is built once per process and never changed."""
import functools
import importlib
import sys
from pathlib import Path

import numpy as np

LDS_NK = 4096      # ORBX_COVIS_LDS_KEYFRAMES: the histogram of a list lives in LDS up to here
SWEEP_NK = (1, 2, 63, 64, 65, 300, LDS_NK, LDS_NK + 1)
SWEEP_SIZES = (0, 1, 14, 15, 16, 1500, 40)      # entries of the lists of a Q = 7 call
SWEEP_FRAME = (1, 4)                            # ... which of them are a Frame's (list_kf = -1)


@functools.lru_cache(maxsize=None)
def _orbx():
    root = str(Path(__file__).resolve().parent.parent)
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module("self_commit_orb-slam2_amd")


def _ranks(rng, NK):
    return (rng.permutation(NK) * 7 - 1000).astype(np.int32)      # distinct, unordered, some negative


@functools.lru_cache(maxsize=None)
def connect_scene(seed, NK, sizes=SWEEP_SIZES, frame=SWEEP_FRAME):
    """UpdateConnections / UpdateLocalKeyFrames: len(sizes) lists; the lists of up to 16 entries take distinct points that two `hot` keyframes
    all observe (their weight IS the list's size: 14 / 15 / 16 around th), the others draw from a pool with 1 to 20 observers per point, with repeats"""
    rng = np.random.default_rng(seed)
    hot = rng.permutation(NK)[:min(NK, 24)]
    nA, nB = 64, max(64, max(sizes))
    owners = [-1 if q in frame else int(hot[(3 + q) % len(hot)]) for q in range(len(sizes))]
    obs = []
    for p in range(nA + nB):
        n = int(rng.integers(1, min(20, NK) + 1))
        pick = np.where(rng.random(n) < 0.7, hot[rng.integers(0, len(hot), n)], rng.integers(0, NK, n))
        if p < nA:
            pick = np.concatenate([hot[:2], pick[:max(0, n - 2)]])
        s = []
        for k in pick:      # a keyframe observes a point once
            if int(k) not in s:
                s.append(int(k))
        obs.append(s)
    lists = []
    for q, n in enumerate(sizes):
        pts = rng.permutation(nA)[:n] if n <= 16 else nA + rng.integers(0, nB, n)
        if owners[q] >= 0:
            for p in pts:
                if rng.random() < 0.9 and owners[q] not in obs[int(p)] and len(obs[int(p)]) < 20:
                    obs[int(p)].append(owners[q])
        lists.append(pts.astype(np.int32))
    off = np.zeros(len(obs) + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in obs])
    T = int(off[-1])
    loff = np.zeros(len(sizes) + 1, np.int32)
    loff[1:] = np.cumsum(sizes)
    S = int(loff[-1])
    flags = (rng.integers(0, 2, NK) * 4 * (rng.random(NK) < 0.4)).astype(np.uint8)      # some bad keyframes: a Frame's vote passes over them
    return dict(kf_rank=_ranks(rng, NK), kf_flags=flags, obs_offset=off, obs_kf=np.array([k for o in obs for k in o], np.int32).reshape(-1),
                obs_octave=rng.integers(0, 8, T).astype(np.uint8), obs_stereo=rng.integers(0, 2, T).astype(np.uint8),
                point_bad=(rng.random(len(obs)) < 0.05).astype(np.uint8), list_offset=loff, list_kf=np.array(owners, np.int32),
                list_point=np.concatenate(lists).astype(np.int32) if S else np.zeros(0, np.int32), list_octave=rng.integers(0, 8, S).astype(np.uint8),
                list_close=rng.integers(0, 2, S).astype(np.uint8))


def one_list(s, q):
    """the slice with list q alone (same keyframes, same points)"""
    t = dict(s)
    a, b = int(s["list_offset"][q]), int(s["list_offset"][q + 1])
    t["list_offset"] = np.array([0, b - a], np.int32)
    t["list_kf"] = np.asarray(s["list_kf"])[q:q + 1].copy()
    for k in ("list_point", "list_octave", "list_close"):
        t[k] = np.asarray(s[k])[a:b].copy()
    return t


@functools.lru_cache(maxsize=None)
def tie_scene():
    """64 keyframes; slot 0 owns list 0, list 1 is the same list as a Frame's.  Slots 1..30 see points 0..19 (weight 20, and 21 through a repeated
    point), slots 31..40 points 20..35 (weight 16), slots 41..50 points 36..49 (weight 14 < th): 38 ties at or above th = 15"""
    rng = np.random.default_rng(5)
    kfs = [[] for _ in range(64)]
    for p in range(50):
        who = [0] + (list(range(1, 31)) if p < 20 else list(range(31, 41)) if p < 36 else list(range(41, 51)))
        for k in who:
            kfs[k].append((p, 0, 0))
    entries = list(kfs[0]) + [(0, 0, 0)]      # point 0 twice
    kfs[0] = entries
    return _orbx().covis_slice(kfs, lists=[0, (-1, entries)], n_points=50, ranks=_ranks(rng, 64))


def ties_at_or_above(conn_weight, conn_offset, th=15):
    """connections whose weight equals their predecessor's in a list's ordered connections"""
    n = 0
    for q in range(len(conn_offset) - 1):
        w = [int(x) for x in conn_weight[conn_offset[q]:conn_offset[q + 1]]]
        n += sum(1 for a, b in zip(w, w[1:]) if a == b and a >= th)
    return n


class _Builder:
    def __init__(self, NK):
        self.kfs = [[] for _ in range(NK)]
        self.M = 0

    def add(self, n, observers, close=None):
        """n new points, each observed by every (slot, octave, stereo) of `observers`"""
        for i in range(n):
            for k, octave, stereo in observers:
                self.kfs[k].append((self.M, octave, stereo, 1 if close is None else close(i)))
            self.M += 1

    def slice(self, lists, ranks, flags=None):
        return _orbx().covis_slice(self.kfs, lists=lists, n_points=self.M, ranks=ranks, flags=flags)


CASCADE_CULLED = (0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def cascade_scene():
    """12 local keyframes (slots 0..11, in this order) and two outside observers.  Keyframes 1, 2 and 7 are culled and erased; keyframe 5 between them
    is culled but mbNotErase; keyframe 0 has mnId 0.  Keyframe 3 is redundant only until 1 and 2 are gone (its `culled` differs from an evaluation
    against the initial state), and the 8 points that keyframe 1 sees in stereo and keyframe 6 in mono go bad with keyframe 1 (keyframe 6's n_mps differs)."""
    b = _Builder(14)
    m = lambda *ks: [(k, 0, 0) for k in ks]      # noqa: E731  mono observers at octave 0
    b.add(30, m(0, 8, 9, 10))                    # Z: keyframe 0 would be culled
    b.add(100, m(1, 2, 3, 4, 12))                # A
    b.add(8, [(1, 0, 1), (6, 0, 0)])             # C: Observations() = 3, 1 after keyframe 1 is erased
    b.add(5, m(3)); b.add(5, m(4))
    b.add(60, m(5, 8, 9, 10))                    # E: keyframe 5 is redundant, and mbNotErase
    b.add(50, m(6))
    b.add(50, m(7, 8, 9, 10, 11)); b.add(2, m(7))      # D
    for k in (8, 9, 10):
        b.add(400, m(k))
    b.add(100, m(11), close=lambda i: i & 1)
    b.add(10, [(11, 0, 0), (8, 2, 0), (9, 2, 0), (10, 2, 0), (13, 1, 1)])      # G: for keyframe 11 only slot 13 is within one octave
    flags = np.zeros(14, np.uint8)
    flags[0], flags[5] = 1, 2
    return b.slice(list(range(12)), _ranks(np.random.default_rng(11), 14), flags)


@functools.lru_cache(maxsize=None)
def all_culled_scene(K, empty_first=False):
    """K keyframes that all see the same 40 points, four outside observers: every keyframe is culled in turn (K rounds; the last erase publishes).
    empty_first: list 0 belongs to a keyframe without points"""
    b = _Builder(K + 4 + (1 if empty_first else 0))
    b.add(40, [(k, k % 3, k & 1) for k in range(K + 4)])
    lists = ([K + 4] if empty_first else []) + list(range(K))
    return b.slice(lists, _ranks(np.random.default_rng(K), len(b.kfs)))


@functools.lru_cache(maxsize=None)
def no_cull_scene(K):
    """nothing is redundant: every point has at most three observers; keyframe K-1 has no points at all"""
    b = _Builder(K + 1)
    for k in range(K - 1):
        b.add(25, [(k, 1, 0)])
        b.add(10, [(k, 0, 1), ((k + 1) % max(K - 1, 1), 0, 0)] if K > 2 else [(k, 0, 1)])
        b.add(5, [(k, 0, 0), (K, 0, 0)])
    return b.slice(list(range(K)), _ranks(np.random.default_rng(100 + K), K + 1))


@functools.lru_cache(maxsize=None)
def random_cull_scene(seed, K=12, P=600):
    """dense random covisibility: most points with 5 to 11 of K + 3 observers, a fifth with 1 to 3, octaves 0..2, a third stereo, random flags and
    depths, some points bad"""
    rng = np.random.default_rng(seed)
    NK = K + 3
    b = _Builder(NK)
    for _ in range(P):
        who = rng.permutation(NK)[:int(rng.integers(1, 4) if rng.random() < 0.06 else rng.integers(5, 12))]
        b.add(1, [(int(k), int(rng.integers(0, 3)), int(rng.random() < 0.33)) for k in who], close=lambda i: int(rng.random() < 0.9))
    for k in range(NK):
        rng.shuffle(b.kfs[k])      # feature order is not point order
    flags = np.where(rng.random(NK) < 0.15, 2, 0).astype(np.uint8)
    flags[int(rng.integers(0, K))] |= 1
    s = b.slice([int(k) for k in rng.permutation(K)], _ranks(rng, NK), flags)
    s["point_bad"] = (rng.random(b.M) < 0.03).astype(np.uint8)
    return s


def latency_keyframes(seed, Q, points=1000, observers=8, NK=None):
    """tools/latency_covis.py: Q keyframes of `points` map points with about `observers` observers each, drawn from a window of neighbouring keyframes"""
    rng = np.random.default_rng(seed)
    NK = max(Q + 40, 64) if NK is None else NK
    M = Q * points // 4 + points
    n = rng.integers(max(2, observers - 3), observers + 4, M)
    off = np.zeros(M + 1, np.int32)
    off[1:] = np.cumsum(n)
    centre = rng.integers(0, NK, M)
    kf = np.concatenate([(centre[p] + rng.permutation(40)[:n[p]]) % NK for p in range(M)]).astype(np.int32)
    T = len(kf)
    lp = np.concatenate([rng.integers(0, M, points) for _ in range(Q)]).astype(np.int32)
    S = len(lp)
    return dict(kf_rank=_ranks(rng, NK), kf_flags=np.zeros(NK, np.uint8), obs_offset=off, obs_kf=kf, obs_octave=rng.integers(0, 4, T).astype(np.uint8),
                obs_stereo=rng.integers(0, 2, T).astype(np.uint8), point_bad=np.zeros(M, np.uint8), list_offset=(np.arange(Q + 1) * points).astype(np.int32),
                list_kf=rng.permutation(NK)[:Q].astype(np.int32), list_point=lp, list_octave=rng.integers(0, 4, S).astype(np.uint8), list_close=np.ones(S, np.uint8))


def compact_list(s, q):
    """list q as a call of its own: only the points under the list (renumbered), every keyframe slot"""
    a, b = int(s["list_offset"][q]), int(s["list_offset"][q + 1])
    lp = np.asarray(s["list_point"])[a:b]
    pts, inv = np.unique(lp, return_inverse=True)
    off = np.asarray(s["obs_offset"])
    n = off[pts + 1] - off[pts]
    new_off = np.zeros(len(pts) + 1, np.int32)
    new_off[1:] = np.cumsum(n)
    idx = np.concatenate([np.arange(off[p], off[p + 1]) for p in pts]) if len(pts) else np.zeros(0, np.int64)
    t = dict(s)
    t.update(obs_offset=new_off, obs_kf=np.asarray(s["obs_kf"])[idx], obs_octave=np.asarray(s["obs_octave"])[idx], obs_stereo=np.asarray(s["obs_stereo"])[idx],
             point_bad=np.asarray(s["point_bad"])[pts], list_offset=np.array([0, b - a], np.int32), list_kf=np.asarray(s["list_kf"])[q:q + 1].copy(),
             list_point=inv.astype(np.int32), list_octave=np.asarray(s["list_octave"])[a:b].copy(), list_close=np.asarray(s["list_close"])[a:b].copy())
    return t


def latency_culling(K, culls, home=1000):
    """tools/latency_covis.py: K local keyframes; keyframe k sees its own `home` points and those of keyframes k+1 and k+2 (three observers per point:
    nothing is redundant), except `culls` keyframes spread over the list that see only their own points, which four outside keyframes see too: those are
    culled"""
    b = _Builder(K + 4)
    chosen = set(((i + 1) * K) // (culls + 1) for i in range(culls))
    rest = [k for k in range(K) if k not in chosen]
    for k in range(K):
        if k in chosen:
            b.add(home, [(k, 0, 0)] + [(K + j, 0, 0) for j in range(4)])
        else:
            i = rest.index(k)
            b.add(home, [(k, 0, 0), (rest[(i + 1) % len(rest)], 0, 0), (rest[(i + 2) % len(rest)], 1, 1)])
    return b.slice(list(range(K)), _ranks(np.random.default_rng(K + culls), K + 4))
