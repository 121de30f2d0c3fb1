"""The scenes of tests/test_kfdb.py as lists of operations, generated once from a seed and replayed on the restatement (tests/kfdb_ref.py) and on the
device class alike:  ("add", id, words, values)  ("erase", id)  ("cov", id, ids)  ("clear",)  ("query", [query dicts]).
"""
import functools

import numpy as np

import kfdb_ref as kr

# name -> seed, n_words, keyframes, BowVector lengths, places, keyframes per visit.  The seeds are recorded here: with them the scenes together contain
# every case of test_kfdb.test_vacuity_guard, which asserts that on the restatement alone.
SCENES = {
    "w1000": dict(seed=3, n_words=1000, n_kf=300, lengths=(63, 64, 65), places=5, visit=6),
    "w1M": dict(seed=1, n_words=1000000, n_kf=120, lengths=(1, 63, 64, 65, 257, 1500), places=3, visit=6),
    "big": dict(seed=2, n_words=1000, n_kf=5000, lengths=(30, 31, 33), places=40, visit=8),
    "seq": dict(seed=5, n_words=1000, n_kf=140, lengths=(20, 64, 65), places=4, visit=5),
}
MAX_QUERY_WORDS = 1536


class _Gen:
    def __init__(self, name, seed=None):
        kw = dict(SCENES[name])
        if seed is not None:
            kw["seed"] = seed
        self.sc = kr.Scene(edge_words=True, **kw)
        self.rng = self.sc.rng
        self.present = set()
        self.ops = []

    def add(self, t, cov=True):
        w, v = self.sc.bows[t]
        self.ops.append(("add", t, w, v))
        self.present.add(t)
        if cov:
            self.cov(t)

    def cov(self, t):
        self.ops.append(("cov", t, self.sc.covisibles(t, self.present)))

    def erase(self, t):
        self.ops.append(("erase", t))
        self.present.discard(t)

    def query(self, qs):
        self.ops.append(("query", list(qs)))

    def pair(self, t):
        """a loop query of keyframe t and a relocalisation query of its place, one call each"""
        self.query([self.sc.loop_query(t, self.present)])
        self.query([self.sc.reloc_query(self.sc.place_of[t])])

    def batch(self, t, n=7):
        qs = []
        for i in range(n):
            u = max(0, t - i)
            qs.append(self.sc.loop_query(u, self.present) if i % 2 == 0 else self.sc.reloc_query(self.sc.place_of[u]))
        self.query(qs)

    def disjoint_query(self, mode):
        """a query that shares no word with any present keyframe"""
        used = set()
        for t in self.present:
            used.update(int(w) for w in self.sc.bows[t][0])
        free = [w for w in range(min(self.sc.n_words, 4000)) if w not in used][:40]
        v = np.full(len(free), 1.0 / max(len(free), 1))
        return dict(mode=mode, words=np.array(free, np.int32), values=v, connected=[], counts=[])


def _grow(name, sizes, seed=None):
    """keyframes added in order with queries at the database sizes `sizes`; a 7-query call and a relocalisation query behind it at the end"""
    g = _Gen(name, seed)
    n = g.sc.n_kf
    g.pair(0)      # the empty database
    g.query([dict(mode=kr.LOOP, words=np.zeros(0, np.int32), values=np.zeros(0), connected=[], counts=[])])
    for t in range(n):
        g.add(t)
        if len(g.present) in sizes:
            g.pair(t)
        if len(g.present) == 1:
            g.query([g.disjoint_query(kr.LOOP)])
            g.query([g.disjoint_query(kr.RELOC)])
            g.query([dict(mode=kr.RELOC, words=np.zeros(0, np.int32), values=np.zeros(0))])
        if len(g.present) == min(63, n // 2):      # every sharer is connected
            q = g.sc.loop_query(t, g.present)
            q["connected"] = sorted(g.present)
            q["counts"] = [1 + (i % 3) for i in range(len(q["connected"]))]
            g.query([q])
        if t % 37 == 36:      # connections change: the covisibles of some older keyframes are pushed again
            for u in range(t - 5, t):
                g.cov(u)
    g.batch(n - 1)
    g.pair(n - 1)
    g.query([g.sc.reloc_query(g.sc.place_of[n - 2])])
    g.batch(n - 3)
    return g.ops


def _big(seed=None):
    """5,000 keyframes, every third erased, some of those added again (behind a compaction), then queries"""
    g = _Gen("big", seed)
    n = g.sc.n_kf
    for t in range(n):
        g.add(t, cov=False)
    for t in range(0, n, 7):
        g.cov(t)
    g.pair(n - 1)
    for t in range(0, n, 3):
        g.erase(t)
    g.pair(n - 2)
    for t in range(0, n, 12):
        g.add(t)
    for t in range(n - 200, n):
        if t in g.present:
            g.cov(t)
    g.pair(n - 1)
    g.batch(n - 1)
    g.query([g.sc.reloc_query(g.sc.place_of[n - 1])])
    return g.ops


def _seq(seed=None):
    """200 steps of add / erase / set_covisibles / query in turn"""
    g = _Gen("seq", seed)
    rng = g.rng
    nxt = 0
    for step in range(200):
        kind = step % 4
        if kind == 0 or len(g.present) < 3:
            if nxt < g.sc.n_kf:
                g.add(nxt, cov=bool(rng.random() < 0.5))
                nxt += 1
        elif kind == 1:
            if rng.random() < 0.7:
                g.erase(int(rng.choice(sorted(g.present))))
            elif nxt < g.sc.n_kf:
                g.add(nxt)
                nxt += 1
        elif kind == 2:
            g.cov(int(rng.choice(sorted(g.present))))
        else:
            t = max(g.present)
            r = rng.random()
            if r < 0.4:
                g.query([g.sc.loop_query(t, g.present)])
            elif r < 0.8:
                g.query([g.sc.reloc_query(g.sc.place_of[t])])
            else:
                g.batch(t, 3)
        if step == 120:      # a keyframe leaves and comes back under its id: a new object
            t = min(g.present)
            g.erase(t)
            g.add(t)
    return g.ops


@functools.lru_cache(maxsize=None)
def ops(name, seed=None):
    if name == "w1000":
        return _grow(name, (1, 2, 63, 64, 65, 150, 300), seed)
    if name == "w1M":
        return _grow(name, (1, 64, 120), seed)
    if name == "big":
        return _big(seed)
    return _seq(seed)


def replay_ref(name, seed=None):
    """-> (results of every query call in order, the database after the scene, per call: (bows, seq, alive ids) needed by the order test)"""
    db = kr.KeyFrameDatabaseRef(SCENES[name]["n_words"])
    out, state = [], []
    seq, bows, n_add = {}, {}, 0
    for op in ops(name, seed):
        if op[0] == "add":
            db.add(op[1], op[2], op[3])
            seq[op[1]] = n_add
            bows[op[1]] = op[2]
            n_add += 1
        elif op[0] == "erase":
            db.erase(op[1])
            seq.pop(op[1], None)
        elif op[0] == "cov":
            db.set_covisibles(op[1], op[2])
        elif op[0] == "clear":
            db.clear()
            seq = {}
        else:
            out.append(db.query_batch(op[1]))
            state.append((dict(seq), {i: list(db.kfs[i].covisibles) for i in db.kfs}))
    return out, db, state, bows


@functools.lru_cache(maxsize=None)
def reference(name):
    return replay_ref(name)
