"""Helpers of the tests that run ComputeBoW / SearchByBoW at the shape of the reference's own vocabulary: k = 10, L = 6 (about 10^6 words,
1.1 M nodes, FeatureVector keys = the at most 100 nodes of tree level 2).  Not a test module and not a conftest: the two trees, the
descriptor sets that exercise them, a census of what a descriptor set exercises, and the recorded results of the compiled reference
(tests/golden/slam/voc_k10_L6_*.npz, written by tools/gen_golden_bow_l6.py)."""
import hashlib
import importlib
from pathlib import Path

import numpy as np

import oracle_lib

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "slam"

# "ragged": inner nodes with 5..10 children.  Its seed is one of the few whose tree has more than 90 nodes at level 2 (a typical one has
# about 56): the root has 10 children and they have 92 between them; levels 3..6 are as uneven as any.
TREES = {"full": dict(k=10, L=6, seed=6, ragged=False), "ragged": dict(k=10, L=6, seed=773, ragged=True)}
DESC_SEED = {"full": 61, "ragged": 62}
N_FIXTURE = 3000
SIZES = (1, 37, 1000, 2049, 3000)
LEVELSUP = (4, 2, 0, 6)
# floors of the census (conditions on the INPUTS at n = N_FIXTURE, asserted by every consumer; never lowered to fit a seed)
MIN_NODES, MIN_REPEATED_WORDS, MIN_TIES_PER_DEPTH, MIN_UNFILED = 90, 50, 20, 20

_POP = np.array([bin(v).count("1") for v in range(256)], np.uint8)
_trees, _fixtures = {}, {}


def _orbx():
    return importlib.import_module("self_commit_orb-slam2_amd")


def tree(name):
    """the tree, built once per process"""
    if name not in _trees:
        _trees[name] = _orbx().voc_synth.make_vocabulary_fast(**TREES[name])
    return _trees[name]


def _children(voc):
    """(first child, number of children) per node: ids are in BFS order, so `parent` ascends and the children of a node are contiguous"""
    if "_child" not in voc:
        par = np.asarray(voc["parent"])[1:]
        assert (np.diff(par) >= 0).all()
        ids = np.arange(voc["num_nodes"])
        lo = np.searchsorted(par, ids, "left")
        voc["_child"] = (lo + 1, np.searchsorted(par, ids, "right") - lo)
    return voc["_child"]


def _depths(voc):
    if "_depth" not in voc:
        first, count = _children(voc)
        depth = np.zeros(voc["num_nodes"], np.int32)
        lo, hi = 0, 1
        for d in range(1, voc["L"] + 1):               # level d = the children of level d - 1, one contiguous range of ids
            lo, hi = int(first[lo]), int(first[hi - 1] + count[hi - 1])
            depth[lo:hi] = d
        assert hi == voc["num_nodes"]
        voc["_depth"] = depth
    return voc["_depth"]


def descend(voc, d):
    """Plain numpy descent, first minimum wins: (path, ties) - path[i, l] = the node feature i passes at depth l + 1, ties[i, l] = more than
    one child was at the minimum distance there (the strict '<' of TemplatedVocabulary.h:1219-1229 then decides)."""
    first, count = _children(voc)
    desc, k, L = voc["desc"], voc["k"], voc["L"]
    d = np.ascontiguousarray(d, np.uint8)
    n = len(d)
    cur = np.zeros(n, np.int64)
    path, ties = np.zeros((n, L), np.int64), np.zeros((n, L), bool)
    col = np.arange(k)
    for l in range(L):
        idx = first[cur][:, None] + col[None, :]
        live = col[None, :] < count[cur][:, None]
        idx = np.where(live, idx, first[cur][:, None])
        dist = _POP[desc[idx] ^ d[:, None, :]].sum(2, dtype=np.int32)
        dist[~live] = 1 << 20
        best = dist.argmin(1)                            # (numpy's argmin returns the first minimum)
        ties[:, l] = (dist == dist.min(1)[:, None]).sum(1) > 1
        cur = idx[np.arange(n), best]
        path[:, l] = cur
    return path, ties


def _flip(d, rng, lo, hi):
    """lo..hi-1 random bit flips per row (positions drawn with replacement), in place"""
    n = len(d)
    cnt = rng.integers(lo, hi, n)
    bits = rng.integers(0, 256, (n, max(hi - 1, 1)))
    for j in range(hi - 1):
        r = np.flatnonzero(cnt > j)
        d[r, bits[r, j] >> 3] ^= (1 << (bits[r, j] & 7)).astype(np.uint8)
    return d


def _forced_ties(voc, rng, depth, want):
    """`want` descriptors whose descent meets two equidistant nearest children at `depth`: one of two siblings with exactly half of the bits
    in which the two differ flipped.  A candidate needs an even sibling distance and no third child nearer; every one is checked with
    descend() and more are drawn until `want` of them tie where they should."""
    first, count = _children(voc)
    desc = voc["desc"]
    parents = np.flatnonzero((_depths(voc) == depth - 1) & (count >= 2))
    out = []
    for _ in range(200):
        cand = []
        for p in rng.choice(parents, 2 * want):
            a, b = first[p] + rng.choice(count[p], 2, replace=False)
            diff = np.flatnonzero(np.unpackbits(desc[a] ^ desc[b]))
            if len(diff) == 0 or len(diff) % 2:
                continue
            x = np.unpackbits(desc[a])
            x[rng.choice(diff, len(diff) // 2, replace=False)] ^= 1
            cand.append(np.packbits(x))
        if cand:
            cand = np.stack(cand)
            _, ties = descend(voc, cand)
            out.extend(cand[ties[:, depth - 1]])
        if len(out) >= want:
            return np.stack(out[:want])
    raise AssertionError("no forced ties at depth %d" % depth)


def _descs_l6(voc, n, seed):
    """n descriptors that exercise an L = 6 tree, shuffled.  Of max(n, 120) drawn (a smaller n takes a random subset):
      - leaf descriptors with 0-29 flipped bits (what is left, about two thirds);
      - pure noise (10 %);
      - REPEATED WORDS (12 %): 2-8 copies of one positive-weight leaf with 0-2 flips each: the BowVector sums and the (word, i) /
        (node, i) tie orders;
      - FORCED TIES (6 %, the same number at every depth 1..L): see _forced_ties;
      - descriptors on ZERO-WEIGHT words (5 %, 0-2 flips): not filed, node -1."""
    rng = np.random.default_rng(seed)
    m = max(n, 120)
    L = voc["L"]
    leaves = np.flatnonzero(voc["is_leaf"])
    wt = voc["weight"][leaves]
    pos, zero = leaves[wt > 0], leaves[wt == 0]
    per_depth = -(-6 * m // (100 * L))
    parts = [_forced_ties(voc, rng, dpt, per_depth) for dpt in range(1, L + 1)]
    n_rep, rep = -(-12 * m // 100), []
    while len(rep) < n_rep:
        rep.extend([rng.choice(pos)] * int(rng.integers(2, 9)))
    parts.append(_flip(voc["desc"][np.array(rep)].copy(), rng, 0, 3))
    parts.append(_flip(voc["desc"][rng.choice(zero, -(-5 * m // 100))].copy(), rng, 0, 3))
    parts.append(rng.integers(0, 256, (m // 10, 32), dtype=np.uint8))
    rest = m - sum(len(p) for p in parts)
    parts.append(_flip(voc["desc"][rng.choice(leaves, rest)].copy(), rng, 0, 30))
    d = np.concatenate(parts)
    return np.ascontiguousarray(d[rng.permutation(len(d))[:n]])


def desc_digest(d):
    return hashlib.sha256(np.ascontiguousarray(d, np.uint8).tobytes()).hexdigest()


def census(voc, d, word, weight, fv_node):
    """What a descriptor set exercises, from a transform's results at levelsup = 4 that did NOT come from the HIP kernels (restatement,
    compiled reference or fixture) and a numpy descent: [distinct filed nodes, words filed more than once, unfiled features, descents with
    a tie for the minimum at depth 1..L]."""
    filed = np.asarray(weight) > 0
    assert (filed == (np.asarray(fv_node) >= 0)).all()
    _, cnt = np.unique(np.asarray(word)[filed], return_counts=True)
    _, ties = descend(voc, d)
    return np.array([len(np.unique(np.asarray(fv_node)[filed])), int((cnt > 1).sum()), int((~filed).sum())] + [int(t) for t in ties.sum(0)], np.int64)


def assert_census(c):
    assert c[0] >= MIN_NODES and c[1] >= MIN_REPEATED_WORDS and c[2] >= MIN_UNFILED and (c[3:] >= MIN_TIES_PER_DEPTH).all(), c


def fixture(name):
    """recorded results of the compiled reference on tree(name) and _descs_l6(tree, N_FIXTURE, DESC_SEED[name]).  Refuses to hand out
    anything unless the regenerated tree and descriptors are the recorded ones (a numpy whose Generator stream differs fails HERE)."""
    if name in _fixtures:
        return _fixtures[name]
    g = dict(np.load(GOLDEN / ("voc_k10_L6_%s.npz" % name)))
    voc = tree(name)
    assert _orbx().voc_synth.tree_digest(voc) == str(g["tree_digest"]), "the regenerated tree is not the one the fixture was recorded on"
    d = _descs_l6(voc, N_FIXTURE, int(g["desc_seed"]))
    assert desc_digest(d) == str(g["desc_digest"]), "the regenerated descriptors are not the ones the fixture was recorded on"
    _fixtures[name] = (g, d)
    return g, d


def restated(oracle, voc, d, levelsup):
    """restatement (oracle/match_oracle.cc: mo_voc_transform) in the reference's terms: word, weight, node, fv_node (-1 = not filed; with
    levelsup >= L the key is node 0), BowVector ids / values"""
    word, node, weight = oracle_lib.voc_transform(oracle, voc, d, levelsup)
    if voc["L"] - levelsup < 1:
        assert (node == 0).all()
    ids, vals = oracle_lib.bow_vector(word, weight)
    return dict(word=word, node=node, weight=weight, fv_node=np.where(weight > 0, node, -1).astype(np.int32), bow_ids=ids, bow_vals=vals)


def pair_l6(orbx, oracle, voc, n, seed):
    """Two feature sets for SearchByBoW whose groups are REAL level-2 nodes: A = _descs_l6, B = A with 0-7 flipped bits, a fifth of it twice,
    200 more from the tree, shuffled; node ids of the restatement at levelsup = 4 (-1 = not filed), MapPoint masks."""
    from test_matcher import _kps
    rng = np.random.default_rng(seed)
    dA = _descs_l6(voc, n, seed + 1000)
    kA = _kps(rng, n, orbx)
    dB = _flip(dA.copy(), rng, 0, 8)
    kB = kA.copy()
    kB["angle"] = (kA["angle"] + rng.normal(0, 4, n).astype(np.float32)) % 360
    dB = np.concatenate([dB, dB[: n // 5], _descs_l6(voc, 200, seed + 2000)])
    kB = np.concatenate([kB, kB[: n // 5], _kps(rng, 200, orbx)])
    p = rng.permutation(len(dB))
    kB, dB = kB[p], np.ascontiguousarray(dB[p])
    gA, gB = restated(oracle, voc, dA, 4)["fv_node"], restated(oracle, voc, dB, 4)["fv_node"]
    vA, vB = (rng.random(n) < 0.85).astype(np.uint8), (rng.random(len(dB)) < 0.9).astype(np.uint8)
    return kA, dA, kB, dB, gA, gB, vA, vB
