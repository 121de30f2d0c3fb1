"""CPU statements of the vocabulary training (orbx_voc_train, csrc/orbx_voc_train.hip): what DBoW2's
TemplatedVocabulary::create(training_features, k, L, weighting, scoring) computes for 256-bit descriptors (reference
Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:557-996, FORB.cpp:28-101), with the three stated differences of include/orbx.h: counter-hash
draws keyed by (seed, heap slot of the node, draw number), an empty cluster keeps its centre, a cap on the assignment passes.

    create(...)          numpy, structured like the reference: the recursion, k-means++ with a loop over the features for the selection,
                         createWords, setNodeWeights through the real descent.  What the device is compared with.
    literal_create(...)  HKmeansStep, initiateClustersKMpp and meanValue loop by loop on Python lists; tiny inputs only, to prove create().
"""
import math

import numpy as np

M64 = (1 << 64) - 1
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def mix(z):
    """splitmix64's output function over a counter"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, slot, j):
    """top 53 bits of the hash of (seed, slot, j)"""
    return mix((mix((mix(seed & M64) + slot) & M64) + j) & M64) >> 11


def first_index(seed, slot, n):
    """RandomInt(0, n - 1), Random.cpp:47-50, with the draw for rand() / RAND_MAX"""
    return min(n - 1, int(math.floor((draw(seed, slot, 0) * 2.0 ** -53) * n)))


def cut_value(seed, slot, j, dist_sum):
    return ((draw(seed, slot, j) + 1) * 2.0 ** -53) * float(dist_sum)


def distances(feats, centre):
    """FORB::distance of every row of feats (n, 32) to one descriptor"""
    return _POP[feats ^ centre[None, :]].sum(1)


def mean_value(feats):
    """FORB::meanValue: bit i is set when count_i >= n / 2 + n % 2; unpackbits / packbits count bit 7 of a byte first, as FORB.cpp:51-58 does"""
    n = len(feats)
    s = np.unpackbits(feats, axis=1).sum(0)
    return np.packbits(s >= n // 2 + n % 2)


def seed_clusters(feats, k, seed, slot):
    """initiateClustersKMpp: the indices of the chosen features"""
    n = len(feats)
    chosen = [first_index(seed, slot, n)]
    min_d = distances(feats, feats[chosen[0]])
    while len(chosen) < k:
        if len(chosen) > 1:
            min_d = np.minimum(min_d, distances(feats, feats[chosen[-1]]))      # the last centre only
        dist_sum = int(min_d.sum())
        if dist_sum == 0:
            break
        cut = cut_value(seed, slot, len(chosen), dist_sum)
        up, pick = 0, n - 1
        for i, d in enumerate(min_d.tolist()):      # exact integers, compared as doubles
            up += d
            if float(up) >= cut:
                pick = i
                break
        chosen.append(pick)
    return chosen


def assign(feats, centres):
    """strict '<': the lowest cluster index wins ties (np.argmin returns the first minimum); also the distance to the winner"""
    d = np.stack([distances(feats, c) for c in centres], 1)
    a = d.argmin(1)
    return a, d[np.arange(len(feats)), a]


def kmeans_node(feats, k, seed, slot, max_iterations, trace=None):
    """One node with n > k features -> (centres, association, passes, hit the cap)."""
    centres = [feats[i].copy() for i in seed_clusters(feats, k, seed, slot)]
    last, passes, costs, empties = None, 0, [], 0
    while True:
        if last is not None:
            for c in range(len(centres)):
                g = feats[last == c]
                if len(g):
                    centres[c] = mean_value(g)
                else:
                    empties += 1      # keeps its previous centre
        cur, dist = assign(feats, centres)
        passes += 1
        costs.append(int(dist.sum()))
        if last is not None and (cur == last).all():
            capped = False
            break
        last = cur
        if passes >= max_iterations:
            capped = True
            break
    if trace is not None:
        trace.append(dict(slot=slot, n=len(feats), costs=costs, empties=empties, passes=passes, capped=capped))
    return centres, cur, passes, capped


def create(desc, image_counts, k, L, seed=0, weighting=TF_IDF, max_iterations=100, trace=None):
    """-> dict in voc_synth's format (k, L, parent, is_leaf, desc, weight, num_nodes) plus ni, num_words, passes_per_level,
    unconverged_nodes, depth (per node) and word_of (the word every training feature descends to)."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    parent, ndesc, children, depth = [0], [np.zeros(32, np.uint8)], [[]], [0]
    passes_per_level, unconverged = [0] * L, [0]

    def step(parent_id, idx, level, slot):      # HKmeansStep; idx = the node's features in training order
        feats = desc[idx]
        if len(idx) <= k:
            centres, groups = [f.copy() for f in feats], [idx[i:i + 1] for i in range(len(idx))]
        else:
            centres, a, passes, capped = kmeans_node(feats, k, seed, slot, max_iterations, trace)
            passes_per_level[level - 1] = max(passes_per_level[level - 1], passes)
            unconverged[0] += capped
            groups = [idx[a == c] for c in range(len(centres))]
        ids = []
        for c in centres:
            ids.append(len(parent))
            parent.append(parent_id); ndesc.append(c); children.append([]); depth.append(level)
        children[parent_id] = ids
        if level < L:
            for c, g in enumerate(groups):
                if len(g) > 1:
                    step(ids[c], g, level + 1, slot * k + c + 1)

    if len(desc):
        step(0, np.arange(len(desc)), 1, 0)
    n = len(parent)
    is_leaf = np.array([i > 0 and not children[i] for i in range(n)], np.uint8)
    word_id = np.full(n, -1, np.int64)
    word_id[is_leaf == 1] = np.arange(int(is_leaf.sum()))
    ndesc = np.stack(ndesc)
    # setNodeWeights: the real descent of every training feature, first minimum wins
    word_of = np.zeros(len(desc), np.int64)

    def descend(node, idx):
        if not children[node]:
            word_of[idx] = word_id[node]
            return
        a, _ = assign(desc[idx], ndesc[children[node]])
        for c, ch in enumerate(children[node]):
            if (a == c).any():
                descend(ch, idx[a == c])

    if len(desc):
        descend(0, np.arange(len(desc)))
    counts = np.asarray(image_counts, np.int64)
    assert counts.sum() == len(desc)
    ndocs, nwords = len(counts), int(is_leaf.sum())
    ni_word = np.zeros(max(nwords, 1), np.int64)
    at = 0
    for c in counts.tolist():
        ni_word[np.unique(word_of[at:at + c])] += 1
        at += c
    ni, weight = np.zeros(n, np.int32), np.zeros(n, np.float64)
    for i in np.nonzero(is_leaf)[0].tolist():
        ni[i] = ni_word[word_id[i]]
        if weighting in (TF, BINARY):
            weight[i] = 1.0
        elif ni[i] > 0:
            weight[i] = math.log(float(ndocs) / float(ni[i]))
    return dict(k=k, L=L, parent=np.array(parent, np.int32), is_leaf=is_leaf, desc=ndesc, weight=weight, num_nodes=n, ni=ni, num_words=nwords,
                passes_per_level=passes_per_level, unconverged_nodes=unconverged[0], depth=np.array(depth, np.int32), word_of=word_of)


# ------------------------------------------------------------------------------------------------------------------------------------
# The literal translation: descriptors are lists of 32 ints, every loop of the reference is a loop here.
# ------------------------------------------------------------------------------------------------------------------------------------
def lit_distance(a, b):
    dist = 0
    for i in range(32):
        v = a[i] ^ b[i]
        while v:
            dist += v & 1
            v >>= 1
    return dist


def lit_mean_value(descriptors):
    if len(descriptors) == 1:
        return list(descriptors[0])
    s = [0] * 256
    for d in descriptors:
        for j in range(32):
            p = d[j]
            if p & (1 << 7): s[j * 8] += 1
            if p & (1 << 6): s[j * 8 + 1] += 1
            if p & (1 << 5): s[j * 8 + 2] += 1
            if p & (1 << 4): s[j * 8 + 3] += 1
            if p & (1 << 3): s[j * 8 + 4] += 1
            if p & (1 << 2): s[j * 8 + 5] += 1
            if p & (1 << 1): s[j * 8 + 6] += 1
            if p & 1: s[j * 8 + 7] += 1
    mean = [0] * 32
    n2 = len(descriptors) // 2 + len(descriptors) % 2
    p = 0
    for i in range(256):
        if s[i] >= n2:
            mean[p] |= 1 << (7 - (i % 8))
        if i % 8 == 7:
            p += 1
    return mean


def lit_initiate_clusters(pfeatures, k, seed, slot):
    clusters = []
    min_dists = [float("inf")] * len(pfeatures)
    ifeature = first_index(seed, slot, len(pfeatures))
    clusters.append(list(pfeatures[ifeature]))
    for i in range(len(pfeatures)):
        min_dists[i] = lit_distance(pfeatures[i], clusters[-1])
    while len(clusters) < k:
        for i in range(len(pfeatures)):
            if min_dists[i] > 0:
                dist = lit_distance(pfeatures[i], clusters[-1])
                if dist < min_dists[i]:
                    min_dists[i] = dist
        dist_sum = 0.0
        for d in min_dists:
            dist_sum += d
        if dist_sum > 0:
            cut_d = cut_value(seed, slot, len(clusters), dist_sum)      # u in (0, 1]: never 0, the do-while does not repeat
            d_up_now = 0.0
            it = 0
            while it < len(min_dists):
                d_up_now += min_dists[it]
                if d_up_now >= cut_d:
                    break
                it += 1
            if it == len(min_dists):
                ifeature = len(pfeatures) - 1
            else:
                ifeature = it
            clusters.append(list(pfeatures[ifeature]))
        else:
            break
    return clusters


def literal_create(desc, k, L, seed=0, max_iterations=100):
    """-> (parent, is_leaf, descriptors, passes_per_level, unconverged_nodes) with the node ids HKmeansStep hands out."""
    features = [[int(b) for b in row] for row in np.asarray(desc, np.uint8).reshape(-1, 32)]
    nodes = [dict(parent=0, descriptor=[0] * 32, children=[])]
    passes_per_level, unconverged = [0] * L, [0]

    def hkmeans_step(parent_id, descriptors, current_level, slot):
        if not descriptors:
            return
        clusters, groups = [], []
        if len(descriptors) <= k:
            for i in range(len(descriptors)):
                groups.append([i])
                clusters.append(list(descriptors[i]))
        else:
            first_time, goon, passes = True, True, 0
            last_association, current_association = [], []
            while goon:
                if first_time:
                    clusters = lit_initiate_clusters(descriptors, k, seed, slot)
                else:
                    for c in range(len(clusters)):
                        cluster_descriptors = [descriptors[i] for i in groups[c]]
                        if cluster_descriptors:      # (difference 2: an empty cluster keeps its centre)
                            clusters[c] = lit_mean_value(cluster_descriptors)
                groups = [[] for _ in clusters]
                current_association = [0] * len(descriptors)
                for f in range(len(descriptors)):
                    best_dist = lit_distance(descriptors[f], clusters[0])
                    icluster = 0
                    for c in range(1, len(clusters)):
                        dist = lit_distance(descriptors[f], clusters[c])
                        if dist < best_dist:
                            best_dist = dist
                            icluster = c
                    groups[icluster].append(f)
                    current_association[f] = icluster
                passes += 1
                if first_time:
                    first_time = False
                else:
                    goon = False
                    for i in range(len(current_association)):
                        if current_association[i] != last_association[i]:
                            goon = True
                            break
                if goon:
                    last_association = list(current_association)
                    if passes >= max_iterations:      # (difference 3: the cap)
                        unconverged[0] += 1
                        goon = False
            passes_per_level[current_level - 1] = max(passes_per_level[current_level - 1], passes)
        for i in range(len(clusters)):
            nid = len(nodes)
            nodes.append(dict(parent=parent_id, descriptor=clusters[i], children=[]))
            nodes[parent_id]["children"].append(nid)
        if current_level < L:
            children_ids = nodes[parent_id]["children"]
            for i in range(len(clusters)):
                child_features = [descriptors[j] for j in groups[i]]
                if len(child_features) > 1:
                    hkmeans_step(children_ids[i], child_features, current_level + 1, slot * k + i + 1)

    hkmeans_step(0, features, 1, 0)
    parent = np.array([nd["parent"] for nd in nodes], np.int32)
    is_leaf = np.array([i > 0 and not nd["children"] for i, nd in enumerate(nodes)], np.uint8)
    return parent, is_leaf, np.array([nd["descriptor"] for nd in nodes], np.uint8), passes_per_level, unconverged[0]


def stage_seed(desc, offsets, slots, k, seed):
    """orbx_voc_seed_segments: chosen[s, j] = index inside segment s of the j-th centre, -1 where the seeding ended early"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    out = np.full((len(slots), k), -1, np.int32)
    for s, slot in enumerate(slots):
        f = desc[offsets[s]:offsets[s + 1]]
        ch = list(range(len(f))) if len(f) <= k else seed_clusters(f, k, seed, int(slot))
        out[s, :len(ch)] = ch
    return out


def stage_lloyd(desc, offsets, centres, num_centres, prev):
    """orbx_voc_lloyd_pass -> (centres, association, changed); centres (S, k, 32)"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    centres = np.array(centres, np.uint8).copy()
    assoc, changed = np.zeros(len(desc), np.int32), np.zeros(len(num_centres), np.uint8)
    for s, nc in enumerate(num_centres):
        lo, hi = offsets[s], offsets[s + 1]
        f = desc[lo:hi]
        if prev is not None:
            for c in range(nc):
                g = f[np.asarray(prev[lo:hi]) == c]
                if len(g):
                    centres[s, c] = mean_value(g)
        a, _ = assign(f, centres[s, :nc])
        assoc[lo:hi] = a
        changed[s] = prev is not None and (a != np.asarray(prev[lo:hi])).any()
    return centres, assoc, changed
