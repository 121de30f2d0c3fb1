"""Inputs of tests/test_voc_train.py: descriptor sets, image splits and the segment layouts of the two stage entry points."""
import numpy as np

import voc_train_ref as vr


def flip_bits(base, nflips, rng):
    """`base` (n, 32) with nflips[i] random bit flips in row i (drawn with replacement: a bit hit twice flips back)"""
    out = base.copy()
    nflips = np.asarray(nflips)
    for j in range(int(nflips.max()) if len(nflips) else 0):      # one flip per row and pass: the fancy-indexed xor sees every row once
        rows = np.nonzero(nflips > j)[0]
        b = rng.integers(0, 256, len(rows))
        out[rows, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return out


def clustered(n, seed, groups=6, flips=24, dup_every=0):
    """n descriptors around `groups` random centres; dup_every > 0: every dup_every-th descriptor repeats its predecessor"""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, (groups, 32), dtype=np.uint8)
    d = flip_bits(centres[rng.integers(0, groups, n)], rng.integers(0, flips + 1, n), rng)
    if dup_every:
        for i in range(1, n):
            if i % dup_every == 0:
                d[i] = d[i - 1]
    return d


def split_images(n, n_images, seed):
    """n features over n_images images of uneven size, some of them empty (every image counts in NDocs)"""
    rng = np.random.default_rng(seed)
    w = rng.random(n_images) ** 2
    w[rng.random(n_images) < 0.1] = 0.0
    if w.sum() == 0:
        w[0] = 1.0
    counts = np.floor(w / w.sum() * n).astype(np.int64)
    counts[int(np.argmax(w))] += n - counts.sum()
    assert counts.sum() == n and (counts >= 0).all()
    return counts


# the numpy restatement against the literal translation: (N, k, L, seed, dup_every)
TINY = [(1, 2, 1, 0, 0), (2, 2, 2, 1, 0), (3, 2, 3, 2, 0), (7, 3, 2, 3, 0), (11, 10, 1, 4, 0), (12, 10, 2, 5, 3), (25, 2, 3, 6, 0), (31, 3, 3, 7, 2),
        (40, 3, 2, 8, 0), (45, 10, 2, 9, 4), (60, 2, 3, 10, 5), (60, 10, 3, 11, 0), (33, 3, 3, 12, 1)]


def tiny(case):
    n, k, L, seed, dup = case
    d = clustered(n, 100 + seed, groups=4, flips=30, dup_every=dup)
    if dup == 1:      # all equal: dist_sum == 0 in the first round
        d[:] = d[0]
    return d


# small trees on the device: (k, L, N)
SMALL = [(k, L, n) for k, L in ((2, 3), (3, 2)) for n in (1, 2, 3, 4, 5, 17, 63, 64, 65, 100, 200, 257)]


def small(case):
    k, L, n = case
    d = clustered(n, 1000 * k + n, groups=5, flips=28, dup_every=7 if n >= 17 else 0)
    return d, split_images(n, max(1, min(9, n // 2 + 1)), n)


def duplicate_scene():
    """three equal descriptors in two images, k = 3: a trivial node whose clusters are the three copies; the descent sends every copy to the
    first of them, so the words of the other two get Ni = 0"""
    d = clustered(1, 77, groups=1, flips=40)
    return np.repeat(d, 3, 0), np.array([2, 1], np.int64)


def around_tree(n, n_images, seed, k=10, L=3):
    """n descriptors drawn around the leaves of a voc_synth.make_vocabulary tree with bit flips: a heavy-tailed number of samples per leaf
    (some leaves are seen once), 0 .. 20 flips per sample, a few samples far from every leaf; images of uneven size, some empty"""
    import importlib
    voc_synth = importlib.import_module("self_commit_orb-slam2_amd").voc_synth
    voc = voc_synth.make_vocabulary(k, L, seed)
    leaves = voc["desc"][voc["is_leaf"] == 1]
    rng = np.random.default_rng(seed + 1)
    w = rng.pareto(1.2, len(leaves)) + 0.01
    pick = rng.choice(len(leaves), n, p=w / w.sum())
    flips = rng.integers(0, 21, n)
    flips[rng.random(n) < 0.002] = 120
    return flip_bits(leaves[pick], flips, rng), split_images(n, n_images, seed + 2)


FULL = {"k10_L3_20000": dict(k=10, L=3, n=20000, images=300, seed=11), "k10_L4_50000": dict(k=10, L=4, n=50000, images=500, seed=12)}


def full(name):
    s = FULL[name]
    return around_tree(s["n"], s["images"], s["seed"], s["k"], 3)


# ---- the stage entry points ----
def mix_inverse(out):
    """the counter z with vr.mix(z) == out (every step of splitmix64's output function is a bijection of 64-bit words)"""
    def unshift(z, s):
        r, t = z, z >> s
        while t:
            r ^= t
            t >>= s
        return r
    z = unshift(out, 31)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & vr.M64
    z = unshift(z, 27)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & vr.M64
    z = unshift(z, 30)
    return (z - 0x9E3779B97F4A7C15) & vr.M64


def slot_for_draw(seed, j, r):
    """the slot for which vr.draw(seed, slot, j) == r: the stage entry point takes any 64-bit slot, so a test can place u exactly"""
    y = (mix_inverse(r << 11) - j) & vr.M64
    return (mix_inverse(y) - vr.mix(seed)) & vr.M64


STAGE_K = 3
STAGE_SEED = 5


def seed_stage_scene():
    """(descriptors, offsets, slots): runs of segments of 1, 2, k and k + 1 features, a segment from the last lane of a wave to the first of
    the next, one of all-equal descriptors, one segment of 5000 features between them, and two segments whose slots place u = 1 (cut_d ==
    dist_sum) and u = 2^-53 (cut_d below the first min_dist) in the first round."""
    k = STAGE_K
    sizes = [1, 2, k, k + 1] * 3 + [7]
    while sum(sizes) != 63:      # the next segment starts on lane 63 ...
        sizes.append(min(k + 1, 63 - sum(sizes)))
    sizes += [2]                 # ... and ends on lane 0 of the next wave
    sizes += [k + 2, 20, 5000] + [1, 2, k, k + 1] * 4 + [9, 9, 300]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    d = clustered(int(offsets[-1]), 31, groups=7, flips=26)
    equal = sizes.index(20)
    d[offsets[equal]:offsets[equal + 1]] = d[offsets[equal]]
    slots = [(s * 2654435761 + 17) % (1 << 40) for s in range(len(sizes))]
    nine = [i for i, n in enumerate(sizes) if n == 9]
    slots[nine[0]] = slot_for_draw(STAGE_SEED, 1, (1 << 53) - 1)
    slots[nine[1]] = slot_for_draw(STAGE_SEED, 1, 0)
    return d, offsets, np.array(slots, np.uint64), dict(equal=equal, u_one=nine[0], u_tiny=nine[1])


def lloyd_stage_scene():
    """(descriptors, offsets, centres (S, k, 32), num_centres, prev): the same ragged layout; hand-made segments: one with a centre that
    attracts no feature, one cluster of four features with exactly half the bits set in byte 0, one feature at distance 1 from two centres."""
    k = STAGE_K
    rng = np.random.default_rng(41)
    sizes = [1, 2, k, k + 1] * 2 + [37]
    while sum(sizes) != 63:
        sizes.append(min(k + 1, 63 - sum(sizes)))
    i_empty, i_tie, i_equi = len(sizes) + 1, len(sizes) + 2, len(sizes) + 3
    sizes += [2, 12, 4, 3, 5000, 1, 2, k, k + 1, 600]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n, S = int(offsets[-1]), len(sizes)
    d = clustered(n, 43, groups=5, flips=26)
    nc = np.array([min(k, max(1, sz)) for sz in sizes], np.int32)
    centres = np.zeros((S, k, 32), np.uint8)
    prev = np.zeros(n, np.int32)
    for s in range(S):
        lo, hi = offsets[s], offsets[s + 1]
        centres[s, :nc[s]] = d[rng.integers(lo, hi, nc[s])]
        prev[lo:hi] = rng.integers(0, nc[s], hi - lo)
    # a centre that attracts nothing: nobody is associated with cluster 2 and its centre is the complement of the segment's first feature
    lo, hi = offsets[i_empty], offsets[i_empty + 1]
    d[lo:hi] = flip_bits(np.repeat(d[lo:lo + 1], hi - lo, 0), rng.integers(0, 9, hi - lo), rng)
    prev[lo:hi] = rng.integers(0, 2, hi - lo)
    centres[i_empty, 2] = ~d[lo]
    # four features in one cluster, byte 0 = ff ff 00 00: count == n / 2 + n % 2 in those eight positions, the tie sets the bit
    lo = offsets[i_tie]
    d[lo:lo + 4] = d[lo]
    d[lo:lo + 2, 0] = 0xFF
    d[lo + 2:lo + 4, 0] = 0x00
    nc[i_tie] = 1
    prev[lo:lo + 4] = 0
    # a, a, g in cluster 0 (its mean is a), clusters 1 and 2 empty with centres one bit away from g each: g goes to the lower index
    lo = offsets[i_equi]
    d[lo + 1] = d[lo]
    d[lo + 2] = ~d[lo]
    nc[i_equi] = 3
    prev[lo:lo + 3] = 0
    centres[i_equi, 1] = d[lo + 2]
    centres[i_equi, 1, 5] ^= 0x10
    centres[i_equi, 2] = d[lo + 2]
    centres[i_equi, 2, 9] ^= 0x01
    return d, offsets, centres, nc, prev, dict(empty=i_empty, tie=i_tie, equi=i_equi)
