"""Scenes for tests/test_loop_correction.py: problem dicts for LoopCorrection.CorrectLoop (sim3_scene) and PropagateGBA (gba_scene, chain_scene), built
to make the restatement's order-dependent parts matter: observers inside the group on both sides of a point's corrector, group orders that are not
slot orders, a relative rotation beyond the trace branch of the quaternion conversion, chains of non-optimised keyframes, unreached subtrees."""
import math

import numpy as np

import loop_ref as lr

f4, f8 = np.float32, np.float64


def rot(axis, ang):
    axis = np.asarray(axis, f8)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def pose12(R, t):
    T = np.zeros((3, 4), f4)
    T[:, :3], T[:, 3] = R, t
    return T.reshape(12)


def quat_of(R):
    """a float64 rotation -> (x, y, z, w), by the textbook formula on the largest of w, x, y, z (independent of the code under test)"""
    w = math.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 0.1:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    x = math.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    return np.array([x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x), (R[2, 1] - R[1, 2]) / (4 * x)])


def sim3_scene(G, M, seed, s=1.1, n_out=6, big=(), permute=True, special_lists=True):
    """A group of G keyframes around the current one and n_out keyframes outside it (more when a point of `big` needs more distinct observers).
    Points lie in front of the current camera; point i < len(big) has big[i] observers, the others 1..12.  From G >= 3 on, two points in five are built
    so that their corrector sits strictly inside the group order with an observer of the group on either side of it and one outside.  One group
    keyframe is rolled by 170 degrees about the optical axis against the current one (its relative rotation has a negative trace).  With
    special_lists (G >= 3) one list is empty and one holds a single entry; point 0 is in every other list.  5 % of the points are bad, 5 % done."""
    g = np.random.default_rng(seed)
    NK = max(G + n_out, max(list(big) + [0]))
    Rc, tc = rot(g.normal(size=3), 0.6), g.normal(size=3) * 2.0
    tcw = np.zeros((NK, 12), f4)
    slots = g.permutation(NK) if permute else np.arange(NK)
    group_kf = slots[:G].astype(np.int32)                         # the group's order is not the slot order
    cur = int(g.integers(1, G)) if G > 1 else 0                   # ... and the current keyframe is not first in it
    rolled = (cur + 1) % G if G > 1 else -1
    for j, k in enumerate(slots):
        if j < G:
            dR = rot([0, 0, 1], math.radians(170.0)) if j == rolled else rot(g.normal(size=3), float(g.uniform(0.02, 0.25)))
            R, t = dR @ Rc, dR @ tc + (g.normal(size=3) * 0.3 if j != cur else 0.0)
            if j == cur:
                R, t = Rc, tc
        else:
            R, t = rot(g.normal(size=3), float(g.uniform(0.1, 2.5))), g.normal(size=3) * 3.0
        tcw[k] = pose12(R, t)
    ow = np.stack([lr.set_pose(lr.mat44(T))[0] for T in tcw])   # as stored by the keyframes' last SetPose
    Rcf, tcf = tcw[group_kf[cur]].reshape(3, 4)[:, :3].astype(f8), tcw[group_kf[cur]].reshape(3, 4)[:, 3].astype(f8)
    dR = rot(g.normal(size=3), 0.05)
    scw = np.concatenate([quat_of(dR @ Rcf), s * (dR @ tcf) + g.normal(size=3) * 0.2, [s]])
    Xc = np.stack([g.uniform(-2, 2, M), g.uniform(-1.5, 1.5, M), g.uniform(3.0, 9.0, M)], 1) if M else np.zeros((0, 3))
    pos = ((Xc - tcf) @ Rcf).astype(f4)
    bad, done = (g.random(M) < 0.05).astype(np.uint8), (g.random(M) < 0.05).astype(np.uint8)
    free = [q for q in range(G)]
    empty = single = -1
    if special_lists and G >= 3:
        empty, single = free[-1], free[0]
        free = free[1:-1]
    members = [[] for _ in range(G)]
    obs = []
    outside = [int(k) for k in slots[G:]]
    for i in range(M):
        n_obs = int(big[i]) if i < len(big) else int(g.integers(1, 13))
        if i == 0 and free:
            mem = list(free)
        elif free:
            mem = sorted(int(q) for q in g.choice(free, size=min(len(free), int(g.integers(1, 4))), replace=False))
        else:
            mem = []
        o = []
        if G >= 3 and i > 0 and i % 5 < 2 and i >= len(big) and free:      # corrector strictly inside, observers before and behind it, one outside
            c = int(g.integers(1, G - 1))
            mem = [q for q in mem if q > c] + [c]
            o = [int(group_kf[int(g.integers(0, c))]), int(group_kf[int(g.integers(c + 1, G))]), outside[int(g.integers(0, len(outside)))]]
            n_obs = max(n_obs, 3)
        rest = [int(k) for k in g.permutation(NK) if int(k) not in o]
        o = o + rest[:n_obs - len(o)]
        obs.append([o[j] for j in g.permutation(len(o))])
        for q in mem:
            members[q].append(i)
    if single >= 0 and M:
        members[single] = [0]
    loff, lpt = [0], []
    for q in range(G):
        ent = [members[q][j] for j in g.permutation(len(members[q]))] if q != empty else []
        if len(ent) > 3:
            ent.insert(int(g.integers(0, len(ent))), -1)        # a NULL match
            ent.append(ent[1])                                   # and a point twice in one list
        lpt += ent
        loff.append(len(lpt))
    ooff = np.zeros(M + 1, np.int32)
    ooff[1:] = np.cumsum([len(o) for o in obs])
    ref = np.array([o[int(g.integers(0, len(o)))] if j % 3 else int(g.integers(0, NK)) for j, o in enumerate(obs)], np.int32).reshape(-1)
    return dict(tcw=tcw, ow=ow.astype(f4), group_kf=group_kf, current=cur, scw=scw.astype(f8), list_offset=np.array(loff, np.int32), list_point=np.array(lpt, np.int32).reshape(-1),
                pos=pos.reshape(-1, 3), point_bad=bad, point_done=done, point_ref=ref, ref_scale=(1.2 ** g.integers(0, 8, M)).astype(f4), top_scale=np.full(M, 1.2 ** 7, f4),
                obs_offset=ooff, obs_kf=np.array([k for o in obs for k in o], np.int32).reshape(-1))


def gba_scene(n, M, seed, n_free=None, n_out=2, origins=1):
    """A random spanning tree over n keyframes (parent[i] < i); n_free of them (default about a fifth) were not optimised, among them a run of parent and
    child; n_out keyframes (and what hangs below them) are outside the tree.  The optimised poses are the old ones moved a little; those of the
    non-optimised keyframes hold a finite sentinel that must not reach any result.  Points are generated in front of their reference keyframe; 5 % are
    bad, 5 % have no reference, 60 % were optimised."""
    g = np.random.default_rng(seed)
    parent = np.array([-1] + [int(g.integers(0, i)) for i in range(1, n)], np.int32)
    for k in range(1, min(origins, n)):
        parent[k] = -1
    if n > 8:
        parent[g.choice(np.arange(4, n), size=min(n_out, n - 4), replace=False)] = -2
    in_gba = np.ones(n, np.uint8)
    nf = max(1, n // 5) if n_free is None else n_free
    if n > 1 and nf:
        free = g.choice(np.arange(1, n), size=min(nf, n - 1), replace=False)
        in_gba[free] = 0
        for k in free[:len(free) // 2]:                           # chains: a non-optimised keyframe's parent is not optimised either
            if parent[k] > 0:
                in_gba[parent[k]] = 0
    tcw, gba = np.zeros((n, 12), f4), np.zeros((n, 12), f4)
    for k in range(n):
        R, t = rot(g.normal(size=3), float(g.uniform(0.1, 2.5))), g.normal(size=3) * 3.0
        tcw[k] = pose12(R, t)
        dR = rot(g.normal(size=3), 0.03)
        gba[k] = pose12(dR @ R, dR @ t + g.normal(size=3) * 0.1) if in_gba[k] or parent[k] == -1 else np.full(12, 777.0, f4)
    ref = g.integers(0, n, M).astype(np.int32)
    ref[g.random(M) < 0.05] = -1
    Xc = np.stack([g.uniform(-2, 2, M), g.uniform(-1.5, 1.5, M), g.uniform(2.0, 9.0, M)], 1) if M else np.zeros((0, 3))
    pos = np.zeros((M, 3), f4)
    for i in range(M):
        T = tcw[max(int(ref[i]), 0)].reshape(3, 4).astype(f8)
        pos[i] = (Xc[i] - T[:, 3]) @ T[:, :3]
    return dict(parent=parent, tcw=tcw, tcw_gba=gba, in_gba=in_gba, pos=pos, pos_gba=(pos + g.normal(size=(M, 3)).astype(f4) * f4(0.05)).astype(f4),
                point_in_gba=(g.random(M) < 0.6).astype(np.uint8), point_bad=(g.random(M) < 0.05).astype(np.uint8), point_ref=ref)


def chain_scene(k, M, seed):
    """origin (optimised) -> k non-optimised keyframes in a row -> an optimised keyframe -> a non-optimised one; every point hangs on the chain"""
    s = gba_scene(k + 3, M, seed, n_free=0, n_out=0)
    s["parent"] = np.arange(-1, k + 2, dtype=np.int32)
    s["in_gba"] = np.array([1] + [0] * k + [1, 0], np.uint8)
    s["tcw_gba"][1:k + 1] = 777.0
    s["tcw_gba"][k + 2] = 777.0
    s["point_in_gba"][:] = 0
    return s
