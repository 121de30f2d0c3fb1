"""Literal restatement of the counting in KeyFrame::UpdateConnections (reference src/KeyFrame.cc:386-507), the vote of
Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1895-1955) and LocalMapping::KeyFrameCulling (src/LocalMapping.cc:873-956) over
the arrays of orbx_covis_slice.  std::map<KeyFrame*, ...> is a dict keyed by RANK and iterated in ascending rank; the culling is
the sequential loop with real erases (MapPoint::EraseObservation / SetBadFlag, src/MapPoint.cc:171-200, 219-236).  Keyframes
leave as slot numbers."""
import numpy as np


def _lists(s):
    off = np.asarray(s["list_offset"])
    return [(int(s["list_kf"][q]), range(int(off[q]), int(off[q + 1]))) for q in range(len(off) - 1)]


def update_connections_list(s, q, th=15):
    """one list -> dict(counter [(slot, weight)] in ascending rank, n_max, kf_max, conn [(slot, weight)] ordered)"""
    rank = [int(r) for r in s["kf_rank"]]
    slot_of = {r: k for k, r in enumerate(rank)}
    owner, entries = int(s["list_kf"][q]), range(int(s["list_offset"][q]), int(s["list_offset"][q + 1]))
    KFcounter = {}
    for e in entries:
        p = int(s["list_point"][e])
        if s["point_bad"][p]:
            continue
        for o in range(int(s["obs_offset"][p]), int(s["obs_offset"][p + 1])):      # (the order inside a point does not matter for a count)
            k = int(s["obs_kf"][o])
            if k == owner:
                continue
            KFcounter[rank[k]] = KFcounter.get(rank[k], 0) + 1
    counter = [(slot_of[r], KFcounter[r]) for r in sorted(KFcounter)]
    if not KFcounter:
        return dict(counter=[], n_max=0, kf_max=-1, conn=[])
    nmax, kfmax = 0, -1
    vPairs = []
    for r in sorted(KFcounter):      # map iteration
        w, k = KFcounter[r], slot_of[r]
        if w > nmax and (owner >= 0 or not (int(s["kf_flags"][k]) & 4)):      # Tracking.cc:1941 for a Frame
            nmax, kfmax = w, k
        if w >= th:
            vPairs.append((w, r))
    if not vPairs and kfmax >= 0:
        vPairs.append((nmax, rank[kfmax]))
    vPairs.sort()      # pair<int, KeyFrame*>: by weight, then by pointer
    conn = []
    for w, r in vPairs:
        conn.insert(0, (slot_of[r], w))      # push_front
    return dict(counter=counter, n_max=nmax, kf_max=kfmax, conn=conn)


def update_connections(s, th=15):
    """every list -> the CSR arrays of Covisibility.UpdateConnections"""
    rs = [update_connections_list(s, q, th) for q in range(len(s["list_kf"]))]
    i4 = np.int32

    def csr(key):
        off = np.zeros(len(rs) + 1, i4)
        off[1:] = np.cumsum([len(r[key]) for r in rs])
        flat = [x for r in rs for x in r[key]]
        return off, np.array([x[0] for x in flat], i4).reshape(-1), np.array([x[1] for x in flat], i4).reshape(-1)
    co, ck, cw = csr("counter")
    no, nk, nw = csr("conn")
    return dict(counter_offset=co, counter_kf=ck, counter_weight=cw, n_max=np.array([r["n_max"] for r in rs], i4), kf_max=np.array([r["kf_max"] for r in rs], i4),
                conn_offset=no, conn_kf=nk, conn_weight=nw)


def update_local_keyframes(s):
    t = dict(s)
    t["list_kf"] = np.full(len(s["list_kf"]), -1, np.int32)
    r = update_connections(t)
    return {k: r[k] for k in ("counter_offset", "counter_kf", "counter_weight", "n_max", "kf_max")}


class _Point:
    def __init__(self, s, p):
        self.bad = bool(s["point_bad"][p])
        self.obs = {}      # mObservations: slot -> (octave, stereo)
        self.nObs = 0
        for o in range(int(s["obs_offset"][p]), int(s["obs_offset"][p + 1])):
            k = int(s["obs_kf"][o])
            assert k not in self.obs, "a keyframe observes a point once"
            self.obs[k] = (int(s["obs_octave"][o]), bool(s["obs_stereo"][o]))
            self.nObs += 2 if s["obs_stereo"][o] else 1      # AddObservation

    def erase(self, k):      # MapPoint::EraseObservation
        if k in self.obs:
            self.nObs -= 2 if self.obs[k][1] else 1
            del self.obs[k]
            if self.nObs <= 2:
                self.bad = True      # SetBadFlag
                self.obs = {}


def keyframe_culling(s, sequential=True):
    """the loop of :884-955 with its erases (sequential=False: every keyframe against the initial state, what a naive parallel version would compute)"""
    pts = [_Point(s, p) for p in range(len(s["point_bad"]))]
    Q = len(s["list_kf"])
    n_mps, n_red, culled = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.uint8)
    for q, (owner, entries) in enumerate(_lists(s)):
        fl = int(s["kf_flags"][owner])
        if fl & 1:
            continue
        thObs, nMPs, nRedundant = 3, 0, 0
        for e in entries:
            pMP = pts[int(s["list_point"][e])]
            if pMP.bad:
                continue
            if not s["list_close"][e]:
                continue
            nMPs += 1
            if pMP.nObs > thObs:
                scaleLevel = int(s["list_octave"][e])
                nObs = 0
                for k, (octave, _) in pMP.obs.items():
                    if k == owner:
                        continue
                    if octave <= scaleLevel + 1:
                        nObs += 1
                        if nObs >= thObs:
                            break
                if nObs >= thObs:
                    nRedundant += 1
        n_mps[q], n_red[q] = nMPs, nRedundant
        if nRedundant > 0.9 * nMPs:
            culled[q] = 1
            if sequential and not (fl & 2):      # SetBadFlag: mbNotErase only marks mbToBeErased
                for p in pts:
                    p.erase(owner)
    return dict(n_mps=n_mps, n_redundant=n_red, culled=culled, point_bad=np.array([p.bad for p in pts], np.uint8).reshape(-1),
                point_obs=np.array([p.nObs for p in pts], np.int32).reshape(-1))
