"""The two map-moving passes of the loop closer restated literally in numpy: correct_loop = LoopClosing::CorrectLoop's Sim3 propagation (reference
src/LoopClosing.cc:617-716), propagate_gba = the map update after global bundle adjustment (:930-1003).  Both are the SEQUENTIAL loops of the reference
with their side effects (a keyframe's SetPose is seen by every UpdateNormalAndDepth behind it; a parent's pose is replaced after its children were
handled), on the arithmetic of the project's OpenCV stand-in (oracle/cvshim/cvshim.hpp: float products of inner dimension 2..4 accumulated left to
right over ALL terms, Mat / double and cv::norm in double) and g2o's Sim3 in double (tests/optsim3_ref.py's group operations, which
test_essential_graph.py holds bit for bit against the device).  The dict keys are those of LoopCorrection.CorrectLoop / PropagateGBA."""
from collections import deque

import numpy as np

import optsim3_ref as g2o

f4, f8 = np.float32, np.float64


def mat44(T12):
    """(12) or (3,4) float32 rows -> the 4x4 cv::Mat the keyframe holds"""
    T = np.zeros((4, 4), f4)
    T[:3] = np.asarray(T12, f4).reshape(3, 4)
    T[3, 3] = 1.0
    return T


def matmul(A, B):
    """cv::Mat * cv::Mat in CV_32F with inner dimension 2..4: s = a0 b0; s = s + ak bk, left to right, every term kept (cvshim.hpp:419-435)"""
    A, B = np.asarray(A, f4), np.asarray(B, f4)
    assert 2 <= A.shape[1] <= 4 and A.shape[1] == B.shape[0]
    C = np.zeros((A.shape[0], B.shape[1]), f4)
    for i in range(A.shape[0]):
        for j in range(B.shape[1]):
            s = A[i, 0] * B[0, j]
            for k in range(1, A.shape[1]):
                s = s + A[i, k] * B[k, j]
            C[i, j] = s
    return C


def set_pose(Tcw):
    """KeyFrame::SetPose (src/KeyFrame.cc:93-114) -> (Ow (3), Twc (4,4)): Rwc = Rcw.t(), Ow = -Rwc * tcw, Twc = [Rwc | Ow] over 0 0 0 1"""
    Tcw = np.asarray(Tcw, f4)
    Rwc = Tcw[:3, :3].T.copy()
    neg = (Rwc.astype(f8) * -1.0).astype(f4)                     # operator-(Mat) = cvshim_scale(a, -1.0)
    Ow = matmul(neg, Tcw[:3, 3:4])
    Twc = np.eye(4, dtype=f4)
    Twc[:3, :3] = Rwc
    Twc[:3, 3:4] = Ow
    return Ow.reshape(3), Twc


def quat_branch(R):
    """which branch Eigen::Quaterniond(Matrix3d) takes: 3 = the trace, else the index of the dominant diagonal element"""
    R = np.asarray(R, f8).reshape(3, 3)
    if (R[0, 0] + R[1, 1]) + R[2, 2] > 0.0:
        return 3
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 2 if R[2, 2] > R[i, i] else i


def sim3_of_pose(T):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of a float pose"""
    T = np.asarray(T, f4)
    return g2o.sim3_from_Rts(T[:3, :3].astype(f8), T[:3, 3].astype(f8), 1.0)


def sim3_row(S):
    return np.array(list(S[0]) + list(S[1]) + [S[2]], f8)


def update_normal_and_depth(pos, observers, ow, ref, ref_scale, top_scale):
    """MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:477-521) with the centres as they stand -> (normal (3), max, min) or None without observations"""
    if len(observers) == 0:
        return None
    normal = np.zeros(3, f4)
    n = 0
    for k in observers:
        v = pos - ow[k]                                            # float
        s = 0.0
        for c in range(3):
            s = s + float(v[c]) * float(v[c])                      # cv::norm: double from 0
        normal = normal + (v.astype(f8) / np.sqrt(f8(s))).astype(f4)      # Mat / double: a double quotient, narrowed; the sum in float
        n += 1
    pc = pos - ow[ref]
    s = 0.0
    for c in range(3):
        s = s + float(pc[c]) * float(pc[c])
    dist = f4(np.sqrt(f8(s)))
    mx = dist * f4(ref_scale)
    mn = mx / f4(top_scale)
    return (normal.astype(f8) / f8(n)).astype(f4), mx, mn


def correct_loop(p):
    """-> the keys of LoopCorrection.CorrectLoop, and "branch" (G): quat_branch of every relative rotation Ric (3 for the current keyframe)"""
    tcw, ow = np.asarray(p["tcw"], f4).reshape(-1, 12), np.array(p["ow"], f4).reshape(-1, 3)      # ow: a copy, SetPose writes into it
    group, cur = [int(k) for k in np.asarray(p["group_kf"]).reshape(-1)], int(p["current"])
    scw = np.asarray(p["scw"], f8).reshape(8)
    Scw = ([float(v) for v in scw[:4]], [float(v) for v in scw[4:7]], float(scw[7]))
    loff, lpt = np.asarray(p["list_offset"]).reshape(-1), np.asarray(p["list_point"]).reshape(-1)
    pos = np.array(p["pos"], f4).reshape(-1, 3)
    bad, done = np.asarray(p["point_bad"]).reshape(-1).astype(bool), np.array(p["point_done"]).reshape(-1).astype(bool)
    ref, rsc, tsc = np.asarray(p["point_ref"]).reshape(-1), np.asarray(p["ref_scale"], f4).reshape(-1), np.asarray(p["top_scale"], f4).reshape(-1)
    ooff, okf = np.asarray(p["obs_offset"]).reshape(-1), np.asarray(p["obs_kf"]).reshape(-1)
    G, M = len(group), len(pos)
    out = dict(noncorrected=np.zeros((G, 8), f8), corrected=np.zeros((G, 8), f8), tiw=np.zeros((G, 12), f4), ow_new=np.zeros((G, 3), f4), scw_mat=np.zeros((G, 12), f4),
               pos=pos, corrected_by=np.full(M, -1, np.int32), normal=np.zeros((M, 3), f4), max_dist=np.zeros(M, f4), min_dist=np.zeros(M, f4), updated=np.zeros(M, np.uint8),
               branch=np.full(G, 3, np.int32))
    # :623-659
    _, Twc = set_pose(mat44(tcw[group[cur]]))                     # GetPoseInverse(): what the current keyframe's last SetPose stored
    corrected, noncorrected = [], []
    for g, k in enumerate(group):
        Tiw = mat44(tcw[k])
        if g != cur:
            Tic = matmul(Tiw, Twc)
            out["branch"][g] = quat_branch(Tic[:3, :3])
            corrected.append(g2o.sim3_mul(sim3_of_pose(Tic), Scw))
        else:
            corrected.append(Scw)
        noncorrected.append(sim3_of_pose(Tiw))
    # :664-716, in the order of the map
    for g, k in enumerate(group):
        Siw, Swi = noncorrected[g], g2o.sim3_inverse(corrected[g])
        for e in range(int(loff[g]), int(loff[g + 1])):
            i = int(lpt[e])
            if i < 0 or bad[i] or done[i]:
                continue
            X = [float(v) for v in pos[i]]
            pos[i] = np.array(g2o.sim3_map(Swi, g2o.sim3_map(Siw, X)), f8).astype(f4)
            done[i] = True
            out["corrected_by"][i] = g
            r = update_normal_and_depth(pos[i], okf[int(ooff[i]):int(ooff[i + 1])], ow, int(ref[i]), rsc[i], tsc[i])
            if r is not None:
                out["normal"][i], out["max_dist"][i], out["min_dist"][i], out["updated"][i] = r[0], r[1], r[2], 1
        q, t, s = corrected[g]
        R = g2o.quat_to_R(q)
        inv = 1.0 / s
        Tn = np.eye(4, dtype=f4)
        Tn[:3, :3] = R.astype(f4)
        Tn[:3, 3] = np.array([t[0] * inv, t[1] * inv, t[2] * inv], f8).astype(f4)
        ow[k], _ = set_pose(Tn)                                    # pKFi->SetPose(correctedTiw): seen by every point moved after this
        out["noncorrected"][g], out["corrected"][g] = sim3_row(noncorrected[g]), sim3_row(corrected[g])
        out["tiw"][g], out["ow_new"][g] = Tn[:3].reshape(12), ow[k]
        Sm = np.zeros((3, 4), f4)
        Sm[:, :3] = (s * R).astype(f4)                             # Converter::toCvMat(g2o::Sim3): toCvSE3(s * eigR, eigt)
        Sm[:, 3] = np.array(t, f8).astype(f4)
        out["scw_mat"][g] = Sm.reshape(12)
    return out


def propagate_gba(p):
    """-> the keys of LoopCorrection.PropagateGBA.  reached = the walk visits the keyframe; a point whose reference keyframe is not reached stays."""
    parent = [int(k) for k in np.asarray(p["parent"]).reshape(-1)]
    n = len(parent)
    pose = [mat44(T) for T in np.asarray(p["tcw"], f4).reshape(-1, 12)]       # Tcw, replaced by SetPose as the walk goes
    gba = [mat44(T) for T in np.asarray(p["tcw_gba"], f4).reshape(-1, 12)]
    flag = np.array(p["in_gba"]).reshape(-1).astype(bool)
    pos, pos_gba = np.array(p["pos"], f4).reshape(-1, 3), np.asarray(p["pos_gba"], f4).reshape(-1, 3)
    pin, pbad, pref = np.asarray(p["point_in_gba"]).reshape(-1), np.asarray(p["point_bad"]).reshape(-1), np.asarray(p["point_ref"]).reshape(-1)
    children = [[] for _ in range(n)]
    for c, k in enumerate(parent):
        if k >= 0:
            children[k].append(c)
    bef = [None] * n
    reached = np.zeros(n, np.uint8)
    todo = deque(k for k in range(n) if parent[k] == -1)
    while todo:      # :933-960
        k = todo[0]
        _, Twc = set_pose(pose[k])
        for c in children[k]:
            if not flag[c]:
                Tchildc = matmul(pose[c], Twc)
                gba[c] = matmul(Tchildc, gba[k])
                flag[c] = True
            todo.append(c)
        bef[k] = pose[k]
        pose[k] = gba[k]
        reached[k] = 1
        todo.popleft()
    moved = np.zeros(len(pos), np.uint8)
    for i in range(len(pos)):      # :966-1004
        if pbad[i]:
            continue
        if pin[i]:
            pos[i], moved[i] = pos_gba[i], 1
            continue
        r = int(pref[i])
        if r < 0 or not reached[r]:
            continue
        Xc = matmul(bef[r][:3, :3], pos[i].reshape(3, 1)) + bef[r][:3, 3:4]
        _, Twc = set_pose(pose[r])
        pos[i] = (matmul(Twc[:3, :3], Xc) + Twc[:3, 3:4]).reshape(3)
        moved[i] = 2
    return dict(tcw_gba=np.stack([T[:3].reshape(12) for T in gba]), reached=reached, pos=pos, moved=moved)
