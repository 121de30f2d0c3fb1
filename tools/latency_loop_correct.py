"""What the loop correction calls cost (profiles/loop_correct_latency.txt), beside a one-thread host baseline.

CorrectLoop (orbx_loop_correct_sim3): groups of 20 / 50 / 100 keyframes (and 20 keyframes outside) whose lists hold about 1000 points each, every point
seen by 8 neighbouring keyframes.  PropagateGBA (orbx_loop_propagate_gba): 500 / 2000 keyframes, 20 of them not optimised, with 100k / 500k points of
which 60 % were optimised.  Device columns: wall clock of the C call alone (ctypes on marshalled arrays) and orbx_loop_last_timing, medians of --calls
calls after --warmup.  Host column: tools/loop_correct_host_baseline.cc (this project's plain C++ statement of the two loops on arrays, one thread,
no locks, no cv::Mat) on the same scene on this machine's host; its checksum must equal the device's.  One process, one device handle; the first
failure ends the run.  NOT measured: the shim's gather on real KeyFrame / MapPoint objects and real maps.  No reference timing exists.

    python tools/latency_loop_correct.py [--calls 9] [--out profiles/loop_correct_latency.txt]
"""
import argparse
import ctypes
import importlib
import shutil
import struct
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
BASELINE = ROOT / "tools" / "_build" / "loop_correct_host_baseline"
f4, f8 = np.float32, np.float64


def build_baseline():
    src = ROOT / "tools" / "loop_correct_host_baseline.cc"
    if BASELINE.exists() and BASELINE.stat().st_mtime >= src.stat().st_mtime:
        return BASELINE
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    BASELINE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run([cxx, "-O2", "-std=c++11", "-ffp-contract=off", "-o", str(BASELINE), str(src)], check=True)
    return BASELINE


def _poses(g, n):
    """n random rigid poses as (n,12) float32 rows and the centres SetPose stores for them"""
    import loop_ref as lr
    import loop_scenes as ls
    tcw = np.stack([ls.pose12(ls.rot(g.normal(size=3), float(g.uniform(0.1, 2.5))), g.normal(size=3) * 3.0) for _ in range(n)])
    return tcw, np.stack([lr.set_pose(lr.mat44(T))[0] for T in tcw])


def sim3_scene(G, seed=1, per_kf=1000, n_obs=8, n_out=20):
    """every point is seen by n_obs keyframes in a row (positions in the group order, the outside keyframes behind it); a keyframe's list holds the points
    it sees, so a list has about per_kf entries"""
    import loop_scenes as ls
    g = np.random.default_rng(seed)
    NK = G + n_out
    M = per_kf * NK // n_obs
    tcw, ow = _poses(g, NK)
    slot = g.permutation(NK).astype(np.int32)                      # position -> slot
    obs_pos = (g.integers(0, NK, M)[:, None] + np.arange(n_obs)[None, :]) % NK
    obs_kf = slot[obs_pos].astype(np.int32)
    pt = np.repeat(np.arange(M, dtype=np.int32), n_obs)
    flat = obs_pos.reshape(-1)
    keep = flat < G
    order = np.lexsort((g.random(int(keep.sum())), flat[keep]))    # by group position, shuffled inside a list
    counts = np.bincount(flat[keep], minlength=G)
    cur = G // 2
    T = tcw[slot[cur]].reshape(3, 4).astype(f8)
    scw = np.concatenate([ls.quat_of(ls.rot(g.normal(size=3), 0.05) @ T[:, :3]), 1.1 * T[:, 3] + 0.1, [1.1]])
    return dict(tcw=tcw, ow=ow.astype(f4), group_kf=slot[:G].copy(), current=cur, scw=scw, list_offset=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                list_point=pt[keep][order], pos=(g.normal(size=(M, 3)) * 4.0).astype(f4), point_bad=(g.random(M) < 0.02).astype(np.uint8), point_done=np.zeros(M, np.uint8),
                point_ref=obs_kf[:, 0].copy(), ref_scale=(1.2 ** g.integers(0, 8, M)).astype(f4), top_scale=np.full(M, 1.2 ** 7, f4),
                obs_offset=(np.arange(M + 1) * n_obs).astype(np.int32), obs_kf=obs_kf.reshape(-1))


def gba_scene(n, M, seed=2, n_free=20):
    g = np.random.default_rng(seed)
    parent = np.maximum(0, np.arange(n) - g.integers(1, 5, n)).astype(np.int32)
    parent[0] = -1
    in_gba = np.ones(n, np.uint8)
    in_gba[g.choice(np.arange(1, n), n_free, replace=False)] = 0
    tcw, _ = _poses(g, n)
    gba = tcw + (g.normal(size=tcw.shape) * 0.01).astype(f4)
    pos = (g.normal(size=(M, 3)) * 4.0).astype(f4)
    return dict(parent=parent, tcw=tcw, tcw_gba=gba.astype(f4), in_gba=in_gba, pos=pos, pos_gba=(pos + f4(0.01)).astype(f4), point_in_gba=(g.random(M) < 0.6).astype(np.uint8),
                point_bad=(g.random(M) < 0.02).astype(np.uint8), point_ref=g.integers(0, n, M).astype(np.int32))


def _bits(a):
    u = np.ascontiguousarray(a, f4).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((u * ((np.arange(len(u), dtype=np.uint64) % np.uint64(7)) + np.uint64(1))).sum(dtype=np.uint64))


def host(orbx, P, a, mode, reps):
    exe = build_baseline()
    if exe is None:
        return None, None
    with tempfile.TemporaryDirectory() as d:
        with open(Path(d) / "scene.bin", "wb") as f:
            if mode == 0:
                f.write(struct.pack("<8i", 0x4c4f4f50, P.num_keyframes, P.num_group, P.current, P.num_entries, P.num_points, P.num_obs, 0))
            else:
                f.write(struct.pack("<8i", 0x4c4f4f50, P.num_keyframes, P.num_points, 0, 0, 0, 0, 0))
            for k, _ in (orbx._LOOP_SIM3_ARRAYS if mode == 0 else orbx._LOOP_GBA_ARRAYS):
                f.write(a[k].tobytes())
        r = subprocess.run([str(exe), str(Path(d) / "scene.bin"), str(mode), str(reps)], capture_output=True, text=True, check=True)
    _, us, chk = r.stdout.split()
    return float(us) / 1e3, int(chk)


def call(orbx, lc, s):
    """(callable that runs the C call and returns its wall ms, checksum reader, mode, struct, arrays)"""
    keep = []
    P, a = orbx.loop_marshal(s, keep)
    sim3 = isinstance(P, orbx.LoopSim3Problem)
    fields = orbx.LOOP_SIM3_FIELDS if sim3 else orbx.LOOP_GBA_FIELDS
    sizes = dict(G=P.num_group, M=P.num_points) if sim3 else dict(n=P.num_keyframes, M=P.num_points)
    o = {k: np.zeros((max(sizes[sz], 1), w), dt) for k, dt, sz, w in fields}
    R = (orbx.LoopSim3Result if sim3 else orbx.LoopGbaResult)(*[o[k].ctypes.data for k, _, _, _ in fields])
    fn, h = (lc._L.orbx_loop_correct_sim3 if sim3 else lc._L.orbx_loop_propagate_gba), lc._h

    def run():
        t0 = time.perf_counter()
        rc = fn(h, ctypes.byref(P), ctypes.byref(R))
        t1 = time.perf_counter()
        orbx._check(rc)
        return (t1 - t0) * 1e3

    def chk():
        c = {k: _bits(o[k][:sizes[sz]]) for k, _, sz, _ in fields if o[k].dtype == f4}
        v = c["pos"] + 3 * c["normal"] + 5 * c["max_dist"] + 7 * c["min_dist"] + 11 * c["tiw"] if sim3 else c["pos"] + 3 * c["tcw_gba"]
        return v % (1 << 64)
    return run, chk, (0 if sim3 else 1), P, a, (keep, o)


def measure(a, lc, run):
    wall, dev = [], []
    for it in range(a.warmup + a.calls):
        w = run()
        if it >= a.warmup:
            wall.append(w)
            dev.append(lc.last_timing()[0])
    return float(np.median(wall)), float(np.percentile(wall, 10)), float(np.percentile(wall, 90)), float(np.median(dev)), lc.last_timing()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    lc = orbx.LoopCorrection()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_loop_*: medians of %d calls after %d; ms.  wall = the C call alone (p10, p90 beside it); device = orbx_loop_last_timing (the launch chain);" % (a.calls, a.warmup))
    say("host = tools/loop_correct_host_baseline.cc (plain arrays, one thread, no locks, no cv::Mat) on the same scene, this machine's host; `equal` = the host's")
    say("checksum of the float results is the device's.  Not measured: the shim's gather on real KeyFrame / MapPoint objects, real maps.")
    say("%-58s | %8s %8s %8s | %8s %4s | %8s | %s" % ("scene", "wall", "p10", "p90", "device", "lnch", "host", "results"))
    scenes = [("CorrectLoop G = %d, %d points, %d list entries", sim3_scene(G)) for G in (20, 50, 100)]
    scenes += [("PropagateGBA n = %d, 20 not optimised, %d points", gba_scene(n, M)) for n in (500, 2000) for M in (100000, 500000)]
    for name, s in scenes:
        run, chk, mode, P, arr, keep = call(orbx, lc, s)
        w = measure(a, lc, run)
        hms, hchk = host(orbx, P, arr, mode, a.calls)
        name = name % ((P.num_group, P.num_points, P.num_entries) if mode == 0 else (P.num_keyframes, P.num_points))
        say("%-58s | %8.3f %8.3f %8.3f | %8.3f %4d | %8s | %s" % (name, w[0], w[1], w[2], w[3], w[4], "-" if hms is None else "%.3f" % hms,
                                                                 "-" if hchk is None else ("equal" if hchk == chk() else "DIFFERENT")))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
