"""What the covisibility calls cost (profiles/covis_latency.txt), beside a one-thread host baseline.

UpdateConnections: one keyframe of 1000 / 2000 map points with about 8 observers each; Q = 50 / 500 such keyframes in ONE call against Q calls of one
keyframe (each with only its own points).  KeyFrameCulling: K = 20 / 50 / 100 local keyframes of 3000 entries with 0 / 3 culls.  Device columns: wall
clock of the C call alone (ctypes on marshalled arrays) and orbx_covis_last_timing, medians of --calls calls after --warmup.  Host column:
tools/covis_host_baseline.cc (this project's plain C++ statement of the two loops on std::map containers, one thread, no locks, no copies) on the
same scene on this machine's host; its checksum must equal the device's.  One process, one device handle; the first failure ends the run.
NOT measured: the shim's gather on real KeyFrame / MapPoint objects, real sequences.  No reference timing exists.

    python tools/latency_covis.py [--calls 9] [--out profiles/covis_latency.txt]
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
BASELINE = ROOT / "tools" / "_build" / "covis_host_baseline"


def build_baseline():
    src = ROOT / "tools" / "covis_host_baseline.cc"
    if BASELINE.exists() and BASELINE.stat().st_mtime >= src.stat().st_mtime:
        return BASELINE
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    BASELINE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run([cxx, "-O2", "-std=c++11", "-o", str(BASELINE), str(src)], check=True)
    return BASELINE


def host(orbx, s, mode, reps):
    exe = build_baseline()
    if exe is None:
        return None, None
    a = {k: np.ascontiguousarray(s[k], dt).reshape(-1) for k, dt in orbx._COVIS_ARRAYS}
    with tempfile.TemporaryDirectory() as d:
        with open(Path(d) / "scene.bin", "wb") as f:
            f.write(struct.pack("<6i", 0x434f5649, len(a["kf_rank"]), len(a["point_bad"]), len(a["obs_kf"]), len(a["list_kf"]), len(a["list_point"])))
            for k, _ in orbx._COVIS_ARRAYS:
                f.write(a[k].tobytes())
        r = subprocess.run([str(exe), str(Path(d) / "scene.bin"), str(mode), str(reps)], capture_output=True, text=True, check=True)
    _, us, chk = r.stdout.split()
    return float(us) / 1e3, int(chk)


def connect_call(orbx, cov, s):
    """(callable that runs the C call and returns its wall ms, checksum reader)"""
    keep = []
    S, a = orbx.covis_marshal(s, keep)
    Q = S.num_lists
    cap = Q + min(Q * S.num_keyframes, int(np.diff(a["obs_offset"])[a["list_point"]].sum()))
    o = [np.zeros(Q + 1, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q + 1, np.int32),
         np.zeros(cap, np.int32), np.zeros(cap, np.int32)]
    R = orbx.CovisConnections(o[0].ctypes.data, o[1].ctypes.data, o[2].ctypes.data, cap, o[3].ctypes.data, o[4].ctypes.data, o[5].ctypes.data, o[6].ctypes.data, o[7].ctypes.data, cap)
    fn, h = cov._L.orbx_covis_update_connections, cov._h

    def run():
        t0 = time.perf_counter()
        rc = fn(h, ctypes.byref(S), 15, ctypes.byref(R))
        t1 = time.perf_counter()
        orbx._check(rc)
        return (t1 - t0) * 1e3
    return run, lambda: int(o[2][:o[0][Q]].sum()) + 1000003 * int(o[5][Q]), keep


def cull_call(orbx, cov, s):
    keep = []
    S, a = orbx.covis_marshal(s, keep)
    Q, M = S.num_lists, S.num_points
    o = [np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.uint8), np.zeros(max(M, 1), np.uint8), np.zeros(max(M, 1), np.int32)]
    R = orbx.CovisCulling(*[x.ctypes.data for x in o])
    fn, h = cov._L.orbx_covis_keyframe_culling, cov._h

    def run():
        t0 = time.perf_counter()
        rc = fn(h, ctypes.byref(S), ctypes.byref(R))
        t1 = time.perf_counter()
        orbx._check(rc)
        return (t1 - t0) * 1e3
    return run, lambda: int(o[2].sum()) + 1000003 * int(o[1].sum()), keep


def measure(a, cov, run):
    wall, dev = [], []
    for it in range(a.warmup + a.calls):
        w = run()
        if it >= a.warmup:
            wall.append(w)
            dev.append(cov.last_timing()[0])
    return float(np.median(wall)), float(np.percentile(wall, 10)), float(np.percentile(wall, 90)), float(np.median(dev)), cov.last_timing()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    import covis_scenes as cs
    cov = orbx.Covisibility()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_covis_*: medians of %d calls after %d; ms.  wall = the C call alone (p10, p90 beside it); device = orbx_covis_last_timing (the chain, the host's" % (a.calls, a.warmup))
    say("decisions between culling rounds included); host = tools/covis_host_baseline.cc (std::map containers, one thread, no locks, no copies) on the same scene,")
    say("this machine's host; `equal` = the host's checksum of the results is the device's.  Not measured: the shim's gather on real objects, real sequences.")
    say("%-44s | %8s %8s %8s | %8s %4s | %8s | %s" % ("scene", "wall", "p10", "p90", "device", "lnch", "host", "results"))

    def row(name, w, hms, same, extra=""):
        say("%-44s | %8.3f %8.3f %8.3f | %8.3f %4d | %8s | %s%s" % (name, w[0], w[1], w[2], w[3], w[4], "-" if hms is None else "%.3f" % hms,
                                                                 "-" if same is None else ("equal" if same else "DIFFERENT"), extra))

    for pts in (1000, 2000):
        s = cs.latency_keyframes(pts, 1, points=pts)
        s = cs.compact_list(s, 0)
        run, chk, keep = connect_call(orbx, cov, s)
        w = measure(a, cov, run)
        hms, hchk = host(orbx, s, 0, a.calls)
        row("UpdateConnections 1 keyframe, %d points" % pts, w, hms, None if hchk is None else hchk == chk())
    for Q in (50, 500):
        s = cs.latency_keyframes(Q, Q)
        run, chk, keep = connect_call(orbx, cov, s)
        w = measure(a, cov, run)
        hms, hchk = host(orbx, s, 0, a.calls)
        row("UpdateConnections %d keyframes in one call" % Q, w, hms, None if hchk is None else hchk == chk())
        singles = [connect_call(orbx, cov, cs.compact_list(s, q)) for q in range(Q)]
        tot = []
        for it in range(a.warmup + a.calls):
            t = sum(r[0]() for r in singles)
            if it >= a.warmup:
                tot.append(t)
        say("%-44s | %8.3f %8.3f %8.3f | %8s %4s | %8s | %s" % ("  the same as %d calls of one keyframe" % Q, float(np.median(tot)), float(np.percentile(tot, 10)),
                                                             float(np.percentile(tot, 90)), "-", "-", "-", "sum of the calls' walls"))
    for K in (20, 50, 100):
        for culls in (0, 3):
            s = cs.latency_culling(K, culls)
            run, chk, keep = cull_call(orbx, cov, s)
            w = measure(a, cov, run)
            hms, hchk = host(orbx, s, 1, a.calls)
            row("KeyFrameCulling K = %d, %d culls" % (K, culls), w, hms, None if hchk is None else hchk == chk(), "; %d culled" % (chk() % 1000003))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
