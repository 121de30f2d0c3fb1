"""What the device chain of LocalMapping::CreateNewMapPoints costs against what a caller had before it (profiles/new_points_latency.txt,
DESIGN.md section 7.3).

chain     one orbx_create_new_map_points: KF1 and the K neighbours staged once, per neighbour SearchForTriangulation + k_triangulate on the
          matcher's stream, k_collect, one wait.  Wall clock of the C call alone (ctypes call on marshalled arrays, no result dict); device
          time, launches and the share of k_triangulate from orbx_new_points_last_timing (a series of its own with profile_kernels: the events cost the others nothing).
baseline  what the parent commit offers for the same work: K synchronous orbx_search_for_triangulation calls, each followed on the host by
          the geometry of tests/triangulate_ref.py vectorised in numpy over the pair's matches and the eligibility update.  On the host the
          reference does at least that much arithmetic, one cv::Mat at a time.  Reported with and without the numpy geometry.
K = 10 and 20 neighbours of 1000 and 2000 features, mono and stereo; medians of --calls calls after --warmup.
One GPU process at a time: this process never opens the device; every shape runs in a child of its own under `timeout -k 10 --step-seconds`
(a hung chain sits inside the C call, where no Python signal handler runs: only an outer timeout ends it), and the first child that fails or
is killed ends the run - nothing more is started on the device.  NOT measured: real keyframes, and the reference's own CreateNewMapPoints on
the CPU (src/LocalMapping.cc is not part of the compiled oracle).

    python tools/latency_new_points.py [--calls 200] [--out profiles/new_points_latency.txt]
"""
import argparse
import ctypes
import importlib
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import triangulate_ref as tr      # noqa: E402


def baseline_prepare(orbx, mt, sc):
    """the K synchronous calls on prebuilt ctypes structs; KF1's validity array is updated in place between the calls"""
    L = mt._L
    kf1 = sc["kf1"]
    n1 = len(kf1["kps"])
    ok1 = (np.asarray(kf1["has_mp"], np.uint8) == 0).astype(np.uint8)
    fs1, keep1 = orbx._host_set(kf1["kps"], kf1["desc"], kf1["groups"], ok1)
    ok1 = keep1[-1]
    st1 = np.ascontiguousarray((kf1["u_right"] >= 0) if kf1.get("u_right") is not None else np.zeros(n1, bool), np.uint8)
    per = []
    for nb in sc["neighbours"]:
        fs2, keep2 = orbx._host_set(nb["kps"], nb["desc"], nb["groups"], (np.asarray(nb["has_mp"], np.uint8) == 0).astype(np.uint8))
        st2 = np.ascontiguousarray((nb["u_right"] >= 0) if nb.get("u_right") is not None else np.zeros(len(nb["kps"]), bool), np.uint8)
        f12, epi = np.ascontiguousarray(nb["F12"], np.float32).reshape(9), np.ascontiguousarray(nb["epipole"], np.float32).reshape(2)
        sf, s2 = np.ascontiguousarray(nb["g"]["scale_factors"], np.float32), np.ascontiguousarray(nb["g"]["level_sigma2"], np.float32)
        prm = orbx.TriangulationParams(f12.ctypes.data, epi.ctypes.data, st1.ctypes.data, st2.ctypes.data, sf.ctypes.data, s2.ctypes.data, len(sf), 0)
        per.append((fs2, prm, [keep2, st2, f12, epi, sf, s2]))
    initial = ok1.copy()
    out = np.full(max(n1, 1), -1, np.int32)
    nm = ctypes.c_int32()

    def run(geometry):
        ok1[:] = initial
        t_calls = 0.0
        created = 0
        for k, (fs2, prm, _) in enumerate(per):
            t0 = time.perf_counter()
            orbx._check(L.orbx_search_for_triangulation(mt._h, ctypes.byref(fs1), ctypes.byref(fs2), ctypes.byref(prm), orbx._ptr(out), ctypes.byref(nm)))
            t_calls += time.perf_counter() - t0
            if geometry:
                i1 = np.nonzero(out[:n1] >= 0)[0]
                nb = sc["neighbours"][k]
                r = tr.triangulate(kf1["g"], nb["g"], kf1, nb, i1, out[i1])
                acc = i1[(r["status"] >= tr.TRIANGULATED) & (r["status"] <= tr.STEREO2)]
                ok1[acc] = 0
                created += len(acc)
        return t_calls, created
    run.keep = [fs1, keep1, st1, per]
    return run


def run_shape(a, K, n, stereo):
    """child process: one shape, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    sc = tr.chain_scene(orbx, seed=7 + K + n, n=n, K=K, stereo_frac=stereo)
    mt = orbx.ORBmatcher(0.6, False, max_features=n)
    call = mt.new_points_prepare(sc["kf1"], sc["neighbours"], full=False)
    wall, dev = [], []
    for it in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        rc = call.raw()
        t1 = time.perf_counter()
        if rc != 0:
            orbx._check(rc)
        if it >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(mt.new_points_last_timing()[0])
    res = (float(np.median(wall)), float(np.percentile(wall, 10)), float(np.percentile(wall, 90)), float(np.median(dev)))
    got = call()
    prof = mt.new_points_prepare(sc["kf1"], sc["neighbours"], full=False, profile_kernels=True)
    share, launches = [], 0
    for it in range(20):
        prof()
        ms, launches, tri = mt.new_points_last_timing()
        share.append(100.0 * tri / ms)
    base = baseline_prepare(orbx, mt, sc)
    only, both, created = [], [], 0
    for it in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        tc, created = base(True)
        t1 = time.perf_counter()
        if it >= a.warmup:
            only.append(tc * 1e3)
            both.append((t1 - t0) * 1e3)
    mt.close()
    print("RESULT " + json.dumps(dict(chain=res, launches=launches, share=float(np.median(share)), only=float(np.median(only)),
                                      both=float(np.median(both)), created=int(got["count"]), created_numpy=int(created), nmatches=int(got["nmatches"].sum()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", nargs=3, default=None, help=argparse.SUPPRESS)      # K n stereo: run as the child of one shape
    a = ap.parse_args()
    if a.shape:
        return run_shape(a, int(a.shape[0]), int(a.shape[1]), float(a.shape[2]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_create_new_map_points (chain) against K synchronous orbx_search_for_triangulation calls + the geometry in numpy (baseline);")
    say("medians of %d calls after %d, ms, wall clock of the C calls.  Not measured: real keyframes, the reference's own CreateNewMapPoints" % (a.calls, a.warmup))
    say("on the CPU.")
    say("%-20s | %8s %8s %8s | %8s | %5s %7s | %10s %11s | %7s %7s | %s" % ("shape", "chain", "p10", "p90", "device", "launches"[:5], "k_tri %", "calls only",
                                                                              "calls+numpy", "matches", "created", "chain vs calls only / calls+numpy"))
    for K in (10, 20):
        for n in (1000, 2000):
            for stereo in (0.0, 1.0):
                name = "K=%d n=%d %s" % (K, n, "stereo" if stereo else "mono")
                cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, str(Path(__file__).resolve()), "--calls", str(a.calls), "--warmup", str(a.warmup),
                       "--shape", str(K), str(n), str(stereo)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                out = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not out:
                    say("%-20s | failed with status %d: stopped, nothing more is started on the device" % (name, r.returncode))
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    _write(a, lines)
                    return r.returncode or 1
                d = json.loads(out[0][7:])
                m = d["chain"]
                say("%-20s | %8.3f %8.3f %8.3f | %8.3f | %5d %7.1f | %10.3f %11.3f | %7d %7d | %.2fx / %.2fx%s"
                    % (name, m[0], m[1], m[2], m[3], d["launches"], d["share"], d["only"], d["both"], d["nmatches"], d["created"], d["only"] / m[0], d["both"] / m[0],
                       "" if d["created"] == d["created_numpy"] else "  (numpy created %d: matches on a threshold)" % d["created_numpy"]))
    _write(a, lines)
    return 0


def _write(a, lines):
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
