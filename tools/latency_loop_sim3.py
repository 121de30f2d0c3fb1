"""What the device chain of LoopClosing::ComputeSim3's refine step costs against what a caller had before it (profiles/loop_sim3_latency.txt,
DESIGN.md section 7.19).

(i)   chain        one orbx_loop_refine_sim3 for all H events: wall clock of the C call alone on marshalled arrays.
(ii)  calls alone  the same work with the parent commit's entry points, per event orbx_fuse_search twice and orbx_optimize_sim3: the time spent INSIDE
                   those C calls during one run of the composition (tests/loop_sim3_ref.py driving ORBmatcher.FuseSearch and Sim3Optimizer.OptimizeSim3);
                   the glue's time is excluded.
(iii) calls+numpy  the wall clock of that whole run: the C calls, their marshalling, and the projection / mutual check / gather / decision in numpy.
Synthetic scenes (tests/loop_sim3_scenes.py): every event is a good estimate of its candidate (the longest path: both searches find their matches, both
rounds of OptimizeSim3 run); further events of a candidate are its first with a few seeds withheld.  After a warm-up, --calls chain calls and --runs
composition runs: median, and the 10th / 90th percentile of the chain as its spread.  The per-kernel device times are those of one more, profiled call
(events between the launches).  The baseline is (ii) on the same machine in the same run.  One fresh process per shape, each under its own time limit (--limit);
a shape that fails or runs out of time ends the run.  NOT measured: real keyframes, the shim's gather and write-back on real KeyFrame / MapPoint objects, the Sim3 solve in front.

    python tools/latency_loop_sim3.py [--calls 50] [--runs 3] [--out profiles/loop_sim3_latency.txt]
"""
import argparse
import importlib
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import loop_sim3_ref as lr      # noqa: E402
import loop_sim3_scenes as ls      # noqa: E402
from latency_relocalize import _TimedLib      # noqa: E402

SHAPES = ((1, 1, 1000), (8, 1, 1000), (8, 3, 1000), (8, 8, 1000), (24, 3, 1000), (24, 8, 1000), (1, 1, 2000), (8, 8, 2000), (24, 8, 2000))      # H, candidates, slots
KERNELS = ("stage", "seed", "project", "search", "mutual", "optimise", "decide")
TH, TH2 = 7.5, 10.0


def scene(orbx, H, C, P):
    shared = min(P - 200, 900)      # at most ORBX_SIM3_OPT_MAX_PAIRS pairs
    kf1, cands, truth = ls.build(orbx, 2000 + H + C + P, [shared] * C, bow=60, decoys=40, extras=P - shared - 40)
    hyps = [ls.hypothesis(kf1, cands, truth, k % C, 50 + k, seeds=60 - k // C) for k in range(H)]
    return kf1, cands, hyps


def measure(orbx, H, C, P, calls, runs):
    """One shape -> its row of the table"""
    kf1, cands, hyps = scene(orbx, H, C, P)
    mt, mt2, so = orbx.ORBmatcher(0.75, True, max_features=4096, max_pairs=8), orbx.ORBmatcher(0.75, True, max_features=4096, max_pairs=8), orbx.Sim3Optimizer(1, 1024)
    call = mt.loop_refine_prepare(kf1, cands, hyps, th=TH, th2=TH2)
    got = call()
    t = []
    for it in range(5 + calls):
        t0 = time.perf_counter()
        rc = call.raw()
        t1 = time.perf_counter()
        assert rc == 0
        if it >= 5:
            t.append((t1 - t0) * 1e3)
    chain, lo, hi = float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))
    mt.track_kernel_times(True)
    assert call.raw() == 0
    km = mt.track_kernel_times()
    mt.track_kernel_times(False)
    acc = [0.0, 0]
    mt2._L = _TimedLib(mt2._L, ("orbx_fuse_search",), acc)
    so._L = _TimedLib(so._L, ("orbx_optimize_sim3",), acc)
    alone, whole, ncalls = [], [], 0
    for it in range(1 + runs):
        acc[0], acc[1] = 0.0, 0
        t0 = time.perf_counter()
        want = lr.run(kf1, cands, hyps, TH, TH2, False, lambda kf, pts: mt2.FuseSearch(kf, pts, False), lambda p, th2, fx: so.OptimizeSim3([p], th2=th2, fix_scale=fx)[0])
        t1 = time.perf_counter()
        if it >= 1:
            alone.append(acc[0] * 1e3)
            whole.append((t1 - t0) * 1e3)
            ncalls = acc[1]
    assert (got["status"] == want["status"]).all() and (got["n_inliers"] == want["n_inliers"]).all() and got["quat"].tobytes() == np.asarray(want["quat"], np.float64).tobytes()
    b, c = float(np.median(alone)), float(np.median(whole))
    mt2._L, so._L = mt2._L.L, so._L.L      # (the handles' destructors call through the library)
    return "%-3d %-2d %-5d %4d..%-4d       %7.3f (%6.3f .. %6.3f) %10.3f %8d %12.3f %18.2f %18.2f  %s" % (
        H, C, P, got["n_pairs"].min(), got["n_pairs"].max(), chain, lo, hi, b, ncalls, c, chain / b, chain / c, " | ".join("%.3f" % v for v in km))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds a shape may take")
    ap.add_argument("--shape", default=None, help="H,C,P: measure this one shape in this process and print its row")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "loop_sim3_latency.txt"))
    a = ap.parse_args()
    if a.shape:
        H, C, P = [int(v) for v in a.shape.split(",")]
        print("ROW " + measure(importlib.import_module("self_commit_orb-slam2_amd"), H, C, P, a.calls, a.runs), flush=True)
        return 0
    lines = ["# H events over C candidates, keyframes of P slots; milliseconds; chain = median (p10 .. p90) of %d calls; kernels = device ms of one profiled call:" % a.calls,
             "#   " + " | ".join(KERNELS),
             "# H  C  P     pairs(min..max)  chain                    calls_alone  n_calls  calls+numpy  chain/calls_alone  chain/calls+numpy  kernels"]
    # one fresh process per shape, each under its own time limit; a shape that fails or runs out of time ends the run (what was measured is kept)
    status = 0
    for H, C, P in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--shape", "%d,%d,%d" % (H, C, P), "--calls", str(a.calls), "--runs", str(a.runs)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        rows = [l[4:] for l in r.stdout.splitlines() if l.startswith("ROW ")]
        if r.returncode != 0 or len(rows) != 1:
            print("shape %d,%d,%d: exit status %d\n%s" % (H, C, P, r.returncode, (r.stdout + r.stderr)[-2000:]), flush=True)
            status = r.returncode or 1
            break
        print(rows[0], flush=True)
        lines.append(rows[0])
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
