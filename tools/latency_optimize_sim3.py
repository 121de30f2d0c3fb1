"""What the device form of Optimizer::OptimizeSim3 costs (profiles/optimize_sim3_latency.txt).

One orbx_optimize_sim3 per call: the problems' pairs through mapped pinned memory, ONE launch of k_optsim3 (a workgroup per problem) on the
handle's stream, one wait.  Wall clock of the C call alone (ctypes call on marshalled arrays, no result objects), device time and launches from
orbx_sim3_optimizer_last_timing; medians of --calls calls after --warmup.  C = 1 / 8 problems of n = 30 / 100 / 300 pairs of the scenes of
tests/optsim3_ref.py (a tenth of the pairs outliers, th2 = 10, free scale), solved in ONE call, and the same problems solved one call each (the
sum of the C calls); `ratio` = wall each / wall.  The Levenberg iterations the problems ran are listed: the time follows them.
One GPU process at a time: this process never opens the device; every n runs in a child of its own under `timeout -k 10 --step-seconds`, and
the first child that fails or is killed ends the run - nothing more is started on the device.  Nothing on the parent commit does this work and
no C entry point of the compiled reference reaches OptimizeSim3: the numbers are a record, not a comparison.  NOT measured: real keyframes,
the shim.

    python tools/latency_optimize_sim3.py [--calls 200] [--out profiles/optimize_sim3_latency.txt]
"""
import argparse
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

import optsim3_ref as osr      # noqa: E402

SHAPES = (30, 100, 300)
PROBLEMS = (1, 8)
TH2 = 10.0


def run_shape(a, n):
    """child process: one n, every C, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    cmax = max(PROBLEMS)
    h = orbx.Sim3Optimizer(max_problems=cmax, max_pairs=n)
    L = h._L
    keep, probs = [], (orbx.Sim3OptProblem * cmax)()
    outs, res = [], (orbx.Sim3OptResult * cmax)()
    for c in range(cmax):
        probs[c], _ = h._problem(osr.make_scene(n, c, outliers=0.1), keep, TH2, False)
        o = dict(n_inliers=np.zeros(1, np.int32), quat=np.zeros(4), t=np.zeros(3), s=np.zeros(1), r12=np.zeros(9, np.float32), removed_first=np.zeros(n, np.uint8),
                 removed_final=np.zeros(n, np.uint8), n_bad=np.zeros(1, np.int32), stats=np.zeros(4))
        outs.append(o)
        res[c] = orbx.Sim3OptResult(*[o[k].ctypes.data if k in o else None for k in orbx._SIM3_OPT_RESULT_FIELDS])
    one_p, one_r = [(orbx.Sim3OptProblem * 1)(probs[c]) for c in range(cmax)], [(orbx.Sim3OptResult * 1)(res[c]) for c in range(cmax)]

    def call(p, C, r):
        t0 = time.perf_counter()
        rc = L.orbx_optimize_sim3(h._h, p, C, r)
        t1 = time.perf_counter()
        if rc != 0:
            orbx._check(rc)
        return (t1 - t0) * 1e6, h.last_timing()
    result = {}
    for C in PROBLEMS:
        wall, dev, wall1, dev1, launches = [], [], [], [], 0
        for it in range(a.warmup + a.calls):
            w, (ms, launches) = call(probs, C, res)
            each = [call(one_p[c], 1, one_r[c]) for c in range(C)]
            if it >= a.warmup:
                wall.append(w)
                dev.append(ms)
                wall1.append(sum(e[0] for e in each))
                dev1.append(sum(e[1][0] for e in each))
        result[str(C)] = dict(wall=[float(np.median(wall)), float(np.percentile(wall, 10)), float(np.percentile(wall, 90))], device=float(np.median(dev)), launches=launches,
                              wall_each=float(np.median(wall1)), device_each=float(np.median(dev1)),
                              iterations=[int(o["stats"][0] + o["stats"][2]) for o in outs[:C]], inliers=[int(o["n_inliers"][0]) for o in outs[:C]])
    h.close()
    print("RESULT " + json.dumps(result), flush=True)


def child(a, n):
    cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, str(Path(__file__).resolve()), "--calls", str(a.calls), "--warmup", str(a.warmup), "--shape", str(n)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not out:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1, None
    return 0, json.loads(out[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None, help=argparse.SUPPRESS)      # run as the child of one n
    a = ap.parse_args()
    if a.shape:
        return run_shape(a, a.shape)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_optimize_sim3, C problems of n pairs, th2 = 10, free scale; medians of %d calls after %d; wall clock of the C call in us, device time in ms." % (a.calls, a.warmup))
    say("`each` = the same C problems solved one call each, summed; ratio = wall each / wall.  Not measured: real keyframes, the shim; there is no reference timing.")
    say("%-5s %-3s | %8s %8s %8s | %8s | %8s | %10s %11s | %6s | %s" % ("n", "C", "wall", "p10", "p90", "device", "launches", "wall each", "device each", "ratio", "Levenberg iterations (both rounds); inliers"))
    for n in SHAPES:
        rc, d = child(a, n)
        if rc:
            say("%-5d     | failed with status %d: stopped, nothing more is started on the device" % (n, rc))
            _write(a, lines)
            return rc
        for C in PROBLEMS:
            r = d[str(C)]
            w = r["wall"]
            say("%-5d %-3d | %8.1f %8.1f %8.1f | %8.3f | %8d | %10.1f %11.3f | %6.2f | %s; %s" % (n, C, w[0], w[1], w[2], r["device"], r["launches"], r["wall_each"], r["device_each"],
                                                                                      r["wall_each"] / w[0], r["iterations"], r["inliers"]))
    _write(a, lines)
    return 0


def _write(a, lines):
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
