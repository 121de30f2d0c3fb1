"""What the device chain of PnPsolver costs (profiles/pnp_latency.txt).

One orbx_pnp_solve per call: the candidates' matches and sets through mapped pinned memory, seven launches on the handle's stream
(k_pnp_prepare, k_pnp_models, k_pnp_check, k_pnp_records, k_pnp_refine, k_pnp_check on the refined models, k_pnp_decide), one wait.  Wall clock
of the C call alone (ctypes call on marshalled arrays, no result objects), device time and launches from orbx_pnp_last_timing; medians of
--calls calls after --warmup.  C = 1 / 8 candidates of n = 50 / 200 / 1000 matches of the scene of tests/pnp_ref.py (30 % gross outliers) at
35 iterations (the reference's defaults on 20 matches and more) and at 300, solved in ONE call, and the same candidates solved one call each
(the sum of the C calls).  The per-kernel share comes from ONE `rocprofv3 --kernel-trace --stats` run of the largest shape (its own child
process, fewer calls), read from the result database.
One GPU process at a time: this process never opens the device; every (n, iterations) runs in a child of its own under
`timeout -k 10 --step-seconds`, and the first child that fails or is killed ends the run - nothing more is started on the device.  Nothing on
the parent commit does this work and the reference's PnPsolver cannot be built on the project's OpenCV stand-in (it uses the C API: cvSVD,
cvSolve, cvInvert, cvMulTransposed, which the stand-in only forward-declares): the numbers are a record, not a comparison.  NOT measured: real
frames, the shim.

    python tools/latency_pnp.py [--calls 200] [--out profiles/pnp_latency.txt]
"""
import argparse
import glob
import importlib
import json
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import pnp_ref as pr      # noqa: E402

SHAPES = (50, 200, 1000)
CANDIDATES = (1, 8)
ITERATIONS = (35, 300)
PARAMS = dict(prob=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.1, th2=5.991)


def run_shape(a, n, iters):
    """child process: one (n, iterations), every C, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    h = orbx.PnPsolver(max_candidates=max(CANDIDATES), max_matches=max(n, 4), max_iterations=iters)
    L = h._L
    cmax = max(a.only_candidates or CANDIDATES)
    keep, probs = [], (orbx.PnPProblem * cmax)()
    outs, res = [], (orbx.PnPResult * cmax)()
    for c in range(cmax):
        sc = pr.scene(n, c + 1, outliers=0.3)
        P, _ = h._problem(sc, keep, PARAMS)
        sets = np.ascontiguousarray(pr.rng_sets(n, iters, 1001 + c), np.int32)
        keep.append(sets)
        P.sets, P.iterations = sets.ctypes.data, iters
        probs[c] = P
        o = dict(count=np.zeros(iters, np.int32), record_of=np.zeros(iters, np.int32), refined_count=np.zeros(iters, np.int32), refined_tcw=np.zeros((iters, 12), np.float32),
                 best_tcw=np.zeros(12, np.float32), first_event=np.zeros(1, np.int32), best_iteration=np.zeros(1, np.int32), nrecords=np.zeros(1, np.int32),
                 no_more=np.zeros(1, np.int32), inliers_first=np.zeros(n, np.uint8), inliers_best=np.zeros(n, np.uint8))
        outs.append(o)
        res[c] = orbx.PnPResult(*[o[k].ctypes.data if k in o else None for k in orbx._PNP_RESULT_FIELDS])
    one_p, one_r = [(orbx.PnPProblem * 1)(probs[c]) for c in range(cmax)], [(orbx.PnPResult * 1)(res[c]) for c in range(cmax)]

    def call(p, C, r):
        t0 = time.perf_counter()
        rc = L.orbx_pnp_solve(h._h, p, C, r)
        t1 = time.perf_counter()
        if rc != 0:
            orbx._check(rc)
        return (t1 - t0) * 1e6, h.last_timing()
    result = {}
    for C in a.only_candidates or CANDIDATES:
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
                              wall_each=float(np.median(wall1)), device_each=float(np.median(dev1)), events=[int(o["first_event"][0]) for o in outs[:C]],
                              records=[int(o["nrecords"][0]) for o in outs[:C]])
    h.close()
    print("RESULT " + json.dumps(result), flush=True)


def kernel_shares(db_dir):
    dbs = sorted(glob.glob(db_dir + "/**/*_results.db", recursive=True))
    if not dbs:
        return None
    agg = {}
    for name, s, e in sqlite3.connect(dbs[0]).execute("select name, start, end from kernels"):
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        v = agg.setdefault(short, [0, 0.0])
        v[0] += 1
        v[1] += (e - s) / 1e3
    return agg


def child(a, n, iters, calls, prefix=(), only=None):
    cmd = list(prefix) + [sys.executable, str(Path(__file__).resolve()), "--calls", str(calls), "--warmup", str(a.warmup), "--shape", str(n), "--iterations", str(iters)]
    if only:
        cmd += ["--only-candidates"] + [str(c) for c in only]
    cmd = ["timeout", "-k", "10", str(a.step_seconds)] + cmd
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
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--shape", type=int, default=None, help=argparse.SUPPRESS)      # run as the child of one (n, iterations)
    ap.add_argument("--iterations", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--only-candidates", type=int, nargs="*", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shape:
        return run_shape(a, a.shape, a.iterations)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_pnp_solve, C candidates of n matches (30 %% outliers), S iterations each; medians of %d calls after %d; wall clock of the C call in us, device time in ms." % (a.calls, a.warmup))
    say("`each` = the same C candidates solved one call each, summed.  Not measured: real frames, the shim; there is no reference timing.")
    say("%-5s %-4s %-3s | %8s %8s %8s | %8s | %8s | %10s %11s | %s | %s" % ("n", "S", "C", "wall", "p10", "p90", "device", "launches", "wall each", "device each", "first events", "records"))
    for n in SHAPES:
        for iters in ITERATIONS:
            rc, d = child(a, n, iters, a.calls)
            if rc:
                say("%-5d %-4d    | failed with status %d: stopped, nothing more is started on the device" % (n, iters, rc))
                _write(a, lines)
                return rc
            for C in CANDIDATES:
                r = d[str(C)]
                w = r["wall"]
                say("%-5d %-4d %-3d | %8.1f %8.1f %8.1f | %8.3f | %8d | %10.1f %11.3f | %s | %s" % (n, iters, C, w[0], w[1], w[2], r["device"], r["launches"], r["wall_each"], r["device_each"],
                                                                                                 r["events"], r["records"]))
    if not a.no_trace and shutil.which("rocprofv3"):
        tmp = tempfile.mkdtemp(prefix="pnp_trace_")
        rc, d = child(a, SHAPES[-1], ITERATIONS[-1], 50, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "pnp", "--"), only=(CANDIDATES[-1],))
        agg = None if rc else kernel_shares(tmp)
        shutil.rmtree(tmp, ignore_errors=True)
        if rc or not agg:
            say("rocprofv3 --kernel-trace --stats: no result (status %d)" % rc)
            _write(a, lines)
            return rc or 1
        tot = sum(v[1] for v in agg.values())
        say("")
        say("Per kernel, one rocprofv3 --kernel-trace --stats run of n = %d, S = %d (%d calls of C = %d and %d x %d calls of C = 1):" % (
            SHAPES[-1], ITERATIONS[-1], 50 + a.warmup, CANDIDATES[-1], 50 + a.warmup, CANDIDATES[-1]))
        for k, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            say("%-20s calls %5d  avg %8.2f us  %5.1f %%" % (k, c, t / c, 100 * t / tot))
    _write(a, lines)
    return 0


def _write(a, lines):
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
