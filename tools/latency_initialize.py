"""What the device chain of Initializer::Initialize costs (profiles/initialize_latency.txt).

One orbx_initialize per call: the matches compacted and both frames normalised on the host, the inputs through mapped pinned memory, six
launches on the handle's stream (k_stage_copy, k_init_models, k_init_decompose, k_init_check_rt, k_init_rank, k_init_decide), one wait.
Wall clock of the C call alone (ctypes call on marshalled arrays, no result dict), device time and launches from
orbx_initializer_last_timing; medians of --calls calls after --warmup.  N = 100 / 300 / 1000 matches of the `general` scene of
tests/initializer_ref.py at 200 iterations.  The per-kernel share comes from ONE `rocprofv3 --kernel-trace --stats` run of the largest shape
(its own child process, fewer calls), read from the result database.
One GPU process at a time: this process never opens the device; every shape runs in a child of its own under `timeout -k 10 --step-seconds`,
and the first child that fails or is killed ends the run - nothing more is started on the device.  Nothing on the parent commit does this
work and the reference's Initializer is not part of the compiled oracle: the numbers are a record, not a comparison.  NOT measured: real frames.

    python tools/latency_initialize.py [--calls 200] [--out profiles/initialize_latency.txt]
"""
import argparse
import ctypes
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

import initializer_ref as ir      # noqa: E402

SHAPES = (100, 300, 1000)
ITERATIONS = 200


def run_shape(a, n):
    """child process: one shape, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    sc = ir.scene("general", n, 2)
    k1, k2, m = np.ascontiguousarray(sc["keys1"], np.float32), np.ascontiguousarray(sc["keys2"], np.float32), np.ascontiguousarray(sc["matches12"], np.int32)
    sets = np.ascontiguousarray(ir.draw_sets(n, ITERATIONS, 1002), np.int32)
    h = orbx.Initializer(sigma=1.0, iterations=ITERATIONS, max_matches=max(n, 8))
    fx, fy, cx, cy = sc["K"]
    P = orbx.InitProblem(k1.ctypes.data, k2.ctypes.data, len(k1), len(k2), m.ctypes.data, sets.ctypes.data, ITERATIONS, 1.0, fx, fy, cx, cy, 1.0, 50)
    success, r21, t21 = np.zeros(1, np.int32), np.zeros(9, np.float32), np.zeros(3, np.float32)
    p3d, tri = np.zeros((len(k1), 3), np.float32), np.zeros(len(k1), np.uint8)
    fields = dict(success=success, r21=r21, t21=t21, p3d=p3d, triangulated=tri)
    R = orbx.InitResult(*[fields[k].ctypes.data if k in fields else None for k in orbx._INIT_RESULT_FIELDS])
    L = h._L
    wall, dev, launches = [], [], 0
    for it in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        rc = L.orbx_initialize(h._h, ctypes.byref(P), ctypes.byref(R))
        t1 = time.perf_counter()
        if rc != 0:
            orbx._check(rc)
        if it >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            ms, launches = h.last_timing()
            dev.append(ms)
    h.close()
    print("RESULT " + json.dumps(dict(wall=[float(np.median(wall)), float(np.percentile(wall, 10)), float(np.percentile(wall, 90))], device=float(np.median(dev)),
                                      launches=launches, success=int(success[0]), triangulated=int(tri.sum()))), flush=True)


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


def child(a, n, calls, env=None, prefix=()):
    cmd = list(prefix) + [sys.executable, str(Path(__file__).resolve()), "--calls", str(calls), "--warmup", str(a.warmup), "--shape", str(n)]
    cmd = ["timeout", "-k", "10", str(a.step_seconds)] + cmd
    full = None
    if env:
        import os
        full = dict(os.environ, **env)
    r = subprocess.run(cmd, capture_output=True, text=True, env=full)
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
    ap.add_argument("--env", nargs="*", default=[], help="NAME=VALUE for the children (measurement switches)")
    ap.add_argument("--shape", type=int, default=None, help=argparse.SUPPRESS)      # run as the child of one shape
    a = ap.parse_args()
    if a.shape:
        return run_shape(a, a.shape)
    env = dict(e.split("=", 1) for e in a.env)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_initialize, %d iterations, `general` scene; medians of %d calls after %d, ms; wall clock of the C call.%s" % (ITERATIONS, a.calls, a.warmup,
                                                                                                                         "  Children run with %s." % env if env else ""))
    say("Not measured: real frames; nothing on the parent commit does this work.")
    say("%-10s | %8s %8s %8s | %8s | %8s | %s" % ("matches", "wall", "p10", "p90", "device", "launches", "success / triangulated"))
    for n in SHAPES:
        rc, d = child(a, n, a.calls, env)
        if rc:
            say("%-10d | failed with status %d: stopped, nothing more is started on the device" % (n, rc))
            _write(a, lines)
            return rc
        w = d["wall"]
        say("%-10d | %8.3f %8.3f %8.3f | %8.3f | %8d | %d / %d" % (n, w[0], w[1], w[2], d["device"], d["launches"], d["success"], d["triangulated"]))
    if not a.no_trace and shutil.which("rocprofv3"):
        tmp = tempfile.mkdtemp(prefix="init_trace_")
        rc, d = child(a, SHAPES[-1], 50, env, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "init", "--"))
        agg = None if rc else kernel_shares(tmp)
        shutil.rmtree(tmp, ignore_errors=True)
        if rc or not agg:
            say("rocprofv3 --kernel-trace --stats: no result (status %d)" % rc)
            _write(a, lines)
            return rc or 1
        tot = sum(v[1] for v in agg.values())
        say("")
        say("Per kernel, one rocprofv3 --kernel-trace --stats run of %d matches (%d calls):" % (SHAPES[-1], 50 + a.warmup))
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
