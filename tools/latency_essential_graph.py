"""What the device form of Optimizer::OptimizeEssentialGraph costs (profiles/essential_graph_latency.txt).

One orbx_optimize_essential_graph per call: the host's symbolic phase, the staged inputs through mapped pinned memory, then per Levenberg iteration
one linearisation (2 launches) and per trial the solve, the errors and the chi2 record (3 launches) with one wait on the record.  Wall clock of the C
call alone (ctypes call on marshalled arrays), device time, launches and the time inside k_eg_solve (its own clock) from
orbx_essential_graph_last_timing; medians of --calls calls after --warmup.  Graphs of tests/essential_graph_ref.py: N = 100 / 500 / 1500 keyframes
(TUM, EuRoC and KITTI-00 sized), covisibility band 8, K = 10 corrected keyframes, 1 / 2 / 4 loop closures (the current one plus 0 / 1 / 3 older
kind-1 loop edges), free and fixed scale; the log-scale drift per step is scaled so that the whole trajectory drifts like the 100-keyframe one.
Then the map-point correction alone: 100 keyframes without an edge and M = 100k points.
One GPU process at a time: this process never opens the device; every graph runs in a child of its own under `timeout -k 10 --step-seconds`, and
the first child that fails or is killed ends the run - nothing more is started on the device.  Nothing on the parent commit does this work and no C
entry point of the compiled reference reaches OptimizeEssentialGraph: the numbers are a record, not a comparison.  NOT measured: real keyframes,
the shim's pointer walk.

    python tools/latency_essential_graph.py [--calls 5] [--out profiles/essential_graph_latency.txt]
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

import essential_graph_ref as eg      # noqa: E402

GRAPHS = ((100, 0), (500, 1), (1500, 3))      # keyframes, older loop edges
BAND, CORRECTED, POINTS = 8, 10, 100000


def run_graph(a, n, older):
    """child process: one graph, free and fixed scale, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    result = {}
    for fs in (False, True):
        if n:
            G = eg.make_scene(n, 0, fix_scale=fs, K=CORRECTED, band=BAND, old_loop=older, scale_drift=(3.0 / n, 0.2 / n ** 0.5))[0]
            g = dict(est=G.est, meas=G.meas, fixed=G.fixed, edges=G.edges)
        else:      # the map-point correction alone
            G = eg.make_scene(100, 0, fix_scale=fs, K=CORRECTED, band=BAND)[0]
            rng = np.random.default_rng(1)
            g = dict(est=G.est, meas=G.meas, fixed=G.fixed, edges=np.zeros((0, 3), np.int32), points=rng.normal(size=(POINTS, 3)).astype(np.float32) * 5,
                     ref=rng.integers(0, 100, POINTS).astype(np.int32))
        h = orbx.EssentialGraphOptimizer(max_keyframes=len(g["est"]), max_edges=max(len(g["edges"]), 1), max_points=POINTS if not n else 0)
        keep = []
        P = h._problem(g, keep, fs, 20, 1e-16)
        o = dict(est=np.zeros((P.n, 8)), tiw=np.zeros((P.n, 12), np.float32), inv=np.zeros((P.n, 8)), points=np.zeros((max(P.n_points, 1), 3), np.float32), chi2=np.zeros(2),
                 iterations=np.zeros(1, np.int32), ended=np.zeros(1, np.int32), iter_trials=np.zeros(20, np.int32), fill_blocks=np.zeros(1, np.int32))
        R = orbx.EssentialGraphCResult(*[o[k].ctypes.data if k in o else None for k in orbx._EG_RESULT_FIELDS])
        wall, dev, solve, launches = [], [], [], 0
        for it in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            rc = h._L.orbx_optimize_essential_graph(h._h, ctypes.byref(P), ctypes.byref(R))
            t1 = time.perf_counter()
            if rc != 0:
                orbx._check(rc)
            ms, launches, sv = h.last_timing()
            if it >= a.warmup:
                wall.append((t1 - t0) * 1e3)
                dev.append(ms)
                solve.append(sv)
        done = int(o["iterations"][0])
        result["fix" if fs else "free"] = dict(edges=int(P.n_edges), wall=[float(np.median(wall)), float(np.percentile(wall, 10)), float(np.percentile(wall, 90))],
                                              device=float(np.median(dev)), solve=float(np.median(solve)), launches=launches, fill=int(o["fill_blocks"][0]), iterations=done,
                                              trials=[int(v) for v in o["iter_trials"][:done]], ended=orbx.EG_ENDED[int(o["ended"][0])], chi2=[float(v) for v in o["chi2"]])
        h.close()
    print("RESULT " + json.dumps(result), flush=True)


def child(a, n, older):
    cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, str(Path(__file__).resolve()), "--calls", str(a.calls), "--warmup", str(a.warmup), "--graph", "%d,%d" % (n, older)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not out:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1, None
    return 0, json.loads(out[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--graph", default=None, help=argparse.SUPPRESS)      # run as the child of one graph
    a = ap.parse_args()
    if a.graph:
        n, older = [int(v) for v in a.graph.split(",")]
        return run_graph(a, n, older)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_optimize_essential_graph, N keyframes, band %d, %d corrected keyframes; medians of %d calls after %d; wall clock of the C call and device time in ms." % (
        BAND, CORRECTED, a.calls, a.warmup))
    say("`solve` = time inside k_eg_solve (factorisation + substitutions), share = solve / device.  fill = blocks of L with the diagonal, of the dense lower triangle in %.")
    say("Not measured: real keyframes, the shim.  No reference timing and no parent-commit timing exist: a baseline, not a comparison.")
    say("%-6s %-5s %-7s %-6s | %8s %8s %8s | %8s %8s %6s | %8s | %8s %6s | %s" % ("N", "scale", "closures", "edges", "wall", "p10", "p90", "device", "solve", "share", "launches", "fill", "%",
                                                                                 "iterations: trials; ending; chi2"))
    for n, older in GRAPHS + ((0, 0),):
        rc, d = child(a, n, older)
        if rc:
            say("%-6d | failed with status %d: stopped, nothing more is started on the device" % (n, rc))
            _write(a, lines)
            return rc
        for key in ("free", "fix"):
            r = d[key]
            w = r["wall"]
            nf = (n or 100) - 1
            name = str(n) if n else "points"
            say("%-6s %-5s %-7d %-6d | %8.2f %8.2f %8.2f | %8.2f %8.2f %5.0f%% | %8d | %8d %5.1f%% | %d: %s; %s; %.4g -> %.4g" % (
                name, key, older + 1 if n else 0, r["edges"], w[0], w[1], w[2], r["device"], r["solve"], 100.0 * r["solve"] / max(r["device"], 1e-9), r["launches"], r["fill"],
                100.0 * r["fill"] / (nf * (nf + 1) / 2), r["iterations"], r["trials"], r["ended"], r["chi2"][0], r["chi2"][1]))
    say("points = the map-point correction alone: 100 keyframes, no edge, M = %d points (staging, one write-back launch, one wait)." % POINTS)
    _write(a, lines)
    return 0


def _write(a, lines):
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
