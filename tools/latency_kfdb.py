"""What place recognition on the device costs (profiles/kfdb_latency.txt), beside a one-thread host baseline.

Databases of 1,000 / 10,000 / 50,000 keyframes of about 800 words over 1,000,000 words (places of 100 keyframes; a keyframe takes 60 % of its words from
its place; ten covisibles each: the nearest keyframes of the place).  Per database: loop queries (ten connected keyframes) and relocalisation queries,
nq = 1 and 8 per call.  Device columns: wall clock of the C call alone (ctypes on marshalled arrays) and orbx_kfdb_last_timing, medians of --calls calls
after --warmup; then one profiled call gives the stages (orbx_kfdb_stage_timing) and the rate at which k_kfdb_intersect reads the pool's words
(4 bytes per alive entry and query).  Host column: tools/kfdb_host_baseline.cc (this project's plain C++ inverted-file walk, std::list per word, one
thread) on the same scene and queries on this machine's host, median per query, times nq.  The loop candidates of both are compared.
One GPU process at a time: every database runs in a child of its own under `timeout -k 10 --step-seconds`; the first child that fails ends the run.
No reference timing exists (no C entry point of the compiled reference reaches the database).  NOT measured: real vocabularies' word statistics, the shim.

    python tools/latency_kfdb.py [--calls 5] [--sizes 1000,10000,50000] [--out profiles/kfdb_latency.txt]
"""
import argparse
import ctypes
import importlib
import json
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
N_WORDS, LENGTH, PLACE_KF, PLACE_WORDS = 1000000, 800, 100, 2000
BASELINE = ROOT / "tools" / "_build" / "kfdb_host_baseline"


def build_baseline():
    src = ROOT / "tools" / "kfdb_host_baseline.cc"
    if BASELINE.exists() and BASELINE.stat().st_mtime >= src.stat().st_mtime:
        return BASELINE
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    BASELINE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run([cxx, "-O2", "-std=c++11", "-o", str(BASELINE), str(src)], check=True)
    return BASELINE


def draw(rng, place_words):
    w = np.unique(np.concatenate([rng.choice(place_words, int(0.6 * LENGTH), replace=False), rng.integers(0, N_WORDS, LENGTH - int(0.6 * LENGTH))])).astype(np.int32)
    v = rng.random(len(w)) + 0.05
    return w, v / v.sum()


def make_scene(n, seed=0):
    rng = np.random.default_rng(seed)
    places = [np.sort(rng.choice(N_WORDS, PLACE_WORDS, replace=False)) for _ in range((n + PLACE_KF - 1) // PLACE_KF)]
    bows = [draw(rng, places[k // PLACE_KF]) for k in range(n)]
    cov = np.full((n, 10), -1, np.int32)
    for k in range(n):
        lo, hi = (k // PLACE_KF) * PLACE_KF, min(n, (k // PLACE_KF + 1) * PLACE_KF)
        near = sorted((u for u in range(max(lo, k - 6), min(hi, k + 7)) if u != k), key=lambda u: (abs(u - k), u))[:10]
        cov[k, :len(near)] = near
    queries = []
    for i in range(8):      # the query keyframe revisits the place of keyframe t; its connected keyframes are the ten before t
        t = n - 1 - i * 3
        w, v = draw(rng, places[t // PLACE_KF])
        con = np.arange(max(0, t - 9), t + 1, dtype=np.int64)
        queries.append(dict(words=w, values=v, connected=con, counts=np.full(len(con), 30, np.int32)))
    return bows, cov, queries


def write_scene(path, bows, cov, queries):
    off = np.zeros(len(bows) + 1, np.int64)
    off[1:] = np.cumsum([len(b[0]) for b in bows])
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", 0x4b464442, N_WORDS, len(bows), 2 * len(queries)))
        f.write(off.tobytes())
        f.write(np.concatenate([b[0] for b in bows]).astype(np.int32).tobytes())
        f.write(np.concatenate([b[1] for b in bows]).astype(np.float64).tobytes())
        f.write(cov.tobytes())
        for mode in (0, 1):
            for q in queries:
                con = q["connected"] if mode == 0 else np.zeros(0, np.int64)
                cnt = q["counts"] if mode == 0 else np.zeros(0, np.int32)
                f.write(struct.pack("<3i", mode, len(q["words"]), len(con)))
                f.write(q["words"].tobytes() + q["values"].astype(np.float64).tobytes() + con.tobytes() + cnt.tobytes())


def run_size(a, n):
    """child process: one database, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    bows, cov, queries = make_scene(n)
    entries = int(sum(len(b[0]) for b in bows))
    result = dict(n=n, entries=entries)
    host = {}
    exe = build_baseline()
    if exe is not None:
        with tempfile.TemporaryDirectory() as d:
            write_scene(Path(d) / "scene.bin", bows, cov, queries)
            r = subprocess.run([str(exe), str(Path(d) / "scene.bin"), str(a.calls)], capture_output=True, text=True, check=True)
        rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("Q ")]
        for mode in (0, 1):
            mine = [row for row in rows if int(row[2]) == mode]
            host[mode] = dict(us=[float(row[3]) for row in mine], cand=[[int(x) for x in row[4:]] for row in mine])
    t0 = time.perf_counter()
    db = orbx.KeyFrameDatabase(N_WORDS, n, entries, max_queries=8, max_query_words=1024)
    for k, (w, v) in enumerate(bows):
        db.add(k, (w, v))
    for k in range(n):
        db.set_covisibles(k, cov[k][cov[k] >= 0])
    result["fill_s"] = time.perf_counter() - t0
    for mode in (0, 1):
        for nq in (1, 8):
            qs = [dict(q, mode=mode) for q in queries[:nq]]
            Q, R, _, keep, outs = db.query(qs, marshal_only=True)
            wall, dev = [], []
            for it in range(a.warmup + a.calls):
                t0 = time.perf_counter()
                rc = db._L.orbx_kfdb_query(db._h, Q, nq, R)
                t1 = time.perf_counter()
                orbx._check(rc)
                if it >= a.warmup:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(db.last_timing()[0])
            db.stage_timing(True)
            orbx._check(db._L.orbx_kfdb_query(db._h, Q, nq, R))
            stages = db.stage_timing(False, read=True)
            cand = [[int(x) for x in o["candidates"][:int(o["n_candidates"][0])]] for o, _ in outs]
            row = dict(wall=[float(np.median(wall)), float(np.percentile(wall, 10)), float(np.percentile(wall, 90))], device=float(np.median(dev)), stages=[float(x) for x in stages],
                       scored=[int(o["n_scored"][0]) for o, _ in outs], sharing=[int(o["n_sharing"][0]) for o, _ in outs], candidates=[len(c) for c in cand])
            if host:
                row["host_ms"] = float(sum(host[mode]["us"][:nq]) / 1e3)
                if mode == 0:
                    row["same_candidates"] = cand == host[mode]["cand"][:nq]
            result["%d_%d" % (mode, nq)] = row
    db.close()
    print("RESULT " + json.dumps(result), flush=True)


def child(a, n):
    cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, str(Path(__file__).resolve()), "--calls", str(a.calls), "--warmup", str(a.warmup), "--size", str(n)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not out:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1, None
    return 0, json.loads(out[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-seconds", type=int, default=300)
    ap.add_argument("--sizes", default="1000,10000,50000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=None, help=argparse.SUPPRESS)      # run as the child of one database
    a = ap.parse_args()
    if a.size:
        return run_size(a, a.size)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_kfdb_query: N keyframes of ~%d words over %d words, ten covisibles each; medians of %d calls after %d; ms." % (LENGTH, N_WORDS, a.calls, a.warmup))
    say("wall = the C call alone; device = orbx_kfdb_last_timing; stages = staging / intersect / score / commit / select of one profiled call;")
    say("GB/s = 4 bytes x alive entries x nq / intersect (the pool's words are read once per query; HBM3E peak 8000 GB/s).")
    say("host = tools/kfdb_host_baseline.cc (inverted file, std::list per word, one thread) on the same scene and queries, this machine's host, sum over the nq queries.")
    say("No reference timing exists.  Not measured: real vocabularies' word statistics, the shim.")
    say("%-6s %-5s %-2s | %8s %8s %8s | %8s | %-38s | %7s | %8s | %s" % ("N", "mode", "nq", "wall", "p10", "p90", "device", "stages", "GB/s", "host", "sharing / scored / candidates of query 0; loop candidates equal the host's"))
    for n in [int(x) for x in a.sizes.split(",")]:
        rc, d = child(a, n)
        if rc:
            say("%-6d | failed with status %d: stopped, nothing more is started on the device" % (n, rc))
            _write(a, lines)
            return rc
        for mode in (0, 1):
            for nq in (1, 8):
                r = d["%d_%d" % (mode, nq)]
                w, st = r["wall"], r["stages"]
                gbs = 4.0 * d["entries"] * nq / max(st[1], 1e-9) / 1e6
                say("%-6d %-5s %-2d | %8.3f %8.3f %8.3f | %8.3f | %-38s | %7.0f | %8s | %d / %d / %d%s" % (
                    n, "loop" if mode == 0 else "reloc", nq, w[0], w[1], w[2], r["device"], " ".join("%.3f" % x for x in st), gbs,
                    "%.3f" % r["host_ms"] if "host_ms" in r else "-", r["sharing"][0], r["scored"][0], r["candidates"][0],
                    "; equal" if r.get("same_candidates") else ("; DIFFERENT" if "same_candidates" in r else "")))
        say("%-6d filled in %.1f s (%d entries: add + set_covisibles per keyframe)" % (n, d["fill_s"], d["entries"]))
    _write(a, lines)
    return 0


def _write(a, lines):
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
