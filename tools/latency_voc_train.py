"""What training a vocabulary on the device costs (profiles/voc_train_latency.txt), beside a one-thread host baseline.

N = 10^5, 10^6 and 10^7 descriptors at k = 10, L = 6, drawn around the leaves of a voc_synth.make_vocabulary_fast tree (a heavy-tailed number of
samples per leaf, 0 .. 20 bit flips each), in images of 1,000 features.  Per size: one training for the wall clock of orbx_voc_train (total and per
level, orbx_voc_trainer_last_timing) and one with profiling for the device time of the stages (HIP events: seeding, assignment, mean, partition,
everything else).  Host column: tools/voc_train_host_baseline.cc (this project's plain C++ statement of the same algorithm with the same draws, one
thread) on the same descriptors on this machine's host, run under --host-seconds and left out when it does not end in time; its tree is compared with the
device's.  One GPU process at a time: every size runs in a child of its own under `timeout -k 10 --step-seconds`; the first child that fails ends the run.
No reference timing exists (the reference's create() draws from rand() and needs OpenCV).  NOT measured: real image descriptors, the shim.

    python tools/latency_voc_train.py [--sizes 100000,1000000,10000000] [--out profiles/voc_train_latency.txt]
"""
import argparse
import hashlib
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
K, LEVELS, SEED, PER_IMAGE = 10, 6, 1, 1000
BASELINE = ROOT / "tools" / "_build" / "voc_train_host_baseline"


def build_baseline():
    src = ROOT / "tools" / "voc_train_host_baseline.cc"
    if BASELINE.exists() and BASELINE.stat().st_mtime >= src.stat().st_mtime:
        return BASELINE
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    BASELINE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run([cxx, "-O2", "-std=c++11", "-mpopcnt", "-ffp-contract=off", "-o", str(BASELINE), str(src)], check=True)
    return BASELINE


def make_scene(orbx, n, seed=0):
    voc = orbx.voc_synth.make_vocabulary_fast(K, 4, seed + 1)
    leaves = voc["desc"][voc["is_leaf"] == 1]
    rng = np.random.default_rng(seed)
    w = rng.pareto(1.2, len(leaves)) + 0.01
    d = leaves[rng.choice(len(leaves), n, p=w / w.sum())].copy()
    flips = rng.integers(0, 21, n)
    for j in range(20):      # one flip per row and pass
        rows = np.nonzero(flips > j)[0]
        b = rng.integers(0, 256, len(rows))
        d[rows, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    counts = np.full((n + PER_IMAGE - 1) // PER_IMAGE, PER_IMAGE, np.int32)
    counts[-1] = n - PER_IMAGE * (len(counts) - 1)
    return d, counts


def digest(parent, leaf, desc, ni):
    h = hashlib.sha256()
    for a, t in ((parent, "<i4"), (leaf, "u1"), (desc, "u1"), (ni, "<i4")):
        h.update(np.ascontiguousarray(a).astype(t, copy=False).tobytes())
    return h.hexdigest()


def run_size(a, n):
    """child process: one size, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    d, counts = make_scene(orbx, n)
    result = dict(n=n, images=len(counts))
    tr = orbx.VocabularyTrainer(K, LEVELS, n, len(counts))
    t0 = time.perf_counter()
    tr.add(np.split(d, np.cumsum(counts)[:-1]))
    result["upload_s"] = time.perf_counter() - t0
    tr.train(seed=SEED)      # warm-up: allocations
    t0 = time.perf_counter()
    v = tr.train(seed=SEED)
    result["wall_ms"] = (time.perf_counter() - t0) * 1e3
    t = tr.last_timing()
    result.update(total_ms=t["total_ms"], level_ms=t["level_ms"], launches=t["launches"], nodes=int(v["num_nodes"]), words=int(v["num_words"]),
                  passes=[int(p) for p in v["passes_per_level"]], unconverged=int(v["unconverged_nodes"]))
    tr.set_profiling(True)
    tr.train(seed=SEED)
    result["stage_ms"] = tr.last_timing()["stage_ms"]
    tr.close()
    result["digest"] = digest(v["parent"], v["is_leaf"], v["desc"], v["ni"])
    exe = build_baseline()
    if exe is not None and a.host_seconds > 0:
        with tempfile.TemporaryDirectory() as tmp:
            scene, out = Path(tmp) / "scene.bin", Path(tmp) / "out.bin"
            with open(scene, "wb") as f:
                f.write(struct.pack("<8iQ", 0x564f4354, n, len(counts), K, LEVELS, 0, 100, 0, SEED))
                f.write(counts.astype(np.int32).tobytes())
                f.write(d.tobytes())
            try:
                r = subprocess.run([str(exe), str(scene), str(out)], capture_output=True, text=True, timeout=a.host_seconds)
                if r.returncode == 0:
                    result["host_ms"] = [float(x) for x in r.stdout.split()[1:4]]
                    raw = out.read_bytes()
                    m = struct.unpack_from("<i", raw, 0)[0]
                    at = 52
                    parent = np.frombuffer(raw, np.int32, m, at); at += 4 * m
                    leaf = np.frombuffer(raw, np.uint8, m, at); at += m
                    desc = np.frombuffer(raw, np.uint8, 32 * m, at); at += 32 * m
                    ni = np.frombuffer(raw, np.int32, m, at)
                    result["same_tree"] = digest(parent, leaf, desc, ni) == result["digest"]
            except subprocess.TimeoutExpired:
                result["host_timeout"] = a.host_seconds
    print("RESULT " + json.dumps(result), flush=True)


def child(a, n):
    cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, str(Path(__file__).resolve()), "--host-seconds", str(a.host_seconds), "--size", str(n)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not out:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1, None
    return 0, json.loads(out[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-seconds", type=int, default=540)
    ap.add_argument("--host-seconds", type=int, default=300)
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=None, help=argparse.SUPPRESS)      # run as the child of one size
    a = ap.parse_args()
    if a.size:
        return run_size(a, a.size)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_voc_train: N descriptors around a synthetic tree, k = %d, L = %d, images of %d features, seed %d, cap 100; ms." % (K, LEVELS, PER_IMAGE, SEED))
    say("device = orbx_voc_train (host clock around the call, second training of the handle); levels = its share per level; stages = device time of a")
    say("third, profiled training (HIP events): seeding / assignment / mean / partition / everything else (uploads, descent, Ni, downloads).")
    say("host = tools/voc_train_host_baseline.cc (same algorithm and draws, plain arrays, one thread) on the same descriptors, this machine's host: total (tree + weights).")
    say("No reference timing exists.  Real image descriptors are not measured.")
    for n in [int(x) for x in a.sizes.split(",")]:
        rc, d = child(a, n)
        if rc:
            say("%-9d | failed with status %d: stopped, nothing more is started on the device" % (n, rc))
            _write(a, lines)
            return rc
        st = d["stage_ms"]
        host = "%.0f (%.0f + %.0f)" % tuple(d["host_ms"]) if "host_ms" in d else ("not finished in %d s" % d["host_timeout"] if "host_timeout" in d else "-")
        say("N = %-9d %d images | device %.1f | levels %s | passes %s | %d launches | %d nodes, %d words, %d unconverged" % (
            n, d["images"], d["total_ms"], " ".join("%.1f" % x for x in d["level_ms"]), " ".join(str(p) for p in d["passes"]), d["launches"], d["nodes"], d["words"], d["unconverged"]))
        tot = max(sum(st.values()), 1e-9)
        say("              stages %s | host %s%s%s" % (
            " / ".join("%s %.1f (%.0f %%)" % (k, st[k], 100 * st[k] / tot) for k in ("seeding", "assignment", "mean", "partition", "other")), host,
            " | %.1f x" % (d["host_ms"][0] / d["total_ms"]) if "host_ms" in d else "",
            "; same tree" if d.get("same_tree") else ("; DIFFERENT TREE" if "same_tree" in d else "")))
    _write(a, lines)
    return 0


def _write(a, lines):
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
