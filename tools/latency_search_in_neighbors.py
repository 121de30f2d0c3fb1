#!/usr/bin/env python3
"""Host-visible latency of steps 2 and 3 of LocalMapping::SearchInNeighbors on synthetic maps (tests/fuse_chain_scenes.py): T = 20 / 60 / 120 targets of about
1000 / 2000 features.

chain     one orbx_search_in_neighbors: the slice staged once, per Fuse call prepare + search + apply on the matcher's stream, the candidate gather on the
          device, ONE host wait (wall time of the C call on marshalled arrays; device ms, launches and the share of the apply kernels from
          orbx_search_in_neighbors_last_timing, the share from a second run with profile_kernels).
baseline  what the shim did before: per Fuse call the projection gates point by point on the host, one synchronous orbx_fuse_search, the surgery on the host
          (tools/sin_host_baseline.cc: plain arrays, one thread, no locks; linked against the same liborbx.so), on the same scene and the same machine.
Both produce the decision log; the tool checks that the two logs have the same checksum and the same nFused per call before it reports a time.

  python tools/latency_search_in_neighbors.py [--reps 7] [--out profiles/search_in_neighbors_latency.txt] [--shapes 20x1000,60x1000,...]
"""
import argparse
import importlib
import shutil
import statistics
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
BASELINE = ROOT / "tools" / "_build" / "sin_host_baseline"


def build_baseline(orbx):
    src = ROOT / "tools" / "sin_host_baseline.cc"
    lib = Path(orbx.lib_path())
    if BASELINE.exists() and BASELINE.stat().st_mtime >= max(src.stat().st_mtime, (ROOT / "include" / "orbx.h").stat().st_mtime):
        return BASELINE
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("no C++ compiler for tools/sin_host_baseline.cc")
    BASELINE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run([cxx, "-O2", "-std=c++11", "-ffp-contract=off", "-o", str(BASELINE), str(src), "-L" + str(lib.parent), "-lorbx", "-Wl,-rpath," + str(lib.parent)], check=True)
    return BASELINE


def write_scene(path, sl, targets):
    import fuse_chain_scenes as fs
    S = len(sl["searchable"])
    assert [int(k["slot"]) for k in sl["searchable"]] == list(range(S))
    P, T0 = len(sl["bad"]), len(sl["obs_kf"])
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", 0x53494e42, len(sl["kf_rank"]), S, P, T0, len(targets), len(fs.SF), 0))
        f.write(np.array(list(fs.CAM) + list(fs.BOUNDS) + [fs.LOG_SF], np.float32).tobytes())
        f.write(fs.SF.tobytes() + fs.INV_SIGMA2.tobytes())
        f.write(np.asarray(sl["kf_rank"], np.int32).tobytes() + np.asarray(sl["kf_bad"], np.uint8).tobytes() + np.asarray(targets, np.int32).tobytes())
        for k in sl["searchable"]:
            f.write(struct.pack("<i", len(k["kps"])))
            f.write(np.ascontiguousarray(k["kps"]).tobytes() + np.ascontiguousarray(k["desc"], np.uint8).tobytes() + np.asarray(k["u_right"], np.float32).tobytes() +
                    np.asarray(k["kf_point"], np.int32).tobytes())
            f.write(np.asarray(k["Tcw"], np.float32).reshape(-1, 4)[:3].tobytes() + np.asarray(k["ow"], np.float32).tobytes())
        for key, dt in (("pos", np.float32), ("normal", np.float32), ("min_dist", np.float32), ("max_dist", np.float32), ("raw_max_dist", np.float32), ("desc", np.uint8),
                        ("bad", np.uint8), ("visible", np.int32), ("found", np.int32), ("obs_offset", np.int32), ("obs_kf", np.int32), ("obs_idx", np.int32),
                        ("obs_stereo", np.uint8), ("obs_desc", np.uint8)):
            f.write(np.ascontiguousarray(sl[key], dt).tobytes())


def checksum(log):
    s = 0
    for d in log:
        s = (s * 1000003 + ((((int(d["call"]) * 31 + int(d["position"])) * 31 + int(d["point"])) * 31 + int(d["feature"])) & 0xffffffffffffffff) * 7 + int(d["kind"])) & 0xffffffffffffffff
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "search_in_neighbors_latency.txt"))
    ap.add_argument("--shapes", default="20x1000,60x1000,120x1000,20x2000,60x2000,120x2000")
    a = ap.parse_args()
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    import fuse_chain_scenes as fs
    exe = build_baseline(orbx)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("orbx_search_in_neighbors (chain: one call, one host wait) against the per-call round trips of the shim before it (baseline: host prepare, one synchronous")
    say("orbx_fuse_search, host surgery per Fuse call; tools/sin_host_baseline.cc).  Wall time of the C call in us, median of %d; same = equal log checksum and nFused." % a.reps)
    say("%-16s %7s %7s %9s | %10s %10s %8s %9s %8s | %10s | %s" % ("T x feat", "points", "obs", "decisions", "chain us", "device us", "launches", "apply us", "apply %", "baseline", "same"))
    for shape in [(kind, sh) for kind in ("few", "sparse", "dense") for sh in a.shapes.split(",")]:
        kind, (T, nf) = shape[0], (int(v) for v in shape[1].split("x"))
        if kind == "few":         # nearly every point is held by the current keyframe and by every target: a handful of decisions per Fuse call
            sl, cur, tg = fs.chain_scene(orbx, 100 + T + nf, T=T, M=nf - 15, mode="mixed", present=0.997, mix=(0.98, 0.005, 0.005, 0.005, 0.005))
        elif kind == "sparse":      # most points are held by the current keyframe and by nearly every target already: tens of decisions per Fuse call
            sl, cur, tg = fs.chain_scene(orbx, 100 + T + nf, T=T, M=nf - 15, mode="mixed", present=0.97, mix=(0.9, 0.03, 0.03, 0.02, 0.02))
        else:                     # the test scenes' mix: a fifth of the list entries of every call is a decision
            sl, cur, tg = fs.chain_scene(orbx, 100 + T + nf, T=T, M=int(nf / 0.8) - 15, mode="mixed")
        nmax = max(len(k["kps"]) for k in sl["searchable"])
        m = orbx.ORBmatcher(0.6, True, max_features=min(65535, max(nmax, len(sl["bad"]))))
        call = m.search_in_neighbors_prepare(sl, cur, tg)
        r = call()      # warm-up, and the result to compare
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rc = call.raw()
            wall.append((time.perf_counter() - t0) * 1e6)
            assert rc == 0
        dev_ms, launches, _ = m.search_in_neighbors_last_timing()
        prof = m.search_in_neighbors_prepare(sl, cur, tg, profile_kernels=True)
        prof()
        pdev, _, apply_ms = m.search_in_neighbors_last_timing()
        m.close()
        with tempfile.TemporaryDirectory() as d:
            write_scene(Path(d) / "scene.bin", sl, tg)
            out = subprocess.run([str(exe), str(Path(d) / "scene.bin"), str(a.reps)], capture_output=True, text=True, check=True).stdout.split()
        base_us, base_dec, base_sum, base_nf = float(out[1]), int(out[2]), int(out[3]), [int(v) for v in out[4:]]
        same = base_dec == len(r["log"]) and base_sum == checksum(r["log"]) and base_nf == r["nfused"].tolist()
        say("%-16s %7d %7d %9d | %10.0f %10.0f %8d %9.0f %7.0f%% | %10.0f | %s" % ("%s %dx%d" % (kind, T, nmax), len(sl["bad"]), len(sl["obs_kf"]), len(r["log"]), statistics.median(wall),
                                                                           dev_ms * 1e3, launches, apply_ms * 1e3, 100.0 * apply_ms / max(pdev, 1e-9), base_us, "yes" if same else "NO"))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
