"""What the batched MapPoint refresh costs (profiles/mappoint_refresh.txt).

Times orbx_mappoint_refresh (MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth for M points in one call) at two shapes:
    new-keyframe   M = 1000 points, n uniform in 2..40 observers          (LocalMapping::ProcessNewKeyFrame-like)
    whole-map      M = 50 000 points, n = 2 + a long tail up to 300       (after a global bundle adjustment)
wall clock per call (median / p10 / p90 of --calls calls after --warmup) and the device time of the call's kernels (orbx_mappoint_last_timing),
next to tests/mappoint_ref.py's numpy RESTATEMENT of the two functions on one host thread (a restatement of their semantics in Python, NOT the
reference's C++: it says what the test oracle costs, not what the reference costs; whole-map: timed on the first --host-points points).
Also: the (row, column) descriptor pairs per second, and the VALU issue rate they amount to - VALU_PER_PAIR wave instructions per pair and
row-wave (counted in the ISA of k_mp_block<64>: 21 for the distance, 9 x 3 for the bisection) - against the measured byte-arithmetic issue rate
of tools/ubench_valu.hip (4.1 cycles per wave64 instruction per SIMD).

    python tools/latency_mappoint.py [--calls 30] [--out profiles/mappoint_refresh.txt]
"""
import argparse
import importlib
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import mappoint_ref as ref      # noqa: E402

VALU_PER_PAIR = 48
PEAK_WAVE_INSTR = 256 * 4 * 2.4e9 / 4.1      # CUs x SIMDs x clock / cycles per wave64 instruction (profiles/r05_valu_issue.txt)


def make_batch(ns, seed, flips=6):
    """vectorised twin of mappoint_ref.synth_batch (the same kind of data, built without a Python loop per point)"""
    rng = np.random.default_rng(seed)
    ns = np.asarray(ns, np.int64)
    M, T = len(ns), int(ns.sum())
    off = np.zeros(M + 1, np.int32)
    off[1:] = np.cumsum(ns)
    owner = np.repeat(np.arange(M), ns)
    base = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    flip = np.zeros((T, 32), np.uint8)
    pos = rng.integers(0, 256, (T, flips))
    np.bitwise_xor.at(flip, (np.arange(T)[:, None], pos >> 3), (1 << (pos & 7)).astype(np.uint8))
    d = rng.normal(size=(T, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cams = (d * rng.uniform(3.0, 7.0, (T, 1))).astype(np.float32)
    sf = ref.scale_factors()
    return dict(obs_offset=off, desc=base[owner] ^ flip, desc_valid=None, cam_center=cams, pos=rng.uniform(-1, 1, (M, 3)).astype(np.float32),
                ref_center=cams[off[:-1]].copy(), ref_scale=sf[rng.integers(0, 8, M)], top_scale=np.full(M, sf[7], np.float32))


def head(b, m):
    """the first m points of a batch"""
    t = int(b["obs_offset"][m])
    return dict(obs_offset=b["obs_offset"][:m + 1], desc=b["desc"][:t], desc_valid=None, cam_center=b["cam_center"][:t], pos=b["pos"][:m], ref_center=b["ref_center"][:m],
                ref_scale=b["ref_scale"][:m], top_scale=b["top_scale"][:m])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    tail = np.minimum(2 + np.floor(rng.pareto(1.6, 50000) * 4.0).astype(np.int64), 300)
    tail[:8] = 300
    shapes = [("new-keyframe", rng.integers(2, 41, 1000)), ("whole-map", tail)]
    say("orbx_mappoint_refresh: wall clock per call and device time of its kernels; restatement = tests/mappoint_ref.py in numpy on one host thread")
    say("(a restatement of the two functions' semantics, not the reference); VALU: %d wave instructions per (row, column) pair and row-wave," % VALU_PER_PAIR)
    say("peak %.0f G wave-instr/s = 256 CUs x 4 SIMDs x 2.4 GHz / 4.1 cycles (tools/ubench_valu.hip)" % (PEAK_WAVE_INSTR / 1e9))
    for name, ns in shapes:
        b = make_batch(ns, seed=2)
        M, T = len(ns), int(ns.sum())
        ops = orbx.MapPointOps(M, T)
        args = [b[k] for k in ("obs_offset", "desc", "cam_center", "pos", "ref_center", "ref_scale", "top_scale")]
        wall, dev = [], []
        for it in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            got = ops.refresh(*args)
            t1 = time.perf_counter()
            if it >= a.warmup:
                wall.append((t1 - t0) * 1e3)
                dev.append(ops.last_timing()[0])
        launches = ops.last_timing()[1]
        ops.close()
        hm = min(M, a.host_points)
        hb = head(b, hm)
        t0 = time.perf_counter()
        want = ref.restate(hb)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = ref.same_bits({k: v[:hm] for k, v in got.items()}, want)
        pairs = float((ns.astype(np.float64) ** 2).sum())
        issued = float((VALU_PER_PAIR * ns * np.ceil(ns / 64.0)).sum())      # a wave instruction serves up to 64 rows of one point
        kd = float(np.median(dev))
        say("%-12s M = %d, T = %d observations, n = %d..%d (mean %.1f), %d launches, %d calls" % (name, M, T, ns.min(), ns.max(), ns.mean(), launches, a.calls))
        say("  wall ms      median %9.3f   p10 %9.3f   p90 %9.3f" % (np.median(wall), np.percentile(wall, 10), np.percentile(wall, 90)))
        say("  kernels ms   median %9.3f   p10 %9.3f   p90 %9.3f" % (kd, np.percentile(dev, 10), np.percentile(dev, 90)))
        say("  restatement  %9.1f ms for the first %d points (%.1f us per point; the device call: %.2f us per point wall); results equal: %s"
            % (host_ms, hm, host_ms * 1e3 / hm, float(np.median(wall)) * 1e3 / M, same))
        say("  pairs        %.3g per call, %.3g pairs/s of kernel time; VALU issued %.3g wave-instr = %.1f G/s = %.1f %% of the byte-arithmetic issue rate"
            % (pairs, pairs / (kd * 1e-3), issued, issued / (kd * 1e-3) / 1e9, 100.0 * issued / (kd * 1e-3) / PEAK_WAVE_INSTR))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
