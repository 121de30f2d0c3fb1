"""What the device chains of Tracking::TrackWithMotionModel / TrackLocalMap cost against what a caller had before them
(profiles/track_chain_latency.txt).

(a) chain        one orbx_track_with_motion_model / orbx_track_local_map: wall clock of the C call alone on marshalled arrays.
(b) calls alone  the parent commit's entry points back to back on the same arrays - orbx_search_by_projection_last (or orbx_search_local_points)
                 and orbx_pose_optimization on a pose problem built ONCE outside the timed region: the glue's time is excluded.
(c) calls+numpy  the same two calls with the glue between and behind them (tests/track_ref.py's steps on preallocated arrays) inside the timed region.
device           milliseconds between the chain's launches (events; a series of its own: the events cost the other series nothing).
Synthetic scenes (tests/track_scenes.py) of 1000 / 2000 features with about 150 / 300 / 600 correspondences; medians of --calls calls after --warmup.
The baseline is (b) on the same machine in the same run.  One GPU process at a time: this process never opens the device; every shape runs in a
child of its own under `timeout -k 10 --step-seconds`, and the first child that fails or is killed ends the run - nothing more is started on the
device.  NOT measured: real frames, the shim on real Frame / MapPoint objects, and bench.py's dropin_track_ms_median, which keeps measuring the
old call chain.

    python tools/latency_track_chain.py [--calls 300] [--out profiles/track_chain_latency.txt]
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

import track_ref      # noqa: E402
import track_scenes as ts      # noqa: E402


def _median_ms(fn, a):
    t = []
    for it in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if it >= a.warmup:
            t.append((t1 - t0) * 1e3)
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def _pose_call(orbx, po, cap):
    """orbx_pose_optimization on preallocated arrays of `cap` edges: fill(prob) -> count, raw() -> rc."""
    poses, cams, counts = np.zeros(16, np.float32), np.zeros(5, np.float32), np.zeros(1, np.int32)
    Xw, obs, inv = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32), np.zeros(cap, np.float32)
    P = orbx.PoseProblem(1, cap, orbx._ptr(poses).value, orbx._ptr(cams).value, orbx._ptr(counts).value, orbx._ptr(Xw).value, orbx._ptr(obs).value, orbx._ptr(inv).value)
    out = np.zeros(16, np.float32), np.zeros(cap, np.uint8), np.zeros(1, np.int32), np.zeros(8, np.float64)
    args = [po._h, ctypes.byref(P)] + [orbx._ptr(o) for o in out]

    def raw():
        return po._L.orbx_pose_optimization(*args)
    raw.arrays, raw.out, raw.keep = (poses, cams, counts, Xw, obs, inv), out, P
    return raw


def run_shape(a, which, n, corr):
    """child process: one shape, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    mt, po = orbx.ORBmatcher(0.8, True, max_features=4096), orbx.PoseOptimizer(max_frames=1, max_features=4096)
    L = mt._L
    pose = _pose_call(orbx, po, n)
    poses, cams, counts, Xw, obs, inv = pose.arrays
    assigned, nm = np.full(n, -1, np.int32), ctypes.c_int32()
    if which == "motion":
        n_last = int(corr * 1.45)                                   # ~70 % of the last frame's features end as correspondences (invalid, wrong, pruned)
        fr, last, meta = ts.motion_scene(900 + n + corr, n_last=n_last, clutter=n - n_last, sensor="mixed")
        frame = dict(fr, kps=ts.struct_kps(orbx, fr["kps7"]))
        lastd = dict(last, kps=ts.struct_kps(orbx, last["kps7"]), valid=(last["valid"] == 1).astype(np.uint8))
        chain = mt.track_motion_prepare(frame, lastd, meta["th"], meta["mono"], ts.INV_SIGMA2)
        cth = ctypes.c_float(meta["th"])

        def search():
            return L.orbx_search_by_projection_last(mt._h, ctypes.byref(chain.F), ctypes.byref(chain.Ls), orbx._ptr(chain.sf), len(chain.sf), cth, 1 if meta["mono"] else 0, 1,
                                                    orbx._ptr(assigned), ctypes.byref(nm))
        k7, ur, lpos, lobs = fr["kps7"], fr["u_right"], np.asarray(last["pos"], np.float32), last["has_obs"]
        poses[:], cams[:] = np.asarray(fr["Tcw"], np.float32).reshape(16), fr["cam"]

        def glue_before():
            idx = np.flatnonzero(assigned >= 0)
            c = len(idx)
            counts[0] = c
            Xw[:c] = lpos[assigned[idx]]
            obs[:c, 0], obs[:c, 1], obs[:c, 2] = k7[idx, 0], k7[idx, 1], ur[idx]
            inv[:c] = ts.INV_SIGMA2[k7[idx, 5].astype(np.int64)]
            return idx

        def glue_after(idx):
            outl = np.zeros(n, np.uint8)
            outl[idx] = pose.out[1][:len(idx)]
            return track_ref.discard(np.where(assigned >= 0, assigned, -1), outl, lobs, nm.value)
    else:
        n_held = corr // 3
        m = int((corr - n_held) * 1.3)
        fr, sc = ts.local_scene(900 + n + corr, m=m, n_held=n_held, clutter=n - m - n_held, sensor="mixed")
        frame = dict(fr, kps=ts.struct_kps(orbx, fr["kps7"]))
        pts = {k: sc[k] for k in ("pos", "normal", "max_distance", "min_distance", "desc", "has_obs")}
        chain = mt.track_local_prepare(frame, sc["Tcw"], sc["cam"], ts.LOG_SCALE, pts, sc["th"], fr["held"], fr["held_pos"], ts.INV_SIGMA2, sc["stereo"])
        z = lambda dt: np.zeros(max(m, 1), dt)
        fv = [z(np.uint8), z(np.float32), z(np.float32), z(np.float32), z(np.int32), z(np.float32)]
        L.orbx_search_local_points.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 8

        def search():
            return L.orbx_search_local_points(mt._h, ctypes.byref(chain.F), ctypes.byref(chain.fr), ctypes.byref(chain.P), orbx._ptr(chain.sf), len(chain.sf), ctypes.c_float(0.5),
                                              ctypes.c_float(sc["th"]), ctypes.c_float(0.8), orbx._ptr(assigned), ctypes.byref(nm), *[orbx._ptr(x) for x in fv])
        k7, ur, ppos, pobs, held, hpos, occ = fr["kps7"], fr["u_right"], np.asarray(sc["pos"], np.float32), sc["has_obs"], fr["held"] != 0, fr["held_pos"], fr["occupied"]
        poses[:], cams[:] = np.asarray(sc["Tcw"], np.float32).reshape(16), sc["cam"]

        def glue_before():
            new = assigned >= 0
            idx = np.flatnonzero(new | held)
            c = len(idx)
            counts[0] = c
            X = hpos.copy()
            X[new] = ppos[assigned[new]]
            Xw[:c] = X[idx]
            obs[:c, 0], obs[:c, 1], obs[:c, 2] = k7[idx, 0], k7[idx, 1], ur[idx]
            inv[:c] = ts.INV_SIGMA2[k7[idx, 5].astype(np.int64)]
            return idx

        def glue_after(idx):
            outl = np.zeros(n, np.uint8)
            outl[idx] = pose.out[1][:len(idx)]
            new = assigned >= 0
            return track_ref.statistics(new | held, outl, np.where(new, pobs[np.maximum(assigned, 0)], occ), sc["stereo"])

    def check(rc):
        if rc != 0:
            orbx._check(rc)
    got = chain()
    a_ms = _median_ms(lambda: check(chain.raw()), a)
    check(search())
    glue_before()                                                   # the pose problem of (b), built once

    def calls_alone():
        check(search())
        check(pose())

    def calls_numpy():
        check(search())
        idx = glue_before()
        check(pose())
        glue_after(idx)
    b_ms, c_ms = _median_ms(calls_alone, a), _median_ms(calls_numpy, a)
    same = bool((pose.out[0].view(np.uint32) == got["pose"].reshape(16).view(np.uint32)).all())      # the baseline computed the chain's pose
    mt.track_kernel_times(True)
    ks = []
    for it in range(30):
        check(chain.raw())
        ks.append(mt.track_kernel_times())
    mt.track_kernel_times(False)
    print("RESULT " + json.dumps(dict(chain=a_ms, alone=b_ms, numpy=c_ms, corr=int(got["n_correspondences"]), same=same, kernels=[float(x) for x in np.median(np.array(ks), 0)])), flush=True)
    mt.close(); po.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", nargs=3, default=None, help=argparse.SUPPRESS)      # which n corr: run as the child of one shape
    a = ap.parse_args()
    if a.shape:
        return run_shape(a, a.shape[0], int(a.shape[1]), int(a.shape[2]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_track_with_motion_model / orbx_track_local_map (chain) against the parent commit's entry points called back to back: (b) calls alone =")
    say("search + orbx_pose_optimization, glue excluded; (c) the same with the glue in numpy.  Medians of %d calls after %d, ms, wall clock of the C" % (a.calls, a.warmup))
    say("calls; device = ms between the chain's launches (motion: stage, pass 1, pass 2 [gated off], gather, pose, discard; local: stage, search,")
    say("gather, pose, statistics).  Not measured: real frames, the shim on real objects, dropin_track_ms_median (still the old call chain).")
    say("%-26s | %5s | %7s %7s %7s | %9s %9s | %-14s | %s" % ("shape", "corr", "chain", "p10", "p90", "(b) alone", "(c) numpy", "(b)/(a) (c)/(a)", "device per launch"))
    for which in ("motion", "local"):
        for n in (1000, 2000):
            for corr in (150, 300, 600):
                name = "%s n=%d ~%d" % (which, n, corr)
                cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, str(Path(__file__).resolve()), "--calls", str(a.calls), "--warmup", str(a.warmup),
                       "--shape", which, str(n), str(corr)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                out = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not out:
                    say("%-26s | failed with status %d: stopped, nothing more is started on the device" % (name, r.returncode))
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    _write(a, lines)
                    return r.returncode or 1
                d = json.loads(out[0][7:])
                m = d["chain"]
                say("%-26s | %5d | %7.3f %7.3f %7.3f | %9.3f %9.3f | %5.2fx %5.2fx%s | %s%s"
                    % (name, d["corr"], m[0], m[1], m[2], d["alone"][0], d["numpy"][0], d["alone"][0] / m[0], d["numpy"][0] / m[0], "  " if d["alone"][0] > m[0] else " !",
                       " ".join("%.3f" % k for k in d["kernels"]), "" if d["same"] else "  (baseline pose differs)"))
    say("'!' marks a shape at which the chain is NOT faster than (b).")
    _write(a, lines)
    return 0


def _write(a, lines):
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
