"""What the device chains of Tracking::TrackReferenceKeyFrame and of the head of Tracking::Relocalization cost against what a caller had before them
(profiles/track_ref_latency.txt).

reference keyframe
(a) chain        one orbx_track_reference_keyframe: wall clock of the C call alone on marshalled arrays.
(b) calls alone  the unchanged entry points back to back on the same arrays - orbx_search_by_bow and orbx_pose_optimization on a pose problem built
                 ONCE outside the timed region: the glue's time is excluded.
(c) calls+numpy  the same two calls with the glue between and behind them (tests/track_ref_kf_ref.py's steps on preallocated arrays) inside the
                 timed region.
candidates
(a) chain        one orbx_reloc_match_candidates for K candidate keyframes.
(b) K calls      K orbx_search_by_bow calls on the same arrays (the gather of the PnP arrays is not part of it).
device           milliseconds between the chain's launches (events; a series of its own: the events cost the other series nothing).
Synthetic scenes (tests/track_ref_kf_scenes.py): frames of 1000 / 2000 features, about 150 / 300 / 600 correspondences, K = 1 / 4 / 8 candidates of
about 1000 slots; medians of --calls calls after --warmup.  The baseline is (b) on the same machine in the same run.  One GPU process at a time:
this process never opens the device; every shape runs in a child of its own under `timeout -k 10 --step-seconds`, and the first child that fails
or is killed ends the run - nothing more is started on the device.  NOT measured: real frames and the shim's gather over real KeyFrame / MapPoint
objects (synthetic scenes only), and bench.py's dropin_track_ms_median, which keeps measuring the old call chain.

    python tools/latency_track_ref.py [--calls 300] [--out profiles/track_ref_latency.txt]
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

import track_ref_kf_ref as kref      # noqa: E402
import track_ref_kf_scenes as ks      # noqa: E402
import track_scenes as ts      # noqa: E402
from latency_track_chain import _median_ms, _pose_call, _write      # noqa: E402


def _bow_call(orbx, mt, kf, fr, nn):
    """orbx_search_by_bow (mode 0) on marshalled arrays: raw() -> rc; the matches land in raw.out, the count in raw.nm"""
    fa, ka = orbx._host_set(ts.struct_kps(orbx, kf["kps7"]), kf["desc"], kf["groups"], kf["valid"])
    fb, kb = orbx._host_set(ts.struct_kps(orbx, fr["kps7"]), fr["desc"], fr["groups"])
    out, nm = np.full(len(fr["kps7"]), -1, np.int32), ctypes.c_int32()
    prm = orbx.BowParams(nn, 1, 0)
    args = [mt._h, ctypes.byref(fa), ctypes.byref(fb), ctypes.byref(prm), orbx._ptr(out), ctypes.byref(nm)]

    def raw():
        return mt._L.orbx_search_by_bow(*args)
    raw.out, raw.nm, raw.keep = out, nm, (fa, ka, fb, kb, prm)
    return raw


def _dev_kf(orbx, kf):
    return dict(kps=ts.struct_kps(orbx, kf["kps7"]), desc=kf["desc"], pos=kf["pos"], groups=kf["groups"], valid=kf["valid"], has_obs=kf["has_obs"])


def run_shape(a, which, n, arg):
    """child process: one shape, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")

    def check(rc):
        if rc != 0:
            orbx._check(rc)
    if which == "track":
        corr = arg
        mt, po = orbx.ORBmatcher(0.7, True, max_features=4096), orbx.PoseOptimizer(max_frames=1, max_features=4096)
        n_seen = int(corr * 1.2)                                    # ~83 % of the seen points end as correspondences (invalid, unfiled, pruned)
        kf, fr, _ = ks.ref_scene(900 + n + corr, n_seen=n_seen, kf_extra=max(1000 - n_seen, 0), clutter=n - n_seen, sensor="mixed")
        frame = dict(kps=ts.struct_kps(orbx, fr["kps7"]), kps_un=ts.struct_kps(orbx, fr["kps7_un"]), desc=fr["desc"], groups=fr["groups"], u_right=fr["u_right"], Tcw=fr["Tcw"],
                     cam=fr["cam"], inv_level_sigma2=ks.INV_SIGMA2)
        chain = mt.track_reference_prepare(_dev_kf(orbx, kf), frame)
        search, pose = _bow_call(orbx, mt, kf, fr, 0.7), _pose_call(orbx, po, n)
        poses, cams, counts, Xw, obs, inv = pose.arrays
        k7u, ur, kpos, kobs, assigned = fr["kps7_un"], fr["u_right"], np.asarray(kf["pos"], np.float32), kf["has_obs"], search.out
        poses[:], cams[:] = np.asarray(fr["Tcw"], np.float32).reshape(16), fr["cam"]

        def glue_before():
            idx = np.flatnonzero(assigned >= 0)
            c = len(idx)
            counts[0] = c
            Xw[:c] = kpos[assigned[idx]]
            obs[:c, 0], obs[:c, 1], obs[:c, 2] = k7u[idx, 0], k7u[idx, 1], ur[idx]
            inv[:c] = ks.INV_SIGMA2[k7u[idx, 5].astype(np.int64)]
            return idx

        def glue_after(idx):
            outl = np.zeros(n, np.uint8)
            outl[idx] = pose.out[1][:len(idx)]
            return kref.discard(assigned, outl, kobs, search.nm.value)
        got = chain()
        a_ms = _median_ms(lambda: check(chain.raw()), a)
        check(search())
        glue_before()                                               # the pose problem of (b), built once

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
        res = dict(chain=a_ms, alone=b_ms, numpy=c_ms, corr=int(got["n_correspondences"]), same=same)
        closers = (mt, po)
    else:
        K = arg
        mt = orbx.ORBmatcher(0.75, True, max_features=4096, max_pairs=8)
        fr, kfs = ks.reloc_scene(950 + n + K, n_frame=n, n_real=int(n * 0.6), kfs=tuple((1000 - 40 * c, 300 + 20 * c) for c in range(K)))
        frame = dict(kps=ts.struct_kps(orbx, fr["kps7"]), kps_un=ts.struct_kps(orbx, fr["kps7_un"]), desc=fr["desc"], groups=fr["groups"], level_sigma2=ks.LEVEL_SIGMA2)
        chain = mt.reloc_match_prepare(frame, [_dev_kf(orbx, kf) for kf in kfs])
        singles = [_bow_call(orbx, mt, kf, fr, 0.75) for kf in kfs]
        got = chain()
        a_ms = _median_ms(lambda: check(chain.raw()), a)

        def calls_alone():
            for s in singles:
                check(s())
        b_ms = _median_ms(calls_alone, a)
        same = all((s.out == got["matches"][c]).all() and s.nm.value == got["nmatches"][c] for c, s in enumerate(singles))
        res = dict(chain=a_ms, alone=b_ms, numpy=b_ms, corr=int(got["n"].sum()), same=bool(same))
        closers = (mt,)
    mt.track_kernel_times(True)
    kt = []
    for it in range(30):
        check(chain.raw())
        kt.append(mt.track_kernel_times())
    mt.track_kernel_times(False)
    res["kernels"] = [float(x) for x in np.median(np.array(kt), 0)]
    print("RESULT " + json.dumps(res), flush=True)
    for h in closers:
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", nargs=3, default=None, help=argparse.SUPPRESS)      # which n arg: run as the child of one shape
    a = ap.parse_args()
    if a.shape:
        return run_shape(a, a.shape[0], int(a.shape[1]), int(a.shape[2]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_track_reference_keyframe / orbx_reloc_match_candidates (chain) against the unchanged entry points called back to back.  track: (b) calls alone =")
    say("orbx_search_by_bow + orbx_pose_optimization, glue excluded; (c) the same with the glue in numpy.  candidates: (b) = K orbx_search_by_bow calls (no (c)).")
    say("Medians of %d calls after %d, ms, wall clock of the C calls, p10 / p90 of the chain beside it; device = ms between the chain's launches (track: stage," % (a.calls, a.warmup))
    say("search, gather, pose, discard; candidates: stage, search, gather).  Synthetic scenes; real frames and the shim's gather not measured.")
    say("%-26s | %5s | %7s %7s %7s | %9s %9s | %-14s | %s" % ("shape", "corr", "chain", "p10", "p90", "(b) alone", "(c) numpy", "(b)/(a) (c)/(a)", "device per launch"))
    shapes = [("track", n, corr) for n in (1000, 2000) for corr in (150, 300, 600)] + [("candidates", n, K) for n in (1000, 2000) for K in (1, 4, 8)]
    for which, n, arg in shapes:
        name = "%s n=%d %s%d" % (which, n, "~" if which == "track" else "K=", arg)
        cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, str(Path(__file__).resolve()), "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--shape", which, str(n), str(arg)]
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
               " ".join("%.3f" % k for k in d["kernels"]), "" if d["same"] else "  (baseline result differs)"))
    say("'!' marks a shape at which the chain is NOT faster than (b).  corr: correspondences of the pose problem / PnP matches over all candidates.")
    _write(a, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
