"""What the RGB-D step costs (profiles/rgbd_latency.txt).

latency form, one 640x480 frame, 1000 features, TUM1 camera; per call = single-frame extractor call + ...
    mono        orbx_frame_finish_begin / _end                      (the monocular constructor's chain: the baseline)
    rgbd        orbx_frame_rgbd_begin / _end, depth looked up on the host (the default)
    rgbd-stage  the same with ORBX_RGBD_STAGE_IMAGE=1: the image copied to pinned memory, gathered by the kernel
for uint16 and float32 depth; the variants alternate call by call in one process, median / p10 / p90 of --calls calls after --warmup.
batch form: frames/s of orbx_extract_batch_device + orbx_frame_finish_device against + orbx_frame_rgbd_device at --batch frames,
wall clock around --reps launches ending in a stream synchronisation, variants alternating.

    python tools/latency_rgbd.py [--calls 1000] [--batch 256] [--out FILE]
"""
import argparse
import ctypes
import importlib
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import rgbd_ref      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    L = orbx.load_library()
    W, H, nf = 640, 480, 1000
    K, dist = rgbd_ref.CAMS["tum1"]
    thd = float(rgbd_ref.th_depth(K[0]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ops = orbx.FrameOps(K[0], K[1], K[2], K[3], dist)
    grid = orbx.FrameGrid.from_bounds(ops.ComputeImageBounds(W, H))
    g = ctypes.byref(grid)
    prm = orbx.RgbdParams(rgbd_ref.BF, thd)
    p = ctypes.byref(prm)
    vp = ctypes.c_void_p
    L.orbx_frame_finish_begin.argtypes = [vp, vp, vp]
    L.orbx_frame_finish_end.argtypes = [vp, vp, vp, vp, vp]

    # ---- latency form ----
    ext = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H)
    frames = [rgbd_ref.gray_frame(s, W, H) for s in range(61, 69)]
    raws = [rgbd_ref.depth_raw(s, W, H) for s in range(61, 69)]
    f32s = [np.multiply(r.astype(np.float32), rgbd_ref.U16_FACTOR) for r in raws]
    d16 = [orbx.DepthDesc.of(r, float(rgbd_ref.U16_FACTOR)) for r in raws]
    d32 = [orbx.DepthDesc.of(r) for r in f32s]
    kp, dp, cnt = vp(), vp(), ctypes.c_int()
    un, off, idx, n, rf = vp(), vp(), vp(), ctypes.c_int(), orbx.RgbdFrame()
    variants = [("mono", None, "0"), ("rgbd u16", d16, "0"), ("rgbd f32", d32, "0"), ("rgbd-stage u16", d16, "1"), ("rgbd-stage f32", d32, "1")]
    times = {v[0]: [] for v in variants}
    for it in range(a.warmup + a.calls):
        f = it % len(frames)
        im = frames[f]
        for name, dds, stage in variants:
            os.environ["ORBX_RGBD_STAGE_IMAGE"] = stage
            t0 = time.perf_counter()
            orbx._check(L.orbx_extract_view_pyramid(ext._h, im.ctypes.data, W, H, W, ctypes.byref(kp), ctypes.byref(dp), ctypes.byref(cnt), None))
            if dds is None:
                orbx._check(L.orbx_frame_finish_begin(ops._h, ext._h, g))
                orbx._check(L.orbx_frame_finish_end(ops._h, ctypes.byref(un), ctypes.byref(off), ctypes.byref(idx), ctypes.byref(n)))
            else:
                orbx._check(L.orbx_frame_rgbd_begin(ops._h, ext._h, g, ctypes.byref(dds[f]), p))
                orbx._check(L.orbx_frame_rgbd_end(ops._h, ctypes.byref(un), ctypes.byref(off), ctypes.byref(idx), ctypes.byref(n), ctypes.byref(rf)))
            t1 = time.perf_counter()
            if it >= a.warmup:
                times[name].append((t1 - t0) * 1e6)
    say("latency form: extractor call + frame finish, %dx%d, %d features, %d calls per variant (alternating), microseconds" % (W, H, nf, a.calls))
    base = float(np.median(times["mono"]))
    for name, _, _ in variants:
        t = np.asarray(times[name])
        say("  %-16s median %8.1f   p10 %8.1f   p90 %8.1f   vs mono %+6.1f" % (name, np.median(t), np.percentile(t, 10), np.percentile(t, 90), np.median(t) - base))
    os.environ["ORBX_RGBD_STAGE_IMAGE"] = "0"
    ext.close()

    # ---- batch form ----
    B = a.batch
    bext = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    dev = bext.upload([frames[i % len(frames)] for i in range(B)])
    depth_dev = ops.upload_depth([raws[i % len(raws)] for i in range(B)], float(rgbd_ref.U16_FACTOR))
    dd = ctypes.byref(depth_dev)
    rates = {"finish": [], "rgbd": []}
    for rep in range(3 + a.reps):
        for name in ("finish", "rgbd"):
            bext.sync()
            t0 = time.perf_counter()
            for _ in range(4):
                bext.run_device(*dev)
                if name == "finish":
                    orbx._check(L.orbx_frame_finish_device(ops._h, bext._h, g))
                else:
                    orbx._check(L.orbx_frame_rgbd_device(ops._h, bext._h, g, dd, p))
            bext.sync()
            t1 = time.perf_counter()
            if rep >= 3:
                rates[name].append(4 * B / (t1 - t0))
    fin, rg = float(np.median(rates["finish"])), float(np.median(rates["rgbd"]))
    say("batch form: B = %d, extract + frame finish, %d timed windows of 4 batches per variant (alternating), frames/s" % (B, a.reps))
    say("  finish  median %10.0f   min %10.0f   max %10.0f" % (fin, min(rates["finish"]), max(rates["finish"])))
    say("  rgbd    median %10.0f   min %10.0f   max %10.0f   ratio rgbd / finish %.4f" % (rg, min(rates["rgbd"]), max(rates["rgbd"]), rg / fin))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
