"""Windows/s of the batched LocalBundleAdjustment (orbx_lba_solve_batch) against the single-window call, in one process.

    python tools/lba_batch_rate.py [--steps 10] [--sizes 1,4,8,16,32] [--out profiles/lba_batch_rate.txt]
    python tools/lba_batch_rate.py --only 16 --steps 3     (one batch size: the workload of a rocprofv3 kernel trace)

Windows are make_window(K=50, P=5000) with distinct seeds (BASELINE config 5's shape).  Reported beside the batch rates: one handle at a
time (the rate of bench.py's `value`) and three handles in flight on their own streams and host threads (bench.py --full's
lba.windows_per_s_3_in_flight), kernel launches per batch call and the FP64 fraction of the device peak."""
import argparse
import importlib
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
FP64_PEAK_TF = 256 * 4 * 16 * 2 * 2.4e9 / 1e12      # as bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="1,4,8,16,32")
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    import ctypes
    L = orbx.load_library()
    L.orbx_debug_lba_batch_launches.argtypes = [ctypes.c_void_p]
    sizes = [a.only] if a.only else [int(x) for x in a.sizes.split(",")]
    nmax = max(sizes)
    ws = [orbx.lba_synth.make_window(K=50, P=5000, seed=9000 + i) for i in range(max(nmax, 3))]
    cap = dict(max_keyframes=50, max_points=max(w["P"] for w in ws), max_edges=max(w["E"] for w in ws))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    b = orbx.BatchOptimizer(nmax, **cap)
    rate = {}
    for n in sizes:
        batch = ws[:n]
        b.LocalBundleAdjustment(batch)      # warm-up
        t0 = time.perf_counter()
        ms, fl = [], 0.0
        for _ in range(a.steps):
            b.LocalBundleAdjustment(batch)
            m, fl = b.last_timing()
            ms.append(m)
        dt = time.perf_counter() - t0
        rate[n] = n * a.steps / dt
        launches = L.orbx_debug_lba_batch_launches(b._h)
        dev = sorted(ms)[len(ms) // 2]
        frac = fl / (dev * 1e-3) / 1e12 / FP64_PEAK_TF if dev > 0 else 0.0
        say("batch N=%2d: %8.1f windows/s  (%.3f ms per call wall, %.3f ms device, %d launches per call, FP64 fraction %.5f)"
            % (n, rate[n], dt / a.steps * 1e3, dev, launches, frac))
    b.close()
    if a.only:
        return
    # one handle at a time
    opt = orbx.Optimizer(**cap)
    opt.LocalBundleAdjustment(ws[0])
    t0 = time.perf_counter()
    for i in range(a.steps * 4):
        opt.LocalBundleAdjustment(ws[i % 8])
    one = a.steps * 4 / (time.perf_counter() - t0)
    say("single, one at a time: %8.1f windows/s" % one)
    # three handles in flight (own stream + host thread each)
    opts = [opt] + [orbx.Optimizer(**cap) for _ in range(2)]
    for o, w in zip(opts, ws):
        o.LocalBundleAdjustment(w)

    def work(i):
        for _ in range(a.steps * 4):
            opts[i].LocalBundleAdjustment(ws[i])
    th = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    three = 3 * a.steps * 4 / (time.perf_counter() - t0)
    say("single, 3 handles in flight: %8.1f windows/s" % three)
    for o in opts:
        o.close()
    for n in sizes:
        say("batch N=%2d / one at a time: %.2fx" % (n, rate[n] / one))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
