"""What loading a DBoW2 text vocabulary costs (profiles/voc_load_latency.txt): orbx_vocabulary_load_text beside three baselines.

Files: voc_synth.make_vocabulary_fast trees at k = 10 with L = 4, 5, 6 written by write_text_fast (repr weights, 16 - 17 digits), and the L = 6 tree
again with '%g' weights - the shape of the reference's ORBvoc.txt.  Per file, page cache warm (the file was just written and is read once before the
clock starts), three alternations of

    device     Vocabulary.from_text(path): total_ms and its split - read (fread into pinned slices), upload (the copies' time on the stream),
               kernels (HIP events around the whole chain: per-stage events are not recorded), host (header, flagged lines)
    reference  the compiled reference's loadFromTextFile through oracle_lib.RefVocabulary (oracle/_ref), when it is built
    host       read() + orbx_voc_text_parse_host (one call, arrays sized from the newline count) + orbx_vocabulary_create, one thread
    create     orbx_vocabulary_create alone from ready arrays: what a C caller pays today AFTER parsing

The chain's bytes per second (text bytes / kernel time: a lower bound for the parse kernel, which is one of eleven launches) stands beside the HBM
peak, the upload beside the pinned PCIe rates of profiles/r05_d2h_pinned.txt.  Every file runs in a child of its own under `timeout -k 10`; the
first child that fails ends the run.  NOT measured: a cold page cache, a real ORBvoc.txt (absent), the shim's fill of 1.1 M cv::Mat nodes.

    python tools/latency_voc_load.py [--files L4,L5,L6,L6g] [--out profiles/voc_load_latency.txt]
"""
import argparse
import ctypes
import importlib
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
FILES = {"L4": (4, "%r"), "L5": (5, "%r"), "L6": (6, "%r"), "L6g": (6, "%g")}
HBM_TBS, PCIE_GBS = 6.29, 52.0      # measured float4 copy (MI355X_MICROARCH); pinned 3 MB transfers (profiles/r05_d2h_pinned.txt)
REPS = 3


def write_text(voc, path, fmt, chunk=1 << 16):
    """voc_synth.write_text_fast's file with the weight through `fmt`"""
    pair = ["%d %d" % (v & 255, v >> 8) for v in range(65536)]
    n = voc["num_nodes"]
    par, leaf = np.asarray(voc["parent"]), np.asarray(voc["is_leaf"])
    d16 = np.ascontiguousarray(voc["desc"], np.uint8).view("<u2")
    wt = np.asarray(voc["weight"], np.float64)
    get = pair.__getitem__
    line = "\n%d %d %s " + fmt
    with open(path, "w") as f:
        f.write("%d %d 0 0" % (voc["k"], voc["L"]))
        for lo in range(1, n, chunk):
            hi = min(n, lo + chunk)
            rows = zip(par[lo:hi].tolist(), leaf[lo:hi].tolist(), d16[lo:hi].tolist(), wt[lo:hi].tolist())
            f.write("".join([line % (p, l, " ".join(map(get, d)), w) for p, l, d, w in rows]))


def run_file(name):
    """child process: one file, one JSON line"""
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    import oracle_lib
    L, fmt = FILES[name]
    voc = orbx.voc_synth.make_vocabulary_fast(10, L, 1, ragged=False)
    lib = orbx.load_library()
    orbx._bind_voc_text(lib)
    res = dict(name=name, L=L, fmt=fmt, nodes=int(voc["num_nodes"]), device=[], reference=[], host=[], create=[])
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "voc.txt"
        if fmt == "%r":
            orbx.voc_synth.write_text_fast(voc, path)
        else:
            write_text(voc, path, fmt)
        data = path.read_bytes()      # (warms the page cache)
        res["bytes"] = len(data)
        have_ref = oracle_lib.slam_lib() is not None
        orbx.Vocabulary.from_text(path).close()      # warm-up: the library, the device, the first allocations
        for _ in range(REPS):
            t0 = time.perf_counter()
            V = orbx.Vocabulary.from_text(path)
            wall = (time.perf_counter() - t0) * 1e3
            res["device"].append(dict(V.text_info, wall_ms=wall))
            got = V.tree() if len(res["device"]) == 1 else None
            V.close()
            if have_ref:
                t0 = time.perf_counter()
                R = oracle_lib.RefVocabulary(path)
                res["reference"].append((time.perf_counter() - t0) * 1e3)
                del R
            t0 = time.perf_counter()
            raw = path.read_bytes()
            cap = raw.count(b"\n") + 2
            par, leaf, desc, wt = np.zeros(cap, np.int32), np.zeros(cap, np.uint8), np.zeros((cap, 32), np.uint8), np.zeros(cap, np.float64)
            info = orbx.VocTextInfo()
            assert lib.orbx_voc_text_parse_host(raw, len(raw), ctypes.byref(info), cap, par.ctypes.data, leaf.ctypes.data, desc.ctypes.data, wt.ctypes.data) == 0
            t1 = time.perf_counter()
            n = info.num_nodes
            H = orbx.Vocabulary(dict(k=info.k, L=info.L, parent=par[:n], is_leaf=leaf[:n], desc=desc[:n], weight=wt[:n]))
            t2 = time.perf_counter()
            H.close()
            res["host"].append(((t2 - t0) * 1e3, (t1 - t0) * 1e3))
            t0 = time.perf_counter()
            C = orbx.Vocabulary(voc)
            res["create"].append((time.perf_counter() - t0) * 1e3)
            C.close()
            if got is not None:      # the loaded tree is the tree that was written (weights: the text's doubles)
                same = all((got[k] == voc[k]).all() for k in ("parent", "is_leaf")) and (got["desc"][1:] == voc["desc"][1:]).all()
                same = same and (got["weight"].view(np.uint64) == wt[:n].view(np.uint64)).all()
                res["same_tree"] = bool(same)
    print("RESULT " + json.dumps(res), flush=True)


def child(a, name):
    cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, str(Path(__file__).resolve()), "--file", name]
    r = subprocess.run(cmd, capture_output=True, text=True)
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not out:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1, None
    return 0, json.loads(out[0][7:])


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (sorted(xs)[len(xs) // 2], min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-seconds", type=int, default=400)
    ap.add_argument("--files", default="L4,L5,L6,L6g")
    ap.add_argument("--out", default=None)
    ap.add_argument("--file", default=None, help=argparse.SUPPRESS)      # run as the child of one file
    a = ap.parse_args()
    if a.file:
        return run_file(a.file)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("orbx_vocabulary_load_text: full k = 10 trees of voc_synth.make_vocabulary_fast as DBoW2 text, page cache warm; ms, median (min .. max) of %d alternations." % REPS)
    say("device = Vocabulary.from_text(path): wall | read + upload + kernels + host (the library's own split; read and upload overlap) | launches, waits, host_lines.")
    say("reference = the compiled reference's loadFromTextFile; host = read + orbx_voc_text_parse_host + orbx_vocabulary_create on one thread (parse share);")
    say("create = orbx_vocabulary_create alone from ready arrays.  chain = text bytes / kernel time, against %.2f TB/s HBM; upload against %.0f GB/s pinned PCIe." % (HBM_TBS, PCIE_GBS))
    say("NOT measured: a cold page cache, a real ORBvoc.txt, the shim's m_nodes fill (1.1 M cv::Mat).")
    for name in a.files.split(","):
        rc, d = child(a, name)
        if rc:
            say("%-4s | failed with status %d: stopped, nothing more is started on the device" % (name, rc))
            _write(a, lines)
            return rc
        dv = d["device"]
        med = lambda key: sorted(x[key] for x in dv)[len(dv) // 2]
        say("%-4s L = %d weights %s: %d nodes, %.1f MB%s" % (name, d["L"], d["fmt"], d["nodes"], d["bytes"] / 1e6, "" if d.get("same_tree") else "  DIFFERENT TREE"))
        say("     device    %s | read %.1f + upload %.1f + kernels %.2f + host %.2f | %d launches, %d waits, %d host lines" % (
            spread([x["wall_ms"] for x in dv]), med("read_ms"), med("upload_ms"), med("kernel_ms"), med("host_ms"), dv[0]["launches"], dv[0]["waits"], dv[0]["host_lines"]))
        say("               chain %.1f GB/s = %.1f %% of HBM peak | upload %.1f GB/s = %.0f %% of pinned PCIe" % (
            d["bytes"] / med("kernel_ms") / 1e6, 100 * d["bytes"] / med("kernel_ms") / 1e6 / (HBM_TBS * 1e3), d["bytes"] / max(med("upload_ms"), 1e-6) / 1e6,
            100 * d["bytes"] / max(med("upload_ms"), 1e-6) / 1e6 / PCIE_GBS))
        if d["reference"]:
            r, w = d["reference"], [x["wall_ms"] for x in dv]
            say("     reference %s | device is %.1f x faster (medians); worst device %.1f vs best reference %.1f" % (spread(r), sorted(r)[1] / sorted(w)[1], max(w), min(r)))
        else:
            say("     reference not built here")
        h = [x[0] for x in d["host"]]
        say("     host      %s (parse %.1f) | create %s" % (spread(h), sorted(x[1] for x in d["host"])[1], spread(d["create"])))
    _write(a, lines)
    return 0


def _write(a, lines):
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
