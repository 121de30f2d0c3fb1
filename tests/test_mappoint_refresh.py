"""Batched MapPoint refresh (orbx_mappoint_refresh / MapPointOps): MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth
(reference src/MapPoint.cc:359-439, 477-521) for M points with ragged observation lists.

Expected values: tests/mappoint_ref.py's numpy restatement of the stated semantics.  Every comparison is exact: ints equal, floats by bit
pattern."""
import ctypes
import functools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mappoint_ref as ref

ROOT = Path(__file__).resolve().parent.parent
ERR_ARG, ERR_NODEVICE = -1, -4
INT_MAX = 2**31 - 1
SIZES = [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 600]      # both sides of every size-class boundary of the kernels (64 / 128 / 256) and the strided class
ORDER_SEED = 7                                             # chosen on the CPU: test_float_sum_depends_on_the_order holds for it


def _gpu():
    import torch
    return torch.cuda.is_available()


@functools.lru_cache(maxsize=None)
def window():
    """300 generated points, 1..12 observers each; computed once, never modified"""
    import importlib
    orbx = importlib.import_module("self_commit_orb-slam2_amd")
    w = orbx.lba_synth.make_window(K=20, P=300, seed=ORDER_SEED, max_obs=12, n_fixed=2)
    return ref.window_batch(w, seed=ORDER_SEED)


@functools.lru_cache(maxsize=None)
def window_expected(reverse=False):
    return ref.restate(ref.reverse(window()) if reverse else window())


@functools.lru_cache(maxsize=None)
def order_sensitive_points():
    """points of the window batch whose normal changes bits when their observers are reversed"""
    f, r = window_expected(False), window_expected(True)
    return np.nonzero((f["normal"].view(np.uint32) != r["normal"].view(np.uint32)).any(1))[0]


def bind(orbx):
    L = orbx.load_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbx_mappoint_ops_create.argtypes = [ci, ci, ci, ctypes.POINTER(vp)]
    L.orbx_mappoint_ops_create.restype = ci
    L.orbx_mappoint_ops_destroy.argtypes = [vp]
    L.orbx_mappoint_ops_destroy.restype = None
    L.orbx_mappoint_refresh.argtypes = [vp, ctypes.POINTER(orbx.MapPointBatch), ctypes.POINTER(orbx.MapPointResult)]
    L.orbx_mappoint_refresh.restype = ci
    L.orbx_mappoint_last_timing.argtypes = [vp, vp, vp]
    L.orbx_mappoint_last_timing.restype = ci
    return L


def run(ops, b):
    return ops.refresh(*[b[k] for k in ("obs_offset", "desc", "cam_center", "pos", "ref_center", "ref_scale", "top_scale")], desc_valid=b["desc_valid"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_median_rule_equals_brute_force():
    """the restatement's order statistic / first arg-min == sorted(row)[(N-1)//2] and a strict `<` scan, 200 random points incl. N = 1, 2, 3"""
    rng = np.random.default_rng(3)
    ns = [1, 2, 3] * 4 + [int(n) for n in rng.integers(1, 41, 188)]
    assert len(ns) == 200
    ties = 0
    for n in ns:
        desc = ref.flipped_descriptors(rng, n, int(rng.integers(0, 5)))
        valid = (rng.random(n) < 0.8).astype(np.uint8) if rng.random() < 0.5 else None
        idx = [i for i in range(n) if valid is None or valid[i]]
        best, best_median = -1, INT_MAX
        meds = []
        for i in idx:
            row = sorted(int(ref.POP[desc[i] ^ desc[j]].sum()) for j in idx)
            median = row[(len(idx) - 1) // 2]
            meds.append(median)
            if median < best_median:
                best, best_median = i, median
        ties += meds.count(best_median) > 1
        assert ref.distinctive(desc, valid) == (best, best_median), (n, valid)
    assert ties >= 20      # the lowest-index rule is actually exercised


def test_float_sum_depends_on_the_order():
    """at least one point of the window batch changes bits when its observers are reversed: a tree reduction on the device cannot pass the
    GPU order test unnoticed"""
    assert np.diff(window()["obs_offset"]).max() >= 3
    assert len(order_sensitive_points()) >= 1
    f, r = window_expected(False), window_expected(True)
    # reversing changes nothing else: the same set of rows, so the same smallest median, and the same distances to the reference keyframe
    assert np.array_equal(f["best_median"], r["best_median"]) and np.array_equal(f["updated"], r["updated"])


def test_restatement_on_hand_made_points():
    a = np.zeros(32, np.uint8)
    c = np.full(32, 255, np.uint8)
    assert ref.distinctive(np.stack([a, c])) == (0, 0)              # N = 2: position (2-1)//2 = 0 of [0, 256]
    assert ref.distinctive(np.stack([a, c, c])) == (1, 0)           # N = 3: rows [0,256,256], [0,0,256], [0,0,256]
    assert ref.distinctive(np.stack([a, c]), np.array([0, 0], np.uint8)) == (-1, INT_MAX)
    nrm, mx, mn = ref.normal_depth(np.array([0, 0, 2], np.float32), np.array([[0, 0, 0], [0, 0, 1]], np.float32), np.zeros(3, np.float32), 2.0, 4.0)
    assert list(nrm) == [0.0, 0.0, 1.0] and mx == 4.0 and mn == 1.0


def test_create_without_a_device(orbx):
    """the four new functions are exported; ORBX_ERR_NODEVICE without a device (no CPU fallback), a handle with one"""
    L = bind(orbx)
    for sym in ("orbx_mappoint_ops_create", "orbx_mappoint_ops_destroy", "orbx_mappoint_refresh", "orbx_mappoint_last_timing"):
        assert hasattr(L, sym), sym
    h = ctypes.c_void_p()
    assert L.orbx_mappoint_ops_create(0, 0, 10, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_mappoint_ops_create(0, 10, 10, None) == ERR_ARG
    rc = L.orbx_mappoint_ops_create(0, 100, 1000, ctypes.byref(h))
    if _gpu():
        assert rc == 0 and h.value
        L.orbx_mappoint_ops_destroy(h)
    else:
        assert rc == ERR_NODEVICE and not h.value
        assert len(L.orbx_last_error()) > 0
        with pytest.raises(orbx.OrbxError) as e:
            orbx.MapPointOps(100, 1000)
        assert e.value.code == ERR_NODEVICE
    # NULL handles are errors, not crashes
    assert L.orbx_mappoint_refresh(None, None, None) == ERR_ARG
    assert L.orbx_mappoint_last_timing(None, None, None) == ERR_ARG
    L.orbx_mappoint_ops_destroy(None)


REF = Path("/root/reference")


@pytest.mark.skipif(not os.access(REF / "include" / "MapPoint.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-DOPTIMIZER_H", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "MapPoint_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    src = (shim / "MapPoint_hip.cc").read_text()
    assert "void RefreshMapPoints(const std::vector<MapPoint *> &pts, bool descriptor, bool normalAndDepth)" in src
    assert "MapPoint_hip" not in (ROOT / "oracle" / "Makefile").read_text()      # not part of the drop-in link


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(orbx):
    o = orbx.MapPointOps(4096, 65536)
    yield o
    o.close()


@pytest.mark.gpu
def test_size_classes(ops):
    """n on both sides of every class boundary, plus the 300 generated points, in ONE ragged batch"""
    b = ref.concat(ref.synth_batch(SIZES, seed=11), window())
    want = ref.restate(b)
    got = run(ops, b)
    assert got["updated"].all()
    assert ref.same_bits(got, want)
    ms, launches = ops.last_timing()
    assert launches == 4 and ms > 0      # one launch per non-empty class


@pytest.mark.gpu
def test_ties_give_the_lowest_index(ops):
    rng = np.random.default_rng(5)
    pts = []
    for n in (1, 2, 5, 64, 65, 130, 257, 300):
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        pts.append(ref.synth_point(rng, n, desc=np.tile(d, (n, 1))))                       # all identical
        e = d.copy(); e[:4] ^= 0xff
        alt = np.stack([d if i % 2 == 0 else e for i in range(n)])                          # two alternating descriptors
        pts.append(ref.synth_point(rng, n, desc=alt))
    # identical descriptors behind an invalid first observer: the first VALID one
    q = ref.synth_point(rng, 7, desc=np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (7, 1)))
    q["valid"] = np.array([0, 0, 1, 1, 0, 1, 1], np.uint8)
    pts.append(q)
    b = ref.pack(pts)
    got = run(ops, b)
    want = ref.restate(b)
    assert ref.same_bits(got, want)
    ident = got["best_obs"][0:-1:2]
    assert (ident == 0).all() and (got["best_median"][0:-1:2] == 0).all()
    assert got["best_obs"][-1] == 2 and got["best_median"][-1] == 0
    # alternating: even rows see ceil(n/2) zeros, odd rows floor(n/2): the median is 0 for row 0 whenever it is for any row
    assert (got["best_obs"][1:-1:2] == 0).all()


@pytest.mark.gpu
def test_complementary_descriptors(ops):
    """a distance of 256 is representable: a row whose median is 256 must lose against one whose median is 0 (stored in 8 bits it would read 0
    and, having the lower index, win)"""
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    c = a ^ 0xff
    pts = [ref.synth_point(rng, 2, desc=np.stack([a, c])), ref.synth_point(rng, 3, desc=np.stack([a, c, c])), ref.synth_point(rng, 3, desc=np.stack([c, a, c])),
           ref.synth_point(rng, 3, desc=np.stack([a, c, c]))]
    pts[3]["valid"] = np.array([1, 1, 0], np.uint8)
    # N = 2: position 0 of [0, 256] is the self-distance.  N = 3, (a, c, c): row 0 = [0, 256, 256] has median 256, rows 1 and 2 = [0, 0, 256] have 0.
    # N = 4, two of each: position 1 of [0, 0, 256, 256] = 0
    pts.append(ref.synth_point(rng, 4, desc=np.stack([a, a, c, c])))
    b = ref.pack(pts)
    got, want = run(ops, b), ref.restate(b)
    assert ref.same_bits(got, want)
    assert list(got["best_obs"]) == [0, 1, 0, 0, 0] and list(got["best_median"]) == [0, 0, 0, 0, 0]
    # the same in the larger size classes: 299 x a then 301 x c, position 299: the rows of a hold 299 zeros (median 256), the rows of c 301 (median 0)
    big = ref.pack([ref.synth_point(rng, 600, desc=np.stack([a] * 299 + [c] * 301)), ref.synth_point(rng, 60, desc=np.stack([a] * 29 + [c] * 31)),
                    ref.synth_point(rng, 200, desc=np.stack([c] * 101 + [a] * 99))])
    got, want = run(ops, big), ref.restate(big)
    assert ref.same_bits(got, want)
    assert list(got["best_obs"]) == [299, 29, 0] and list(got["best_median"]) == [0, 0, 0]
    only = ref.pack([ref.synth_point(rng, 2, desc=np.stack([a, c]))])
    only["desc_valid"] = np.array([0, 1], np.uint8)
    assert list(run(ops, only)["best_obs"]) == [1]


@pytest.mark.gpu
def test_desc_valid_and_empty_points(ops):
    rng = np.random.default_rng(8)
    pts = []
    for n in (3, 9, 40, 64, 100, 256, 300, 600):
        q = ref.synth_point(rng, n)
        q["valid"] = (rng.random(n) < 0.6).astype(np.uint8)
        q["valid"][0] = 0                                        # the first observer is always skipped
        q["valid"][n - 1] = 1
        pts.append(q)
        z = ref.synth_point(rng, n)
        z["valid"] = np.zeros(n, np.uint8)                       # all observers bad
        pts.append(z)
        pts.append(ref.synth_point(rng, 0))                      # no observations at all
    b = ref.pack(pts)
    got, want = run(ops, b), ref.restate(b)
    assert ref.same_bits(got, want)
    assert list(got["updated"]) == [1, 1, 0] * 8
    assert (got["best_obs"][1::3] == -1).all() and (got["best_median"][1::3] == INT_MAX).all()
    assert (got["best_obs"][0::3] > 0).all()                     # an index into the FULL list: never the skipped first observer
    for p in range(0, len(pts), 3):
        assert pts[p]["valid"][got["best_obs"][p]] == 1
    # the normal runs over ALL observers: equal to the same batch without a mask
    nomask = dict(b, desc_valid=None)
    free = run(ops, nomask)
    m = got["updated"] != 0
    for k in ("normal", "max_dist", "min_dist"):
        assert np.array_equal(got[k][m].view(np.uint32), free[k][m].view(np.uint32))
    assert np.isfinite(got["normal"][1::3]).all() and (got["max_dist"][1::3] > 0).all()


@pytest.mark.gpu
def test_observation_order_is_kept(ops):
    fwd, rev = run(ops, window()), run(ops, ref.reverse(window()))
    assert ref.same_bits(fwd, window_expected(False))
    assert ref.same_bits(rev, window_expected(True))
    p = int(order_sensitive_points()[0])
    assert (fwd["normal"][p].view(np.uint32) != rev["normal"][p].view(np.uint32)).any()


@pytest.mark.gpu
def test_scale_inputs_every_level(ops):
    """ref_scale = 1.2^level for every level 0..7, top_scale = 1.2^7 and 1.2^level: max_dist / min_dist bit-equal"""
    rng = np.random.default_rng(9)
    sf = ref.scale_factors()
    pts = []
    for lvl in range(8):
        for top in (7, lvl):
            for _ in range(8):
                q = ref.synth_point(rng, int(rng.integers(1, 9)))
                q["ref_scale"], q["top_scale"] = sf[lvl], sf[top]
                pts.append(q)
    b = ref.pack(pts)
    d = np.linalg.norm(b["cam_center"].astype(np.float64) - np.repeat(b["pos"], np.diff(b["obs_offset"]), axis=0), axis=1)
    assert d.min() >= 0.1 and np.linalg.norm(b["pos"].astype(np.float64) - b["ref_center"], axis=1).min() >= 0.1
    got, want = run(ops, b), ref.restate(b)
    assert np.array_equal(got["max_dist"].view(np.uint32), want["max_dist"].view(np.uint32))
    assert np.array_equal(got["min_dist"].view(np.uint32), want["min_dist"].view(np.uint32))
    assert ref.same_bits(got, want)


@pytest.mark.gpu
def test_determinism_and_handle_reuse(orbx, ops):
    big = ref.concat(ref.synth_batch([1, 64, 65, 257, 0, 300], seed=12), window())
    small = ref.synth_batch([5, 0, 70], seed=13)
    allrows = np.ones(len(big["obs_offset"]) - 1, bool)
    a = run(ops, big)
    b = run(ops, big)
    s = run(ops, small)
    c = run(ops, big)
    assert ref.same_bits(a, b, allrows) and ref.same_bits(a, c, allrows)
    assert ref.same_bits(s, ref.restate(small))
    empty = ref.pack([])
    e = run(ops, empty)
    assert len(e["best_obs"]) == 0
    assert ops.last_timing() == (0.0, 0)
    assert ref.same_bits(run(ops, big), a, allrows)


@pytest.mark.gpu
def test_argument_errors(orbx):
    L = bind(orbx)
    o = orbx.MapPointOps(8, 64)
    b = ref.synth_batch([3, 4, 2], seed=14)
    keep = {k: b[k] for k in ref.KEYS if b[k] is not None}
    alive = []      # the offset arrays the structures below point to

    def batch(M=3, T=9, off=None):
        off = keep["obs_offset"] if off is None else off
        alive.append(off)
        return orbx.MapPointBatch(M, T, off.ctypes.data, keep["desc"].ctypes.data, None, keep["cam_center"].ctypes.data, keep["pos"].ctypes.data,
                                  keep["ref_center"].ctypes.data, keep["ref_scale"].ctypes.data, keep["top_scale"].ctypes.data)
    res = orbx.MapPointResult()      # every output NULL
    cases = [(None, batch()), (o._h, None), (o._h, batch(M=9)), (o._h, batch(T=65)),
             (o._h, batch(off=np.array([1, 3, 7, 9], np.int32))), (o._h, batch(off=np.array([0, 5, 3, 9], np.int32)))]
    for h, bb in cases:
        L.orbx_last_error.restype = ctypes.c_char_p
        rc = L.orbx_mappoint_refresh(h, None if bb is None else ctypes.byref(bb), ctypes.byref(res))
        assert rc == ERR_ARG, rc
        assert len(L.orbx_last_error()) > 0
    assert L.orbx_mappoint_refresh(o._h, ctypes.byref(batch(M=0, T=0)), ctypes.byref(res)) == 0      # M = 0 is OK and launches nothing
    assert o.last_timing()[1] == 0
    assert L.orbx_mappoint_refresh(o._h, ctypes.byref(batch()), ctypes.byref(res)) == 0               # all outputs NULL
    assert ref.same_bits(run(o, b), ref.restate(b))                                                    # and the handle still works
    o.close()


@pytest.mark.gpu
def test_python_surface_equals_the_c_abi(orbx, ops):
    L = bind(orbx)
    b = window()
    M, T = len(b["obs_offset"]) - 1, len(b["desc"])
    valid = (np.arange(T) % 5 != 0).astype(np.uint8)
    py = ops.refresh(b["obs_offset"], b["desc"], b["cam_center"], b["pos"], b["ref_center"], b["ref_scale"], b["top_scale"], desc_valid=valid)
    B = orbx.MapPointBatch(M, T, b["obs_offset"].ctypes.data, b["desc"].ctypes.data, valid.ctypes.data, b["cam_center"].ctypes.data, b["pos"].ctypes.data,
                           b["ref_center"].ctypes.data, b["ref_scale"].ctypes.data, b["top_scale"].ctypes.data)
    raw = dict(best_obs=np.zeros(M, np.int32), best_median=np.zeros(M, np.int32), normal=np.zeros((M, 3), np.float32), max_dist=np.zeros(M, np.float32),
               min_dist=np.zeros(M, np.float32), updated=np.zeros(M, np.uint8))
    R = orbx.MapPointResult(*[raw[k].ctypes.data for k in ("best_obs", "best_median", "normal", "max_dist", "min_dist", "updated")])
    h = ctypes.c_void_p()
    assert L.orbx_mappoint_ops_create(0, M, T, ctypes.byref(h)) == 0      # exactly the batch's size
    assert L.orbx_mappoint_refresh(h, ctypes.byref(B), ctypes.byref(R)) == 0
    L.orbx_mappoint_ops_destroy(h)
    assert ref.same_bits(py, raw, np.ones(M, bool))
    assert ref.same_bits(py, ref.restate(dict(b, desc_valid=valid)))
