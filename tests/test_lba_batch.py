"""Batched LocalBundleAdjustment (orbx_lba_solve_batch / BatchOptimizer): one handle solves many independent windows, every
kernel launch covers all of them, and every window's result is bit-identical to the single-window call (orbx_lba_solve) on it."""
import ctypes

import numpy as np
import pytest

import oracle_lib
from test_lba import _compare, _with_unused_vertices

ERR_ARG, ERR_CAPACITY, ERR_NODEVICE = -1, -3, -4


def _gpu():
    import torch
    return torch.cuda.is_available()


# ---- without a device ----

def test_batch_create_rejects_bad_arguments(orbx):
    L = orbx.load_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbx_lba_batch_create.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.orbx_lba_batch_create.restype = ci
    h = vp()
    assert L.orbx_lba_batch_create(0, 0, 50, 5000, 60000, ctypes.byref(h)) == ERR_ARG           # max_windows < 1
    assert L.orbx_lba_batch_create(0, -3, 50, 5000, 60000, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_lba_batch_create(0, 4, 342, 5000, 60000, ctypes.byref(h)) in (ERR_ARG, ERR_CAPACITY)   # 6 K > 2048
    assert L.orbx_lba_batch_create(0, 4, 0, 5000, 60000, ctypes.byref(h)) == ERR_ARG
    assert L.orbx_lba_batch_create(0, 4, 50, 5000, 60000, None) == ERR_ARG                       # NULL out
    assert len(L.orbx_last_error()) > 0


def test_batch_create_without_a_device(orbx):
    """Valid arguments: ORBX_ERR_NODEVICE without a device (no CPU fallback); a handle with one."""
    L = orbx.load_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbx_lba_batch_create.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.orbx_lba_batch_destroy.argtypes = [vp]
    L.orbx_lba_batch_destroy.restype = None
    h = vp()
    rc = L.orbx_lba_batch_create(0, 2, 341, 100, 1000, ctypes.byref(h))
    if _gpu():
        assert rc == 0 and h.value
        L.orbx_lba_batch_destroy(h)
    else:
        assert rc == ERR_NODEVICE and not h.value
        with pytest.raises(orbx.OrbxError) as e:
            orbx.BatchOptimizer(4, 50, 5000, 60000)
        assert e.value.code == ERR_NODEVICE


def test_batch_null_handle_is_an_error_not_a_crash(orbx):
    L = orbx.load_library()
    none = ctypes.c_void_p(None)
    for fn, args in ((L.orbx_lba_solve_batch, [none, 1, none, none, none]), (L.orbx_lba_batch_last_timing, [none, none, none])):
        fn.restype = ctypes.c_int
        fn.argtypes = None
        assert fn(*args) < 0, fn.__name__
        assert len(L.orbx_last_error()) > 0
    L.orbx_lba_batch_destroy.argtypes = [ctypes.c_void_p]
    L.orbx_lba_batch_destroy.restype = None
    L.orbx_lba_batch_destroy(none)


# ---- on the GPU: bit-equality with the single-window call ----

def _bits_equal(a, b):
    return ((np.asarray(a["stats"], np.float64).view(np.uint64) == np.asarray(b["stats"], np.float64).view(np.uint64)).all()
            and (a["poses"].view(np.uint32) == b["poses"].view(np.uint32)).all()
            and (a["points"].view(np.uint32) == b["points"].view(np.uint32)).all()
            and (np.asarray(a["chi2"], np.float64).view(np.uint64) == np.asarray(b["chi2"], np.float64).view(np.uint64)).all()
            and (a["outlier"] == b["outlier"]).all())


def _assert_bits(got, want, tag):
    assert _bits_equal(got, want), (tag, got["stats"], want["stats"])


def _singles(orbx, windows, stop_flags=None):
    opt = orbx.Optimizer(max_keyframes=max(w["K"] for w in windows), max_points=max(w["P"] for w in windows), max_edges=max(w["E"] for w in windows))
    out = [opt.LocalBundleAdjustment(w, None if stop_flags is None else stop_flags[i]) for i, w in enumerate(windows)]
    opt.close()
    return out


def _batch_opt(orbx, windows, n=None):
    return orbx.BatchOptimizer(n or len(windows), max(w["K"] for w in windows), max(w["P"] for w in windows), max(w["E"] for w in windows))


def _ragged(orbx):
    mk = orbx.lba_synth.make_window
    ws = [mk(K=6, P=120, seed=21, n_fixed=6, stereo_frac=0.5),                       # every keyframe fixed: no reduced system
          mk(K=12, P=400, seed=31, n_fixed=2),                                        # n = 60: k_chol_solve
          mk(K=30, P=1500, seed=32),                                                  # n = 120: backsub_reg<4>
          mk(K=45, P=2500, seed=33),                                                  # n = 210: backsub_reg<7>
          mk(K=50, P=3000, seed=34),                                                  # n = 240: backsub_reg<8>
          mk(K=60, P=3000, seed=35),                                                  # n = 300: backsub_reg<10>
          mk(K=80, P=3000, seed=36),                                                  # n = 420: the LDS back-substitution
          mk(K=20, P=1500, seed=7, stereo_frac=0.9),                                  # stereo-heavy
          mk(K=12, P=400, seed=1, n_fixed=2, pose_noise=(np.deg2rad(6.0), 0.25), point_noise=0.25, stereo_frac=0.3),   # rejected trials
          mk(K=12, P=400, seed=6, n_fixed=2, pose_noise=(np.deg2rad(12.0), 0.5), point_noise=0.4, stereo_frac=0.3),
          _with_unused_vertices(mk(K=7, P=150, seed=22, n_fixed=1, stereo_frac=0.3)),  # vertices without edges
          mk(K=3, P=12, seed=23, n_fixed=1, max_obs=3)]                               # E < 64
    assert ws[-1]["E"] < 64
    return ws


@pytest.mark.gpu
def test_batch_of_eight_equals_single(orbx, oracle):
    ws = [orbx.lba_synth.make_window(K=50, P=5000, seed=1000 + i) for i in range(8)]
    want = _singles(orbx, ws)
    b = _batch_opt(orbx, ws)
    got = b.LocalBundleAdjustment(ws)
    for i in range(8):
        _assert_bits(got[i], want[i], i)
    _compare(got[3], oracle_lib.local_bundle_adjustment(oracle, ws[3]), ws[3])
    ms, fl = b.last_timing()
    assert ms > 0 and fl > 0
    b.close()


@pytest.mark.gpu
def test_ragged_batch_covers_every_route(orbx):
    ws = _ragged(orbx)
    want = _singles(orbx, ws)
    b = _batch_opt(orbx, ws)
    got = b.LocalBundleAdjustment(ws)
    for i in range(len(ws)):
        _assert_bits(got[i], want[i], i)
    b.close()


@pytest.mark.gpu
def test_batch_same_bits_in_any_order_and_every_run(orbx):
    ws = [orbx.lba_synth.make_window(K=50, P=5000, seed=2000 + i) for i in range(3)]
    ws.append(orbx.lba_synth.make_window(K=12, P=400, seed=6, n_fixed=2, pose_noise=(np.deg2rad(12.0), 0.5), point_noise=0.4, stereo_frac=0.3))
    want = _singles(orbx, ws)
    b = _batch_opt(orbx, ws)
    one = b.LocalBundleAdjustment(ws[:1])
    _assert_bits(one[0], want[0], "batch of one")
    rev = b.LocalBundleAdjustment(ws[::-1])
    for i in range(len(ws)):
        _assert_bits(rev[len(ws) - 1 - i], want[i], ("reversed", i))
    for run in range(20):
        got = b.LocalBundleAdjustment(ws)
        for i in range(len(ws)):
            _assert_bits(got[i], want[i], (run, i))
    b.close()


@pytest.mark.gpu
def test_batch_stop_flag_affects_only_its_window(orbx):
    ws = [orbx.lba_synth.make_window(K=30, P=2000, seed=3000 + i) for i in range(6)]
    want = _singles(orbx, ws)
    raised = np.ones(1, np.uint8)
    want3 = _singles(orbx, ws[3:4], [raised])[0]
    assert (want3["stats"] == 0).all()
    flags = [np.zeros(1, np.uint8) for _ in ws]
    flags[3][0] = 1
    b = _batch_opt(orbx, ws)
    got = b.LocalBundleAdjustment(ws, stop_flags=flags)
    _assert_bits(got[3], want3, "stopped")
    for i in range(len(ws)):
        if i != 3:
            _assert_bits(got[i], want[i], i)
    b.close()


@pytest.mark.gpu
def test_batch_bad_window_fails_the_whole_call(orbx):
    ws = [orbx.lba_synth.make_window(K=20, P=1000, seed=4000 + i) for i in range(4)]
    want = _singles(orbx, ws)
    b = _batch_opt(orbx, ws)
    bad = dict(ws[2])
    bad["edge_point"] = ws[2]["edge_point"].copy()
    bad["edge_point"][5] = ws[2]["P"] + 7
    # the result buffers of the C call stay untouched
    L = orbx.load_library()
    n = len(ws)
    keep = []
    probs = (orbx.LbaProblem * n)()
    results = (orbx.LbaResult * n)()
    sentinel = []
    for i, w in enumerate(ws[:2] + [bad] + ws[3:]):
        a = {k: np.ascontiguousarray(w[k]) for k in ("poses", "fixed", "intr", "points", "edge_point", "edge_kf", "edge_obs", "edge_inv_sigma2")}
        keep.append(a)
        probs[i] = orbx.LbaProblem(w["K"], a["poses"].ctypes.data, a["fixed"].ctypes.data, a["intr"].ctypes.data, w["P"], a["points"].ctypes.data, w["E"],
                                   a["edge_point"].ctypes.data, a["edge_kf"].ctypes.data, a["edge_obs"].ctypes.data, a["edge_inv_sigma2"].ctypes.data)
        o = dict(poses=np.full((w["K"], 16), 7.0, np.float32), points=np.full((w["P"], 3), 7.0, np.float32), chi2=np.full(w["E"], 7.0), outlier=np.full(w["E"], 7, np.uint8))
        sentinel.append(o)
        results[i] = orbx.LbaResult(o["poses"].ctypes.data, o["points"].ctypes.data, o["chi2"].ctypes.data, o["outlier"].ctypes.data, (ctypes.c_double * 8)(*[7.0] * 8))
    rc = L.orbx_lba_solve_batch(b._h, n, probs, None, results)
    assert rc == ERR_ARG
    assert b"window 2" in L.orbx_last_error()
    for i, o in enumerate(sentinel):
        assert (o["poses"] == 7).all() and (o["points"] == 7).all() and (o["chi2"] == 7).all() and (o["outlier"] == 7).all()
        assert list(results[i].stats) == [7.0] * 8
    with pytest.raises(orbx.OrbxError) as e:
        b.LocalBundleAdjustment(ws[:2] + [bad] + ws[3:])
    assert e.value.code == ERR_ARG
    got = b.LocalBundleAdjustment(ws)      # the handle still solves the next good batch
    for i in range(n):
        _assert_bits(got[i], want[i], i)
    with pytest.raises(orbx.OrbxError) as e:
        b.LocalBundleAdjustment(ws + ws[:1])      # num_windows > max_windows
    assert e.value.code in (ERR_ARG, ERR_CAPACITY)
    b.close()


@pytest.mark.gpu
def test_batch_of_32_interleaved_with_single_calls(orbx):
    ws = [orbx.lba_synth.make_window(K=50, P=5000, seed=5000 + i) for i in range(32)]
    want = _singles(orbx, ws)
    b = _batch_opt(orbx, ws)
    single = orbx.Optimizer(max_keyframes=64, max_points=6000, max_edges=80000)
    got = b.LocalBundleAdjustment(ws)
    for i in range(32):
        _assert_bits(got[i], want[i], i)
    for rnd in range(2):      # batch and single calls on two handles of one device, back to back
        s0 = single.LocalBundleAdjustment(ws[rnd])
        got = b.LocalBundleAdjustment(ws)
        s1 = single.LocalBundleAdjustment(ws[31 - rnd])
        _assert_bits(s0, want[rnd], ("single", rnd))
        _assert_bits(s1, want[31 - rnd], ("single", 31 - rnd))
        for i in range(32):
            _assert_bits(got[i], want[i], (rnd, i))
    single.close()
    b.close()
