"""The keyframe database on the device (csrc/orbx_kfdb.hip, orbx_kfdb_*, KeyFrameDatabase) against tests/kfdb_ref.py, a literal restatement of the reference's
inverted-file walk.  CPU tests: the restatement itself (the score against dense vectors, the order of the walk against the (first shared word, add sequence) key
that the device relies on, the vacuity guard of the scenes), the ABI without a device, the shim.  GPU tests: every result field equals the restatement, integers
and ids equal and floats bit-equal, with no tolerance and no excluded case."""
import ctypes
import functools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import kfdb_ref as kr
import kfdb_scenes as ks
from test_initializer import REF, ROOT

ERR_ARG, ERR_CAPACITY, ERR_NODEVICE, ERR_STATE = -1, -3, -4, -5
NAMES = list(ks.SCENES)
INT_FIELDS = ("n_sharing", "max_common_words", "min_common_words")
LIST_INT_FIELDS = ("scored_id", "scored_words", "kept", "best_id", "candidates")
FLOAT_FIELDS = ("min_score", "best_acc_score")
LIST_FLOAT_FIELDS = ("connected_score", "scored_score", "acc_score")


def _gpu():
    import torch
    return torch.cuda.is_available()


@functools.lru_cache(maxsize=None)
def _orbx():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1)).view(np.uint32)


def _same(got, want, where):
    """every field of a device result against the restatement's"""
    for k in INT_FIELDS:
        assert int(got[k]) == int(want[k]), (where, k, got[k], want[k])
    for k in LIST_INT_FIELDS:
        assert [int(x) for x in got[k]] == [int(x) for x in want[k]], (where, k)
    for k in FLOAT_FIELDS + LIST_FLOAT_FIELDS:
        g, w = _bits(got[k]), _bits(want[k])
        assert len(g) == len(w) and (g == w).all(), (where, k, np.asarray(got[k]), np.asarray(want[k]))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_restated_score_against_dense_vectors():
    rng = np.random.default_rng(0)
    for n_words, la, lb in ((50, 20, 30), (1000, 65, 64), (1000, 1, 300), (200, 0, 10), (100000, 1500, 1400)):
        for _ in range(5):
            wa, wb = np.sort(rng.choice(n_words, la, replace=False)), np.sort(rng.choice(n_words, lb, replace=False))
            if la and lb:
                wb[: min(la, lb) // 2] = wa[: min(la, lb) // 2]      # make them share words
                wb = np.unique(wb)
            va, vb = rng.random(len(wa)) + 0.01, rng.random(len(wb)) + 0.01
            va, vb = va / max(va.sum(), 1e-300), vb / vb.sum()
            da, db = np.zeros(n_words), np.zeros(n_words)
            da[wa], db[wb] = va, vb
            want = 1.0 - 0.5 * np.abs(da - db).sum() if la else 0.0      # (an empty vector has no L1 norm of 1: the sum over shared words is 0)
            got = kr.l1_score(kr.as_bow(wa, va), kr.as_bow(wb, vb))
            assert abs(got - want) <= 1e-12, (n_words, la, lb, got, want)


def _first_shared(qw, kw):
    c = np.intersect1d(qw, kw)
    return int(c[0]) if len(c) else None


@pytest.mark.parametrize("name", NAMES)
def test_walk_order_equals_first_word_then_add_sequence(name):
    """the order of lKFsSharingWords produced by the literal walk == a sort by (first shared word, add sequence), after erasures and re-adds too"""
    out, _, state, bows = ks.reference(name)
    calls = [op[1] for op in ks.ops(name) if op[0] == "query"]
    checked = 0
    for qs, rs, (seq, _) in zip(calls, out, state):
        for q, r in zip(qs, rs):
            con = set(int(i) for i in q.get("connected", ())) if q["mode"] == kr.LOOP else set()
            keyed = []
            for i, sq in seq.items():
                if i in con:
                    continue
                c = np.intersect1d(q["words"], bows[i])
                if len(c):
                    keyed.append((int(c[0]), sq, i, len(c)))
            keyed.sort()
            assert [k[2] for k in keyed] == r["sharing_id"] or (r["early"] == "sharing" and not keyed)
            if r["early"] != "sharing":
                assert [k[3] for k in keyed] == r["sharing_words"]
                checked += len(keyed)
    assert checked > 100


@functools.lru_cache(maxsize=None)
def _guard(names=tuple(NAMES), seeds=None):
    """which of the cases the GPU comparison must contain do the scenes contain (on the restatement alone)"""
    found = dict(loop3=0, foreign_best=0, shared_best=0, below_min_adds=0, same_first_word=0, truncation=0, stale_reloc=0, early_loop_sharing=0, early_loop_score=0,
                 early_reloc_sharing=0)
    for name in names:
        out, db, state, bows = ks.reference(name) if seeds is None else ks.replay_ref(name, dict(seeds)[name])
        calls = [op[1] for op in (ks.ops(name) if seeds is None else ks.ops(name, dict(seeds)[name])) if op[0] == "query"]
        found["stale_reloc"] += db.stale_reads
        for qs, rs, (seq, cov) in zip(calls, out, state):
            for q, r in zip(qs, rs):
                loop = q["mode"] == kr.LOOP
                if r["early"] == "sharing":
                    found["early_loop_sharing" if loop else "early_reloc_sharing"] += 1
                    continue
                if r["early"] == "score":
                    found["early_loop_score"] += 1
                    continue
                if loop and len(r["candidates"]) >= 3:
                    found["loop3"] += 1
                own = [r["scored_id"][k] for k in r["kept"]]
                found["foreign_best"] += sum(1 for o, b in zip(own, r["best_id"]) if o != b)
                retain = np.float32(0.75) * r["best_acc_score"]
                passing = [b for a, b in zip(r["acc_score"], r["best_id"]) if a > retain]
                if len(passing) != len(set(passing)):
                    assert len(r["candidates"]) == len(set(passing))
                    found["shared_best"] += 1
                if loop:
                    low = set(i for i, s in zip(r["scored_id"], r["scored_score"]) if s < r["min_score"])
                    found["below_min_adds"] += sum(1 for o in own if low & set(i for i in cov[o] if i in seq))
                firsts = [_first_shared(q["words"], bows[i]) for i in r["scored_id"]]
                found["same_first_word"] += sum(1 for a, b in zip(firsts, firsts[1:]) if a == b)
                if r["max_common_words"] % 5 and r["min_common_words"] in r["sharing_words"]:
                    found["truncation"] += 1
    return found


def test_vacuity_guard():
    """the scenes used on the GPU contain every case that makes the comparison mean something (seeds recorded in kfdb_scenes.SCENES)"""
    found = _guard()
    assert all(v > 0 for v in found.values()), found


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a device, the shim
# ---------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("orbx_kfdb_create", "orbx_kfdb_destroy", "orbx_kfdb_add", "orbx_kfdb_erase", "orbx_kfdb_clear", "orbx_kfdb_set_covisibles", "orbx_kfdb_size",
           "orbx_kfdb_query", "orbx_kfdb_last_timing", "orbx_kfdb_reloc_score")


def _bind(L):
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.orbx_kfdb_create.argtypes = [ci, ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.orbx_kfdb_destroy.argtypes = [vp]
    L.orbx_kfdb_destroy.restype = None
    L.orbx_kfdb_add.argtypes = [vp, i64, vp, vp, ci]
    L.orbx_kfdb_erase.argtypes = [vp, i64]
    L.orbx_kfdb_clear.argtypes = [vp]
    L.orbx_kfdb_set_covisibles.argtypes = [vp, i64, vp, ci]
    L.orbx_kfdb_size.argtypes = [vp, vp, vp, vp]
    L.orbx_kfdb_reloc_score.argtypes = [vp, i64, vp]
    L.orbx_kfdb_query.argtypes = [vp, vp, ci, vp]
    L.orbx_kfdb_last_timing.argtypes = [vp, vp, vp]
    L.orbx_last_error.restype = ctypes.c_char_p


def test_exports_and_create_without_a_device(orbx):
    L = orbx.load_library()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
    assert all(hasattr(orbx.KeyFrameDatabase, k) for k in ("add", "erase", "clear", "set_covisibles", "__len__", "DetectLoopCandidates", "DetectRelocalizationCandidates",
                                                           "query", "last_timing"))
    assert "orbx_kfdb_query" in (ROOT / "__graft_entry__.py").read_text()
    _bind(L)
    h = ctypes.c_void_p()
    good = [1000, 16, 1024, 4, 128]
    for i, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 8193)):      # the argument checks come before the device
        a = list(good)
        a[i] = bad
        assert L.orbx_kfdb_create(0, *a, ctypes.byref(h)) == ERR_ARG, (i, bad)
    assert L.orbx_kfdb_create(0, *good, None) == ERR_ARG
    rc = L.orbx_kfdb_create(0, *good, ctypes.byref(h))
    if _gpu():
        assert rc == 0 and h.value
        L.orbx_kfdb_destroy(h)
    else:
        assert rc == ERR_NODEVICE and not h.value
        assert len(L.orbx_last_error()) > 0
        with pytest.raises(orbx.OrbxError) as e:
            orbx.KeyFrameDatabase(1000, 16, 1024)
        assert e.value.code == ERR_NODEVICE


def test_null_handle_is_an_argument_error(orbx):
    L = orbx.load_library()
    _bind(L)
    w, v = np.zeros(1, np.int32), np.ones(1)
    assert L.orbx_kfdb_add(None, 1, w.ctypes.data, v.ctypes.data, 1) == ERR_ARG
    assert L.orbx_kfdb_erase(None, 1) == ERR_ARG
    assert L.orbx_kfdb_clear(None) == ERR_ARG
    assert L.orbx_kfdb_set_covisibles(None, 1, None, 0) == ERR_ARG
    assert L.orbx_kfdb_size(None, None, None, None) == ERR_ARG
    assert L.orbx_kfdb_query(None, None, 1, None) == ERR_ARG
    assert L.orbx_kfdb_last_timing(None, None, None) == ERR_ARG
    assert L.orbx_kfdb_reloc_score(None, 1, None) == ERR_ARG
    L.orbx_kfdb_destroy(None)
    with pytest.raises(ValueError):
        orbx._kfdb_bow(([1, 2], [0.5]))
    w2, v2 = orbx._kfdb_bow({7: 0.25, 3: 0.75})
    assert list(w2) == [3, 7] and list(v2) == [0.75, 0.25]


@pytest.mark.skipif(not os.access(REF / "include" / "KeyFrameDatabase.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_body_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-include", str(shim / "ORBextractor.h"), "-I" + str(ROOT / "include"),
               "-fsyntax-only", str(shim / "KeyFrameDatabase_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "KeyFrameDatabase_hip.cc").read_text()
    for piece in ("orbx_kfdb_query(", "orbx_kfdb_add(", "orbx_kfdb_erase(", "orbx_kfdb_set_covisibles(", "GetBestCovisibilityKeyFrames(10)", "GetConnectedKeyFrames()", "isBad()",
                  "mnLoopQuery", "mnLoopWords", "mLoopScore", "mnRelocQuery", "mnRelocWords", "mRelocScore", "RefreshCovisibles(", "DetectLoopMinScore(", "shim_error.h"):
        assert piece in text, piece
    head = (shim / "KeyFrameDatabase_hip.h").read_text()
    for piece in ("class KeyFrameDatabase_hip", "DetectLoopCandidates(", "DetectRelocalizationCandidates(", "DetectLoopMinScore(", "RefreshCovisibles("):
        assert piece in head, piece
    assert "KeyFrameDatabase_hip" not in (ROOT / "oracle" / "Makefile").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    assert "UpdateConnections" in integ and "UpdateBestCovisibles" in integ and "as last pushed" in integ


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
def _capacity(name):
    adds = [op for op in ks.ops(name) if op[0] == "add"]
    return len(adds) + 8, sum(len(op[2]) for op in adds) + 64


def _device(name, max_keyframes=None, max_entries=None):
    mk, me = _capacity(name)
    return _orbx().KeyFrameDatabase(ks.SCENES[name]["n_words"], max_keyframes or mk, max_entries or me, max_queries=8, max_query_words=ks.MAX_QUERY_WORDS)


def _replay_device(name, db, calls=None):
    """every query call of the scene on the device against the restatement's, then the reloc_score state"""
    out, ref, _, _ = ks.reference(name)
    k = 0
    for op in ks.ops(name):
        if op[0] == "add":
            db.add(op[1], (op[2], op[3]))
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "cov":
            db.set_covisibles(op[1], op[2])
        elif op[0] == "clear":
            db.clear()
        else:
            got = db.query(op[1])
            assert len(got) == len(out[k])
            for i, (g, w) in enumerate(zip(got, out[k])):
                _same(g, w, (name, k, i))
            if calls is not None:
                calls.append((op[1], got))
            k += 1
    assert k == len(out) and len(db) == len(ref)
    ids = sorted(ref.kfs)
    step = max(1, len(ids) // 400)
    for i in ids[::step]:
        assert _bits(db.reloc_score(i))[0] == _bits(ref.reloc_score(i))[0], (name, i)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w1000", "w1M", "seq"])
def test_scene_equals_the_restatement(name):
    """n_words 1,000 / 1,000,000; BowVector lengths 1, 63, 64, 65, 257, 1,500; databases of 0, 1, 63-65, 300 keyframes; words 0 and n_words - 1; a query sharing no
    word; a query whose every sharer is connected; nq = 1 and 7 (3 in `seq`); `seq`: 200 add / erase / set_covisibles / query steps"""
    db = _device(name)
    _replay_device(name, db)
    ms, launches = db.last_timing()
    assert launches == 5 and ms > 0.0
    db.close()


@pytest.mark.gpu
def test_big_scene_across_a_compaction():
    """5,000 keyframes, every third erased, some added again: the pool is sized so that the re-adds need the compaction"""
    mk, me = _capacity("big")
    adds = [op for op in ks.ops("big") if op[0] == "add"]
    first = sum(len(op[2]) for op in adds[:5000])
    db = _device("big", max_keyframes=5004, max_entries=first + 64)
    seen = []
    orig_add = db.add

    def add(i, bow):
        orig_add(i, bow)
        seen.append(db.size())
    db.add = add
    _replay_device("big", db)
    assert any(b[1] < a[1] for a, b in zip(seen, seen[1:])), "no compaction happened"
    assert db.size()[2] == 0 or db.size()[2] * 2 <= db.size()[1]
    db.close()


@pytest.mark.gpu
def test_loop_queries_of_a_batch_equal_their_single_calls():
    db = _device("w1000")
    calls = []
    _replay_device("w1000", db, calls)
    qs, got = [c for c in calls if len(c[0]) == 7][-1]
    for q, g in zip(qs, got):
        if q["mode"] == kr.LOOP:
            _same(db.query([q])[0], g, "single")
    db.close()


@pytest.mark.gpu
def test_c_abi_equals_the_python_class():
    orbx = _orbx()
    L = orbx.load_library()
    _bind(L)
    out, _, _, _ = ks.reference("w1000")
    h = ctypes.c_void_p()
    mk, me = _capacity("w1000")
    assert L.orbx_kfdb_create(0, 1000, mk, me, 8, ks.MAX_QUERY_WORDS, ctypes.byref(h)) == 0
    py = _device("w1000")
    k = 0
    for op in ks.ops("w1000"):
        if op[0] == "add":
            w, v = np.ascontiguousarray(op[2], np.int32), np.ascontiguousarray(op[3], np.float64)
            assert L.orbx_kfdb_add(h, op[1], w.ctypes.data, v.ctypes.data, len(w)) == 0
            py.add(op[1], (w, v))
        elif op[0] == "cov":
            a = np.ascontiguousarray(op[2], np.int64)
            assert L.orbx_kfdb_set_covisibles(h, op[1], a.ctypes.data, len(a)) == 0
            py.set_covisibles(op[1], op[2])
        elif op[0] == "query":
            want = py.query(op[1])
            if k % 5 == 0 and len(op[1]) == 1:      # the candidates alone, every other pointer NULL
                q = op[1][0]
                w, v = np.ascontiguousarray(q["words"], np.int32), np.ascontiguousarray(q["values"], np.float64)
                con, cnt = np.ascontiguousarray(q.get("connected", ()), np.int64), np.ascontiguousarray(q.get("counts", ()), np.int32)
                Q = orbx.KfdbQuery(q["mode"], w.ctypes.data, v.ctypes.data, len(w), con.ctypes.data, cnt.ctypes.data, len(con), q.get("min_score_in", 1.0), 400)
                cand, n = np.zeros(400, np.int64), np.zeros(1, np.int32)
                R = orbx.KfdbCResult()
                R.candidates, R.n_candidates = cand.ctypes.data, n.ctypes.data
                assert L.orbx_kfdb_query(h, ctypes.byref(Q), 1, ctypes.byref(R)) == 0
                assert list(cand[:n[0]]) == [int(x) for x in want[0]["candidates"]] == [int(x) for x in out[k][0]["candidates"]]
            else:
                L_db = orbx.KeyFrameDatabase.__new__(orbx.KeyFrameDatabase)      # the class's marshalling over the C handle made here
                L_db._L, L_db._h = L, h
                for g, w_ in zip(L_db.query(op[1]), want):
                    _same(g, w_, ("abi", k))
                L_db._h = None
            k += 1
    L.orbx_kfdb_destroy(h)
    py.close()


@pytest.mark.gpu
def test_argument_state_and_capacity_errors_leave_the_database_usable():
    orbx = _orbx()
    sc = kr.Scene(11, 1000, 12, (20, 33), places=2, visit=6)
    db = orbx.KeyFrameDatabase(1000, 8, 200, max_queries=2, max_query_words=40)
    ref = kr.KeyFrameDatabaseRef(1000)

    def code(f, *a, **kw):
        with pytest.raises(orbx.OrbxError) as e:
            f(*a, **kw)
        return e.value.code

    for t in range(6):
        db.add(t, sc.bows[t])
        ref.add(t, *sc.bows[t])
        ids = [u for u in range(6) if u != t][:3] + [99]
        db.set_covisibles(t, ids)
        ref.set_covisibles(t, ids)
    assert code(db.add, 20, ([5, 3], [0.5, 0.5])) == ERR_ARG          # unsorted
    assert code(db.add, 20, ([3, 3], [0.5, 0.5])) == ERR_ARG          # repeated
    assert code(db.add, 20, ([3, 1000], [0.5, 0.5])) == ERR_ARG       # outside 0..n_words-1
    assert code(db.add, 20, ([-1, 3], [0.5, 0.5])) == ERR_ARG
    assert code(db.add, 3, sc.bows[6]) == ERR_STATE                   # present
    assert code(db.set_covisibles, 77, [1]) == ERR_STATE              # absent
    assert code(db.set_covisibles, 1, list(range(11))) == ERR_ARG     # n > 10
    db.erase(77)                                                      # absent: fine, as the reference
    w, v = sc.bows[7]
    q = dict(mode=kr.RELOC, words=w, values=v)
    assert code(db.query, [dict(mode=5, words=w, values=v)]) == ERR_ARG
    assert code(db.query, [dict(mode=kr.RELOC, words=w[::-1].copy(), values=v)]) == ERR_ARG
    assert code(db.query, [q, q, q]) == ERR_CAPACITY                  # more queries than the handle takes
    big = np.arange(41, dtype=np.int32)
    assert code(db.query, [dict(mode=kr.RELOC, words=big, values=np.full(41, 1 / 41))]) == ERR_CAPACITY
    L = orbx.load_library()
    _bind(L)
    assert L.orbx_kfdb_add(db._h, 30, w.ctypes.data, v.ctypes.data, -1) == ERR_ARG
    assert L.orbx_kfdb_query(db._h, None, 1, None) == ERR_ARG
    _same(db.query([q])[0], ref.query(q), "after the argument errors")
    # slots and pool
    small = (np.array([1, 2], np.int32), np.array([0.5, 0.5]))
    db.add(6, small)
    ref.add(6, *small)
    db.add(7, small)
    ref.add(7, *small)
    assert code(db.add, 8, small) == ERR_CAPACITY                     # no slot
    db.erase(6)
    ref.erase(6)
    huge = (np.arange(100, dtype=np.int32), np.full(100, 0.01))
    assert code(db.add, 8, huge) == ERR_CAPACITY                      # no room in the pool, even compacted
    assert len(db) == len(ref) == 7
    _same(db.query([q])[0], ref.query(q), "after the capacity errors")
    # an output list that does not fit: nothing is written, the queries have run
    q2 = dict(mode=kr.RELOC, words=sc.bows[8][0], values=sc.bows[8][1])
    want = ref.query(q2)
    assert len(want["scored_id"]) >= 1
    assert code(db.query, [dict(q2, capacity=0)]) == ERR_CAPACITY
    _same(db.query([q])[0], ref.query(q), "after the output capacity error")
    loop = dict(mode=kr.LOOP, words=w, values=v, connected=[0, 1, 50], counts=[3, 0, 2], min_score_in=0.5)
    _same(db.query([loop])[0], ref.query(loop), "loop")
    db.clear()
    ref.clear()
    assert len(db) == 0
    _same(db.query([loop])[0], ref.query(loop), "cleared")
    assert db.last_timing() == (0.0, 0)
    db.add(1, sc.bows[1])
    ref.add(1, *sc.bows[1])
    _same(db.query([loop])[0], ref.query(loop), "refilled")
    db.close()


@pytest.mark.gpu
def test_convenience_calls_return_the_candidates():
    db = _device("w1000")
    ref = kr.KeyFrameDatabaseRef(1000)
    sc = kr.Scene(4, 1000, 40, (64, 65), places=2, visit=5)
    for t in range(40):
        db.add(t, dict(zip((int(w) for w in sc.bows[t][0]), sc.bows[t][1])))      # a bow as a dict
        ref.add(t, *sc.bows[t])
    w, v = sc.bows[39]
    con = {38: 50, 37: 0, 36: 20}
    want = ref.DetectLoopCandidates(w, v, list(con), list(con.values()), 1.0)
    assert db.DetectLoopCandidates((w, v), con) == want["candidates"]
    _same(db.DetectLoopCandidates((w, v), list(con.items()), full=True), ref.DetectLoopCandidates(w, v, list(con), list(con.values()), 1.0), "full")
    want = ref.DetectRelocalizationCandidates(w, v)
    assert db.DetectRelocalizationCandidates((w, v)) == want["candidates"] and len(want["candidates"]) >= 1
    db.close()


@pytest.mark.gpu
def test_dead_entries_above_half_compact_on_the_next_add():
    """erase clears `alive`; the next add compacts once the dead entries exceed half of those in use, and the survivors keep their add order"""
    orbx = _orbx()
    db = orbx.KeyFrameDatabase(1000, 16, 4096)
    ref = kr.KeyFrameDatabaseRef(1000)
    rng = np.random.default_rng(7)
    bows = []
    for t in range(9):
        w = np.unique(np.concatenate([[5], rng.choice(np.arange(6, 200), 70 + t, replace=False)])).astype(np.int32)      # all share word 5: ordered by seq alone
        v = rng.random(len(w)) + 0.1
        bows.append((w, v / v.sum()))
    for t in range(8):
        db.add(t, bows[t])
        ref.add(t, *bows[t])
        db.set_covisibles(t, [u for u in range(8) if u != t])
        ref.set_covisibles(t, [u for u in range(8) if u != t])
    q = dict(mode=kr.RELOC, words=bows[8][0], values=bows[8][1])
    _same(db.query([q])[0], ref.query(q), "full")
    for t in (0, 2, 3, 5, 6):
        db.erase(t)
        ref.erase(t)
    alive, used, dead = db.size()
    assert alive == 3 and dead * 2 > used and dead == sum(len(bows[t][0]) for t in (0, 2, 3, 5, 6))
    _same(db.query([q])[0], ref.query(q), "erased")      # before the compaction: dead slots in between
    db.add(2, bows[2])                                   # comes back behind the others
    ref.add(2, *bows[2])
    alive, used, dead = db.size()
    assert alive == 4 and dead == 0 and used == sum(len(bows[t][0]) for t in (1, 4, 7, 2))
    r = db.query([q])[0]
    _same(r, ref.query(q), "compacted")
    assert [int(i) for i in r["scored_id"]] == [i for i in (1, 4, 7, 2) if i in set(int(x) for x in r["scored_id"])]
    for t in (1, 4, 7, 2):
        assert _bits(db.reloc_score(t))[0] == _bits(ref.reloc_score(t))[0]
    db.close()
