"""Vocabulary training on the device (orbx_voc_train and friends, Python VocabularyTrainer, shim/ORBVocabulary_hip.cc) against the CPU
restatement tests/voc_train_ref.py.  Nothing here has a tolerance except the weights: within 1 ulp of math.log(ndocs / ni), ni itself exact."""
import ctypes
import functools
import math
import os
import shutil
import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import voc_train_ref as vr
import voc_train_scenes as vs

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
ERR_ARG, ERR_NODEVICE, ERR_STATE = -1, -4, -5
gpu = pytest.mark.gpu
SEED = 1


def images_of(d, counts):
    at = np.concatenate([[0], np.cumsum(counts)])
    return [d[at[i]:at[i + 1]] for i in range(len(counts))]


@functools.lru_cache(maxsize=None)
def small_ref(case):
    d, counts = vs.small(case)
    tr = []
    return d, counts, vr.create(d, counts, case[0], case[1], seed=SEED, trace=tr), tr


@functools.lru_cache(maxsize=None)
def full_ref(name, max_iterations=100, weighting=0, seed=SEED):
    s = vs.FULL[name]
    d, counts = full_scene(name)
    tr = []
    return vr.create(d, counts, s["k"], s["L"], seed=seed, weighting=weighting, max_iterations=max_iterations, trace=tr), tr


@functools.lru_cache(maxsize=None)
def full_scene(name):
    return vs.full(name)


def check_weights(voc, ndocs, weighting=0):
    leaf = voc["is_leaf"] == 1
    assert (voc["weight"][~leaf] == 0).all() and (voc["ni"][~leaf] == 0).all()
    for i in np.nonzero(leaf)[0].tolist():
        w, ni = float(voc["weight"][i]), int(voc["ni"][i])
        if weighting in (vr.TF, vr.BINARY):
            assert w == 1.0
        elif ni == 0:
            assert w == 0.0
        else:
            want = math.log(ndocs / ni)
            assert abs(w - want) <= np.spacing(abs(want)), (i, w, want)


def same_tree(got, want, ndocs, weighting=0):
    assert got["num_nodes"] == want["num_nodes"] and got["num_words"] == want["num_words"]
    for key in ("parent", "is_leaf", "desc", "ni"):
        assert (np.asarray(got[key]) == np.asarray(want[key])).all(), key
    assert list(got["passes_per_level"]) == list(want["passes_per_level"]) and got["unconverged_nodes"] == want["unconverged_nodes"]
    check_weights(got, ndocs, weighting)
    check_weights(want, ndocs, weighting)


def train(orbx, d, counts, k, L, **kw):
    tr = orbx.VocabularyTrainer(k, L, max(1, len(d)), max(1, len(counts)))
    tr.add(images_of(d, counts))
    assert tr.size() == (len(d), len(counts))
    return tr, tr.train(**kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vs.TINY, ids=lambda c: "N%d_k%d_L%d_s%d_d%d" % c)
def test_numpy_restatement_equals_the_literal_translation(case):
    n, k, L, seed, _ = case
    d = vs.tiny(case)
    for cap in (100, 2):
        a = vr.create(d, [n], k, L, seed, max_iterations=cap)
        parent, leaf, desc, passes, unconverged = vr.literal_create(d, k, L, seed, cap)
        assert (a["parent"] == parent).all() and (a["is_leaf"] == leaf).all() and (a["desc"] == desc).all()
        assert a["passes_per_level"] == passes and a["unconverged_nodes"] == unconverged


def test_tiny_inputs_cover_duplicates_early_stops_and_the_cap():
    seen = dict(capped=0, short=0, trivial=0)
    for case in vs.TINY:
        n, k, L, seed, dup = case
        d = vs.tiny(case)
        seen["capped"] += vr.create(d, [n], k, L, seed, max_iterations=2)["unconverged_nodes"] > 0
        seen["trivial"] += n <= k
        if n > k:
            seen["short"] += len(vr.seed_clusters(d, k, seed, 0)) < k
    assert all(v > 0 for v in seen.values()), seen


def test_summed_distance_never_rises_and_every_scene_converges():
    """within every node the summed distance to the assigned centre never rises from one pass to the next (the majority mean minimises it
    bit by bit, an empty cluster changes nothing); every scene used on the device converges below the cap of 100"""
    traces = [small_ref(c)[3] for c in vs.SMALL] + [full_ref(name)[1] for name in vs.FULL]
    vocs = [small_ref(c)[2] for c in vs.SMALL] + [full_ref(name)[0] for name in vs.FULL]
    assert sum(len(t) for t in traces) > 400      # nodes clustered by k-means over all scenes
    for t in traces:
        for node in t:
            assert all(a >= b for a, b in zip(node["costs"], node["costs"][1:])), node
            assert not node["capped"] and node["passes"] < 100
    assert all(v["unconverged_nodes"] == 0 for v in vocs)
    assert sum(node["empties"] for t in traces for node in t) > 0      # the empty-cluster rule is exercised by the scenes


def test_the_capped_scene_is_capped_and_the_full_scenes_are_ragged():
    capped, _ = full_ref("k10_L3_20000", 2)
    assert capped["unconverged_nodes"] > 0 and capped["passes_per_level"] == [2, 2, 2]
    for name, s in vs.FULL.items():
        v = full_ref(name)[0]
        assert ((v["is_leaf"] == 1) & (v["depth"] < s["L"])).sum() > 0      # leaves above depth L
        assert (full_scene(name)[1] == 0).sum() > 0                        # empty images count in NDocs


def test_stage_scenes_hold_what_they_promise():
    d, off, centres, nc, prev, info = vs.lloyd_stage_scene()
    c2, a, changed = vr.stage_lloyd(d, off, centres, nc, prev)
    s = info["empty"]
    lo, hi = off[s], off[s + 1]
    assert (prev[lo:hi] != 2).all() and (a[lo:hi] != 2).all() and (c2[s, 2] == centres[s, 2]).all()      # attracts nothing, keeps its centre
    s = info["tie"]
    assert c2[s, 0, 0] == 0xFF and (c2[s, 0, 1:] == d[off[s], 1:]).all()                                  # the tie sets the bit
    s = info["equi"]
    g = d[off[s] + 2]
    assert vr.distances(c2[s, 1:3], g).tolist() == [1, 1] and a[off[s] + 2] == 1                           # the lowest index of two
    assert changed.any() and not changed.all()
    d, off, slots, info = vs.seed_stage_scene()
    ch = vr.stage_seed(d, off, slots, vs.STAGE_K, vs.STAGE_SEED)
    assert ch[info["equal"]].tolist()[1:] == [-1, -1]                                                     # dist_sum == 0: one centre
    assert vr.draw(vs.STAGE_SEED, int(slots[info["u_one"]]), 1) == (1 << 53) - 1 and vr.draw(vs.STAGE_SEED, int(slots[info["u_tiny"]]), 1) == 0
    for key, last in (("u_one", True), ("u_tiny", False)):
        s = info[key]
        f = d[off[s]:off[s + 1]]
        md = vr.distances(f, f[ch[s, 0]])
        nz = np.nonzero(md)[0]
        assert ch[s, 1] == (nz[-1] if last else nz[0])      # cut_d == dist_sum: the last feature that adds to the sum; cut_d tiny: the first
    sizes = np.diff(off)
    assert {1, 2, vs.STAGE_K, vs.STAGE_K + 1, 5000} <= set(sizes.tolist()) and any(off[s] % 64 == 63 and off[s + 1] % 64 == 1 for s in range(len(sizes)))


def test_duplicate_scene_yields_a_word_nobody_reaches():
    d, counts = vs.duplicate_scene()
    v = vr.create(d, counts, 3, 2, seed=SEED)
    assert v["num_words"] == 3 and v["ni"].tolist() == [0, 2, 0, 0] and v["weight"].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_exports_and_sources(orbx):
    L = orbx.load_library()
    for name in ("orbx_voc_trainer_create", "orbx_voc_trainer_destroy", "orbx_voc_trainer_add", "orbx_voc_trainer_add_extracted", "orbx_voc_trainer_clear",
                 "orbx_voc_trainer_size", "orbx_voc_train", "orbx_voc_trainer_result", "orbx_voc_trainer_vocabulary", "orbx_voc_trainer_last_timing",
                 "orbx_voc_trainer_set_profiling", "orbx_voc_seed_segments", "orbx_voc_lloyd_pass"):
        assert hasattr(L, name), name
    assert "orbx_voc_train.hip" in orbx.build_mod.HIP_SOURCES
    assert (orbx.VOC_MAX_K, orbx.VOC_MAX_L) == (32, 10)
    text = (ROOT / "include" / "orbx.h").read_text()
    assert "#define ORBX_VOC_MAX_K 32" in text and "#define ORBX_VOC_MAX_L 10" in text


def test_bad_arguments_are_refused_before_a_device_is_looked_for(orbx):
    """ORBX_ERR_ARG whether or not there is a device; with good arguments ORBX_ERR_NODEVICE without one (no CPU fallback)"""
    import torch
    L = orbx.load_library()
    h = ctypes.c_void_p()
    L.orbx_voc_trainer_create.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_void_p)]
    for k, lv, nd, ni in ((1, 3, 100, 1), (33, 3, 100, 1), (10, 0, 100, 1), (10, 11, 100, 1), (32, 7, 100, 1), (9, 10, 100, 1), (10, 3, 0, 1), (10, 3, (1 << 26) + 1, 1),
                          (10, 3, 100, 0)):
        assert L.orbx_voc_trainer_create(0, k, lv, nd, ni, ctypes.byref(h)) == ERR_ARG, (k, lv, nd, ni)
        assert len(L.orbx_last_error()) > 0 and not h.value
    assert L.orbx_voc_trainer_create(0, 10, 3, 100, 1, None) == ERR_ARG
    if not torch.cuda.is_available():
        assert L.orbx_voc_trainer_create(0, 10, 6, 1000, 10, ctypes.byref(h)) == ERR_NODEVICE
        assert L.orbx_voc_trainer_create(0, 8, 10, 1000, 10, ctypes.byref(h)) == ERR_NODEVICE      # (1 + 8 + ... + 8^10 < 2^31)
        with pytest.raises(orbx.OrbxError) as e:
            orbx.VocabularyTrainer(10, 6, 1000, 10)
        assert e.value.code == ERR_NODEVICE


def test_null_handles_are_errors_not_crashes(orbx):
    L = orbx.load_library()
    vp = ctypes.c_void_p
    for fn, args in ((L.orbx_voc_trainer_add, [None, None, None, 0]), (L.orbx_voc_trainer_add_extracted, [None, None]), (L.orbx_voc_trainer_clear, [None]),
                     (L.orbx_voc_trainer_size, [None, None, None]), (L.orbx_voc_train, [None, None, None]), (L.orbx_voc_trainer_result, [None] * 6 + [0]),
                     (L.orbx_voc_trainer_vocabulary, [None, None]), (L.orbx_voc_trainer_last_timing, [None] * 5), (L.orbx_voc_trainer_set_profiling, [None, 1]),
                     (L.orbx_voc_seed_segments, [None, None, 0, None, None, 0, 0, None]), (L.orbx_voc_lloyd_pass, [None, None, 0, None, 0] + [None] * 6)):
        fn.restype = ctypes.c_int
        fn.argtypes = None
        assert fn(*[vp(a) if a is None else a for a in args]) == ERR_ARG, fn.__name__
    L.orbx_voc_trainer_destroy.restype = None
    L.orbx_voc_trainer_destroy(vp(None))


def test_host_baseline_equals_the_restatement():
    """tools/voc_train_host_baseline.cc (the one-thread C++ statement the latency tool runs beside the device) gives the restatement's tree"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    case = (3, 2, 257)
    d, counts, want, _ = small_ref(case)
    with tempfile.TemporaryDirectory() as tmp:
        exe, scene, out = Path(tmp) / "baseline", Path(tmp) / "scene.bin", Path(tmp) / "out.bin"
        subprocess.run([cxx, "-O2", "-std=c++11", "-ffp-contract=off", "-o", str(exe), str(ROOT / "tools" / "voc_train_host_baseline.cc")], check=True)
        scene.write_bytes(struct.pack("<8iQ", 0x564f4354, len(d), len(counts), case[0], case[1], 0, 100, 0, SEED) + np.asarray(counts, np.int32).tobytes() + d.tobytes())
        subprocess.run([str(exe), str(scene), str(out)], check=True, capture_output=True)
        raw = out.read_bytes()
    n, words, unconverged = struct.unpack_from("<3i", raw, 0)
    passes = list(struct.unpack_from("<10i", raw, 12))[:case[1]]
    at = 52
    parent = np.frombuffer(raw, np.int32, n, at); at += 4 * n
    leaf = np.frombuffer(raw, np.uint8, n, at); at += n
    desc = np.frombuffer(raw, np.uint8, 32 * n, at).reshape(n, 32); at += 32 * n
    ni = np.frombuffer(raw, np.int32, n, at); at += 4 * n
    weight = np.frombuffer(raw, np.float64, n, at)
    same_tree(dict(num_nodes=n, num_words=words, parent=parent, is_leaf=leaf, desc=desc, ni=ni, weight=weight, passes_per_level=passes, unconverged_nodes=unconverged), want,
              len(counts))


@pytest.mark.skipif(not os.access(REF / "Thirdparty" / "DBoW2" / "DBoW2" / "TemplatedVocabulary.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-I" + str(ROOT / "include"), "-fsyntax-only", str(shim / "ORBVocabulary_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_is_not_linked_into_the_drop_in_library():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text = (shim / "ORBVocabulary_hip.cc").read_text()
    for piece in ("orbx_voc_trainer_create(", "orbx_voc_trainer_add(", "orbx_voc_train(", "orbx_voc_trainer_result(", "createScoringObject()", "m_nodes", "m_words", "word_id",
                  "ORBX_VOC_SEED", "shim_error.h", "orbx_shim::Fail("):
        assert piece in text, piece
    assert "public ORBVocabulary" in (shim / "ORBVocabulary_hip.h").read_text()
    assert "ORBVocabulary_hip" not in (ROOT / "oracle" / "Makefile").read_text()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", vs.SMALL, ids=lambda c: "k%d_L%d_N%d" % c)
def test_small_trees(orbx, case):
    d, counts, want, _ = small_ref(case)
    tr, got = train(orbx, d, counts, case[0], case[1], seed=SEED)
    same_tree(got, want, len(counts))
    tr.close()


@gpu
def test_seeding_at_segment_edges(orbx):
    d, off, slots, info = vs.seed_stage_scene()
    tr = orbx.VocabularyTrainer(vs.STAGE_K, 3, len(d), 1)
    got = tr.seed_segments(d, off, slots, vs.STAGE_SEED)
    want = vr.stage_seed(d, off, slots, vs.STAGE_K, vs.STAGE_SEED)
    assert (got == want).all(), np.nonzero((got != want).any(1))[0]
    assert (tr.seed_segments(d, off, slots, vs.STAGE_SEED + 1) != want).any()
    tr.close()


@gpu
def test_lloyd_pass_at_segment_edges(orbx):
    d, off, centres, nc, prev, info = vs.lloyd_stage_scene()
    tr = orbx.VocabularyTrainer(vs.STAGE_K, 3, len(d), 1)
    for pv in (prev, None):
        c2, a, changed = tr.lloyd_pass(d, off, centres, nc, pv)
        wc, wa, wchanged = vr.stage_lloyd(d, off, centres, nc, pv)
        assert (a == wa).all() and (changed == wchanged).all()
        for s in range(len(nc)):
            assert (c2[s, :nc[s]] == wc[s, :nc[s]]).all(), s
    # a second pass from the first one's results, and the fixed point: a pass on a converged association changes nothing
    c, a = centres, prev
    for _ in range(40):
        c, a2, changed = tr.lloyd_pass(d, off, c, nc, a)
        done = not changed.any()
        assert done == (a2 == a).all()
        a = a2
        if done:
            break
    assert done
    c3, a3, changed = tr.lloyd_pass(d, off, c, nc, a)
    assert (c3 == c).all() and (a3 == a).all() and not changed.any()
    tr.close()


@gpu
@pytest.mark.parametrize("name", sorted(vs.FULL))
def test_full_sized_ragged_trees(orbx, name):
    s = vs.FULL[name]
    d, counts = full_scene(name)
    want, _ = full_ref(name)
    assert ((want["is_leaf"] == 1) & (want["depth"] < s["L"])).sum() > 0
    tr, got = train(orbx, d, counts, s["k"], s["L"], seed=SEED)
    same_tree(got, want, len(counts))
    tr.close()


@gpu
def test_iteration_cap(orbx):
    d, counts = full_scene("k10_L3_20000")
    want, _ = full_ref("k10_L3_20000", 2)
    tr, got = train(orbx, d, counts, 10, 3, seed=SEED, max_iterations=2)
    same_tree(got, want, len(counts))
    assert got["unconverged_nodes"] > 0
    with pytest.raises(orbx.OrbxError) as e:
        tr.train(seed=SEED, max_iterations=1)
    assert e.value.code == ERR_ARG
    tr.close()


@gpu
def test_weightings(orbx):
    case = (3, 2, 257)
    d, counts, want, _ = small_ref(case)
    tr = orbx.VocabularyTrainer(3, 2, len(d), len(counts))
    tr.add(images_of(d, counts))
    for weighting in (vr.TF_IDF, vr.TF, vr.IDF, vr.BINARY):
        got = tr.train(seed=SEED, weighting=weighting)
        same_tree(got, vr.create(d, counts, 3, 2, seed=SEED, weighting=weighting), len(counts), weighting)
    with pytest.raises(orbx.OrbxError) as e:
        tr.train(weighting=4)
    assert e.value.code == ERR_ARG
    tr.close()


@gpu
def test_seeds_and_trainer_state(orbx):
    case = (3, 2, 200)
    d, counts, want, _ = small_ref(case)
    tr = orbx.VocabularyTrainer(3, 2, len(d), len(counts))
    for call, code in ((lambda: tr.train(), ERR_STATE), (lambda: tr.vocabulary(), ERR_STATE)):      # nothing added, nothing trained
        with pytest.raises(orbx.OrbxError) as e:
            call()
        assert e.value.code == code
    tr.add(images_of(d, counts))
    with pytest.raises(orbx.OrbxError) as e:
        tr.add([d[:1]])
    assert e.value.code == -3 and tr.size() == (len(d), len(counts))
    a, b, a2 = tr.train(seed=SEED), tr.train(seed=SEED + 1), tr.train(seed=SEED)
    same_tree(a, want, len(counts))
    same_tree(a2, want, len(counts))
    assert a["num_nodes"] != b["num_nodes"] or (a["desc"] != b["desc"]).any()
    same_tree(b, vr.create(d, counts, 3, 2, seed=SEED + 1), len(counts))
    t = tr.last_timing()
    assert t["total_ms"] > 0 and t["launches"] > 0 and len(t["level_ms"]) == 2
    tr.clear()
    assert tr.size() == (0, 0)
    tr.add(images_of(d[:64], [64]))
    same_tree(tr.train(seed=SEED), vr.create(d[:64], [64], 3, 2, seed=SEED), 1)
    tr.close()


@gpu
def test_duplicates_leave_a_word_with_ni_zero(orbx):
    d, counts = vs.duplicate_scene()
    tr, got = train(orbx, d, counts, 3, 2, seed=SEED)
    same_tree(got, vr.create(d, counts, 3, 2, seed=SEED), len(counts))
    assert got["ni"].tolist() == [0, 2, 0, 0]
    tr.close()


@gpu
def test_round_trip_through_the_vocabulary(orbx, tmp_path):
    name = "k10_L3_20000"
    d, counts = full_scene(name)
    want, _ = full_ref(name)
    tr, got = train(orbx, d, counts, 10, 3, seed=SEED)
    for voc in (tr.vocabulary(), orbx.Vocabulary(got)):
        assert voc.size() == want["num_words"]
        w, _, wt = voc.transform(d, levelsup=1)
        assert (w == want["word_of"]).all()
        leaf_ids = np.nonzero(want["is_leaf"])[0]
        assert (wt == got["weight"][leaf_ids[w]]).all()
        voc.close()
    orbx.voc_synth.write_text(dict(got, desc=got["desc"]), tmp_path / "voc.txt")
    assert (tmp_path / "voc.txt").read_text().splitlines()[0] == "10 3 0 0"
    tr.close()


@gpu
def test_extractor_path(orbx):
    W, H, nf = 320, 240, 300
    ext = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=130)
    frames = [orbx.synth_frame(8100 + i, W, H) for i in range(8)]
    ext.run_device(*ext.upload(frames))
    tr = orbx.VocabularyTrainer(4, 3, 8 * ext.capacity, 16)
    tr.add_extracted(ext)
    _, desc, counts = ext.download(8)
    assert counts.sum() > 500 and tr.size() == (int(counts.sum()), 8)
    a = tr.train(seed=SEED)
    tr2 = orbx.VocabularyTrainer(4, 3, 16 * ext.capacity, 16)
    tr2.add([desc[f, :counts[f]] for f in range(8)])
    b = tr2.train(seed=SEED)
    same_tree(a, b, 8)
    assert a["num_words"] > 8
    # appended behind host images, and a batch that does not fit is reported once and dropped whole
    tr2.add_extracted(ext)
    assert tr2.size() == (2 * int(counts.sum()), 16)
    tr2.add_extracted(ext)
    with pytest.raises(orbx.OrbxError) as e:
        tr2.size()
    assert e.value.code == -3 and tr2.size() == (2 * int(counts.sum()), 16)
    # a chunked host batch leaves only its last chunk on the device: the "last batch" views are state errors, and so is this
    ext.extract_batch([orbx.synth_frame(8000 + (i % 7), W, H) for i in range(130)])
    with pytest.raises(orbx.OrbxError) as e:
        tr.add_extracted(ext)
    assert e.value.code == ERR_STATE
    tr.close(); tr2.close()
