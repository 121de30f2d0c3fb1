"""ComputeBoW and SearchByBoW at the shape of the reference's own vocabulary: k = 10, L = 6 - 1,111,111 nodes, 10^6 words, a 35 MB child
descriptor table that does not fit in L2, FeatureVector keys = the (at most) 100 nodes of tree level 2 - and a ragged tree of the same
depth (341,039 nodes, 92 level-2 nodes).  Every other test of the suite stops at L <= 5 and at most 14 synthetic groups.

The inputs (tests/bow_l6.py: _descs_l6) mix leaf descriptors, noise, repeated words, forced ties at every depth and zero-weight words;
their census on 3000 descriptors, from the compiled reference's results:

    tree     filed nodes   words filed > once   unfiled   ties at depth 1 / 2 / 3 / 4 / 5 / 6
    full         100               75             285       51 / 129 / 149 / 215 / 304 / 321
    ragged        92               74             273       45 / 115 / 147 / 189 / 270 / 277
    floors        90               50              20       20 at every depth

The floors are asserted wherever the inputs are used.  All comparisons are exact (integers, bit patterns)."""
import ctypes
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import bow_l6
import oracle_lib
from bow_l6 import LEVELSUP, N_FIXTURE, SIZES, _descs_l6, restated

HAVE_REF = oracle_lib.slam_lib() is not None
NAMES = ("full", "ragged")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- per-module state
@pytest.fixture(scope="module")
def text_files(orbx, tmp_path_factory):
    """the DBoW2 text file of each tree, written once (153 MB / 47 MB)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = tmp_path_factory.mktemp("voc_l6") / ("%s.txt" % name)
            orbx.voc_synth.write_text_fast(bow_l6.tree(name), made[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def ref_vocs(text_files):
    """the compiled reference's ORBVocabulary of each tree, loaded once through its own loadFromTextFile (about 5 s for the full tree)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = oracle_lib.RefVocabulary(text_files(name))
        return made[name]
    return get


@pytest.fixture(scope="module")
def dev_vocs(orbx):
    """the device vocabulary of each tree, created once"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = orbx.Vocabulary(bow_l6.tree(name))
        return made[name]
    yield get
    for V in made.values():
        V.close()


# ---------------------------------------------------------------------------------------------------------------- CPU: the generator
@pytest.mark.parametrize("k,L,seed", [(10, 4, 5), (6, 5, 13)])
def test_fast_writer_is_byte_identical_to_write_text(orbx, tmp_path, k, L, seed):
    vs = orbx.voc_synth
    voc = vs.make_vocabulary(k, L, seed)
    vs.write_text(voc, tmp_path / "a.txt")
    vs.write_text_fast(voc, tmp_path / "b.txt", chunk=1000)        # (several chunks, a short last one)
    vs.write_text_fast(voc, tmp_path / "c.txt")
    a = (tmp_path / "a.txt").read_bytes()
    assert a == (tmp_path / "b.txt").read_bytes() == (tmp_path / "c.txt").read_bytes() and len(a) > 100000


def test_make_vocabulary_stream_is_unchanged(orbx):
    """make_vocabulary's trees are what tools/bench_configs.py, tools/latency_*.py and every other test's seeds stand on"""
    vs = orbx.voc_synth
    assert vs.tree_digest(vs.make_vocabulary(10, 4, 5)) == "eb8dfaada89033f4e2f09ae854bc085402951070bbb9725818294974b3199fce"
    assert vs.tree_digest(vs.make_vocabulary(10, 4, 7, ragged=False)) == "e3fd52c0b2db71b4a71585f762a81ced9de2d06314c4465b54e6b3aa511f7579"


@pytest.mark.parametrize("name", NAMES)
def test_fast_vocabulary_invariants(orbx, name):
    voc = bow_l6.tree(name)
    k, L, n = voc["k"], voc["L"], voc["num_nodes"]
    par, leaf, wt = voc["parent"], voc["is_leaf"], voc["weight"]
    assert par.dtype == np.int32 and leaf.dtype == np.uint8 and voc["desc"].dtype == np.uint8 and wt.dtype == np.float64
    assert len(par) == len(leaf) == len(voc["desc"]) == len(wt) == n and voc["desc"].shape[1] == 32
    assert (par[1:] < np.arange(1, n)).all() and (par[1:] >= 0).all() and (np.diff(par[1:]) >= 0).all()      # BFS: parents first, children contiguous
    depth = bow_l6._depths(voc)
    assert (depth[1:] == depth[par[1:]] + 1).all()
    assert ((leaf == 1) == (depth == L)).all()                                                                # all leaves at depth L, nothing else is a leaf
    nchild = np.bincount(par[1:], minlength=n)
    inner = leaf == 0
    if name == "full":
        assert (nchild[inner] == k).all() and n == 1111111 and int(leaf.sum()) == 1000000
    else:
        assert nchild[inner].min() == k // 2 and nchild[inner].max() == k and len(np.unique(nchild[inner])) == k - k // 2 + 1
        assert int(leaf.sum()) == int(nchild[depth == L - 1].sum())
    assert (nchild[~inner] == 0).all()
    assert (wt[inner] == 0).all() and (wt[~inner] >= 0).all() and (wt[~inner] < 9.0).all() and (wt[~inner][wt[~inner] > 0] >= 0.5).all()
    zero = float((wt[~inner] == 0).mean())
    assert 0.045 < zero < 0.055, zero                      # 5 % of 10^5..10^6 draws: far inside
    # children = the parent with max(4, 128 >> depth) flips drawn with replacement: never more bits apart, and mostly close to it
    dist = bow_l6._POP[voc["desc"][1:] ^ voc["desc"][par[1:]]].sum(1, dtype=np.int32)
    for d in range(2, L + 1):
        at = dist[depth[1:] == d]
        assert at.max() <= max(4, 128 >> d) and at.mean() > 0.7 * max(4, 128 >> d), d
    assert (np.count_nonzero(depth == 2) >= bow_l6.MIN_NODES)
    assert orbx.voc_synth.tree_digest(voc) == orbx.voc_synth.tree_digest(orbx.voc_synth.make_vocabulary_fast(**bow_l6.TREES[name]))   # deterministic


def test_fast_and_slow_generators_make_the_same_family(orbx):
    """small trees of both generators: same layout, same invariants (not the same stream)"""
    for ragged in (True, False):
        a, b = orbx.voc_synth.make_vocabulary(6, 3, 3, ragged=ragged), orbx.voc_synth.make_vocabulary_fast(6, 3, 3, ragged=ragged)
        assert set(a) == set(b)
        for key in ("parent", "is_leaf", "desc", "weight"):
            assert a[key].dtype == b[key].dtype and a[key].ndim == b[key].ndim
        for v in (a, b):
            nchild = np.bincount(v["parent"][1:], minlength=v["num_nodes"])[v["is_leaf"] == 0]
            assert nchild.min() >= (3 if ragged else 6) and nchild.max() <= 6


@pytest.mark.parametrize("name", NAMES)
def test_descs_l6_classes_and_census(oracle, name):
    """the input generator itself: the census floors hold on the restatement's results at n = 3000, every size has the right shape, and the
    small sizes are still mixed"""
    voc = bow_l6.tree(name)
    d = _descs_l6(voc, N_FIXTURE, bow_l6.DESC_SEED[name])
    r = restated(oracle, voc, d, 4)
    c = bow_l6.census(voc, d, r["word"], r["weight"], r["fv_node"])
    bow_l6.assert_census(c)
    assert (_descs_l6(voc, N_FIXTURE, bow_l6.DESC_SEED[name]) == d).all()
    for n in SIZES:
        dn = _descs_l6(voc, n, 500 + n)
        assert dn.shape == (n, 32) and dn.dtype == np.uint8
    # the numpy descent of the census is the restatement's descent
    path, _ = bow_l6.descend(voc, d)
    wid = np.cumsum(voc["is_leaf"]) - 1
    assert (wid[path[:, -1]] == r["word"]).all() and (path[:, 1] == r["node"]).all()


# ---------------------------------------------------------------------------------------------------------------- CPU: restatement, reference, fixture
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_fixture_l6(oracle, name):
    """runs wherever the fixture is: no compiled reference needed"""
    voc = bow_l6.tree(name)
    g, d = bow_l6.fixture(name)
    r = restated(oracle, voc, d, 4)
    c = bow_l6.census(voc, d, g["word"], g["weight"], g["fv_node"])
    bow_l6.assert_census(c)
    assert (c == g["census"]).all()
    for key in ("word", "node", "fv_node", "bow_ids"):
        assert (r[key] == g[key]).all(), key
    assert (_bits(r["weight"]) == _bits(g["weight"])).all() and (_bits(r["bow_vals"]) == _bits(g["bow_vals"])).all()
    for lu in (2, 0, 6):
        q = restated(oracle, voc, d, lu)
        assert (q["word"] == g["word_%d" % lu]).all() and (q["fv_node"] == g["fv_node_%d" % lu]).all(), lu
    assert (g["fv_node_6"][g["weight"] > 0] == 0).all()


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/liborbslam.so not built (needs the reference sources); test_restatement_equals_fixture_l6 is the twin")
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference_vocabulary_l6(oracle, ref_vocs, name):
    voc = bow_l6.tree(name)
    ref = ref_vocs(name)
    assert ref.size() == int(voc["is_leaf"].sum())           # the text round-trips through the reference's loader
    g, d = bow_l6.fixture(name)
    for lu in LEVELSUP:
        want = ref.transform(d, lu)
        r = restated(oracle, voc, d, lu)
        assert (r["word"] == want["word"]).all() and (_bits(r["weight"]) == _bits(want["weight"])).all(), lu
        if voc["L"] - lu >= 1:
            assert (r["node"] == want["node"]).all(), lu
        assert (r["fv_node"] == want["fv_node"]).all() and (want["fv_node"] == -1).sum() >= bow_l6.MIN_UNFILED, lu
        assert (r["bow_ids"] == want["bow_ids"]).all() and (_bits(r["bow_vals"]) == _bits(want["bow_vals"])).all(), lu
        if lu == 4:                                          # ... and the fixture is what the reference gives today
            for key in ("word", "node", "fv_node", "bow_ids"):
                assert (want[key] == g[key]).all(), key
            assert (_bits(want["weight"]) == _bits(g["weight"])).all() and (_bits(want["bow_vals"]) == _bits(g["bow_vals"])).all()


# ---------------------------------------------------------------------------------------------------------------- GPU: the transform, all four forms
def _check_sorted(got, want, tag):
    w, nd, wt, bw, bn = got
    assert (w == want["word"]).all() and (nd == want["fv_node"]).all() and (_bits(wt) == _bits(want["weight"])).all(), tag
    filed = np.flatnonzero(want["fv_node"] >= 0)
    assert len(bw) == len(filed) == len(bn), tag
    assert (bw == filed[np.lexsort((filed, want["word"][filed]))]).all(), tag
    assert (bn == filed[np.lexsort((filed, want["fv_node"][filed]))]).all(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("levelsup", LEVELSUP)
@pytest.mark.parametrize("name", NAMES)
def test_hip_host_forms_equal_restatement_and_fixture_l6(orbx, oracle, dev_vocs, name, levelsup):
    """Vocabulary.transform and transform_sorted at every size of the list; at n = 3000 on the fixture's descriptors, against the compiled
    reference's recorded results too."""
    voc, V = bow_l6.tree(name), dev_vocs(name)
    assert V.size() == int(voc["is_leaf"].sum())
    g, dfix = bow_l6.fixture(name)
    bow_l6.assert_census(bow_l6.census(voc, dfix, g["word"], g["weight"], g["fv_node"]))
    for n in SIZES:
        d = dfix if n == N_FIXTURE else _descs_l6(voc, n, 500 + n)
        want = restated(oracle, voc, d, levelsup)
        t0 = time.perf_counter()
        word, node, weight = V.transform(d, levelsup)
        dt = time.perf_counter() - t0
        print("transform %s n=%d levelsup=%d: %.0f us" % (name, n, levelsup, dt * 1e6))
        assert (word == want["word"]).all() and (node == want["fv_node"]).all() and (_bits(weight) == _bits(want["weight"])).all(), n
        _check_sorted(V.transform_sorted(d, levelsup), want, n)
        if n == N_FIXTURE:
            sfx = "" if levelsup == 4 else "_%d" % levelsup
            assert (word == g["word" + sfx]).all() and (node == g["fv_node" + sfx]).all()
            if levelsup == 4:
                assert (_bits(weight) == _bits(g["weight"])).all()
                ids, vals = oracle_lib.bow_vector(word, weight)
                assert (ids == g["bow_ids"]).all() and (_bits(vals) == _bits(g["bow_vals"])).all()


@pytest.fixture(scope="module")
def four_frames(orbx):
    W, H, B = 640, 480, 4
    ext = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    frames = orbx.synth_sequence(77, B, W, H)
    yield ext, frames, B
    ext.close()


@pytest.fixture(scope="module")
def single_ext(orbx):
    """(the job form takes the features a single-frame handle left on the device)"""
    ext = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    yield ext
    ext.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_job_and_device_forms_equal_restatement_l6(orbx, oracle, dev_vocs, four_frames, single_ext, name):
    """job_transform on the descriptors a single-frame extraction left on the device, and transform_device + download on a batch of 4 frames"""
    voc, V = bow_l6.tree(name), dev_vocs(name)
    ext, frames, B = four_frames
    for levelsup in LEVELSUP:
        for im in frames[:2]:
            kps, desc = single_ext(im)
            got = V.job_transform(single_ext, levelsup)
            assert len(got[0]) == len(desc) > 500
            _check_sorted(got, restated(oracle, voc, desc, levelsup), ("job", levelsup))
        ext.run_device(*ext.upload(frames))
        V.transform_device(ext, levelsup)
        kps, desc, counts = ext.download(B)
        word, node, weight = V.download(ext, B)
        for f in range(B):
            n = int(counts[f])
            want = restated(oracle, voc, desc[f, :n], levelsup)
            assert (word[f, :n] == want["word"]).all() and (node[f, :n] == want["fv_node"]).all() and (_bits(weight[f, :n]) == _bits(want["weight"])).all(), (levelsup, f)


# ---------------------------------------------------------------------------------------------------------------- GPU: SearchByBoW on about 100 real groups
def _populated(g):
    return len(np.unique(g[g >= 0]))


def _device_chain(orbx, oracle, voc, V, ext, frames, B, modes=(0, 1)):
    """groups_device() afresh -> search_by_bow_device -> download, everything against the restatement on the downloaded descriptors;
    returns the number of matches"""
    groups, cap = V.groups_device()
    fs = orbx.ORBmatcher.features_of(ext, B)
    assert cap == fs.capacity
    fs.groups = groups.value
    kps, desc, counts = ext.download(B)
    word, node, weight = V.download(ext, B)
    want = [restated(oracle, voc, desc[f, :int(counts[f])], 4) for f in range(B)]
    for f in range(B):
        n = int(counts[f])
        assert (word[f, :n] == want[f]["word"]).all() and (node[f, :n] == want[f]["fv_node"]).all() and (_bits(weight[f, :n]) == _bits(want[f]["weight"])).all(), f
        assert _populated(want[f]["fv_node"]) >= bow_l6.MIN_NODES, f
    mt = orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=B - 1)
    pa, pb = np.arange(B - 1, dtype=np.int32), np.arange(1, B, dtype=np.int32)
    total = 0
    for mode in modes:
        mt.search_by_bow_device(fs, fs, pa, pb, mode=mode, after=ext)
        m, dd, nm = mt.download(B - 1)
        for p in range(B - 1):
            a, b = int(pa[p]), int(pb[p])
            na, nb = int(counts[a]), int(counts[b])
            wn, wm = oracle_lib.search_by_bow(oracle, mode, kps[a, :na], desc[a, :na], kps[b, :nb], desc[b, :nb], 0.7, True, want[a]["fv_node"], want[b]["fv_node"])
            assert nm[p] == wn and (m[p, :len(wm)] == wm).all(), (mode, p)
            total += int(wn)
    mt.close()
    return total


@pytest.mark.gpu
def test_transform_feeds_search_by_bow_on_device_l6(orbx, oracle, dev_vocs, four_frames):
    """extract -> transform_device (level-2 node ids of the 1.1 M node tree stay on the device) -> SearchByBoW gated by them, both modes"""
    voc, V = bow_l6.tree("full"), dev_vocs("full")
    ext, frames, B = four_frames
    ext.run_device(*ext.upload(frames))
    V.transform_device(ext, 4)
    assert _device_chain(orbx, oracle, voc, V, ext, frames, B) > 50


_SPLIT_CHILD = r'''
import importlib, json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
orbx = importlib.import_module("self_commit_orb-slam2_amd")
import bow_l6, oracle_lib
orc = oracle_lib.Oracle()
voc = bow_l6.tree("full")
mt = orbx.ORBmatcher(0.7, True, max_features=3400)
out = []
for n in (40, 1000, 2500):
    kA, dA, kB, dB, gA, gB, vA, vB = bow_l6.pair_l6(orbx, orc, voc, n, 900 + n)
    for mode in (0, 1):
        nm, m = mt.SearchByBoW(kA, dA, kB, dB, gA, gB, vA, vB, mode=mode)
        out.append([int(nm), [int(x) for x in m]])
print(json.dumps(out))
'''


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["1", "0"])
def test_single_pair_search_by_bow_on_real_groups_l6(orbx, oracle, split):
    """mt.SearchByBoW(kA, dA, kB, dB, gA, gB, vA, vB) with the level-2 nodes of the L = 6 transform as groups (-1 = not filed) and MapPoint
    masks, n in {40, 1000, 2500}, both modes, vs the restatement.  ORBX_BOW_SINGLE_SPLIT is read once per process: each value in a child."""
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, ORBX_BOW_SINGLE_SPLIT=split)
    r = subprocess.run([sys.executable, "-c", _SPLIT_CHILD % (str(root), str(root / "tests"))], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    voc = bow_l6.tree("full")
    total, i = 0, 0
    for n in (40, 1000, 2500):
        kA, dA, kB, dB, gA, gB, vA, vB = bow_l6.pair_l6(orbx, oracle, voc, n, 900 + n)
        if n >= 1000:
            assert _populated(gA) >= bow_l6.MIN_NODES and _populated(gB) >= bow_l6.MIN_NODES and (gA < 0).sum() >= bow_l6.MIN_UNFILED
        for mode in (0, 1):
            wn, wm = oracle_lib.search_by_bow(oracle, mode, kA, dA, kB, dB, 0.7, True, gA, gB, vA, vB)
            assert got[i][0] == wn and (np.array(got[i][1], np.int32) == wm).all(), (n, mode)
            total += wn
            i += 1
    assert total > 50


@pytest.fixture(scope="module")
def shim_vocs(text_files):
    """the L = 6 text vocabulary loaded by both libraries, once"""
    hip, ref = oracle_lib.slam_hip_lib(), oracle_lib.slam_lib()
    if hip is None or ref is None:
        pytest.skip("oracle/_ref/liborbslam{,_hip}.so not built (needs the reference sources)")
    path = text_files("full")
    return ref, hip, oracle_lib.RefVocabulary(path, lib=ref), oracle_lib.RefVocabulary(path, lib=hip)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_compute_bow_and_search_by_bow_dropin_l6(orbx, oracle, shim_vocs, which):
    """Frame::ComputeBoW / KeyFrame::ComputeBoW on the L = 6 vocabulary in the drop-in library vs the all-reference library, then
    ORBmatcher::SearchByBoW of both libraries on real objects whose FeatureVectors hold the node ids that came out."""
    orbx.load_library()
    ref, hip, vr, vh = shim_vocs
    hip.orbx_shim_compute_bow_calls.restype = ctypes.c_ulong
    hip.orbx_shim_search_by_bow_calls.restype = ctypes.c_ulong
    voc = bow_l6.tree("full")
    before = hip.orbx_shim_compute_bow_calls()
    before_s = hip.orbx_shim_search_by_bow_calls()
    total, nsearch = 0, 0
    for n, seed in ((2000, 1), (1000, 2)):
        kA, dA, kB, dB, _, _, vA, vB = bow_l6.pair_l6(orbx, oracle, voc, n, 700 + seed)
        fv = []
        for d in (dA, dB):
            want, got = vr.compute_bow(d, which), vh.compute_bow(d, which)
            assert (got["fv_node"] == want["fv_node"]).all() and (want["fv_node"] >= 0).sum() > n // 2
            assert (got["bow_ids"] == want["bow_ids"]).all() and (_bits(got["bow_vals"]) == _bits(want["bow_vals"])).all()
            assert (want["fv_node"] == restated(oracle, voc, d, 4)["fv_node"]).all()
            assert _populated(want["fv_node"]) >= bow_l6.MIN_NODES and (want["fv_node"] < 0).sum() >= bow_l6.MIN_UNFILED
            fv.append(got["fv_node"])
        for mode in (0, 1):
            args = (mode, kA, dA, kB, dB, 0.7, True, fv[0], fv[1], vA, vB if mode == 1 else None)
            want_n, want = oracle_lib.ref_search_by_bow(*args, lib=ref)
            got_n, got = oracle_lib.ref_search_by_bow(*args, lib=hip)
            nsearch += 1
            assert got_n == want_n and (got == want).all(), (n, mode)
            total += want_n
    assert total > 50
    assert hip.orbx_shim_compute_bow_calls() - before == 4
    assert hip.orbx_shim_search_by_bow_calls() - before_s == nsearch, "the HIP bodies were not the ones linked"


# ---------------------------------------------------------------------------------------------------------------- GPU: host and device forms on one Vocabulary
@pytest.mark.gpu
@pytest.mark.parametrize("ndevice", [2, 1, 3])
def test_host_and_device_forms_interleaved_on_one_vocabulary(orbx, oracle, four_frames, ndevice):
    """transform_device x ndevice, then the host forms on MORE features than the device batch holds and on fewer, then the device batch's
    results again: download and search_by_bow_device (through a groups_device() pointer fetched AFTER the host calls - no pointer handed
    out before them is touched) must still be the device batch's.

    With the sorted host form keeping its word / node copy for k_bow_ranks in the device form's result buffer 0 - as it did before it got
    buffers of its own - this fails for ndevice = 2 (established by reading the code, not by running it): after an even number of device
    calls buffer 0 IS the last batch's, the larger host call frees and reallocates it, and download returns the host call's words and nodes
    next to the batch's weights."""
    voc = bow_l6.tree("full")
    V = orbx.Vocabulary(voc)              # its own: the double-buffer parity is what is under test
    ext, frames, B = four_frames
    try:
        for _ in range(ndevice):
            ext.run_device(*ext.upload(frames))
            V.transform_device(ext, 4)
        _, cap = V.groups_device()
        for n in (B * cap + 777, 500):
            d = _descs_l6(voc, n, 300 + n % 97)
            want = restated(oracle, voc, d, 4)
            _check_sorted(V.transform_sorted(d, 4), want, ("host sorted", n))
            word, node, weight = V.transform(d, 4)
            assert (word == want["word"]).all() and (node == want["fv_node"]).all() and (_bits(weight) == _bits(want["weight"])).all(), n
        assert _device_chain(orbx, oracle, voc, V, ext, frames, B, modes=(0,)) > 25
    finally:
        V.close()
