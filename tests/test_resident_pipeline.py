"""The in-flight extract + match pipeline, batch by batch, against the CPU oracle (tests/pipeline_ref.py).

bench.py's headline, `--workload sequence` and bench_stereo all issue the same schedule: several extractor / matcher handle pairs take
resident batches in turn - run_device, features_of, search_by_bow_device(..., after=ext) - and nothing is synchronised between the calls.
What keeps that correct is a handful of events:
  producer -> consumer           prep_pairs records evDep (evDep2) on the extractor's stream, the matcher's stream waits for it
  consumer -> producer, results  the extractor's results are double buffered; chain_back hands it an event, run_batch waits for the events of
                                 a buffer in front of the one launch that overwrites it (orbx_launch_orient_describe)
  consumer -> producer, pyramid  single buffered; orbx_compute_stereo_matches_device hands over an event, run_batch waits for it first
  pointers                       features_of returns the CURRENT buffer: it is asked after every run_device
  slots                          every consumer stream of a buffer is waited for, not only the one that chained last
Here every batch of such a run is compared with the oracle (section 2), every guard is put under an overwriter that would win the race
without it (section 3), and the edges of a batch are run inside the pipeline (section 4).  Keypoints are compared as bit patterns;
descriptor bytes, match indices, distances and nmatches must be equal.  Expected values never come from the device.

The scene checks (section 1) run on the CPU: they hold the properties of the inputs that make the device checks mean something."""
import ctypes

import numpy as np
import pytest

import bench
import pipeline_ref as pr
from pipeline_ref import B, FLAT, NBATCH, NS
from test_pyr_fast_plan import plan


def _ref(orbx, oracle, geom):
    return pr.ref_for(orbx, oracle, *pr.GEOMS[geom])


# =====================================================================================
# 1. the scenes, on the oracle alone
# =====================================================================================
@pytest.fixture(scope="module", params=sorted(pr.GEOMS))
def scene(request, orbx, oracle):
    ref = _ref(orbx, oracle, request.param)
    run = pr.run_keys(request.param)
    ref.prefetch([k for keys in run for k in keys])
    return ref, run


def test_scenes_textured_frames_have_keypoints_and_the_flat_frame_none(scene):
    ref, run = scene
    flats = [keys.index(FLAT) if FLAT in keys else None for keys in run]
    assert len(run) == NBATCH and all(len(keys) == B for keys in run)
    assert len({f for f in flats if f is not None}) >= 3 and None in flats, "the flat frame takes different positions, and some batches have none"
    for keys in run:
        for k in keys:
            assert (ref.frame(k) == pr.FLAT_LEVEL).all() == (k == FLAT)
            assert (ref.count(k) == 0) == (k == FLAT), k


def test_scenes_consecutive_textured_frames_match_and_flat_pairs_do_not(scene):
    ref, run = scene
    pa, pb = pr.ring_pairs()
    for keys in run:
        for a, b in zip(pa, pb):
            ka, kb = keys[a], keys[b]
            n, m, d = ref.match(ka, kb)
            assert len(m) == ref.count(kb) and n == int((m >= 0).sum()) and ((d < 256) == (m >= 0)).all()
            if FLAT in (ka, kb):
                assert n == 0 and (m == -1).all()
            elif abs(ka[2] - kb[2]) == 1:      # consecutive views of one scene
                assert n > 20, (ka, kb, n)


def test_scenes_batches_of_a_handle_pair_differ_at_every_frame_position(scene):
    """Handle pair k sees the batches k, k + NS, k + 2 NS; a result buffer holds batch j - 2 NS (the same buffer) or j - NS (the other one) when
    batch j is written.  A call that read a stale buffer must not find equal data there: at every frame position the count differs and so do the
    descriptor bytes (over the rows both frames have), and at every pair position the match rows differ."""
    ref, run = scene
    pa, pb = pr.ring_pairs()
    for j in range(NS, NBATCH):
        for jj in (j - NS, j - 2 * NS):
            if jj < 0:
                continue
            for f in range(B):
                (_, d1, _), (_, d0, _) = ref.features(run[j][f]), ref.features(run[jj][f])
                assert len(d1) != len(d0), (j, jj, f, len(d1))
                n = min(len(d1), len(d0))
                assert n == 0 or (d1[:n] != d0[:n]).any(axis=1).mean() > 0.9, (j, jj, f)
            new, old = [[ref.match(run[x][a], run[x][b]) for a, b in zip(pa, pb)] for x in (j, jj)]
            assert all(len(m1[1]) != len(m0[1]) for m1, m0 in zip(new, old)), (j, jj)      # (a row has one entry per feature of the Frame)
            assert [m[0] for m in new] != [m[0] for m in old], (j, jj)


# =====================================================================================
# device helpers
# =====================================================================================
def _joint(orbx, ext):
    fn = orbx.load_library().orbx_debug_last_batch_pyr_fast
    fn.argtypes = [ctypes.c_void_p]
    return bool(fn(ext._h))


def _resident(orbx, ext, frames, nb):
    """bench.py's input layout (row stride, frame pitch) for batches of nb frames: [(tensor kept alive, run_device arguments)]."""
    import torch
    return bench.resident_batches(orbx, torch, torch.device("cuda:0"), ext, frames, nb)


def _extractor(orbx, ref, max_batch):
    return orbx.ORBextractor(ref.nf, 1.2, 8, 20, 7, max_width=ref.W, max_height=ref.H, max_batch=max_batch)


def _issue(orbx, ext, mt, batch, pa, pb, nframes=B):
    """One batch exactly as bench.py::step issues it."""
    ext.run_device(*batch[1])
    fs = orbx.ORBmatcher.features_of(ext, nframes)      # results are double buffered: ask every time
    mt.search_by_bow_device(fs, fs, pa, pb, mode=0, after=ext)


def _close(*handles):
    for h in handles:
        h.close()


# =====================================================================================
# 2. the benchmark's call order, every prefix
# =====================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["ragged", "joint"])
def test_benchmark_call_order_every_prefix_equals_the_oracle(orbx, oracle, geom):
    """NS = 3 handle pairs, B = 5 frames per batch, batches j = 0 .. T - 1 issued as bench.py::step does (handle pair j % NS, pairs (i, (i + 1) % B),
    mode 0, after = the extractor, features_of asked each time, nothing synchronising in between) for every prefix length T = 1 .. 3 NS on ONE
    persistent set of handles.  After each prefix every handle pair used so far holds the oracle's results of its last batch: every batch
    position is the checked one at some T, both result buffers of every handle are checked and so is their reuse.  `--workload sequence`
    is the same schedule with more batches.  "joint" is the benchmark's geometry (the joint pyramid + detector launches, read from the tap)."""
    import torch
    ref = _ref(orbx, oracle, geom)
    run = pr.run_keys(geom)
    ref.prefetch([k for keys in run for k in keys])
    exts = [_extractor(orbx, ref, 8) for _ in range(NS)]
    mts = [orbx.ORBmatcher(0.7, True, max_features=exts[0].capacity, max_pairs=B) for _ in range(NS)]
    batches = _resident(orbx, exts[0], [f for keys in run for f in ref.frames(keys)], B)
    assert len(batches) == NBATCH
    pa, pb = pr.ring_pairs()
    for T in range(1, NBATCH + 1):
        for j in range(T):
            _issue(orbx, exts[j % NS], mts[j % NS], batches[j], pa, pb)
        for e, m in zip(exts[:min(T, NS)], mts):
            e.sync()
            m.sync()
        torch.cuda.synchronize()
        for k in range(min(T, NS)):
            j = max(x for x in range(T) if x % NS == k)      # the pair's last batch
            what = "%s T=%d handle pair %d batch %d:" % (geom, T, k, j)
            assert exts[k].status() == 0, what
            ref.check_features(run[j], *exts[k].download(B), what=what)
            ref.check_matches(run[j], pa, pb, *mts[k].download(B), what=what)
            assert _joint(orbx, exts[k]) == plan(ref.W, ref.H, 1.2, 8)["joint"], what
            if geom == "joint":
                assert _joint(orbx, exts[k]), "the benchmark's geometry must run the joint pyramid + detector launches"
    _close(*exts, *mts)


# =====================================================================================
# 3. the overwrite guards, one test per hazard
#
# The call at risk is the last one on its matcher, so its results survive; the calls that would overwrite its inputs are issued behind it,
# before anything synchronises.  The matcher call is sized to outlast them: durations of each call ALONE on an MI355X, the library's own
# timers (ORBextractor.last_timing after 30 warm-up calls / ORBmatcher.last_timing), every docstring carries its own.  Timed on the host,
# the extractor's stream of every schedule below drains 2.6 - 3.0 ms after the first call was issued, within 0.03 ms of the matcher's
# (its own calls alone: 0.3 - 0.5 ms): it is the wait that holds it.  The tests assert results, not times.
# =====================================================================================
HAZ_SEARCH = (640, 480, 2000)       # geometry of the SearchByBoW hazards, 4 frames per batch
HAZ_STEREO = (640, 480, 1000)       # smallest geometry of test_matcher.py::test_compute_stereo_matches_hip_bit_exact, 2 stereo pairs
HEAVY_REPEATS = 85                  # x 12 ordered pairs = 1020 SearchByBoW pairs in one call
STEREO_REPEATS = 1024               # x 4 (left, right) combinations = 4096 ComputeStereoMatches pairs in one call
BF = 40.0


def _ordered_pairs(n, repeats):
    o = [(a, b) for a in range(n) for b in range(n) if a != b]
    return np.array([p[0] for p in o] * repeats, np.int32), np.array([p[1] for p in o] * repeats, np.int32)


def _search_setup(orbx, oracle):
    ref = pr.ref_for(orbx, oracle, *HAZ_SEARCH)
    keys = [[("view", 4300 + b, v) for v in range(4)] for b in range(3)]
    ref.prefetch([k for ks in keys for k in ks])
    ext = _extractor(orbx, ref, 4)
    batches = _resident(orbx, ext, [f for ks in keys for f in ref.frames(ks)], 4)
    return ref, keys, ext, batches


@pytest.mark.gpu
@pytest.mark.parametrize("both_slots", [False, True], ids=["one_consumer", "second_matcher_behind_b1"])
def test_result_buffer_is_not_overwritten_under_its_matcher(orbx, oracle, both_slots):
    """Hazard a.  ext.run(b0); mt.search(b0, 1020 pairs, after=ext); ext.run(b1); ext.run(b2) - b2 is written into b0's buffer.
    Measured alone: the matcher call 2.6 ms (2.58 - 2.72), one extractor call of this geometry (640x480, 2000 features, 4 frames) 0.157 ms:
    the matcher outlasts the two extractor calls behind it 8.3 times (asked: 5).  Without the wait in front of orbx_launch_orient_describe b2's
    descriptors land under the matcher's reads.  Variant: a second matcher is chained behind b1, so both buffers' slots are in use."""
    ref, keys, ext, batches = _search_setup(orbx, oracle)
    pa, pb = _ordered_pairs(4, HEAVY_REPEATS)
    la, lb = _ordered_pairs(4, 1)
    mt = orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=len(pa))
    m2 = orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=len(la)) if both_slots else None
    _issue(orbx, ext, mt, batches[0], pa, pb, 4)
    ext.run_device(*batches[1][1])
    if both_slots:
        fs = orbx.ORBmatcher.features_of(ext, 4)
        m2.search_by_bow_device(fs, fs, la, lb, mode=0, after=ext)
    ext.run_device(*batches[2][1])
    ref.check_matches(keys[0], pa, pb, *mt.download(len(pa)), what="b0 under b1, b2:")      # every repeat
    if both_slots:
        ref.check_matches(keys[1], la, lb, *m2.download(len(la)), what="b1 under b2:")
    assert ext.status() == 0
    ref.check_features(keys[2], *ext.download(4), what="b2:")
    _close(ext, mt, *([m2] if m2 else []))


@pytest.mark.gpu
@pytest.mark.parametrize("n_light", [1, 4], ids=["two_matchers", "five_matchers"])
def test_matchers_behind_one_batch_are_all_waited_for(orbx, oracle, n_light):
    """Hazard c, result buffer.  ext.run(b0); M1.search(b0, 1020 pairs, after=ext); M2.search(b0, 12 pairs, after=ext) [.. M5]; ext.run(b1);
    ext.run(b2).  Measured alone: M1's call 2.6 ms, a light call 0.25 ms, an extractor call 0.157 ms: M1 outlasts the two extractor calls 8.3 times
    and the light calls by 2.3 ms.  The light matchers chain last: an extractor that kept one event per buffer waited for the last of them alone
    and wrote b2 under M1's reads.  Five matchers are one more than a buffer's list holds: M1's event, the oldest, is waited for when the fifth
    arrives."""
    ref, keys, ext, batches = _search_setup(orbx, oracle)
    pa, pb = _ordered_pairs(4, HEAVY_REPEATS)
    la, lb = _ordered_pairs(4, 1)
    m1 = orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=len(pa))
    light = [orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=len(la)) for _ in range(n_light)]
    ext.run_device(*batches[0][1])
    fs = orbx.ORBmatcher.features_of(ext, 4)
    m1.search_by_bow_device(fs, fs, pa, pb, mode=0, after=ext)
    for m in light:
        m.search_by_bow_device(fs, fs, la, lb, mode=0, after=ext)
    ext.run_device(*batches[1][1])
    ext.run_device(*batches[2][1])
    ref.check_matches(keys[0], pa, pb, *m1.download(len(pa)), what="M1 (heavy, chained first):")
    for i, m in enumerate(light):
        ref.check_matches(keys[0], la, lb, *m.download(len(la)), what="M%d (light):" % (i + 2))
    assert ext.status() == 0
    ref.check_features(keys[2], *ext.download(4), what="b2:")
    _close(ext, m1, *light)


def _stereo_keys(seeds):
    return [("eye", s, 0) for s in seeds], [("eye", s, 1) for s in seeds]


STEREO_SEEDS = [(31, 32), (47, 48), (51, 52)]      # batch 0 (the checked one) and the overwriters
COMBOS = [(0, 0), (1, 1), (0, 1), (1, 0)]          # (left, right) of a call: the two stereo pairs and the two crossed ones


def _stereo_pairs(repeats):
    return np.array([c[0] for c in COMBOS] * repeats, np.int32), np.array([c[1] for c in COMBOS] * repeats, np.int32)


def _check_stereo(ref, kl, kr, fl, fr, mt, what):
    n = len(fl)
    u, z = mt.download_stereo(n)
    bi, bd, nm = mt.download(n)
    ref.check_stereo([kl[i] for i in fl], [kr[i] for i in fr], BF, u, z, bi, bd, nm, what=what)      # every repeat
    assert int(nm[0]) > 50, "the synthetic stereo pair must match"


@pytest.mark.gpu
@pytest.mark.parametrize("two_consumers", [False, True], ids=["one_consumer", "two_matchers"])
def test_pyramid_of_one_handle_is_not_overwritten_under_stereo_matching(orbx, oracle, two_consumers):
    """Hazards b (one handle) and c (pyramid slot).  ext.run(L+R batch 0); mt.compute_stereo_matches_device(ext, ext, 4096 pairs);
    [M2.compute_stereo_matches_device(ext, ext, 4 pairs);] ext.run(batch 1); ext.run(batch 2).  The pyramid is single buffered: batch 1's
    first launch overwrites what the SAD search reads.  Measured alone: the 4096-pair call 2.21 ms (2.21 - 2.28), the 4-pair call 0.04 ms,
    one extractor call (640x480, 1000 features, 4 frames) 0.145 ms: the matcher outlasts the two extractor calls 7.6 times (asked: 5)."""
    ref = pr.ref_for(orbx, oracle, *HAZ_STEREO)
    keys = [sum(_stereo_keys(s), []) for s in STEREO_SEEDS]      # a batch = left 0, left 1, right 0, right 1
    ref.prefetch(keys[0] + keys[2])
    ext = _extractor(orbx, ref, 4)
    batches = _resident(orbx, ext, [f for ks in keys for f in ref.frames(ks)], 4)
    fl, fr = _stereo_pairs(STEREO_REPEATS)
    ll, lr = _stereo_pairs(1)
    mt = orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=len(fl))
    m2 = orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=len(ll)) if two_consumers else None
    ext.run_device(*batches[0][1])
    mt.compute_stereo_matches_device(ext, ext, fl, fr + 2, BF, 0.0)
    if two_consumers:
        m2.compute_stereo_matches_device(ext, ext, ll, lr + 2, BF, 0.0)
    ext.run_device(*batches[1][1])
    ext.run_device(*batches[2][1])
    _check_stereo(ref, keys[0][:2], keys[0][2:], fl, fr, mt, "batch 0 under batches 1, 2:")
    if two_consumers:
        _check_stereo(ref, keys[0][:2], keys[0][2:], ll, lr, m2, "batch 0, second matcher:")
    assert ext.status() == 0
    ref.check_features(keys[2], *ext.download(4), what="batch 2:")
    _close(ext, mt, *([m2] if m2 else []))


@pytest.mark.gpu
def test_pyramids_of_two_handles_are_not_overwritten_under_stereo_matching(orbx, oracle):
    """Hazard b, two handles.  eL.run(left 0); eR.run(right 0); mt.compute_stereo_matches_device(eL, eR, 4096 pairs); eL.run(left 1);
    eR.run(right 1).  Measured alone: the matcher call 2.21 ms (2.21 - 2.22), the two extractor calls behind it (640x480, 1000 features,
    2 frames each) 0.142 + 0.140 ms: 7.8 times (asked: 5)."""
    ref = pr.ref_for(orbx, oracle, *HAZ_STEREO)
    kl, kr = zip(*[_stereo_keys(s) for s in STEREO_SEEDS[:2]])
    ref.prefetch(kl[0] + kr[0] + kl[1] + kr[1])
    eL, eR = _extractor(orbx, ref, 2), _extractor(orbx, ref, 2)
    bl = _resident(orbx, eL, [f for ks in kl for f in ref.frames(ks)], 2)
    br = _resident(orbx, eR, [f for ks in kr for f in ref.frames(ks)], 2)
    fl, fr = _stereo_pairs(STEREO_REPEATS)
    mt = orbx.ORBmatcher(0.7, True, max_features=eL.capacity, max_pairs=len(fl))
    eL.run_device(*bl[0][1])
    eR.run_device(*br[0][1])
    mt.compute_stereo_matches_device(eL, eR, fl, fr, BF, 0.0)
    eL.run_device(*bl[1][1])
    eR.run_device(*br[1][1])
    _check_stereo(ref, kl[0], kr[0], fl, fr, mt, "pair batch 0 under batch 1:")
    assert eL.status() == 0 and eR.status() == 0
    ref.check_features(kl[1], *eL.download(2), what="left 1:")
    ref.check_features(kr[1], *eR.download(2), what="right 1:")
    _close(eL, eR, mt)


# =====================================================================================
# 4. batch edges inside the pipeline (the small geometry)
# =====================================================================================
@pytest.mark.gpu
def test_flat_frames_inside_the_pipeline_match_nothing(orbx, oracle):
    """Pairs (textured, flat), (flat, flat) and (flat, textured) of a batch that follows two textured batches on the same handles (both result
    buffers hold textured frames at the flat positions): nmatches 0 and -1 for every feature of the Frame; the neighbouring pairs equal the oracle."""
    ref = _ref(orbx, oracle, "ragged")
    run = pr.run_keys("ragged")
    edge = [("view", 4200, 0), FLAT, FLAT, ("view", 4200, 1), ("view", 4200, 2)]
    seq = [run[1], run[5], edge]
    ref.prefetch([k for ks in seq for k in ks])
    ext = _extractor(orbx, ref, 8)
    mt = orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=B)
    batches = _resident(orbx, ext, [f for ks in seq for f in ref.frames(ks)], B)
    pa, pb = pr.ring_pairs()
    for b in batches:
        _issue(orbx, ext, mt, b, pa, pb)
    m, d, nm = mt.download(B)
    kps, desc, counts = ext.download(B)
    assert ext.status() == 0
    ref.check_features(edge, kps, desc, counts, what="edge batch:")
    assert list(counts[[1, 2]]) == [0, 0] and counts[[0, 3, 4]].min() > 0
    for p in (0, 1, 2):      # (textured, flat), (flat, flat), (flat, textured)
        assert nm[p] == 0 and (m[p, :int(counts[pb[p]])] == -1).all(), p
    assert nm[3] > 20 and nm[4] > 0
    ref.check_matches(edge, pa, pb, m, d, nm, what="edge batch:")
    _close(ext, mt)


def _shrunk(orbx, oracle):
    """A handle pair after two batches of 5 (one in each result buffer) and then a batch of 3 of the same geometry."""
    ref = _ref(orbx, oracle, "ragged")
    run = pr.run_keys("ragged")
    three = run[6][:3]
    ref.prefetch(run[1] + run[5] + three)
    ext = _extractor(orbx, ref, 8)
    mt = orbx.ORBmatcher(0.7, True, max_features=ext.capacity, max_pairs=B)
    five = _resident(orbx, ext, ref.frames(run[1] + run[5]), B)
    small = _resident(orbx, ext, ref.frames(three), 3)
    pa, pb = pr.ring_pairs()
    for b in five:
        _issue(orbx, ext, mt, b, pa, pb)
    return ref, three, ext, mt, small, (five, run)


@pytest.mark.gpu
def test_shrinking_batch_does_not_read_the_tails_of_the_result_buffers(orbx, oracle):
    ref, three, ext, mt, small, keep = _shrunk(orbx, oracle)
    p3 = pr.ring_pairs(3)
    _issue(orbx, ext, mt, small[0], *p3, nframes=3)
    ref.check_matches(three, *p3, *mt.download(3), what="batch of 3 behind batches of 5:")
    assert ext.status() == 0
    ref.check_features(three, *ext.download(3), what="batch of 3:")
    _close(ext, mt)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [3, 4])
def test_pair_past_the_batch_is_refused_and_the_next_call_is_correct(orbx, oracle, bad):
    """features_of(ext, 3) after a batch of 3: a pair that names frame 3 or 4 - frames the buffers still hold from the batches of 5 - is refused
    with ORBX_ERR_ARG before anything is enqueued, and the next valid call on the same handles is the oracle's."""
    ref, three, ext, mt, small, keep = _shrunk(orbx, oracle)
    ext.run_device(*small[0][1])
    fs = orbx.ORBmatcher.features_of(ext, 3)
    for pa, pb in (([0, bad], [1, 0]), ([0, 1], [1, bad])):
        with pytest.raises(orbx.OrbxError) as e:
            mt.search_by_bow_device(fs, fs, pa, pb, mode=0, after=ext)
        assert e.value.code == -1, "ORBX_ERR_ARG"
    p3 = pr.ring_pairs(3)
    mt.search_by_bow_device(fs, fs, *p3, mode=0, after=ext)
    ref.check_matches(three, *p3, *mt.download(3), what="valid call behind the refused ones:")
    assert ext.status() == 0
    ref.check_features(three, *ext.download(3), what="batch of 3:")
    _close(ext, mt)
