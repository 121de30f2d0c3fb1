"""A SEQUENCE of frames through the tracking front end and the local mapper's optimiser, in the all-reference library and in the drop-in
library side by side (oracle/refslam_wrap.cc: orbslam_sequence).

Single-call drop-in tests build fresh objects for one call; what they cannot see is state that survives from call to call - in the drop-in:
the extractor's double-buffered result arenas and pinned views, the combiner's engines, thread-local matcher handles, the cached device
vocabulary, the optimiser handles.  Here 30 translating views of one plane go through, per frame, the reference's own monocular Frame
constructor -> ComputeBoW -> SearchByBoW(KF, F) -> PoseOptimization -> SearchLocalPoints -> PoseOptimization, every 5th frame a KeyFrame,
new MapPoints and LocalBundleAdjustment (src/Tracking.cc:1180-1230, 1700-1830; src/LocalMapping.cc:123), all on real Frame / KeyFrame /
MapPoint / Map objects.  The drop-in run continues from the reference run's optimiser outputs (they agree to 1e-5, not to the bit), so every
index / bit-pattern result of every step must be IDENTICAL and every optimiser output within 1e-5."""
import ctypes

import numpy as np
import pytest

import oracle_lib

W, H, NF = 640, 480, 1000
FX, FY, CX, CY, PLANE_Z = 500.0, 500.0, 320.0, 240.0, 2.0
MAXKF, MAXPT = 16, 16384


def _run(lib, orbx, tmp_path, frames, kf_every, force=None, l6=False):
    """l6: the k = 10, L = 6 tree of tests/bow_l6.py - with the levelsup = 4 of ComputeBoW the FeatureVector then has the 100 level-2 nodes the
    reference's own vocabulary gives, where the L = 4 tree has ONE (node 0: SearchByBoW is brute force)."""
    path = tmp_path / "voc.txt"
    if l6:
        import bow_l6
        if not path.exists():
            orbx.voc_synth.write_text_fast(bow_l6.tree("full"), path)
    else:
        voc = orbx.voc_synth.make_vocabulary(10, 4, 5)
        orbx.voc_synth.write_text(voc, path)
    V = oracle_lib.RefVocabulary(path, lib)
    n = len(frames)
    arr = (ctypes.c_void_p * n)(*[f.ctypes.data for f in frames])
    rec = np.zeros((n, 64), np.float64)
    kf = np.zeros((64, MAXKF, 17), np.float32)
    pt = np.zeros((64, MAXPT, 4), np.float32)
    ne = ctypes.c_int(0)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    lib.orbslam_sequence.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] + [ctypes.c_float] * 5 + [ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    f_rec, f_kf, f_pt = (force if force else (None, None, None))
    rc = lib.orbslam_sequence(arr, n, W, H, W, NF, V.h, FX, FY, CX, CY, PLANE_Z, kf_every, P(f_rec), P(f_kf), P(f_pt), P(rec), P(kf), P(pt), MAXKF, MAXPT, ctypes.byref(ne))
    assert rc == 0
    return rec, kf[:ne.value], pt[:ne.value], ne.value


def _frames(orbx, n):
    return orbx.synth_sequence(4242, n, W, H, views_per_scene=n, step=(3, 1), low_texture_every=0)


def test_the_reference_sequence_runs_and_is_deterministic(orbx, tmp_path):
    """CPU: the all-reference library alone - the loop tracks (matches, inliers), inserts keyframes, optimises - and two runs agree bit for bit."""
    lib = oracle_lib.slam_lib()
    if lib is None:
        pytest.skip("oracle/_ref/liborbslam.so not built")
    frames = _frames(orbx, 7)
    a = _run(lib, orbx, tmp_path, frames, 3)
    b = _run(lib, orbx, tmp_path, frames, 3)
    rec, kf, pt, ne = a
    assert ne == 2 and rec[0, 4] > 500                                  # initial map from frame 0
    assert (rec[1:, 5] > 100).all() and (rec[1:, 7] > 50).all()       # SearchByBoW matches, PoseOptimization inliers
    assert (rec[1:, 25] > 0).all() and (rec[1:, 29] > 100).all()      # SearchLocalPoints finds more; second optimisation keeps them
    # the camera follows the plane's translation: 3 px per frame at depth 2, fx 500 -> about 0.012 per frame (keyframes and their bundle
    # adjustment re-anchor the map on the way, so not exactly)
    tx = np.abs(rec[1:, 30 + 3])
    assert (np.diff(tx) > 0).all() and 0.5 * 0.012 * len(tx) < tx[-1] < 1.5 * 0.012 * len(tx), tx
    assert (a[0].view(np.uint64) == b[0].view(np.uint64)).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all() and (a[2].view(np.uint32) == b[2].view(np.uint32)).all()


# counts and hashes: keypoints + descriptors, BoW, match lists, outlier flags, frustum views, keyframe events, undistorted keypoints + grid (52), the map as
# SearchLocalPoints sees it - positions, normals, descriptors, distance ranges, observation counts, flags of every point (53)
EXACT = [0, 1, 2, 3, 4, 5, 6, 24, 25, 26, 27, 28, 46, 47, 48, 49, 50, 51, 52, 53]


def _thirty_frames(orbx, tmp_path, l6):
    ref, hip = oracle_lib.slam_lib(), oracle_lib.slam_hip_lib()
    if ref is None or hip is None:
        pytest.skip("oracle/_ref libraries not built")
    frames = _frames(orbx, 30)
    r_rec, r_kf, r_pt, r_ne = _run(ref, orbx, tmp_path, frames, 5, l6=l6)
    force_kf = np.zeros((64, MAXKF, 17), np.float32); force_kf[:r_ne] = r_kf
    force_pt = np.zeros((64, MAXPT, 4), np.float32); force_pt[:r_ne] = r_pt
    h_rec, h_kf, h_pt, h_ne = _run(hip, orbx, tmp_path, frames, 5, force=(r_rec, force_kf, force_pt), l6=l6)
    assert r_ne == h_ne == 5
    # (L = 6: a match needs both features under the same level-2 node, so SearchByBoW finds fewer than the brute-force search of the one-node tree does.
    # The floor there is the reference's own: Tracking::TrackReferenceKeyFrame gives up below 15 matches, src/Tracking.cc:1201)
    min_bow = 14 if l6 else 100
    assert (r_rec[1:, 5] > min_bow).all() and (r_rec[1:, 29] > 100).all(), "the reference loop lost track: the comparison would be empty"
    for i in range(30):
        bad = [c for c in EXACT if r_rec[i, c] != h_rec[i, c]]
        # PoseOptimization's inlier counts (7, 29) and flags (24, 46) are exact unless an edge rides the chi2 threshold within 1e-5 - not on this data
        assert not bad and r_rec[i, 7] == h_rec[i, 7] and r_rec[i, 29] == h_rec[i, 29], ("frame", i, bad, r_rec[i, :8], h_rec[i, :8])
        for lo in (8, 30):                                              # the two optimised poses
            assert np.abs(r_rec[i, lo:lo + 16] - h_rec[i, lo:lo + 16]).max() <= 1e-5, ("pose", i, lo)
    for e in range(r_ne):
        nk, npt = int(r_rec[5 * (e + 1), 48]), int(r_rec[5 * (e + 1), 49])
        assert (r_kf[e, :nk, 0] == h_kf[e, :nk, 0]).all() and (r_pt[e, :npt, 0] == h_pt[e, :npt, 0]).all()
        assert np.abs(r_kf[e, :nk, 1:] - h_kf[e, :nk, 1:]).max() <= 1e-5, ("LBA keyframe poses", e)
        assert np.abs(r_pt[e, :npt, 1:] - h_pt[e, :npt, 1:]).max() <= 1e-5, ("LBA points", e)
    # the HIP bodies were the ones that ran
    hip.orbx_shim_extract_orb_calls.restype = ctypes.c_ulong
    assert hip.orbx_shim_extract_orb_calls() >= 30
    # ... and Frame::ComputeBoW of every frame was served by the descent its constructor began on the device-resident descriptors (shim/Frame_hip.cc:
    # PostExtract -> orbx_bow_job_begin; the BowVector / FeatureVector hashes above are those of the reference's own transform())
    hip.orbx_shim_early_bow.restype = ctypes.c_ulong
    assert hip.orbx_shim_early_bow() >= 30


@pytest.mark.gpu
def test_thirty_frames_in_both_libraries(orbx, tmp_path):
    _thirty_frames(orbx, tmp_path, l6=False)


@pytest.mark.gpu
def test_thirty_frames_in_both_libraries_on_the_l6_tree(orbx, tmp_path):
    """The same sequence and the same comparisons with the k = 10, L = 6 vocabulary: ComputeBoW descends 1.1 M nodes and SearchByBoW(KF, F) walks
    the about 100 level-2 groups of its FeatureVector instead of one (the all-reference run finds 100 or more matches per frame there)."""
    _thirty_frames(orbx, tmp_path, l6=True)
