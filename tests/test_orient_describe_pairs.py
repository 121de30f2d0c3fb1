"""k_orient_describe carries TWO keypoints per wave (one per half-wave) and eight per workgroup: the slots whose neighbours are missing.

A wave's halves are independent: a slot past its level's count, an odd last slot, a frame without keypoints or a level without keypoints leaves
its half (or the whole wave, or most of a workgroup) idle while the other half works.  Every case compares keypoints (as float bit patterns)
and descriptors with the CPU oracle, through the batch path (k_blur's prefix in outBase) and through the single-frame call (the combined
launch set: the kernel's own level prefix, outBase == nullptr).  227 x 227 is near the smallest frame the 8-level pyramid accepts.

Case 2 note: a level's slot capacity is quota + 3 + 4 * (initial quadtree nodes) >= 8 and the library asks for nfeatures >= 1, so a frame's
slot CAPACITY cannot be below 8; what is below 8 and odd here is the number of slots IN USE (a one-level frame with three keypoints: one
full wave, one wave with an idle half, two idle waves), once in a capacity of exactly one workgroup and once in an odd capacity (whose last
wave owns one slot only)."""
import threading

import numpy as np
import pytest

import texture_frames as tf

pytestmark = pytest.mark.gpu

W = H = 227


def kp_matrix(k):
    return np.stack([k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"].astype(np.float32),
                     k["class_id"].astype(np.float32)], 1)


def level_counts(ko, nlevels):
    return np.bincount(ko[:, 5].astype(np.int64), minlength=nlevels) if len(ko) else np.zeros(nlevels, np.int64)


def check_batch_and_single(orbx, frames, want, cfg, w=W, h=H):
    """frames through ONE batch call and, one by one, through the single-frame call (twice over the list: both result buffers)."""
    ext = orbx.ORBextractor(*cfg, max_width=w, max_height=h, max_batch=len(frames))
    kps, desc, counts = ext.extract_batch(frames)
    for f, (ko, do) in enumerate(want):
        n = int(counts[f])
        assert n == len(ko), ("batch count", f, n, len(ko))
        assert (kp_matrix(kps[f, :n]).view(np.uint32) == ko.view(np.uint32)).all(), ("batch keypoints", f)
        assert (desc[f, :n] == do).all(), ("batch descriptors", f)
    ext.close()
    one = orbx.ORBextractor(*cfg, max_width=w, max_height=h)
    for rep in range(2):
        for f, (ko, do) in enumerate(want):
            k, d = one(frames[f])
            assert len(k) == len(ko), ("single count", f, len(k), len(ko))
            if len(ko):
                assert (kp_matrix(k).view(np.uint32) == ko.view(np.uint32)).all(), ("single keypoints", f)
                assert (d == do).all(), ("single descriptors", f)
    one.close()


def test_blank_frame_between_textured_frames(orbx, oracle):
    cfg = (300, 1.2, 8, 20, 7)
    rst = oracle.restatement(*cfg)
    frames = [orbx.synth_frame(1, W, H), np.full((H, W), 90, np.uint8), orbx.synth_frame(2, W, H)]
    want = [rst.extract(im) for im in frames]
    assert len(want[0][0]) > 100 and len(want[1][0]) == 0 and len(want[2][0]) > 100
    check_batch_and_single(orbx, frames, want, cfg)


@pytest.mark.parametrize("nf", [1, 4])      # the level's slots (quota + 3 + 4 x one initial node): 8 = one workgroup, and 11 = odd, the last wave owns one slot
def test_fewer_than_eight_slots_in_use_and_odd(orbx, oracle, nf):
    cfg = (nf, 1.2, 1, 20, 7)
    rst = oracle.restatement(*cfg)
    frames = [tf.texture_frame("flat", 1, W, H), tf.texture_frame("weak", 1, W, H), tf.texture_frame("flat", 3, W, H)]
    want = [rst.extract(im) for im in frames]
    n = [len(ko) for ko, _ in want]
    assert 0 < n[0] < 8 and n[0] % 2 == 1, n      # three keypoints: an idle half-wave behind them, then idle waves
    assert all(0 < c < 8 for c in n), n
    check_batch_and_single(orbx, frames, want, cfg)


def test_odd_levels_and_empty_levels(orbx, oracle):
    cfg = (300, 1.2, 8, 20, 7)
    rst = oracle.restatement(*cfg)
    frames = [tf.texture_frame("gradient", 19, W, H), tf.texture_frame("weak", 2, W, H), tf.texture_frame("gradient", 33, W, H)]
    want = [rst.extract(im) for im in frames]
    c = [level_counts(ko, 8) for ko, _ in want]
    assert (c[0] % 2 == 1).any() and (c[0] == 0).any() and c[0].sum() > 0, c[0]      # an odd level AND an empty level in one frame
    assert (c[1] % 2 == 1).sum() >= 3 and (c[1] > 0).all(), c[1]                     # odd levels in front of used levels: the next level starts in a fresh wave
    assert c[2][0] % 2 == 1 and (c[2][1:] == 0).all(), c[2]                          # seven empty levels
    check_batch_and_single(orbx, frames, want, cfg)


def test_stereo_pair_1241x376(orbx, oracle):
    w, h, cfg = 1241, 376, (2000, 1.2, 8, 20, 7)
    rst = oracle.restatement(*cfg)
    pair = [orbx.synth_frame(41, w, h, 0, 0, 0, 0), orbx.synth_frame(41, w, h, 0, 1, 7, 0)]      # two views of one scene
    want = [rst.extract(im) for im in pair]
    assert min(len(ko) for ko, _ in want) > 1000
    ext = orbx.ORBextractor(*cfg, max_width=w, max_height=h, max_batch=2)
    kps, desc, counts = ext.extract_batch(pair)
    for f, (ko, do) in enumerate(want):
        n = int(counts[f])
        assert n == len(ko) and (kp_matrix(kps[f, :n]).view(np.uint32) == ko.view(np.uint32)).all() and (desc[f, :n] == do).all(), f
    ext.close()
    # the stereo Frame constructor's shape: two one-frame handles called from two threads at once (one launch set of two when they meet)
    left, right = (orbx.ORBextractor(*cfg, max_width=w, max_height=h) for _ in range(2))
    out, bar = {}, threading.Barrier(2)

    def run(i, e):
        bar.wait()
        out[i] = e(pair[i])
    ts = [threading.Thread(target=run, args=(i, e)) for i, e in enumerate((left, right))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for f, (ko, do) in enumerate(want):
        k, d = out[f]
        assert len(k) == len(ko) and (kp_matrix(k).view(np.uint32) == ko.view(np.uint32)).all() and (d == do).all(), f
    left.close(); right.close()
