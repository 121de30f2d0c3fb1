"""The batch path's joint launches (k_pyr_band_fast: launch l = blur of level l + resize of level l + 1 + FAST cells of level l, for levels 0 and 1;
k_fast_cells then takes the cells from level 2 on) against the launches they replace (8 x k_pyr_band, then k_fast_cells over every cell;
ORBX_FAST_SPLIT=1), on the same handle, byte for byte: keypoints, descriptors and counts of every frame, every pyramid level and every blurred level.

Frames: textured, low texture (the minThFAST retry), white with dots (skipped and empty cells), repeated over the batch.
Shapes: the flagship; ragged last cells and bands; few levels with large cells; the stereo geometry (another detector instantiation); 320x240, which
the plan refuses (the call must fall back and still match); 170x170 with two levels, whose level 1 has fewer cells than one detector block.  Batch 3
runs one cell per detector wave, batch 33 four (tests/test_pyr_fast_plan.py checks that a joined level's cell count is then no multiple of 16).
Both blur instantiations (taps summing to 256 and to 257).
Which form a call took is read from the developer tap orbx_debug_last_batch_pyr_fast and compared with the restated plan.
Fallbacks: with the parity taps on the handle keeps the split launches and agrees; ORBX_PYR_SPLIT=1 (the new switch unset) runs as before.
"""
import ctypes

import numpy as np
import pytest

from test_pyr_fast_plan import plan

pytestmark = pytest.mark.gpu

SHAPES = [
    # (W, H, nfeatures, scale factor, levels)
    (640, 480, 1000, 1.2, 8),
    (641, 479, 1000, 1.2, 8),
    (643, 397, 800, 2.2, 3),
    (1241, 376, 2000, 1.2, 8),
    (320, 240, 500, 1.2, 8),      # (its top levels' single cells are 57 px wide: four detector regions leave the LDS limit, the plan falls back)
    (170, 170, 300, 1.2, 2),      # level 1: nine cells, fewer than one detector block
]
TAPS = [None, (19, 34, 48, 56, 48, 34, 18)]      # the default taps (sum 256); sum 257: the clamping instantiation

_frames = {}


def _three_frames(orbx, W, H):
    if (W, H) not in _frames:
        white = np.full((H, W), 255, np.uint8)
        white[::37, ::41] = 0
        _frames[(W, H)] = [orbx.synth_frame(71, W, H), orbx.synth_frame(72, W, H, orbx.SYNTH_LOW_TEXTURE), white]
    return _frames[(W, H)]


def _joint(orbx, ext):
    fn = orbx.load_library().orbx_debug_last_batch_pyr_fast
    fn.argtypes = [ctypes.c_void_p]
    return bool(fn(ext._h))


def _run(ext, frames, nl):
    kps, desc, counts = ext.extract_batch(frames)
    out = []
    for f in range(len(frames)):
        n = int(counts[f])
        out.append((kps[f, :n].copy(), desc[f, :n].copy(), [ext.mvImagePyramid(l, frame=f) for l in range(nl)],
                    [ext.mvImagePyramid(l, frame=f, blurred=True) for l in range(nl)]))
    return counts.copy(), out


def _assert_same(a, b, nl, what):
    (ca, fa), (cb, fb) = a, b
    assert (ca == cb).all(), "%s: counts" % what
    for f in range(len(fa)):
        (ka, da, pa, ba), (kb, db, pb, bb) = fa[f], fb[f]
        for l in range(nl):
            assert (pa[l] == pb[l]).all(), "%s: pyramid, frame %d level %d" % (what, f, l)
            assert (ba[l] == bb[l]).all(), "%s: blurred pyramid, frame %d level %d" % (what, f, l)
        assert len(ka) == len(kb) and (ka.view(np.uint8) == kb.view(np.uint8)).all(), "%s: keypoints, frame %d" % (what, f)
        assert (da == db).all(), "%s: descriptors, frame %d" % (what, f)


@pytest.mark.parametrize("taps", TAPS, ids=["taps256", "taps257"])
@pytest.mark.parametrize("batch", [3, 33])
@pytest.mark.parametrize("W,H,nf,sf,nl", SHAPES)
def test_joint_launches_equal_split_launches(orbx, monkeypatch, W, H, nf, sf, nl, batch, taps):
    kw = {} if taps is None else {"gauss_taps": taps}
    ext = orbx.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H, max_batch=batch, **kw)
    three = _three_frames(orbx, W, H)
    frames = [three[i % 3] for i in range(batch)]
    monkeypatch.delenv("ORBX_PYR_SPLIT", raising=False)
    monkeypatch.delenv("ORBX_FAST_SPLIT", raising=False)
    joint = _run(ext, frames, nl)      # (first on the fresh handle: a cell that no wave took would keep whatever the buffers held)
    # the stereo geometry may be refused by the plan (four detector regions above 48 KB): then the call falls back and still has to match
    assert _joint(orbx, ext) == plan(W, H, sf, nl)["joint"], "the handle's choice of launch form differs from the restated plan"
    if (W, H) == (640, 480):
        assert _joint(orbx, ext), "the flagship geometry must run the joint launches"
    assert int(joint[0].sum()) > 0
    monkeypatch.setenv("ORBX_FAST_SPLIT", "1")
    split = _run(ext, frames, nl)
    assert not _joint(orbx, ext), "ORBX_FAST_SPLIT=1 must keep the detector's own launch"
    _assert_same(joint, split, nl, "joint vs ORBX_FAST_SPLIT=1")
    ext.close()


@pytest.mark.parametrize("W,H,nf,sf,nl", SHAPES[:2])
def test_fallbacks_take_the_split_launches_and_agree(orbx, monkeypatch, W, H, nf, sf, nl):
    ext = orbx.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H, max_batch=3)
    frames = _three_frames(orbx, W, H)
    monkeypatch.delenv("ORBX_PYR_SPLIT", raising=False)
    monkeypatch.delenv("ORBX_FAST_SPLIT", raising=False)
    joint = _run(ext, frames, nl)
    assert _joint(orbx, ext)
    # the pyramid's own A/B switch with the new one unset: split pyramid launches, the detector's own launch, as before
    monkeypatch.setenv("ORBX_PYR_SPLIT", "1")
    pyr_split = _run(ext, frames, nl)
    assert not _joint(orbx, ext), "ORBX_PYR_SPLIT=1 must keep the split launches"
    _assert_same(joint, pyr_split, nl, "joint vs ORBX_PYR_SPLIT=1")
    monkeypatch.delenv("ORBX_PYR_SPLIT", raising=False)
    # parity taps: the score map is written by the detector's own launch
    ext.set_debug_taps(True)
    taps = _run(ext, frames, nl)
    assert not _joint(orbx, ext), "with the parity taps the handle must keep the detector's own launch"
    _assert_same(joint, taps, nl, "joint vs parity taps")
    assert ext.debug_scores(0, frame=0).any(), "the parity tap's score map is empty"
    ext.set_debug_taps(False)
    again = _run(ext, frames, nl)
    assert _joint(orbx, ext)
    _assert_same(joint, again, nl, "joint, again after the taps")
    ext.close()
