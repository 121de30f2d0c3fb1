"""k_pyr_band's packed resize blend, copy-free row reuse and scalar-based stores (pyr_band_body, shared by k_pyr_band and k_pyr_band_fast) against
the split launches, whose kernels keep the byte-wise blend (k_resize, k_blur; ORBX_PYR_SPLIT=1): every byte of every pyramid level and of every
blurred level, keypoints and descriptors, with the default launches and with the split ones on the same handle.

Shapes are the smallest at which the new code can go wrong: widths that are no multiple of 4 (the tail column group), last chunks with fewer than 8
output rows, last bands with fewer than 8 blur rows, bands with and without mirrored rows, one band per level and several.  A level must be at least
62 pixels a side (two borders and one cell), so the small shapes reach their depth with a scale factor close to 1 - then EVERY output row reuses
a source row of the row before, the case the role swap of the two register sets is for; 1.2 mixes reuse and rows that recompute both sets; 2.2
never reuses a row and takes the byte-gather form of the horizontal pass (a column group spans more than eight source bytes).
Contents drive the blend sums to their extremes: all 255, all 0, 0 / 255 checkerboards of period 1 and 3, and seeded noise.
Both blur instantiations (taps summing to 256 and to 257).  Which launches a call took is read from the developer tap
orbx_debug_last_batch_pyr_band: a geometry whose plan falls back to the split launches would compare them with themselves."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [
    # (W, H, frames per batch, nfeatures, scale factor, levels)
    (95, 67, 2, 200, 1.01, 8),
    (95, 67, 2, 200, 1.03, 3),
    (129, 98, 2, 300, 1.06, 8),
    (129, 98, 2, 300, 1.2, 3),
    (322, 242, 2, 500, 1.2, 8),
    (322, 242, 2, 500, 1.2, 3),
    (640, 480, 1, 1000, 1.2, 8),
    (640, 480, 1, 1000, 2.2, 3),
]
TAPS = [None, (19, 34, 48, 56, 48, 34, 18)]      # the default taps (sum 256); sum 257: the clamping instantiation

_contents = {}


def _frames(W, H):
    if (W, H) not in _contents:
        y, x = np.mgrid[0:H, 0:W]
        rng = np.random.default_rng(1000 * W + H)
        _contents[(W, H)] = [np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8),
                             (((x + y) & 1) * 255).astype(np.uint8), (((x // 3 + y // 3) & 1) * 255).astype(np.uint8),
                             rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)]
    return _contents[(W, H)]


def _banded(orbx, ext):
    fn = orbx.load_library().orbx_debug_last_batch_pyr_band
    fn.argtypes = [ctypes.c_void_p]
    return bool(fn(ext._h))


def _run(orbx, ext, frames, nl, banded):
    kps, desc, counts = ext.extract_batch(frames)
    assert _banded(orbx, ext) == banded, "the batch ran the %s launches" % ("split" if banded else "band")
    out = []
    for f in range(len(frames)):
        n = int(counts[f])
        out.append((kps[f, :n].copy(), desc[f, :n].copy(), [ext.mvImagePyramid(l, frame=f).copy() for l in range(nl)],
                    [ext.mvImagePyramid(l, frame=f, blurred=True).copy() for l in range(nl)]))
    return out


@pytest.mark.parametrize("taps", TAPS, ids=["taps256", "taps257"])
@pytest.mark.parametrize("W,H,batch,nf,sf,nl", CASES)
def test_packed_blend_bands_equal_split_launches(orbx, monkeypatch, W, H, batch, nf, sf, nl, taps):
    kw = {} if taps is None else {"gauss_taps": taps}
    # (a handle for one frame at most answers a one-frame batch with its single-frame graph, which has no band launches: room for two)
    ext = orbx.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H, max_batch=2, **kw)
    contents = _frames(W, H)
    for i in range(0, len(contents), batch):
        frames = contents[i:i + batch]
        monkeypatch.delenv("ORBX_PYR_SPLIT", raising=False)
        fused = _run(orbx, ext, frames, nl, True)
        monkeypatch.setenv("ORBX_PYR_SPLIT", "1")
        split = _run(orbx, ext, frames, nl, False)
        monkeypatch.delenv("ORBX_PYR_SPLIT", raising=False)
        for f in range(len(frames)):
            (ka, da, pa, ba), (kb, db, pb, bb) = fused[f], split[f]
            for l in range(nl):
                assert (pa[l] == pb[l]).all(), "pyramid: content %d level %d" % (i + f, l)
                assert (ba[l] == bb[l]).all(), "blurred pyramid: content %d level %d" % (i + f, l)
            assert len(ka) == len(kb) and (ka.view(np.uint8) == kb.view(np.uint8)).all(), "keypoints: content %d" % (i + f)
            assert (da == db).all(), "descriptors: content %d" % (i + f)
    ext.close()
