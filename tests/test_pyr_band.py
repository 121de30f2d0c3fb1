"""The batch path's fused pyramid + blur launches (k_pyr_band: level l blurred and level l+1 resized from one LDS band) against the split
launches it replaced (7 x k_resize ... k_blur behind the quadtree, ORBX_PYR_SPLIT=1): every pyramid byte, every blurred byte, keypoints and
descriptors, on the flagship and stereo geometries, odd sizes, a tight (unpadded) caller stride, a scale whose column groups span more than
eight source bytes (the resize's byte-gather groups), and both blur instantiations (taps summing to 256 and to 257)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [
    # (W, H, nfeatures, scale factor, levels, gauss taps or None)
    (640, 480, 1000, 1.2, 8, None),
    (640, 480, 1000, 1.2, 8, (19, 34, 48, 56, 48, 34, 18)),      # sums to 257: the clamping instantiation
    (1241, 376, 2000, 1.2, 8, None),
    (641, 479, 1000, 1.2, 8, None),
    (641, 479, 1000, 1.2, 8, (4, 20, 60, 88, 52, 24, 8)),
    (643, 397, 800, 2.2, 3, None),                                  # 4 output columns span > 8 source bytes
    (1001, 333, 900, 1.3, 5, (19, 34, 48, 56, 48, 34, 18)),
]


def _run(orbx, ext, frames, W, H, nl, monkeypatch, split, tight):
    if split:
        monkeypatch.setenv("ORBX_PYR_SPLIT", "1")
    else:
        monkeypatch.delenv("ORBX_PYR_SPLIT", raising=False)
    if tight:
        import torch
        buf = torch.from_numpy(np.stack(frames)).cuda()          # stride W, frame pitch W * H
        ext.run_device(ctypes.c_void_p(buf.data_ptr()), W, W * H, (len(frames), W, H))
        kps, desc, counts = ext.download(len(frames))
    else:
        kps, desc, counts = ext.extract_batch(frames)
    out = []
    for f in range(len(frames)):
        n = int(counts[f])
        pyr = [ext.mvImagePyramid(l, frame=f).copy() for l in range(nl)]
        blur = [ext.mvImagePyramid(l, frame=f, blurred=True).copy() for l in range(nl)]
        out.append((kps[f, :n].copy(), desc[f, :n].copy(), pyr, blur))
    return out


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("W,H,nf,sf,nl,taps", CASES)
def test_fused_pyramid_equals_split_launches(orbx, monkeypatch, W, H, nf, sf, nl, taps, tight):
    kw = {} if taps is None else {"gauss_taps": taps}
    ext = orbx.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H, max_batch=3, **kw)
    ext.set_debug_taps(True)
    white = np.full((H, W), 255, np.uint8)
    white[::37, ::41] = 0
    frames = [orbx.synth_frame(71, W, H), orbx.synth_frame(72, W, H, orbx.SYNTH_LOW_TEXTURE), white]
    fused = _run(orbx, ext, frames, W, H, nl, monkeypatch, False, tight)
    split = _run(orbx, ext, frames, W, H, nl, monkeypatch, True, tight)
    for f in range(len(frames)):
        (ka, da, pa, ba), (kb, db, pb, bb) = fused[f], split[f]
        for l in range(nl):
            assert (pa[l] == pb[l]).all(), "pyramid: frame %d level %d" % (f, l)
            assert (ba[l] == bb[l]).all(), "blurred pyramid: frame %d level %d" % (f, l)
        assert len(ka) == len(kb) and (ka.view(np.uint8) == kb.view(np.uint8)).all(), "keypoints: frame %d" % f
        assert (da == db).all(), "descriptors: frame %d" % f
    ext.close()
