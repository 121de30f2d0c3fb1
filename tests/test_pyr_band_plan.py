"""k_pyr_band's host plan and the two pieces of integer arithmetic its item loops rest on.

(a) The division constants (csrc/orbx_internal.h: orbx_band_div, m | S << 20 with S = 14 + ceil(log2 n), m = ceil(2^S / n)).  build_geometry's plan is
    not reachable without a device (a handle is created on one), so the FORMULA is restated here and checked, exhaustively: for every divisor a handle
    can plan (chunks and column groups per row of levels up to the maximum 4111 px: n <= 1028, taken here up to 4112) and for the divisors of every level
    of the geometries of tests/test_pyr_band.py plus 640x480, 1241x376, 752x480 and the maximum size, every item index below ORBX_BAND_MAX_ITEMS = 2^14
    (build_geometry refuses a geometry whose bands form more items, so this covers every index the kernel can form) gives item / n and item % n in the
    32-bit arithmetic of the kernel.
(b) The resize blend's single multiply: ((b << 12) * (h << 4)) >> 32 == (b * h) >> 16 for every row weight 0 .. 2048 and every horizontal value
    h < 2^16 (134 M pairs), and the operands stay below 2^24.
(c) GPU: fused launches == split launches (ORBX_PYR_SPLIT=1) on two geometries whose levels end inside a 16-byte chunk, a 4-pixel group and an
    8-row group, so that the tail chunks of the staging, blur and resize loops all run.
"""
import numpy as np
import pytest

MAX_ITEMS = 1 << 14
MAX_SIDE = 4111


def band_div(n):
    S = 14
    while (1 << (S - 14)) < n:
        S += 1
    m = ((1 << S) + n - 1) // n
    return m | (S << 20)


def level_sizes(W, H, scale_factor, nlevels):
    """build_tables / build_geometry: float scale chain, invScale = 1 / scale, lrintf(W * invScale)."""
    sf = np.float64(np.float32(scale_factor))
    scale, out = np.float32(1.0), []
    for l in range(nlevels):
        if l:
            scale = np.float32(np.float64(scale) * sf)
        inv = np.float32(1.0) / scale
        out.append((int(np.rint(np.float32(W) * inv)), int(np.rint(np.float32(H) * inv))))
    return out


GEOMETRIES = [(640, 480, 1.2, 8), (1241, 376, 1.2, 8), (641, 479, 1.2, 8), (643, 397, 2.2, 3), (1001, 333, 1.3, 5), (752, 480, 1.2, 8),
              (MAX_SIDE, MAX_SIDE, 1.2, 8), (701, 517, 1.2, 8), (1243, 379, 1.25, 6)]


def _check_divisor(n, items):
    dv = band_div(n)
    m, S = dv & 0xfffff, dv >> 20
    assert m < (1 << 20) and S < 32 and (m >> 24) == 0
    prod = items * np.uint64(m)
    assert int(prod.max()) < (1 << 32), "item * m leaves 32 bits (n = %d)" % n
    q = (prod & np.uint64(0xffffffff)) >> np.uint64(S)
    assert (q == items // np.uint64(n)).all(), "quotient, n = %d" % n
    assert (items - q * np.uint64(n) == items % np.uint64(n)).all(), "remainder, n = %d" % n


def test_division_constants_exact_for_every_item():
    items = np.arange(MAX_ITEMS, dtype=np.uint64)
    for n in range(1, MAX_SIDE + 2):
        _check_divisor(n, items)
    seen = set()
    for W, H, sf, nl in GEOMETRIES:
        for w, h in level_sizes(W, H, sf, nl):
            nc, g4 = (w + 15) >> 4, (w + 3) >> 2
            pitch = ((w + 15) & ~15) + 32
            band_h = min(32, ((48 * 1024) // pitch - 6) & ~7)
            if band_h >= 8:      # (otherwise the level has no band plan and the batch path keeps the split launches)
                assert (band_h + 6) * nc <= MAX_ITEMS and (band_h >> 3) * g4 <= MAX_ITEMS
                assert (g4 * ((band_h + 2 + 7) >> 3)) <= MAX_ITEMS      # resize rows of a band: at most its own rows + 2 (scale factors >= 1)
            seen.update((nc, g4))
    for n in sorted(seen):
        _check_divisor(n, items)


def test_blend_single_multiply_equals_truncating_blend():
    h = np.arange(1 << 16, dtype=np.uint64)
    assert int((h << np.uint64(4)).max()) < (1 << 24)
    for b in range(0, 2049):
        bs = np.uint64(b << 12)
        assert int(bs) < (1 << 24)
        assert (((bs * (h << np.uint64(4))) >> np.uint64(32)) == ((np.uint64(b) * h) >> np.uint64(16))).all(), "b = %d" % b


TAIL_CASES = [(701, 517, 900, 1.2, 8), (1243, 379, 1500, 1.25, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,nf,sf,nl", TAIL_CASES)
def test_fused_equals_split_on_tail_geometries(orbx, monkeypatch, W, H, nf, sf, nl):
    sizes = level_sizes(W, H, sf, nl)
    ok = False
    for l in range(nl - 1):
        (w, h), (wn, _) = sizes[l], sizes[l + 1]
        pitch = ((w + 15) & ~15) + 32
        band_h = min(32, ((48 * 1024) // pitch - 6) & ~7)
        ok = ok or (w % 16 != 0 and w % 4 != 0 and wn % 4 != 0 and (h % band_h) % 8 != 0)
    assert ok, "the geometry has no level that ends inside a chunk, a column group and a row group"
    ext = orbx.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H, max_batch=2)
    ext.set_debug_taps(True)
    frames = [orbx.synth_frame(81, W, H), orbx.synth_frame(82, W, H, orbx.SYNTH_LOW_TEXTURE)]
    res = []
    for split in (False, True):
        if split:
            monkeypatch.setenv("ORBX_PYR_SPLIT", "1")
        else:
            monkeypatch.delenv("ORBX_PYR_SPLIT", raising=False)
        kps, desc, counts = ext.extract_batch(frames)
        per = []
        for f in range(len(frames)):
            n = int(counts[f])
            shapes = [ext.mvImagePyramid(l, frame=f).shape for l in range(nl)]
            assert shapes == [(h, w) for w, h in sizes], "level sizes differ from the restated plan: %r" % (shapes,)
            per.append((kps[f, :n].copy(), desc[f, :n].copy(), [ext.mvImagePyramid(l, frame=f).copy() for l in range(nl)],
                        [ext.mvImagePyramid(l, frame=f, blurred=True).copy() for l in range(nl)]))
        res.append(per)
    for f in range(len(frames)):
        (ka, da, pa, ba), (kb, db, pb, bb) = res[0][f], res[1][f]
        for l in range(nl):
            assert (pa[l] == pb[l]).all(), "pyramid: frame %d level %d" % (f, l)
            assert (ba[l] == bb[l]).all(), "blurred pyramid: frame %d level %d" % (f, l)
        assert len(ka) == len(kb) and (ka.view(np.uint8) == kb.view(np.uint8)).all(), "keypoints: frame %d" % f
        assert (da == db).all(), "descriptors: frame %d" % f
    ext.close()
