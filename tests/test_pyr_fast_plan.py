"""The host partition of k_pyr_band_fast (batches: launch l = the pyramid bands of level l + the FAST cells of level l, for the first
ORBX_PF_JOIN_LEVELS = 2 levels; the cells of the levels behind them stay in k_fast_cells, which then starts at the first cell of level 2).

build_geometry's plan is not reachable without a device (a handle is created on one), so - as tests/test_pyr_band_plan.py does for the band plan - the
FORMULAS of csrc/orbx_internal.h (orbx_fast_blocks, orbx_pyr_fast_lds), csrc/orbx_extractor.hip (build_geometry: cells per level, the detector's LDS
carve-up, the band plan) and the kernel's block mapping (csrc/orbx_kernels.hip: k_pyr_band_fast) are restated here and checked:

  launch l, grid x = nBands(l) + nFastBlocks(l);  block bx >= nBands(l), wave w (four per block) takes the cells
      cellBase[l] + ((bx - nBands(l)) * 4 + w) * K  ..  + K,  cut at the level's last cell;  waves that start past it leave.
  k_fast_cells behind the pyramid: wave bx takes the cells  cellBase[2] + bx * K  ..  + K,  cut at the frame's last cell.

For the geometries of tests/test_pyr_fast.py, the flagship / stereo sizes and a sweep of odd sizes, with K = 1 (batch < 32) and K = 4:
  - every cell of every level is assigned to exactly one (launch, block, wave, position);
  - each cell of a joined level is assigned in its own level's launch, no wave of a joint launch crosses a level, and the detector's own launch
    takes cells of the other levels only;
  - the dynamic LDS of every launch, max(band rows, four detector regions), stays within the 48 KB a launch may ask for without an attribute,
    and the joint form is planned exactly when the four detector regions fit.
tests/test_pyr_fast.py (GPU) asserts that the handle's choice of form agrees with `plan()` here.
"""
import math

import numpy as np
import pytest

from test_pyr_band_plan import level_sizes

BORDER, CELL_W, PF_WAVES, PF_JOIN_LEVELS, LDS_LIMIT = 16, 30, 4, 2, 48 * 1024


def _align_up(x, a):
    return (x + a - 1) // a * a


def plan(W, H, scale_factor, nlevels):
    """build_geometry restated: per level (w, h, cellBase, cells, nBands, band LDS bytes), the detector's LDS bytes per wave, and whether the joint
    form is planned.  (The band plan's second condition - both source rows of every resized row inside the staged band - holds for scale factors
    >= 1, tests/test_pyr_band.py; a handle that finds otherwise keeps the split launches and tests/test_pyr_fast.py would report the disagreement.)"""
    levels, cells, band_ok = [], 0, True
    max_wcell = max_hcell = 0
    max_aw = 1
    for w, h in level_sizes(W, H, scale_factor, nlevels):
        width, height = np.float32(w - 2 * BORDER), np.float32(h - 2 * BORDER)
        ncols, nrows = int(width / np.float32(CELL_W)), int(height / np.float32(CELL_W))
        wcell, hcell = int(math.ceil(width / np.float32(ncols))), int(math.ceil(height / np.float32(nrows)))
        max_wcell, max_hcell = max(max_wcell, wcell), max(max_hcell, hcell)
        for cj in range(ncols):
            ini_x = BORDER + cj * wcell
            max_aw = max(max_aw, (min(ini_x + wcell + 6, w - BORDER) - 3) - (ini_x + 3))
        band_pitch = _align_up(w, 16) + 32
        band_h = min(32, (LDS_LIMIT // band_pitch - 6) & ~7)
        if band_h < 8:
            band_ok = False
            band_h = 8
        levels.append(dict(w=w, h=h, cellBase=cells, cells=ncols * nrows, nBands=(h + band_h - 1) // band_h, bandLds=(band_h + 6) * band_pitch))
        cells += ncols * nrows
    fc_pitch = 48 if max_wcell <= 32 else 64 if max_wcell <= 48 else 80
    fc_sc_pitch = 48 if max_aw + 2 <= 48 else 80
    if fc_sc_pitch == 80:
        fc_pitch = 80
    fc_lds = fc_pitch * (max_hcell + 6) + fc_sc_pitch * (max_hcell + 2) + _align_up(max_wcell * max_hcell * 2, 16)
    return dict(levels=levels, cellsPerFrame=cells, fcLds=fc_lds, joint=band_ok and PF_WAVES * fc_lds <= LDS_LIMIT)


def fast_blocks(cells, K):
    return (cells + PF_WAVES * K - 1) // (PF_WAVES * K)


def wave_range(lv, K, bx, w):
    """the kernel's mapping: cells [first, end) of detector wave w of block bx of the level's launch, or None for a wave that leaves"""
    first = lv["cellBase"] + ((bx - lv["nBands"]) * PF_WAVES + w) * K
    hi = lv["cellBase"] + lv["cells"]
    return None if first >= hi else (first, min(first + K, hi))


GEOMETRIES = [(640, 480, 1.2, 8), (641, 479, 1.2, 8), (643, 397, 2.2, 3), (1241, 376, 1.2, 8), (320, 240, 1.2, 8), (170, 170, 1.2, 2), (752, 480, 1.2, 8)]
SWEEP = [(W, H, 1.2, 8) for W in range(301, 1400, 97) for H in (241, 375, 517)] + [(W, 333, 1.3, 5) for W in range(331, 1100, 111)]


@pytest.mark.parametrize("K", [1, 4])
def test_every_cell_in_exactly_one_wave_of_its_level(K):
    for W, H, sf, nl in GEOMETRIES + SWEEP:
        p = plan(W, H, sf, nl)
        owner = np.full(p["cellsPerFrame"], -1, np.int64)
        seen = np.zeros(p["cellsPerFrame"], np.int32)
        n_join = min(PF_JOIN_LEVELS, nl) if p["joint"] else 0
        for l, lv in enumerate(p["levels"][:n_join]):
            nfb = fast_blocks(lv["cells"], K)
            assert nfb >= 1 and (nfb - 1) * PF_WAVES * K < lv["cells"] <= nfb * PF_WAVES * K, (W, H, l)
            for bx in range(lv["nBands"], lv["nBands"] + nfb):
                for w in range(PF_WAVES):
                    r = wave_range(lv, K, bx, w)
                    if r is None:
                        continue
                    first, end = r
                    assert lv["cellBase"] <= first < end <= lv["cellBase"] + lv["cells"], "a wave's range leaves level %d (%dx%d)" % (l, W, H)
                    assert end - first <= K
                    seen[first:end] += 1
                    owner[first:end] = l
            # blocks below nBands are bands, never detector blocks; the block behind the last one would start past the level
            assert wave_range(lv, K, lv["nBands"] + nfb, 0) is None
        # the detector's own launch: the cells behind the joined levels, K per wave from the first of them (waves may cross levels there, as ever)
        cell0 = p["levels"][n_join]["cellBase"] if n_join < nl else p["cellsPerFrame"]
        for bx in range((p["cellsPerFrame"] - cell0 + K - 1) // K):
            first, end = cell0 + bx * K, min(cell0 + bx * K + K, p["cellsPerFrame"])
            assert cell0 <= first < end
            seen[first:end] += 1
            for c in range(first, end):
                owner[c] = max(l for l, lv in enumerate(p["levels"]) if lv["cellBase"] <= c)
                assert owner[c] >= n_join, "the detector's own launch takes a cell of a joined level"
        assert (seen == 1).all(), "cells assigned %s times (%dx%d, K = %d)" % (sorted(set(seen.tolist())), W, H, K)
        for l, lv in enumerate(p["levels"]):
            assert (owner[lv["cellBase"]:lv["cellBase"] + lv["cells"]] == l).all(), "a cell of level %d runs in another level's launch" % l


def test_lds_of_every_launch_within_the_limit():
    for W, H, sf, nl in GEOMETRIES + SWEEP:
        p = plan(W, H, sf, nl)
        assert p["fcLds"] % 16 == 0      # (the waves' regions stay 16-byte aligned)
        assert p["joint"] == (PF_WAVES * p["fcLds"] <= LDS_LIMIT)
        if p["joint"]:
            for lv in p["levels"]:
                assert max(lv["bandLds"], PF_WAVES * p["fcLds"]) <= LDS_LIMIT, (W, H, lv)


def test_cases_of_the_gpu_test_cover_the_partition_edges():
    joined = lambda g: plan(*g)["levels"][:PF_JOIN_LEVELS]
    # batch 33 (K = 4): a joined level's cell count is no multiple of 16, so its last detector block is ragged and waves of it leave
    for g in [(640, 480, 1.2, 8), (641, 479, 1.2, 8), (1241, 376, 1.2, 8), (170, 170, 1.2, 2)]:
        assert plan(*g)["joint"] and any(lv["cells"] % (PF_WAVES * 4) for lv in joined(g)), g
    # batch 3 (K = 1): the same with blocks of four cells
    assert any(lv["cells"] % PF_WAVES for lv in joined((1241, 376, 1.2, 8)))
    # 170x170: a joined level with fewer cells than one detector block of four cells per wave
    assert any(lv["cells"] < PF_WAVES * 4 and lv["cells"] % PF_WAVES for lv in joined((170, 170, 1.2, 2)))
    # 320x240: the top levels' single cells are so large that four detector regions leave the LDS limit - the plan refuses the joint form
    assert not plan(320, 240, 1.2, 8)["joint"]
