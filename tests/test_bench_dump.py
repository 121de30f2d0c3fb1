"""bench.py --dump-outputs on the host: the arrays it writes, their dtypes, the masking past each frame's count and the size budget
(stand-in handles; the GPU path is the same code behind orbx's download calls)."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
bench = importlib.import_module("bench")


class _Ext:
    capacity = 40

    def __init__(self, seed, kp_dtype):
        self.seed, self.kp_dtype = seed, kp_dtype

    def download(self, batch):
        r = np.random.default_rng(self.seed)
        k = np.zeros((batch, self.capacity), self.kp_dtype)
        for n in k.dtype.names:
            k[n] = r.integers(1, 100, k.shape)
        return k, r.integers(0, 256, (batch, self.capacity, 32)).astype(np.uint8), r.integers(20, 35, batch).astype(np.int32)


class _Matcher:
    max_features = 40

    def __init__(self, seed):
        self.seed = seed

    def download(self, npairs):
        r = np.random.default_rng(self.seed + 7)
        return r.integers(0, 30, (npairs, self.max_features)).astype(np.int32), None, r.integers(0, 20, npairs).astype(np.int32)


def test_dump_extract_match_writes_the_held_batches(orbx, tmp_path):
    exts = [_Ext(i, orbx.KEYPOINT_DTYPE) for i in range(3)]
    mts = [_Matcher(i) for i in range(3)]
    B, nbatches = 16, 8
    issued = 25 * nbatches                       # 25 steps of 8 batches on 3 handle pairs
    bench.dump_extract_match(tmp_path, exts, mts, B, nbatches, nbatches, issued)
    names = sorted(p.stem for p in tmp_path.glob("*.npy"))
    assert names == sorted(["sample_frames"] + ["batch%d_%s" % (b, n) for b in (5, 6, 7)
                                                for n in ("counts", "keypoints", "descriptors", "matches", "nmatches")])
    pick = np.load(tmp_path / "sample_frames.npy").astype(int)
    assert len(pick) == B and (pick == np.arange(B)).all()
    for b in (5, 6, 7):
        h = (issued - nbatches + b) % 3
        kps, desc, counts = exts[h].download(B)
        m = mts[h].download(B)[0]
        kp = np.load(tmp_path / ("batch%d_keypoints.npy" % b))
        de = np.load(tmp_path / ("batch%d_descriptors.npy" % b))
        mm = np.load(tmp_path / ("batch%d_matches.npy" % b))
        assert kp.dtype == de.dtype == mm.dtype == np.float32
        assert (np.load(tmp_path / ("batch%d_counts.npy" % b)) == counts).all()
        for j, f in enumerate(pick):
            c = counts[f]
            assert (kp[j, :c, 0] == kps[f, :c]["x"]).all() and (kp[j, :c, 5] == kps[f, :c]["octave"]).all() and (kp[j, c:] == 0).all()
            assert (de[j, :c] == desc[f, :c]).all() and (de[j, c:] == 0).all()
            assert (mm[j, :c] == m[f, :c]).all() and (mm[j, c:] == -1).all()


def test_dump_sample_is_seeded_and_within_budget():
    a = bench.dump_sample(256, 3, 1152 * 40 * 4)
    assert (a == bench.dump_sample(256, 3, 1152 * 40 * 4)).all() and len(a) == 64 and len(np.unique(a)) == 64
    big = bench.dump_sample(256, 3, 8 << 20)
    assert 1 <= len(big) and 3 * len(big) * (8 << 20) <= bench.DUMP_BUDGET


def test_write_outputs_types_and_budget(tmp_path):
    bench.write_outputs(tmp_path, {"a": np.arange(5, dtype=np.int32), "b": np.ones(3, np.float64)})
    assert np.load(tmp_path / "a.npy").dtype == np.float32 and np.load(tmp_path / "b.npy").dtype == np.float64
    with pytest.raises(RuntimeError):
        bench.write_outputs(tmp_path / "x", {"c": np.zeros(bench.DUMP_BUDGET // 4 + 1, np.float32)})
    assert not (tmp_path / "x").exists()
