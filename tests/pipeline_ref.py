"""What the resident extract + match pipeline has to compute, from the CPU oracle alone (tests/test_resident_pipeline.py).

The pipeline is the call order of bench.py's step(): NS extractor / matcher handle pairs take resident batches in turn - run_device,
features_of, search_by_bow_device(..., after=ext) - with no host synchronisation in between.  This module lays out the batches of such a
run (SCENES), names every frame by a key, and caches the oracle's work per distinct frame and per distinct ordered pair:
  * keypoints and descriptors:  oracle.restatement(nf).extract(frame)
  * SearchByBoW:                oracle_lib.search_by_bow(oracle, 0, ...) on those features; the distance of a match is the Hamming distance
                                of the two oracle descriptors, an entry without a match is (-1, 256) over the whole row (k_bow_greedy
                                initialises the row and clears what the rotation histogram removes)
  * ComputeStereoMatches:       oracle_lib.compute_stereo_matches on the oracle's features and pyramids
Nothing here touches the device: the expected values exist before the first launch.

A frame key is ("flat",) = np.full((H, W), 90) (no keypoints), ("view", seed, v) = view v of synthetic scene `seed`, translated by 3 x 1 px per
view as orbx.synth_sequence lays a scene out, or ("eye", seed, right) = one image of a synthetic stereo pair."""
import concurrent.futures as cf
import os

import numpy as np

import oracle_lib

NS, B, NBATCH = 3, 5, 9      # handle pairs, frames per batch (odd, below max_batch = 8), batches of a run: every result buffer of every handle is used twice
FLAT = ("flat",)
FLAT_LEVEL = 90
STEP = (3, 1)                # px per view (orbx.synth_sequence's default)

# geometry -> (W, H, nfeatures).  "ragged" = the smallest ragged geometry of test_extractor_gpu.py::ODD; "joint" = the benchmark's
# (test_pyr_fast.py::SHAPES[0]: the joint pyramid + detector launches).
GEOMS = {"ragged": (333, 251, 500), "joint": (640, 480, 1000)}

# Batch j of a run = (scene seed, first view, position of the flat frame or None): B consecutive views of the scene - one fewer with a flat frame,
# which takes a position of its own.  The oracle extracts nfeatures + a few keypoints from nearly every textured frame, so two frames often have
# the SAME count; the seeds and first views below were picked (by a search over the oracle's counts) so that on every handle pair the three
# batches it sees (j, j + NS, j + 2 NS) differ in the count of EVERY frame position.  test_scenes_* hold that - a changed oracle or generator
# shows there, not as a coincidence on the device.
SCENES = {
    "ragged": [(4100, 0, 2), (4110, 0, None), (4120, 0, 0), (4130, 1, 4), (4140, 0, 1), (4150, 2, None), (4160, 2, None), (4170, 8, 3), (4181, 0, 2)],
    "joint": [(4100, 0, 2), (4110, 0, None), (4120, 0, 0), (4130, 1, 4), (4140, 4, 1), (4150, 3, None), (4160, 1, None), (4170, 0, 3), (4180, 2, 2)],
}


def batch_keys(geom, j):
    """Frame keys of batch j of the run at `geom`."""
    seed, v0, flat = SCENES[geom][j]
    views = [("view", seed, v0 + i) for i in range(B - (flat is not None))]
    if flat is not None:
        views.insert(flat, FLAT)
    return views


def run_keys(geom):
    return [batch_keys(geom, j) for j in range(NBATCH)]


def ring_pairs(n=B):
    """bench.py's pairs: frame i (as KeyFrame) against frame (i + 1) % n (as Frame)."""
    return np.arange(n, dtype=np.int32), (np.arange(n, dtype=np.int32) + 1) % n


def kp7(k):
    """structured device keypoints -> the oracle's 7 float32 per keypoint."""
    return np.stack([k[c].astype(np.float32) for c in ("x", "y", "size", "angle", "response", "octave", "class_id")], 1)


class Ref:
    """Frames and the oracle's results for one geometry, cached per key / per ordered pair of keys."""

    def __init__(self, orbx, oracle, W, H, nf):
        self.orbx, self.oracle, self.W, self.H, self.nf = orbx, oracle, W, H, nf
        self._frames, self._feat, self._match, self._pyr, self._stereo = {}, {}, {}, {}, {}
        self._rst = oracle.restatement(nf)

    def frame(self, key):
        if key not in self._frames:
            o, W, H = self.orbx, self.W, self.H
            if key == FLAT:
                im = np.full((H, W), FLAT_LEVEL, np.uint8)
            elif key[0] == "view":
                im = o.synth_frame(key[1], W, H, 0, key[2], key[2] * STEP[0], key[2] * STEP[1])
            elif key[0] == "eye":
                im = o.synth_frame(key[1], W, H, o.SYNTH_STEREO_RIGHT if key[2] else 0)
            else:
                raise KeyError(key)
            im.setflags(write=False)
            self._frames[key] = im
        return self._frames[key]

    def frames(self, keys):
        return [self.frame(k) for k in keys]

    def prefetch(self, keys):
        """Extract the frames not yet cached on a few threads (one oracle instance per thread: an instance is not re-entrant)."""
        todo = [k for k in dict.fromkeys(keys) if k not in self._feat]
        if not todo:
            return
        nthr = max(1, min(8, os.cpu_count() or 1, len(todo)))

        def work(t):
            rst = self.oracle.restatement(self.nf)
            return [(k, rst.extract(self.frame(k))) for k in todo[t::nthr]]
        for k in todo:
            self.frame(k)
        with cf.ThreadPoolExecutor(nthr) as ex:
            for part in ex.map(work, range(nthr)):
                for k, (ko, do) in part:
                    self._store(k, ko, do)

    def _store(self, key, ko, do):
        ks = np.zeros(len(ko), self.orbx.KEYPOINT_DTYPE)
        for i, c in enumerate(("x", "y", "size", "angle", "response", "octave", "class_id")):
            ks[c] = ko[:, i]
        for a in (ko, do, ks):
            a.setflags(write=False)
        self._feat[key] = (ko, do, ks)

    def features(self, key):
        """(7 float32 per keypoint, descriptors, the same keypoints as structured array) of the oracle."""
        if key not in self._feat:
            self._store(key, *self._rst.extract(self.frame(key)))
        return self._feat[key]

    def count(self, key):
        return len(self.features(key)[0])

    def match(self, ka, kb, nnratio=0.7, check_ori=True):
        """SearchByBoW mode 0, one node, frame `ka` as KeyFrame against frame `kb` as Frame: (nmatches, matches[nB], dists[nB])."""
        k = (ka, kb, nnratio, check_ori)
        if k not in self._match:
            _, dA, sA = self.features(ka)
            _, dB, sB = self.features(kb)
            n, m = oracle_lib.search_by_bow(self.oracle, 0, sA, dA, sB, dB, nnratio, check_ori)
            d = np.full(len(m), 256, np.int32)
            hit = m >= 0
            d[hit] = np.unpackbits(dA[m[hit]] ^ dB[hit], axis=1).sum(1)
            m = m.astype(np.int32)
            m.setflags(write=False)
            d.setflags(write=False)
            self._match[k] = (int(n), m, d)
        return self._match[k]

    def pyramid(self, key):
        if key not in self._pyr:
            self._pyr[key] = self.oracle.pyramid(self._rst, self.frame(key))
        return self._pyr[key]

    def stereo(self, kl, kr, bf):
        """Frame::ComputeStereoMatches of (left key, right key): (mvuRight, mvDepth) of the oracle, and (bestDist, bestIdxR) of its Hamming
        stage (oracle_lib.stereo_hamming with mb = 0: no disparity limit), which the matcher's download returns beside them."""
        k = (kl, kr, bf)
        if k not in self._stereo:
            t = self._rst.tables()[0]
            (koL, dL, sL), (koR, dR, sR) = self.features(kl), self.features(kr)
            u, z, _ = oracle_lib.compute_stereo_matches(self.oracle, koL, dL, koR, dR, self.pyramid(kl), self.pyramid(kr), t[0], t[1], bf, 0.0)
            bd, bi = oracle_lib.stereo_hamming(self.oracle, sL, dL, sR, dR, t[0], self.H, float("inf"))
            self._stereo[k] = (u.copy(), z.copy(), bd.copy(), bi.copy())
        return self._stereo[k]

    # ---- a download against the oracle: bit patterns and bytes, no tolerance ----
    def check_features(self, keys, kps, desc, counts, what=""):
        assert len(counts) == len(keys)
        for f, key in enumerate(keys):
            ko, do, _ = self.features(key)
            n = int(counts[f])
            assert n == len(ko), "%s frame %d %r: %d keypoints, the oracle has %d" % (what, f, key, n, len(ko))
            assert (kp7(kps[f, :n]).view(np.uint32) == ko.view(np.uint32)).all(), "%s frame %d %r: keypoints differ" % (what, f, key)
            assert (desc[f, :n] == do).all(), "%s frame %d %r: descriptors differ" % (what, f, key)

    def check_matches(self, keys, pa, pb, m, d, nm, what=""):
        """Rows of ORBmatcher.download for the pairs (keys[pa[p]], keys[pb[p]]): the whole row, match indices, distances and nmatches."""
        assert len(nm) == len(pa)
        for p, (a, b) in enumerate(zip(pa, pb)):
            wn, wm, wd = self.match(keys[int(a)], keys[int(b)])
            em, ed = np.full(m.shape[1], -1, np.int32), np.full(m.shape[1], 256, np.int32)
            em[:len(wm)], ed[:len(wd)] = wm, wd
            assert int(nm[p]) == wn, "%s pair %d (%d, %d): nmatches %d, the oracle has %d" % (what, p, a, b, int(nm[p]), wn)
            assert (m[p] == em).all(), "%s pair %d (%d, %d): match indices differ" % (what, p, a, b)
            assert (d[p] == ed).all(), "%s pair %d (%d, %d): distances differ" % (what, p, a, b)

    def check_stereo(self, keys_l, keys_r, bf, u, z, bi, bd, nm, what=""):
        """Rows of ORBmatcher.download_stereo and ORBmatcher.download for the stereo pairs (keys_l[p], keys_r[p])."""
        for p, (kl, kr) in enumerate(zip(keys_l, keys_r)):
            wu, wz, wd, wi = self.stereo(kl, kr, bf)
            n = len(wu)
            assert (bd[p, :n] == wd).all() and (bi[p, :n] == wi).all(), "%s pair %d: bestDist / bestIdxR differ" % (what, p)
            assert (u[p, :n].view(np.uint32) == wu.view(np.uint32)).all(), "%s pair %d: mvuRight differs" % (what, p)
            assert (z[p, :n].view(np.uint32) == wz.view(np.uint32)).all(), "%s pair %d: mvDepth differs" % (what, p)
            assert int(nm[p]) == int((wu >= 0).sum()), "%s pair %d: nmatches" % (what, p)


_refs = {}


def ref_for(orbx, oracle, W, H, nf):
    """The one Ref of a geometry in this process (its caches are shared by every test)."""
    if (W, H, nf) not in _refs:
        _refs[(W, H, nf)] = Ref(orbx, oracle, W, H, nf)
    return _refs[(W, H, nf)]
