#!/usr/bin/env python3
"""Generate tests/golden/slam/voc_k10_L6_{full,ragged}.npz: what the COMPILED REFERENCE's own TemplatedVocabulary (oracle/_ref/liborbslam.so,
vendored DBoW2, tree loaded through loadFromTextFile) gives on the k = 10, L = 6 trees of tests/bow_l6.py.

    make -f oracle/Makefile all && python tools/gen_golden_bow_l6.py

Data only.  Neither the tree (1.1 M nodes) nor the 3000 descriptors are stored: consumers regenerate both from their seeds and compare
the digests stored here first (tests/bow_l6.py: fixture).  Per file, for levelsup = 4: word, node, weight, fv_node, bow_ids, bow_vals;
for levelsup = 2, 0 and 6 (>= L: the key is node 0): word and fv_node; tree_digest, desc_seed, desc_digest and the census
[distinct filed nodes, words filed more than once, unfiled features, ties at depth 1..6]."""
import importlib
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import bow_l6  # noqa: E402
import oracle_lib  # noqa: E402

orbx = importlib.import_module("self_commit_orb-slam2_amd")


def main():
    assert oracle_lib.slam_lib() is not None, "build oracle/_ref first (needs the reference sources)"
    out = bow_l6.GOLDEN
    out.mkdir(parents=True, exist_ok=True)
    for name in bow_l6.TREES:
        voc = bow_l6.tree(name)
        with tempfile.TemporaryDirectory() as tmp:
            path = Path(tmp) / "voc.txt"
            orbx.voc_synth.write_text_fast(voc, path)
            ref = oracle_lib.RefVocabulary(path)
        assert ref.size() == int(voc["is_leaf"].sum())
        seed = bow_l6.DESC_SEED[name]
        d = bow_l6._descs_l6(voc, bow_l6.N_FIXTURE, seed)
        r = ref.transform(d, 4)
        c = bow_l6.census(voc, d, r["word"], r["weight"], r["fv_node"])
        bow_l6.assert_census(c)
        data = dict(tree_digest=orbx.voc_synth.tree_digest(voc), desc_seed=np.int64(seed), desc_digest=bow_l6.desc_digest(d), census=c,
                    num_nodes=np.int64(voc["num_nodes"]), **r)
        for lu in (2, 0, 6):
            q = ref.transform(d, lu)
            data["word_%d" % lu], data["fv_node_%d" % lu] = q["word"], q["fv_node"]
        np.savez_compressed(out / ("voc_k10_L6_%s.npz" % name), **data)
        print(name, voc["num_nodes"], "census", c.tolist(), (out / ("voc_k10_L6_%s.npz" % name)).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
