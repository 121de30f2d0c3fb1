"""Synthetic DBoW2 vocabulary trees (the reference's ORBvoc.txt is not in the mount: it is listed
in .MISSING_LARGE_BLOBS).  Same structure and text format as the file ORBVocabulary::
loadFromTextFile reads (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1420):
first line "k L scoring weighting", then one line per node in id order:
"parent isLeaf d0 ... d31 weight".  Test / benchmark data only."""
import numpy as np


def make_vocabulary(k=10, L=3, seed=1, zero_weight_frac=0.05, ragged=True):
    """Hierarchical tree: every child is its parent's descriptor with (128 >> depth) random bit
    flips, so the descent is meaningful; inner nodes have 1..k children (ragged) or exactly k;
    all leaves sit at depth L; a few words carry weight 0 (stopped words, :1160-1166)."""
    rng = np.random.default_rng(seed)
    parent, is_leaf, desc, weight, depth = [0], [0], [np.zeros(32, np.uint8)], [0.0], [0]
    frontier = [0]
    for d in range(1, L + 1):
        nxt = []
        for p in frontier:
            nchild = int(rng.integers(max(1, k // 2), k + 1)) if ragged else k
            for _ in range(nchild):
                if d == 1:
                    dd = rng.integers(0, 256, 32, dtype=np.uint8)
                else:
                    dd = desc[p].copy()
                    for b in rng.integers(0, 256, max(4, 128 >> d)):
                        dd[b >> 3] ^= np.uint8(1 << (b & 7))
                parent.append(p); desc.append(dd); depth.append(d)
                leaf = d == L
                is_leaf.append(1 if leaf else 0)
                w = float(rng.uniform(0.5, 9.0)) if leaf else 0.0
                if leaf and rng.random() < zero_weight_frac:
                    w = 0.0
                weight.append(w)
                nxt.append(len(parent) - 1)
        frontier = nxt
    parent = np.array(parent, np.int32)
    # ids must be assigned level by level with parents first: already the case (BFS)
    return dict(k=k, L=L, parent=parent, is_leaf=np.array(is_leaf, np.uint8), desc=np.stack(desc).astype(np.uint8),
                weight=np.array(weight, np.float64), num_nodes=len(parent))


def write_text(voc, path, scoring=0, weighting=0):
    """DBoW2 text format; NO trailing newline (the reference's reader loops on !eof() and would
    parse an empty last line into a garbage node)."""
    lines = ["%d %d %d %d" % (voc["k"], voc["L"], scoring, weighting)]
    for i in range(1, voc["num_nodes"]):
        lines.append("%d %d %s %s" % (voc["parent"][i], voc["is_leaf"][i], " ".join(str(int(b)) for b in voc["desc"][i]), repr(float(voc["weight"][i]))))
    with open(path, "w") as f:
        f.write("\n".join(lines))


def make_vocabulary_fast(k=10, L=6, seed=1, zero_weight_frac=0.05, ragged=True):
    """make_vocabulary's tree family, drawn one LEVEL at a time (the k = 10, L = 6 tree of the reference's ORBvoc.txt - 1,111,111
    nodes, 10^6 words - in a fraction of a second instead of minutes).  Same dict layout and invariants: ids in BFS order with every parent
    before its children and the children of a node contiguous, inner nodes with max(1, k // 2)..k children (ragged) or exactly k, all
    leaves at depth L, level-1 descriptors random, deeper children = the parent with max(4, 128 >> depth) random bit flips (drawn with
    replacement, a bit hit twice flips back), leaf weights in [0.5, 9) with a share of zero-weight words.  Its random stream is its own:
    NOT the tree make_vocabulary(k, L, seed) gives."""
    rng = np.random.default_rng(seed)
    parent, desc, weight = [np.zeros(1, np.int32)], [np.zeros((1, 32), np.uint8)], [np.zeros(1, np.float64)]
    first, count = 0, 1          # the frontier: ids first .. first + count - 1
    for d in range(1, L + 1):
        nchild = rng.integers(max(1, k // 2), k + 1, count) if ragged else np.full(count, k, np.int64)
        par = np.repeat(np.arange(first, first + count, dtype=np.int32), nchild)
        m = len(par)
        if d == 1:
            dd = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        else:
            dd = desc[-1][par - first].copy()
            bits = rng.integers(0, 256, (m, max(4, 128 >> d)))
            rows = np.arange(m)
            for j in range(bits.shape[1]):          # one flip per row and pass: the fancy-indexed xor sees every row once
                dd[rows, bits[:, j] >> 3] ^= (1 << (bits[:, j] & 7)).astype(np.uint8)
        w = np.zeros(m, np.float64)
        if d == L:
            w = rng.uniform(0.5, 9.0, m)
            w[rng.random(m) < zero_weight_frac] = 0.0
        parent.append(par); desc.append(dd); weight.append(w)
        first, count = first + count, m
    parent = np.concatenate(parent)
    is_leaf = np.zeros(len(parent), np.uint8)
    is_leaf[first:] = 1
    return dict(k=k, L=L, parent=parent, is_leaf=is_leaf, desc=np.concatenate(desc), weight=np.concatenate(weight), num_nodes=len(parent))


def write_text_fast(voc, path, scoring=0, weighting=0, chunk=1 << 16):
    """write_text's file, byte for byte, written a chunk of nodes at a time: the 32 descriptor bytes of a node through a table of the 65536
    "a b" strings of a byte pair, the weight through the same repr(float).  1.1 M nodes (about 150 MB) in seconds."""
    pair = ["%d %d" % (v & 255, v >> 8) for v in range(65536)]          # little-endian uint16 view: low byte first
    n = voc["num_nodes"]
    par, leaf = np.asarray(voc["parent"]), np.asarray(voc["is_leaf"])
    d16 = np.ascontiguousarray(voc["desc"], np.uint8).view("<u2")
    wt = np.asarray(voc["weight"], np.float64)
    get = pair.__getitem__
    with open(path, "w") as f:
        f.write("%d %d %d %d" % (voc["k"], voc["L"], scoring, weighting))
        for lo in range(1, n, chunk):
            hi = min(n, lo + chunk)
            rows = zip(par[lo:hi].tolist(), leaf[lo:hi].tolist(), d16[lo:hi].tolist(), wt[lo:hi].tolist())
            f.write("".join(["\n%d %d %s %r" % (p, l, " ".join(map(get, d)), w) for p, l, d, w in rows]))


def tree_digest(voc):
    """sha256 over the parent, is_leaf, descriptor and weight bytes: names a tree, so that a consumer of recorded results can tell that the
    tree it regenerated from a seed is the one they were recorded on."""
    import hashlib
    h = hashlib.sha256()
    for key, dt in (("parent", "<i4"), ("is_leaf", "u1"), ("desc", "u1"), ("weight", "<f8")):
        h.update(np.ascontiguousarray(voc[key]).astype(dt, copy=False).tobytes())
    return h.hexdigest()
