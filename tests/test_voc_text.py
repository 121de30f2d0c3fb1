"""Loading a DBoW2 text vocabulary on the device (orbx_vocabulary_load_text*, orbx_vocabulary_tree, orbx_voc_text_parse_host; Python
Vocabulary.from_text / .tree / voc_text_parse_host; shim ORBVocabulary_hip::loadFromTextFile) against the restatement tests/voc_text_ref.py.
Everything is compared exactly: integers, and doubles as their 64 bits."""
import functools
import os
import subprocess
import tempfile
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import voc_text_ref as vt

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
HAVE_REF = oracle_lib.slam_lib() is not None
ERR_ARG = -1
gpu = pytest.mark.gpu
CHUNK = vt.CHUNK          # bytes of text per workgroup of the line index and the parse (VT_CHUNK); the overhang behind it is vt.OVERHANG
HEADER = ("k", "L", "scoring", "weighting", "num_nodes", "num_words", "final_newline")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _vs():
    import importlib
    return importlib.import_module("self_commit_orb-slam2_amd").voc_synth


# ---- the files (made once, never changed) -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tree(name):
    vs = _vs()
    if name == "tiny3":
        return vt.tiny3()
    if name == "ragged":
        return vs.make_vocabulary(3, 2, 4)
    if name == "k10L3":
        return vs.make_vocabulary(10, 3, 2)
    if name == "k10L3_dfs":
        return vt.renumber(tree("k10L3"), vt.dfs_order(tree("k10L3")))
    if name == "k10L3_random":
        return vt.renumber(tree("k10L3"), vt.random_order(tree("k10L3"), 5))
    if name == "messy":          # 2380 nodes in a random order: parents of 1 - 4 digits
        t = vs.make_vocabulary(13, 3, 3, ragged=False)
        return vt.renumber(t, vt.random_order(t, 9))
    if name == "k10L4":          # 11,111 nodes
        return vs.make_vocabulary_fast(10, 4, 6, ragged=False)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def text(name):
    if name == "messy":
        return vt.messy_text(tree("messy"), 11)
    if name == "messy_nl":
        return vt.messy_text(tree("messy"), 11, final_newline=True)
    if name == "messy_long":          # one line longer than the overhang, by separators in its middle, that runs out of its chunk's staged bytes
        lines = text("messy").split(b"\n")
        at = np.cumsum([len(l) + 1 for l in lines])          # at[i - 1]: where line i starts
        i = next(i for i in range(1000, len(lines)) if CHUNK - 100 < at[i - 1] % CHUNK < CHUNK - 10)
        t = lines[i].split()
        lines[i] = b" ".join(t[:20]) + b" " * (vt.OVERHANG + 40) + b" ".join(t[20:])
        return b"\n".join(lines)
    if name == "numbers":
        return vt.text_of(tree("k10L3"), tokens=vt.NUMBER_FORMS)
    if name == "k10L4_repr":
        return vt.text_of(tree("k10L4"))
    if name == "k10L4_g":
        return vt.text_of(tree("k10L4"), weight_fmt=lambda w: "%g" % w, final_newline=True)
    if name.endswith("_nl"):
        return vt.text_of(tree(name[:-3]), final_newline=True, scoring=1, weighting=2)
    return vt.text_of(tree(name))


FILES = ("tiny3", "tiny3_nl", "ragged", "k10L3", "k10L3_nl", "k10L3_dfs", "k10L3_random", "messy", "messy_nl", "messy_long", "numbers", "k10L4_repr", "k10L4_g")


@functools.lru_cache(maxsize=None)
def want(name):
    return vt.parse(text(name))


def same(got, ref, info=None):
    for key in ("parent", "is_leaf", "desc"):
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape and (got[key] == ref[key]).all(), key
    assert (_bits(got["weight"]) == _bits(ref["weight"])).all()
    assert got["k"] == ref["k"] and got["L"] == ref["L"] and got["num_nodes"] == ref["num_nodes"]
    if info is not None:
        assert [info[f] for f in HEADER] == [ref[f] for f in HEADER] and info["error_line"] == 0


@functools.lru_cache(maxsize=None)
def error_cases():
    """(name, text, line of the error).  The base: the ragged k = 3, L = 2 tree, whose node 1 is inner and whose last node is a leaf."""
    base = vt.text_of(tree("ragged")).split(b"\n")
    n = len(base)
    assert n >= 8
    first_leaf = int(np.flatnonzero(tree("ragged")["is_leaf"])[0])

    def edit(line, fn):
        b = list(base)
        b[line - 1] = fn(b[line - 1].split())
        return b"\n".join(b)

    def tok(i, v):
        return lambda t: b" ".join(t[:i] + [v] + t[i + 1:])
    out = [("short line", edit(5, lambda t: b" ".join(t[:20])), 5),
           ("abc byte", edit(6, tok(7, b"abc")), 6),
           ("256 byte", edit(6, tok(33, b"256")), 6),
           ("1e weight", edit(n, tok(34, b"1e")), n),
           ("inf weight", edit(n, tok(34, b"inf")), n),
           ("hex weight", edit(n, tok(34, b"0x1p3")), n),
           ("parent own id", edit(4, tok(0, b"3")), 4),
           ("parent -1", edit(4, tok(0, b"-1")), 4),
           ("child under leaf", edit(n, tok(0, b"%d" % first_leaf)), n),
           ("childless inner", edit(n, tok(1, b"0")), n),
           ("empty middle line", b"\n".join(base[:4] + [b""] + base[4:]), 5),
           ("blank middle line", b"\n".join(base[:4] + [b" \t\r"] + base[4:]), 5),
           ("header k 21", b"\n".join([b"21 2 0 0"] + base[1:]), 1),
           ("header short", b"\n".join([b"3 2 0"] + base[1:]), 1),
           ("header only", base[0], 1),
           ("header only newline", base[0] + b"\n", 1),
           ("empty buffer", b"", 1)]
    # the same line errors on a line the device cannot take itself: separators for more than a chunk and its overhang inside the line
    pad = b" " * (CHUNK + vt.OVERHANG + 8)
    forced = []
    for name, data, line in out:
        if line > 1 and "middle" not in name:
            b = data.split(b"\n")
            t = b[line - 1].split()
            b[line - 1] = b" ".join(t[:3]) + pad + b" ".join(t[3:])
            forced.append((name + " (host path)", b"\n".join(b), line))
    return out + forced


RANDOM_TOKENS = 20000


def random_weight_tokens(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = i % 5
        x = float(rng.uniform(0.5, 9.0)) if kind < 2 else float(np.ldexp(rng.random(), int(rng.integers(-1070, 1020))))
        if kind == 0:
            s = repr(x)
        elif kind == 1:
            s = "%g" % x
        elif kind == 2:
            s = repr(x)
        elif kind == 3:
            s = "%.*e" % (int(rng.integers(0, 20)), x)
        else:          # an odd integer in [2^53, 2^54): exactly half way between two doubles, 16 digits - a tie
            s = str(int(rng.integers(1 << 53, 1 << 54)) | 1)
        out.append(s.encode())
    return out


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------
def test_midpoint_token_is_the_midpoint():
    assert Fraction(vt.NUMBER_FORMS[-1]) == 1 + Fraction(1, 2 ** 53) and len(vt.NUMBER_FORMS[-1]) == 55
    assert vt.device_weight(vt.NUMBER_FORMS[-1].encode()) is None and vt.device_weight(b"9007199254740993") is None          # more than 19 digits; a tie


def test_restated_accept_rule_never_guesses():
    """whatever the restated device rule accepts is float(token), bit for bit; on repr and %g tokens it accepts all but a sliver"""
    toks = random_weight_tokens(RANDOM_TOKENS, 3) + [t.encode() for t in vt.NUMBER_FORMS]
    flagged = 0
    for t in toks:
        got = vt.device_weight(t)
        if got is None:
            flagged += 1
        else:
            assert _bits([got])[0] == _bits([float(t)])[0], t
    plain = [t for i, t in enumerate(toks[:RANDOM_TOKENS]) if i % 5 < 2]
    assert sum(vt.device_weight(t) is None for t in plain) <= len(plain) // 100
    assert flagged >= 5          # the ties, the long tokens and the subnormals are flagged


def test_library_accept_rule_equals_the_restatement(orbx):
    """the __host__ __device__ code of the kernel, run on the host, token by token: same decision, same bits"""
    for t in random_weight_tokens(RANDOM_TOKENS, 4) + [t.encode() for t in vt.NUMBER_FORMS] + [b"1e", b"abc", b".", b"+", b"-.e1", b"1e400", b"1e-400", b"00012.5000", b"1.5x"]:
        a, b = orbx.voc_text_weight_rule(t), vt.device_weight(t)
        assert (a is None) == (b is None) and (a is None or _bits([a])[0] == _bits([b])[0]), t


def test_committed_power_table_is_the_restatement_s(orbx):
    lines = [l for l in (ROOT / "self_commit_orb-slam2_amd" / "csrc" / "orbx_pow5_128.inc").read_text().splitlines() if l.startswith("{")]
    assert len(lines) == 651
    for q, l in zip(range(-342, 309), lines):
        hi, lo = [int(x.strip(" {},ul"), 16) for x in l.split(",")[:2]]
        assert (hi << 64) | lo == vt.pow5_128(q), q


@pytest.mark.parametrize("name", FILES)
def test_host_statement_equals_restatement(orbx, name):
    got = orbx.voc_text_parse_host(text(name))
    same(got, want(name), got)
    assert got["host_lines"] == got["num_nodes"] - 1


def test_restatement_reads_back_the_trees():
    for name in ("tiny3", "ragged", "k10L3", "k10L3_random", "messy", "k10L4_repr"):
        t = tree({"k10L4_repr": "k10L4"}.get(name, name))
        same(want(name), dict(t, num_nodes=t["num_nodes"]))
    assert want("messy_nl")["final_newline"] == 1 and want("messy")["final_newline"] == 0 and want("tiny3_nl")["scoring"] == 1 and want("tiny3_nl")["weighting"] == 2
    w = want("numbers")
    leaves = np.flatnonzero(w["is_leaf"])
    assert len(leaves) > 2 * len(vt.NUMBER_FORMS)
    for i in range(1, w["num_nodes"]):
        assert _bits([w["weight"][i]])[0] == _bits([float(vt.NUMBER_FORMS[(i - 1) % len(vt.NUMBER_FORMS)])])[0]


@pytest.mark.parametrize("case", range(len(error_cases())), ids=lambda i: error_cases()[i][0].replace(" ", "_"))
def test_host_statement_refuses_what_the_restatement_refuses(orbx, case):
    name, data, line = error_cases()[case]
    with pytest.raises(vt.FormatError) as r:
        vt.parse(data)
    assert r.value.line == line
    with pytest.raises(orbx.OrbxError) as e:
        orbx.voc_text_parse_host(data)
    assert e.value.code == ERR_ARG and e.value.text_info["error_line"] == line and ("line %d:" % line) in str(e.value), str(e.value)


def test_host_lines_cap_of_the_restated_rule():
    """the cap of the number-forms test, without a device: the restated rule flags at most 1 % of the lines of the 11,111-node files"""
    for name in ("k10L4_repr", "k10L4_g"):
        assert vt.device_host_lines(text(name)) <= (want(name)["num_nodes"] - 1) // 100, name
    assert vt.device_host_lines(text("messy_long")) == 1 and vt.device_host_lines(text("messy")) == 0          # the line that leaves its chunk's staged bytes


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/liborbslam.so not built (needs the reference sources)")
def test_restatement_equals_reference_loader(oracle, tmp_path):
    """messy whitespace, CRLF, no final newline: the restatement's tree through the vocabulary transform of oracle_lib == the compiled reference's
    vocabulary loaded from the same file by its own loadFromTextFile"""
    import bow_l6
    (tmp_path / "messy.txt").write_bytes(text("messy"))
    ref = oracle_lib.RefVocabulary(tmp_path / "messy.txt")
    w = want("messy")
    assert ref.size() == w["num_words"]
    d = descriptors("messy")
    for lu in (1, 2):
        r, g = bow_l6.restated(oracle, w, d, lu), ref.transform(d, lu)
        assert (r["word"] == g["word"]).all() and (_bits(r["weight"]) == _bits(g["weight"])).all() and (r["fv_node"] == g["fv_node"]).all(), lu


@pytest.mark.skipif(not os.access(REF / "Thirdparty" / "DBoW2" / "DBoW2" / "TemplatedVocabulary.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_load_compiles_against_the_reference_headers():
    shim = ROOT / "self_commit_orb-slam2_amd" / "shim"
    text_ = (shim / "ORBVocabulary_hip.cc").read_text()
    for piece in ("orbx_vocabulary_load_text(", "orbx_vocabulary_tree(", "loadFromTextFile", "createScoringObject()", "orbx_shim::Fail("):
        assert piece in text_, piece
    assert "Device() const" in (shim / "ORBVocabulary_hip.h").read_text()
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-I" + str(ROOT / "include"), "-fsyntax-only", str(shim / "ORBVocabulary_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@functools.lru_cache(maxsize=None)
def descriptors(name, n=2000):
    """n descriptors: leaves of the tree with a few flipped bits, and noise"""
    t = want(name)
    rng = np.random.default_rng(17)
    leaves = np.flatnonzero(t["is_leaf"])
    d = t["desc"][rng.choice(leaves, n)].copy()
    for j in range(3):
        b = rng.integers(0, 256, n)
        d[np.arange(n), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    d[::7] = rng.integers(0, 256, (len(d[::7]), 32), dtype=np.uint8)
    return d


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
def load(orbx, data):
    V = orbx.Vocabulary.from_text(data)
    try:
        return V.tree(), V.text_info
    finally:
        V.close()


@gpu
@pytest.mark.parametrize("name", ["tiny3", "tiny3_nl", "ragged", "k10L3", "k10L3_nl"])
def test_smallest_trees(orbx, name, tmp_path):
    got, info = load(orbx, text(name))
    same(got, want(name), info)
    assert info["host_lines"] == 0 and info["waits"] == 1 and info["bytes"] == len(text(name))
    (tmp_path / "v.txt").write_bytes(text(name))          # ... and the file form
    got, info = load(orbx, tmp_path / "v.txt")
    same(got, want(name), info)


@gpu
def test_both_writers_and_created_handles_round_trip(orbx, tmp_path):
    vs = orbx.voc_synth
    vs.write_text(tree("k10L3"), tmp_path / "a.txt")
    vs.write_text_fast(tree("k10L3"), tmp_path / "b.txt")
    for f in ("a.txt", "b.txt"):
        got, info = load(orbx, tmp_path / f)
        same(got, want("k10L3"), info)
    for name in ("tiny3", "ragged", "k10L3"):          # the getter on a created handle
        V = orbx.Vocabulary(tree(name))
        same(V.tree(), dict(tree(name), desc=np.concatenate([np.zeros((1, 32), np.uint8), tree(name)["desc"][1:]])))
        V.close()


@gpu
def test_trained_vocabulary_through_tree(orbx):
    rng = np.random.default_rng(8)
    d = rng.integers(0, 256, (257, 32), dtype=np.uint8)
    tr = orbx.VocabularyTrainer(3, 2, 257, 4)
    tr.add([d[:64], d[64:128], d[128:200], d[200:]])
    flat = tr.train(seed=1)
    V = tr.vocabulary()
    got = V.tree()
    flat = dict(flat, desc=np.concatenate([np.zeros((1, 32), np.uint8), flat["desc"][1:]]))
    same(got, flat)
    V.close()
    tr.close()


@gpu
@pytest.mark.parametrize("name", ["messy", "messy_nl"])
def test_every_offset(orbx, name):
    """the header padded by 0 .. S spaces, S >= the longest line: every byte of a line meets every chunk and 16-byte boundary, the size takes every
    residue mod 16; the file spans len / CHUNK >= 3 chunks"""
    data, ref = text(name), want(name)
    lines = data.split(b"\n")
    S = max(len(l) for l in lines) + 1
    assert len(data) >= 3 * CHUNK and S > 150 and ref["num_nodes"] == 2380
    assert max(len(l.split()[0]) for l in lines[1:] if l) == 4 and min(len(l.split()[0]) for l in lines[1:] if l) == 1
    assert b"\r\n" in data and b"\t \t" in data
    nl = data.index(b"\n")
    for s in range(S + 1):
        got, info = load(orbx, data[:nl] + b" " * s + data[nl:])
        same(got, ref, info)
        assert info["host_lines"] == 0 and info["waits"] == 1, s


@gpu
def test_line_longer_than_the_overhang_takes_the_host_path(orbx):
    got, info = load(orbx, text("messy_long"))
    same(got, want("messy_long"), info)
    assert info["host_lines"] == vt.device_host_lines(text("messy_long")) == 1 and info["waits"] == 2
    same(want("messy_long"), want("messy"))


@gpu
def test_number_forms(orbx):
    got, info = load(orbx, text("numbers"))
    same(got, want("numbers"), info)
    assert 1 <= info["host_lines"] == vt.device_host_lines(text("numbers"))


@gpu
@pytest.mark.parametrize("name", ["k10L4_repr", "k10L4_g"])
def test_host_lines_cap(orbx, name):
    """a condition, not a measurement: at most 1 % of the lines go to the host, and exactly the lines the restated rule names"""
    got, info = load(orbx, text(name))
    same(got, want(name), info)
    print("%s: host_lines %d of %d" % (name, info["host_lines"], info["num_nodes"] - 1))
    assert info["host_lines"] <= (info["num_nodes"] - 1) // 100
    assert info["host_lines"] == vt.device_host_lines(text(name))


@gpu
@pytest.mark.parametrize("name", ["k10L3_dfs", "k10L3_random"])
def test_line_order(orbx, name):
    data, ref = text(name), want(name)
    sib = np.flatnonzero(ref["parent"][1:] == 0) + 1
    if name == "k10L3_random":
        assert (np.diff(sib) > 1).any()          # siblings interleaved with other parents' children
    V, W = orbx.Vocabulary.from_text(data), orbx.Vocabulary(ref)
    same(V.tree(), ref, V.text_info)
    d = descriptors(name)
    for a, b in zip(V.transform_sorted(d, 2), W.transform_sorted(d, 2)):
        assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()
    V.close()
    W.close()


@gpu
def test_same_handle_either_way(orbx, tmp_path):
    """from_text(path), from_text(bytes) and Vocabulary(voc) on the 11,111-node file: the existing entry points on a loaded handle"""
    data, ref = text("k10L4_repr"), want("k10L4_repr")
    (tmp_path / "v.txt").write_bytes(data)
    vocs = [orbx.Vocabulary.from_text(tmp_path / "v.txt"), orbx.Vocabulary.from_text(data), orbx.Vocabulary(ref)]
    assert [v.size() for v in vocs] == [ref["num_words"]] * 3
    ext = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    kps, desc = ext(orbx.synth_frame(5, 640, 480))
    assert len(desc) > 500
    res = [(v.transform(desc, 2), v.job_transform(ext, 2)) for v in vocs]
    for t, j in res[:2]:
        for a, b in zip(t + j, res[2][0] + res[2][1]):
            assert a.dtype == b.dtype and len(a) == len(b) and (a.view(np.uint8) == b.view(np.uint8)).all()
    for v in vocs:
        v.close()
    ext.close()


@gpu
@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/liborbslam.so not built (needs the reference sources)")
def test_loaded_handle_equals_reference_vocabulary(orbx, tmp_path):
    (tmp_path / "messy.txt").write_bytes(text("messy"))
    ref = oracle_lib.RefVocabulary(tmp_path / "messy.txt")
    V = orbx.Vocabulary.from_text(tmp_path / "messy.txt")
    d = descriptors("messy")
    g = ref.transform(d, 1)
    word, node, weight = V.transform(d, 1)
    assert (word == g["word"]).all() and (node == g["fv_node"]).all() and (_bits(weight) == _bits(g["weight"])).all() and ref.size() == V.size()
    V.close()


@gpu
def test_errors_are_refused_and_a_valid_load_follows(orbx, tmp_path):
    """refusals of bad input, on lines the device parses and on lines forced through the host path; nothing here is out of bounds for a kernel"""
    for name, data, line in error_cases():
        with pytest.raises(orbx.OrbxError) as e:
            orbx.Vocabulary.from_text(data)
        assert e.value.code == ERR_ARG and e.value.text_info["error_line"] == line and ("line %d:" % line) in str(e.value), (name, str(e.value))
    with pytest.raises(orbx.OrbxError) as e:
        orbx.Vocabulary.from_text(tmp_path / "missing.txt")
    assert e.value.code == ERR_ARG and "missing.txt" in str(e.value)
    (tmp_path / "bad.txt").write_bytes(error_cases()[6][1])          # ... and one through the file form
    with pytest.raises(orbx.OrbxError) as e:
        orbx.Vocabulary.from_text(tmp_path / "bad.txt")
    assert e.value.code == ERR_ARG and e.value.text_info["error_line"] == error_cases()[6][2]
    got, info = load(orbx, text("ragged"))
    same(got, want("ragged"), info)
