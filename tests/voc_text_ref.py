"""CPU restatement of the DBoW2 text vocabulary parse (orbx_vocabulary_load_text, orbx_voc_text_parse_host) and the files its tests share.

parse(data): split at '\\n', split(), int(), float().  Python's float() is correctly rounded, so it is the double glibc's strtod - and with it the
reference's `istream >> double` (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1406) - gives.  Same grammar and same refusals as include/orbx.h
states; format errors come before structure errors, each kind at its first line.

device_weight(token): the device's accept / flag rule for a weight token, restated with Python integers: at most 19 significant digits, the
Eisel-Lemire product against 128-bit powers of five computed here from scratch (not read from the library's table), flagged where the rounding is
not proven.  Returns the double or None (flagged)."""
import re
import struct

import numpy as np

INT_RE = re.compile(rb"[+-]?[0-9]+\Z")
WEIGHT_RE = re.compile(rb"([+-]?)([0-9]*)(?:(\.)([0-9]*))?(?:[eE]([+-]?[0-9]+))?\Z")
CHUNK, OVERHANG = 16384, 1024          # VT_CHUNK, VT_OVER of csrc/orbx_voc_text.hip


class FormatError(Exception):
    def __init__(self, line, msg):
        super().__init__("line %d: %s" % (line, msg))
        self.line = line


def _int(tok, line, what):
    if not INT_RE.match(tok) or not -2 ** 31 <= int(tok) < 2 ** 31:
        raise FormatError(line, what + " is not an integer")
    return int(tok)


def weight_of(tok):
    """float(token) for a token of the weight grammar, None otherwise"""
    m = WEIGHT_RE.match(tok)
    if not m or not (m.group(2) or m.group(4)):
        return None
    return float(tok)


def parse(data):
    """-> voc_synth's dict + k, L, scoring, weighting, num_words, final_newline, error_line = 0; raises FormatError"""
    data = bytes(data)
    if not data:
        raise FormatError(1, "empty")
    pieces = data.split(b"\n")
    final_newline = int(data.endswith(b"\n"))
    if final_newline:
        pieces.pop()
    head = pieces[0].split()
    if len(head) < 4:
        raise FormatError(1, "header")
    k, L, scoring, weighting = [_int(t, 1, "header field") for t in head[:4]]
    if not (1 <= k <= 20 and 1 <= L <= 10 and 0 <= scoring <= 5 and 0 <= weighting <= 3):
        raise FormatError(1, "header out of range")
    if len(pieces) < 2:
        raise FormatError(1, "no node lines")
    n = len(pieces)
    parent, leaf, desc, weight = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.float64)
    for i in range(1, n):
        t = pieces[i].split()
        if len(t) < 35:
            raise FormatError(i + 1, "too few tokens")
        parent[i] = _int(t[0], i + 1, "parent")
        leaf[i] = _int(t[1], i + 1, "isLeaf") > 0
        for j in range(32):
            v = _int(t[2 + j], i + 1, "descriptor byte")
            if not 0 <= v <= 255:
                raise FormatError(i + 1, "descriptor byte outside 0..255")
            desc[i, j] = v
        w = weight_of(t[34])
        if w is None:
            raise FormatError(i + 1, "weight")
        weight[i] = w
    nchild = np.zeros(n, np.int64)
    for i in range(1, n):
        p = int(parent[i])
        if p < 0 or p >= i:
            raise FormatError(i + 1, "parent must be a smaller node id")
        if leaf[p]:
            raise FormatError(i + 1, "hangs under a leaf")
        nchild[p] += 1
    for i in range(n):
        if not (i > 0 and leaf[i]) and nchild[i] == 0:
            raise FormatError(i + 1, "inner node without children")
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, num_nodes=n, num_words=int(leaf[1:].sum()), final_newline=final_newline, error_line=0,
                parent=parent, is_leaf=leaf, desc=desc, weight=weight)


# ---- the device's accept rule ------------------------------------------------------------------------------------------------------------
def pow5_128(q):
    if q >= 0:
        p = 5 ** q
        while p < (1 << 127):
            p *= 2
        while p >= (1 << 128):
            p //= 2
        return p
    p = 5 ** -q
    z = 0
    while (1 << z) < p:
        z += 1
    c = (1 << (z + 127 if q >= -27 else 2 * z + 128)) // p + 1
    while c >= (1 << 128):
        c //= 2
    return c


_POW5 = {}
M64 = (1 << 64) - 1


def eisel_lemire(w, q):
    """w * 10^q (0 < w < 2^64, -342 <= q <= 308) -> the double's bits, or None: not proven"""
    if q not in _POW5:
        _POW5[q] = pow5_128(q)
    lz = 64 - w.bit_length()
    w <<= lz
    p5hi, p5lo = _POW5[q] >> 64, _POW5[q] & M64
    prod = w * p5hi
    lo, hi = prod & M64, prod >> 64
    if hi & 0x1ff == 0x1ff:
        shi = (w * p5lo) >> 64
        lo = (lo + shi) & M64
        if shi > lo:
            hi += 1
    if lo == M64 and (q < -27 or q > 55):
        return None
    upperbit = hi >> 63
    shift = upperbit + 9
    m = hi >> shift
    power2 = ((217706 * q) >> 16) + 63 + upperbit - lz + 1023
    if power2 <= 0:
        return None
    if lo <= 1 and -4 <= q <= 23 and m & 3 == 1 and (m << shift) == hi:
        return None
    m += m & 1
    m >>= 1
    if m >= (2 << 52):
        m = 1 << 52
        power2 += 1
    m &= ~(1 << 52)
    if power2 >= 0x7ff:
        return None
    return m | (power2 << 52)


def device_weight(tok):
    m = WEIGHT_RE.match(tok)
    if not m or not (m.group(2) or m.group(4)):
        return None
    w = nd = q = 0
    over = False
    for c in m.group(2):
        if w or c != 48:
            if nd < 19:
                w, nd = w * 10 + c - 48, nd + 1
            else:
                over = True
    for c in m.group(4) or b"":
        if w or c != 48:
            if nd < 19:
                w, nd, q = w * 10 + c - 48, nd + 1, q - 1
            else:
                over = True
        else:
            q -= 1
    if m.group(5):
        q += int(m.group(5))
    if over:
        return None
    sign = 1 << 63 if m.group(1) == b"-" else 0
    if w == 0:
        bits = sign
    else:
        if not -342 <= q <= 308:
            return None
        bits = eisel_lemire(w, q)
        if bits is None:
            return None
        bits |= sign
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def device_flags_line(line, start=1, size=None):
    """does the device flag this (well-formed) node line, which starts at byte `start` of a text of `size` bytes?  Plain unsigned tokens of at most
    9 / 9 / 3 digits, a weight it proves, and the weight token must end inside the bytes staged for the chunk that holds the newline in front of
    the line: CHUNK + OVERHANG bytes from the chunk's first (a line of up to OVERHANG - 1 bytes always does)."""
    t = line.split()
    if len(t) < 35:
        return True
    if not (t[0].isdigit() and len(t[0]) <= 9 and t[1].isdigit() and len(t[1]) <= 9):
        return True
    if not all(x.isdigit() and len(x) <= 3 and int(x) <= 255 for x in t[2:34]):
        return True
    if device_weight(t[34]) is None:
        return True
    at = 0
    for x in t[:35]:          # the offset behind the weight token
        at = line.index(x, at) + len(x)
    staged_end = (start - 1) // CHUNK * CHUNK + CHUNK + OVERHANG
    return size is not None and staged_end < size and start + at >= staged_end


def device_host_lines(data):
    data = bytes(data)
    pieces = data.split(b"\n")
    if data.endswith(b"\n"):
        pieces.pop()
    n, start = 0, len(pieces[0]) + 1
    for p in pieces[1:]:
        n += device_flags_line(p, start, len(data))
        start += len(p) + 1
    return n


# ---- trees and files -----------------------------------------------------------------------------------------------------------------------
def tiny3():
    """k = 2, L = 1: the root and two words"""
    d = np.zeros((3, 32), np.uint8)
    d[1], d[2] = np.arange(32), 255 - np.arange(32)
    return dict(k=2, L=1, parent=np.array([0, 0, 0], np.int32), is_leaf=np.array([0, 1, 1], np.uint8), desc=d, weight=np.array([0.0, 1.25, 0.1]), num_nodes=3)


def renumber(voc, order):
    """the same tree with node order[i] renamed i (order[0] == 0, every parent in front of its children)"""
    order = np.asarray(order)
    pos = np.zeros(len(order), np.int64)
    pos[order] = np.arange(len(order))
    out = dict(voc)
    out["parent"] = pos[voc["parent"][order]].astype(np.int32)
    for key in ("is_leaf", "desc", "weight"):
        out[key] = voc[key][order].copy()
    assert out["parent"][0] == 0 and (out["parent"][1:] < np.arange(1, len(order))).all()
    return out


def _children(voc):
    ch = [[] for _ in range(voc["num_nodes"])]
    for i in range(1, voc["num_nodes"]):
        ch[int(voc["parent"][i])].append(i)
    return ch


def dfs_order(voc):
    ch, order, stack = _children(voc), [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        stack.extend(reversed(ch[i]))
    return order


def random_order(voc, seed):
    """a random order that keeps parent < id: siblings end up interleaved with other parents' children"""
    rng = np.random.default_rng(seed)
    ch, order, avail = _children(voc), [0], list(_children(voc)[0])
    while avail:
        j = int(rng.integers(len(avail)))
        avail[j], avail[-1] = avail[-1], avail[j]
        i = avail.pop()
        order.append(i)
        avail.extend(ch[i])
    return order


def text_of(voc, weight_fmt=repr, scoring=0, weighting=0, final_newline=False, tokens=None):
    """write_text's file as bytes; weight_fmt formats a float; tokens: weight tokens used instead, node i takes tokens[(i - 1) % len]"""
    lines = ["%d %d %d %d" % (voc["k"], voc["L"], scoring, weighting)]
    for i in range(1, voc["num_nodes"]):
        w = tokens[(i - 1) % len(tokens)] if tokens else weight_fmt(float(voc["weight"][i]))
        lines.append("%d %d %s %s" % (voc["parent"][i], voc["is_leaf"][i], " ".join(str(int(b)) for b in voc["desc"][i]), w))
    return ("\n".join(lines) + ("\n" if final_newline else "")).encode()


def messy_text(voc, seed, final_newline=False, header_pad=0):
    """random separator runs (1 - 4 of space or tab), leading and trailing separators on some lines, CRLF on a fifth of them"""
    rng = np.random.default_rng(seed)

    def sep():
        return "".join(" \t"[int(c)] for c in rng.integers(0, 2, int(rng.integers(1, 5))))
    lines = ["%d %d 0 0" % (voc["k"], voc["L"]) + " " * header_pad]
    for i in range(1, voc["num_nodes"]):
        t = [str(int(voc["parent"][i])), str(int(voc["is_leaf"][i]))] + [str(int(b)) for b in voc["desc"][i]] + [repr(float(voc["weight"][i]))]
        s = "".join(x + sep() for x in t[:-1]) + t[-1]
        r = rng.random()
        if r < 0.2:
            s = sep() + s
        if 0.1 < r < 0.3:
            s = s + sep()
        if rng.random() < 0.2:
            s += "\r"
        lines.append(s)
    return ("\n".join(lines) + ("\n" if final_newline else "")).encode()


NUMBER_FORMS = ["0", "0.0", "-0.0", "+3.5", ".5", "5.", "1e-05", "1E+2", "%g" % 3.14159265, "%g" % 0.000123456, "%g" % 8.76543, repr(0.1), repr(2.0 / 3.0), repr(8.123456789012345),
                "4.9e-324", "2.2250738585072014e-308", "1.7976931348623157e308", "9007199254740993", "123456789012345678901234567890", "0.000000000000000000000000001",
                "1." + str(5 ** 53).zfill(53)]          # the last: 1 + 2^-53 = 1 + 5^53 / 10^53, the exact midpoint between 1 and 1 + 2^-52 (53 decimals)
