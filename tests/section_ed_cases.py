"""Sync sections with freely chosen strings, for pinning the section edit distance (ref_ed) at its edges.

A truth deletion of X = ref[p : p + nx] with an insertion of Y directly behind it (position p + nx) makes ONE sync section;
its ref_ed is lev(X, Y) for arbitrary X and Y, because whatever flank the section carries is the same bases on both sides.
This module holds the independent reference (`lev`, a plain two-row DP), the trimming rule and the inline rule restated,
a builder that turns (X-spec, Y-spec, seed, query mode) into a contig and a supercluster, and the table of cases by group.
Nothing here touches a GPU, the library or the oracle; tests/test_section_ed_cases.py shows on the CPU that the table is what
it claims, tests/test_gpu_section_ed.py runs it through the kernels.

Lengths in the table are POST-TRIM lengths (nx, ny) = (reference side, truth side): what is left once the common prefix and
then the common suffix are gone, which is what k_ed_bits (pr_ed.hip) sees as pattern and text.  The group `inline_borders` is
the exception: the inline rule of credit_walk looks at the section's own lengths, flank included, so those cases are declared by
SECTION lengths (`sec`); with the query equal to the truth the flank is exactly one base (the matching base behind the insertion),
so nx = rl - 1 and ny = tl - 1."""
from collections import namedtuple

import numpy as np

_BASES = np.frombuffer(b"ACGT", np.uint8)
FLANK = 120             # random bases on either side of the section(s) in a case's contig
SC_MARGIN = 100         # the supercluster region starts / ends this far from the first / last variant


def lev(a: bytes, b: bytes) -> int:
    """Levenshtein distance of two byte strings: two-row DP in int64, a row at a time.  cand[j] = min(up[j] + 1, up[j-1] + (a_i != b_j))
    holds the vertical and diagonal moves; the horizontal move row[j] = min(cand[j], row[j-1] + 1) unrolls to
    row[j] = min_k<=j (cand[k] + j - k) = min.accumulate(cand - j) + j.  Bytes compare as bytes: N == N, a != A."""
    if len(a) < len(b):
        a, b = b, a                     # (symmetric; the shorter string along the row)
    if not b:
        return len(a)
    bv = np.frombuffer(b, np.uint8)
    j = np.arange(len(b) + 1, dtype=np.int64)
    row = j.copy()
    cand = np.empty(len(b) + 1, np.int64)
    for i, ai in enumerate(a, 1):
        cand[0] = i
        np.minimum(row[1:] + 1, row[:-1] + (bv != ai), out=cand[1:])
        row = np.minimum.accumulate(cand - j) + j
    return int(row[-1])


def trimmed(X: bytes, Y: bytes):
    """lengths of (X, Y) once the common prefix and then the common suffix (of what is left) are removed"""
    nx, ny = len(X), len(Y)
    pre = 0
    while pre < nx and pre < ny and X[pre] == Y[pre]:
        pre += 1
    nx -= pre
    ny -= pre
    suf = 0
    while suf < nx and suf < ny and X[len(X) - 1 - suf] == Y[len(Y) - 1 - suf]:
        suf += 1
    return nx - suf, ny - suf


def is_inline(rl: int, tl: int) -> bool:
    """a section (with variants) of rl reference and tl truth bases gets its distance inside the credit walk: an empty side, one
    base each, or the short side up to 32 with the long side up to 256; everything else is deferred to the k_ed kernels"""
    return rl == 0 or tl == 0 or (rl == 1 and tl == 1) or (min(rl, tl) <= 32 and max(rl, tl) <= 256)


# ----------------------------------------------------------------------------------------------------------------------
# strings
# ----------------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return bytearray(rng.choice(_BASES, n).tobytes()) if n else bytearray()


def _other(rng, *avoid):
    return int(rng.choice([c for c in b"ACGT" if c not in avoid]))


def _sprinkle(rng, s, n_n=40):
    """n_n N and one lower-case base, away from the two ends"""
    pos = rng.choice(np.arange(1, len(s) - 1), n_n + 1, replace=False)
    for i in pos[:-1]:
        s[int(i)] = ord("N")
    i = int(pos[-1])
    s[i] = ord(chr(s[i]).lower())
    return s


def _mutate(rng, X, n):
    """X with about 2 % substitutions, three one-base insertions and deletions, and one block inserted or deleted to reach length n"""
    y = bytearray(X)
    for i in np.flatnonzero(rng.random_sample(len(y)) < 0.02):
        y[int(i)] = _other(rng, y[int(i)])
    for _ in range(3 if len(y) > 16 else 0):
        del y[int(rng.randint(1, len(y) - 1))]
        y.insert(int(rng.randint(1, len(y) - 1)), int(rng.choice(_BASES)))
    if n < len(y):
        at = int(rng.randint(1, n)) if n > 1 else 0
        del y[at:at + len(y) - n]
    elif n > len(y):
        at = int(rng.randint(1, len(y) - 1))
        y[at:at] = _rand(rng, n - len(y))
    return y


def _plant(rng, X, n):
    """X with n edits planted: n // 2 substitutions, then n // 4 one-base deletions and as many one-base insertions (same length)"""
    y = bytearray(X)
    for i in rng.choice(np.arange(1, len(y) - 1), n // 2, replace=False):
        y[int(i)] = _other(rng, y[int(i)])
    for _ in range(n // 4):
        del y[int(rng.randint(1, len(y) - 1))]
        y.insert(int(rng.randint(1, len(y) - 1)), int(rng.choice(_BASES)))
    return y


def _differ_at_the_ends(rng, X, y):
    """first and last base of y made unlike X's, so that nothing is trimmed"""
    if X and y:
        if len(y) == 1:
            y[0] = _other(rng, X[0], X[-1])
        else:
            if y[0] == X[0]:
                y[0] = _other(rng, X[0])
            if y[-1] == X[-1]:
                y[-1] = _other(rng, X[-1])
    return y


def make_pair(xspec, yspec, rng):
    """X-spec: ("rand", n) | ("rand_n", n): with 40 N and a lower-case base | ("homo", n): A^n | ("none",)
    Y-spec: ("rand", n) | ("mut", n) | ("mut_n", n): X mutated to length n (then N and lower case); all three unlike X at both ends
            | ("planted", n, k): X with k planted edits, unlike X at both ends | ("x-bases", (i, ...)) / ("x+bases", (i, ...)): X less / plus one base at each i
            | ("x+tail", k): X + k bases | ("x-tail", k): X without its last k | ("homo", n) | ("sub_mid",) | ("sub_ends",) | ("none",)"""
    kx = xspec[0]
    if kx == "rand":
        X = _rand(rng, xspec[1])
    elif kx == "rand_n":
        X = _sprinkle(rng, _rand(rng, xspec[1]))
    elif kx == "homo":
        X = bytearray(b"A" * xspec[1])
    elif kx == "none":
        X = bytearray()
    else:
        raise ValueError(xspec)
    ky = yspec[0]
    if ky == "rand":
        Y = _differ_at_the_ends(rng, X, _rand(rng, yspec[1]))
    elif ky == "mut":
        Y = _differ_at_the_ends(rng, X, _mutate(rng, X, yspec[1]))
    elif ky == "mut_n":
        Y = _differ_at_the_ends(rng, X, _sprinkle(rng, _mutate(rng, X, yspec[1])))
    elif ky == "planted":           # ("planted", n, k): length n == len(X), at most k + 2 edits away from X
        assert yspec[1] == len(X)
        Y = _differ_at_the_ends(rng, X, _plant(rng, X, yspec[2]))
    elif ky == "x-bases":           # ("x-bases", (i, ...)): X without its bases i, ..., each made unlike both neighbours (the gap cannot move)
        for i in yspec[1]:
            X[i] = _other(rng, X[i - 1], X[i + 1])
        Y = bytearray(c for i, c in enumerate(X) if i not in yspec[1])
    elif ky == "x+bases":           # ("x+bases", (i, ...)): X with one more base in front of its bases i, ..., unlike both neighbours
        Y = bytearray()
        for i, c in enumerate(X):
            if i in yspec[1]:
                Y.append(_other(rng, X[i - 1], c))
            Y.append(c)
    elif ky == "x+tail":
        Y = X + _rand(rng, yspec[1])
    elif ky == "x-tail":
        Y = X[:len(X) - yspec[1]]
    elif ky == "homo":
        Y = bytearray(b"A" * yspec[1])
    elif ky == "sub_mid":
        Y = bytearray(X)
        Y[len(Y) // 2] = _other(rng, Y[len(Y) // 2])
    elif ky == "sub_ends":
        Y = bytearray(X)
        Y[0], Y[-1] = _other(rng, Y[0]), _other(rng, Y[-1])
    elif ky == "none":
        Y = bytearray()
    else:
        raise ValueError(yspec)
    return bytes(X), bytes(Y)


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
# pairs: ((X-spec, Y-spec), ...), one per section (more than one: `packed`, one matching base between consecutive sections)
# trim: the declared post-trim lengths of each pair; deferred: how many of the sections the k_ed kernels get
# sec: the declared section lengths (inline_borders only)
Case = namedtuple("Case", "name pairs seed mode trim deferred sec")
Built = namedtuple("Built", "case contig sc pairs var_pair pos")
# Built.pairs: [(X, Y)]; Built.var_pair[k]: which pair the k-th truth variant of the supercluster belongs to; Built.pos[i]: where
# pair i's X begins in the contig

TYPE_INS, TYPE_DEL = 2, 3       # include/vcfdist_pr.h (asserted against the ABI in tests/test_section_ed_cases.py)


def build(case, ctg=0):
    """-> Built: the contig (str), the supercluster dict for Variants.from_sites, the (X, Y) pairs and the truth variants' pairs.
    Mode `same`: the query equals the truth (distance 0: the lane levels emit the jobs); `near`: the query's deletion lacks a few
    bases at either end and its insertion a few at the end (the window or dense levels emit them); `fn`: the query has no variant
    at all (its haplotypes are the reference; every truth variant is a false negative)."""
    rng = np.random.RandomState(case.seed)
    pairs = [make_pair(xs, ys, rng) for xs, ys in case.pairs]
    homo = any(xs[0] == "homo" for xs, _ in case.pairs)
    left = _rand(rng, FLANK) + (bytearray(b"A" * 6) if homo else bytearray())
    right = (bytearray(b"A" * 6) if homo else bytearray()) + _rand(rng, FLANK)
    contig = bytearray(left)
    t, q, var_pair, pos = [], [], [], []
    for k, (X, Y) in enumerate(pairs):
        if k:
            contig += _rand(rng, 1)             # the one matching base between two sections
        p = len(contig)
        pos.append(p)
        contig += X
        nx, ny = len(X), len(Y)
        cut = min(5, (nx - 1) // 4) if case.mode == "near" else 0
        short = min(20, ny // 4) if case.mode == "near" else 0
        if nx:
            t.append((p, TYPE_DEL, X.decode(), "", 40.0))
            if case.mode != "fn":
                q.append((p + cut, TYPE_DEL, X[cut:nx - cut].decode(), "", 30.0))
            var_pair.append(k)
        if ny:
            t.append((p + nx, TYPE_INS, "", Y.decode(), 40.0))
            if case.mode != "fn":
                q.append((p + nx, TYPE_INS, "", Y[:ny - short].decode(), 30.0))
            var_pair.append(k)
    end = len(contig)
    contig += right
    sc = dict(ctg=ctg, beg=len(left) - SC_MARGIN, end=end + SC_MARGIN, vars=[q, q, t, t])
    return Built(case, contig.decode(), sc, pairs, var_pair, pos)


def build_group(cases):
    """one batch's worth: -> (contigs, superclusters, [Built]), a contig and a supercluster per case"""
    built = [build(c, ctg=i) for i, c in enumerate(cases)]
    return [b.contig for b in built], [b.sc for b in built], built


def _one(name, xs, ys, seed, mode, trim, deferred=True, sec=None):
    return Case(name, ((xs, ys),), seed, mode, (trim,), int(deferred), sec)


def _rr(nx, ny, seed, mode, y="rand", x="rand"):
    return _one(f"{x}{nx}_{y}{ny}_{mode}", (x, nx), (y, ny), seed, mode, (nx, ny))


def _inline_borders():
    out = []
    for k, (rl, tl) in enumerate([(32, 32), (32, 33), (33, 32), (33, 33), (32, 256), (256, 32), (32, 257), (257, 32), (33, 256),
                                  (256, 33), (33, 257), (257, 33)]):
        out.append(_one(f"sec{rl}x{tl}", ("rand", rl - 1), ("rand", tl - 1), 1000 + k, "same", (rl - 1, tl - 1),
                        deferred=not (min(rl, tl) <= 32 and max(rl, tl) <= 256), sec=(rl, tl)))
    return out


def _empty_and_trim():
    out = []
    for k, mode in enumerate(("same", "near")):
        s = 2000 + 20 * k
        out += [
            _one(f"ins257_{mode}", ("none",), ("rand", 257), s, mode, (0, 257)),            # empty reference segment
            _one(f"ins300_{mode}", ("none",), ("rand", 300), s + 1, mode, (0, 300)),
            _one(f"del257_{mode}", ("rand", 257), ("none",), s + 2, mode, (257, 0)),        # empty truth segment
            _one(f"del300_{mode}", ("rand", 300), ("none",), s + 3, mode, (300, 0)),
            _one(f"x_plus_tail_{mode}", ("rand", 300), ("x+tail", 40), s + 4, mode, (0, 40)),       # the trim eats X whole
            _one(f"x_minus_tail_{mode}", ("rand", 300), ("x-tail", 40), s + 5, mode, (40, 0)),      # ... Y whole
            _one(f"homopolymer_{mode}", ("homo", 300), ("homo", 299), s + 6, mode, (1, 0)),
            _one(f"sub_mid_{mode}", ("rand", 300), ("sub_mid",), s + 7, mode, (1, 1)),
            _one(f"sub_ends_{mode}", ("rand", 300), ("sub_ends",), s + 8, mode, (300, 300)),
        ]
    return out


def _one_group():
    out = []
    s = 3000
    modes = ("same", "near")
    for m in (63, 64, 65, 127, 128):
        out.append(_rr(m, 40, s, modes[s & 1])); s += 1
        out.append(_rr(m, m, s, modes[s & 1])); s += 1
        out.append(_rr(m, m - 1, s, modes[s & 1], y="mut")); s += 1
    for m in (4095, 4096):
        out.append(_rr(m, 40, s, modes[s & 1])); s += 1
        out.append(_rr(m, m, s, modes[s & 1], y="mut")); s += 1
    out += [
        _rr(40, 64, s + 1, "near"), _rr(40, 4096, s + 2, "same"),        # the long string on the truth side
        _rr(4096, 4000, s + 3, "same"),                                  # random, high distance
        _rr(128, 2000, s + 4, "near"), _rr(2000, 128, s + 5, "same"),    # steps(): the longer string is the pattern on either side
        _rr(64, 65, s + 6, "same"), _rr(65, 64, s + 7, "near"),          # steps(64, 65) == steps(65, 64) == 65: no swap
    ]
    return out


def _multi_group():
    out = []
    s = 4000
    modes = ("same", "near")
    for n in (1, 31, 32, 33, 63, 64, 65, 100):
        out.append(_rr(4097, n, s, modes[s & 1])); s += 1
    out += [
        _rr(4097, 4097, s + 1, "near", y="mut"),
        _rr(8192, 200, s + 2, "same"),                      # exactly two groups: last_bit 63, the tap is lane 63
        _rr(8192, 4200, s + 3, "same", y="mut"),            # (8 192 x 8 192 costs the CPU oracle 2 s: the text shrunk, the pattern not)
        _rr(8193, 200, s + 4, "near"),                      # three groups, one block in the third; the middle group reads and writes planes
        _rr(5000, 4200, s + 5, "same", y="mut"),
        _rr(4500, 4600, s + 6, "near", y="mut_n", x="rand_n"),       # 40 N and a lower-case base on each side
        _rr(100, 4097, s + 7, "same"),                      # the long string on the truth side
    ]
    return out


def _packed():
    a33 = (("rand", 33), ("rand", 33))
    return [
        Case("40x33x33", (a33,) * 40, 5000, "same", ((33, 33),) * 40, 40, None),
        Case("12_alternating_33x33_1x257", (a33, (("rand", 1), ("rand", 257))) * 6, 5001, "same", ((33, 33), (1, 257)) * 6, 12, None),
        Case("12_alternating_257x1_33x33", ((("rand", 257), ("rand", 1)), a33) * 6, 5002, "same", ((257, 1), (33, 33)) * 6, 12, None),
    ]


GROUPS = {
    "inline_borders": _inline_borders(),
    "empty_and_trim": _empty_and_trim(),
    "one_group": _one_group(),
    "multi_group": _multi_group(),
    "packed": _packed(),
}
