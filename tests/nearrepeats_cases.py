"""Planted genomes for the near-repeat strata (include/vcfdist_nearrepeats.h): random flanks, fixed seeds, each case small.  A case
is a Case(name, contigs, specs, near, clean, total, min_run): `specs` the (k, m) it runs at (two to four, the first one is the one
it is built for), `near` / `clean` the starts (k, m, contig, start) it declares flagged / not flagged, `total` the exact count of
near-repeated starts per (k, m) where the case pins it, `min_run` a bound the longest run of equal block keys must reach.
tests/test_nearrepeats_model.py checks that every case is what it declares (against the model), the GPU test that the
implementation equals the model on it."""
import itertools
from collections import namedtuple

import numpy as np

import nearrepeats_model as NM

Case = namedtuple("Case", "name contigs specs near clean total min_run")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
BASES = b"ACGT"
PAD = 4                                    # bases on either side of a copy that differ from the original's, so that no shift matches


def rnd(rng, n):
    return bytes(rng.choice(list(BASES), n).tolist()) if n else b""


def rc(s):
    return s.translate(COMP)[::-1]


def mutate(s, positions, rng=None):
    """another base at every position (the next one in ACGT, or a random other one)"""
    s = bytearray(s)
    for p in positions:
        step = 1 if rng is None else int(rng.integers(1, 4))
        s[p] = BASES[(BASES.index(s[p]) + step) % 4]
    return bytes(s)


class Genome:
    """one contig under construction: pieces appended, starts remembered"""

    def __init__(self, rng, flank=40):
        self.rng, self.flank, self.s = rng, flank, bytearray()

    def gap(self, n=None):
        self.s += rnd(self.rng, self.flank if n is None else n)

    def put(self, piece):
        at = len(self.s)
        self.s += piece
        return at

    def pair(self, k, positions, reverse):
        """an original and its copy with the positions mutated (placed reverse-complemented with `reverse`), both inside PAD
        bases that differ pairwise, between random flanks: (start of the original, start of the copy)"""
        ext = rnd(self.rng, k + 2 * PAD)
        cp = mutate(ext, list(range(PAD)) + [PAD + p for p in positions] + list(range(PAD + k, k + 2 * PAD)))
        self.gap()
        a = self.put(ext) + PAD
        self.gap()
        b = self.put(rc(cp) if reverse else cp) + PAD
        return a, b

    def done(self):
        self.gap()
        return bytes(self.s)


def _case(name, contigs, specs, near=(), clean=(), total=None, min_run=0):
    return Case(name, [bytes(c) for c in contigs], list(specs), list(near), list(clean), dict(total or {}), min_run)


def _second_spec(k, m):
    """a companion entry, so that every call has at least two"""
    return (k, m - 1) if m > 0 else (k, 1)


# ---- pos_*: every block border

def position_sets(k, m):
    if m == 1:
        return [(p,) for p in range(k)]
    if m == 2:
        return list(itertools.combinations(range(k), 2))
    bl = NM.blocks(k, m)                               # m = 3: one clean block each, mismatches at the others' first, middle and last base
    out = []
    for clean in range(m + 1):
        rest = [b for j, b in enumerate(bl) if j != clean]
        for pick in (lambda b: b[0], lambda b: (b[0] + b[1]) // 2, lambda b: b[1] - 1):
            out.append(tuple(pick(b) for b in rest))
    out += [(0, 1, k - 1), (0, k - 2, k - 1), (0, 8, 31), (7, 8, 15)]
    return out


def pos_case(k, m, seed):
    rng = np.random.default_rng(seed)
    g = Genome(rng, flank=24)
    near = []
    for pos in position_sets(k, m):
        for reverse in (False, True):
            a, b = g.pair(k, pos, reverse)
            near += [(k, m, 0, a), (k, m, 0, b)]
    return _case(f"pos_k{k}_m{m}", [g.done()], [(k, m), _second_spec(k, m)], near=near)


POS = [(16, 1), (25, 1), (31, 1), (32, 1), (24, 2), (31, 2), (32, 2), (32, 3)]


# ---- over_*: the same copies with m + 1 mismatches: nothing is flagged

def over_sets(k, m):
    bl = NM.blocks(k, m)
    out = []
    for pick in (lambda b: b[0], lambda b: (b[0] + b[1]) // 2, lambda b: b[1] - 1):
        out.append(tuple(pick(b) for b in bl))                                  # one mismatch in every block
    out.append(tuple(b[0] if j % 2 else b[1] - 1 for j, b in enumerate(bl)))
    for b in bl:                                                                # all of them in one block: the others match
        out.append(tuple(range(b[0], b[0] + m + 1)))
        out.append(tuple(range(b[1] - m - 1, b[1])))
    return out


def over_case(k, m, seed):
    rng = np.random.default_rng(seed)
    g = Genome(rng, flank=12 if k == 16 else 24)
    clean = []
    for pos in over_sets(k, m):
        for reverse in (False, True):
            a, b = g.pair(k, pos, reverse)
            clean += [(k, m, 0, a), (k, m, 0, b)]
    return _case(f"over_k{k}_m{m}", [g.done()], [(k, m), _second_spec(k, m)], clean=clean, total={(k, m): 0})


# ---- self_*: a k-mer and its own reverse complement

def self_cases():
    out = []
    rng = np.random.default_rng(701)
    half = rnd(rng, 16)
    pal = half + rc(half)                              # an exact reverse palindrome of 32 bases
    g = Genome(rng)
    g.gap()
    g.put(b"C")                                        # (not the complement of the base behind: the palindrome does not go on)
    a = g.put(pal)
    g.put(b"C")
    specs = [(32, 0), (32, 1), (32, 2), (32, 3)]
    out.append(_case("self_palindrome_once", [g.done()], specs, clean=[(32, m, 0, a) for m in range(4)], total={(32, 0): 0}))
    # one mutated base breaks two positions: distance 2 to its own reverse complement
    for k, seed in ((32, 702), (24, 703)):
        rng = np.random.default_rng(seed)
        half = rnd(rng, k // 2)
        bent = mutate(half + rc(half), [3])
        g = Genome(rng)
        g.gap()
        a = g.put(bent)
        out.append(_case(f"self_bent_once_k{k}", [g.done()], [(k, 2), (k, 1)], clean=[(k, 2, 0, a), (k, 1, 0, a)], total={(k, 1): 0}))
        g = Genome(rng)
        g.gap()
        a = g.put(bent)
        g.gap()
        b = g.put(bent)
        out.append(_case(f"self_bent_twice_k{k}", [g.done()], [(k, 2), (k, 0)],
                         near=[(k, 2, 0, a), (k, 2, 0, b), (k, 0, 0, a), (k, 0, 0, b)]))
    # odd k: X c rc(X) is at distance 1 from its own reverse complement
    rng = np.random.default_rng(704)
    half = rnd(rng, 12)
    odd = half + b"C" + rc(half)
    g = Genome(rng)
    g.gap()
    a = g.put(odd)
    out.append(_case("self_odd_once_k25", [g.done()], [(25, 1), (25, 0)], clean=[(25, 1, 0, a), (25, 0, 0, a)], total={(25, 0): 0}))
    return out


# ---- shift_*: low-complexity tracts whose partners are their own one-base shifts

def shift_cases():
    out = []
    for k in (16, 32):
        for extra in (0, 1):
            rng = np.random.default_rng(800 + k + extra)
            g = Genome(rng)
            g.gap()
            g.put(b"C")
            a = g.put(b"A" * (k + extra))
            g.put(b"G")
            near = [(k, 1, 0, a + d) for d in range(-1, 2 + extra)] + ([(k, 0, 0, a), (k, 0, 0, a + 1)] if extra else [])
            clean = [] if extra else [(k, 0, 0, a)]
            out.append(_case(f"shift_homopolymer_k{k}_plus{extra}", [g.done()], [(k, 1), (k, 0)], near=near, clean=clean,
                             total={(k, 0): 2 * extra}))
    rng = np.random.default_rng(820)
    g = Genome(rng)
    g.gap()
    a = g.put(mutate(b"AC" * 40, [41]))
    out.append(_case("shift_dinucleotide_impure", [g.done()], [(16, 1), (32, 1), (32, 2)],
                     near=[(16, 1, 0, a + 30), (32, 1, 0, a + 20), (32, 2, 0, a + 20)]))
    rng = np.random.default_rng(821)
    poly = b"A" * 20000                                # one run of 20 000 records a strand, all flagged: the early stop
    out.append(_case("shift_polyA_20kb", [rnd(rng, 300), poly], [(32, 1), (24, 2)],
                     near=[(32, 1, 1, 0), (32, 1, 1, 19968), (24, 2, 1, 19976)], total={(32, 1): 20000 - 31, (24, 2): 20000 - 23},
                     min_run=20000 - 31))
    return out


# ---- run_*: R distinct k-mers that share one block's bases, exactly one near pair among them

RUN_R = (63, 64, 65, 255, 256, 257, 4097)
RUN_KM = ((32, 1), (24, 2))


def far_words(rng, n, length, dist):
    """n words of `length` bases, pairwise at Hamming distance >= dist (random candidates, the close ones rejected)"""
    kept = np.zeros(n, np.uint64)
    have = 0
    while have < n:
        cand = rng.integers(0, 1 << (2 * length), 2 * (n - have) + 8, dtype=np.uint64)
        for c in cand:
            if have == n:
                break
            if have == 0 or int(NM.ham(c, kept[:have]).min()) >= dist:
                kept[have] = c
                have += 1
    return [bytes(BASES[(int(v) >> (2 * (length - 1 - j))) & 3] for j in range(length)) for v in kept]


def run_case(k, m, block, R, middle, seed):
    """the k-mers stand alone between Ns, so the valid starts are exactly theirs; all share the bases of `block`, the other bases
    are pairwise at distance >= 2 m + 1, and one of them is swapped for a copy of another with m mutated bases.  The sort is stable,
    so the run's forward records stand in genome order: the pair is its first and last record, or two in its middle."""
    rng = np.random.default_rng(seed)
    b0, b1 = NM.blocks(k, m)[block]
    shared = rnd(rng, b1 - b0)
    words = far_words(rng, R, k - (b1 - b0), 2 * m + 1)
    i, j = (R // 2 - 1, R // 2 + 1) if middle else (0, R - 1)
    words[j] = mutate(words[i], list(range(0, 2 * m, 2)), rng)
    kmers = [w[:b0] + shared + w[b0:] for w in words]
    contig = b"N".join(kmers)
    near = [(k, m, 0, i * (k + 1)), (k, m, 0, j * (k + 1))]
    return _case(f"run_k{k}_m{m}_b{block}_R{R}_{'mid' if middle else 'ends'}", [contig], [(k, m), _second_spec(k, m)], near=near,
                 total={(k, m): 2, (k, m - 1): 0}, min_run=R)


def run_cases():
    out, seed = [], 900
    for k, m in RUN_KM:
        for block in range(m + 1):
            for R in RUN_R:
                for middle in (False, True):
                    seed += 1
                    out.append(run_case(k, m, block, R, middle, seed))
    return out


# ---- strand_*: a pair that exists only across strands

def strand_cases():
    out = []
    rng = np.random.default_rng(1001)
    g = Genome(rng)
    a, b = g.pair(32, (20,), True)                     # the run of g's block 0 holds F(g) and RC(h) alone
    out.append(_case("strand_alone", [g.done()], [(32, 1), (32, 0)], near=[(32, 1, 0, a), (32, 1, 0, b)], total={(32, 1): 2, (32, 0): 0}))
    # the same with 70 forward decoys that share g's block 0 and are far in block 1: the partner's record stands behind them all
    rng = np.random.default_rng(1002)
    orig = rnd(rng, 32)
    tails = far_words(rng, 71, 16, 5)
    kmers = [orig[:16] + t for t in tails[:70]]
    orig = orig[:16] + tails[70]
    pieces = [orig] + kmers + [rc(mutate(orig, [25]))]
    contig = b"N".join(pieces)
    out.append(_case("strand_behind_decoys", [contig], [(32, 1), (32, 0)], near=[(32, 1, 0, 0), (32, 1, 0, 71 * 33)],
                     clean=[(32, 1, 0, 33 * d) for d in range(1, 71)], total={(32, 1): 2, (32, 0): 0}, min_run=72))
    return out


# ---- seam_*, n_*, edge_*

def edge_cases():
    out = []
    k, m = 32, 1
    rng = np.random.default_rng(1101)
    orig = rnd(rng, k)
    cp = mutate(orig, [9])
    c0 = rnd(rng, 100) + orig + rnd(rng, 100) + cp[:16]
    c1 = cp[16:] + rnd(rng, 100)
    out.append(_case("seam_copy_split", [c0, c1], [(k, m), (k, 0)], clean=[(k, m, 0, 100)], total={(k, m): 0}))
    rng = np.random.default_rng(1102)
    orig = rnd(rng, k)
    cp = bytearray(orig); cp[9] = ord("N")
    out.append(_case("n_copy_with_N", [rnd(rng, 100) + orig + rnd(rng, 100) + bytes(cp) + rnd(rng, 100)], [(k, m), (k, 0)],
                     clean=[(k, m, 0, 100)], total={(k, m): 0}))
    rng = np.random.default_rng(1103)
    orig = rnd(rng, k)
    cp, cq = mutate(orig, [0]), rc(mutate(orig, [31]))
    # partners on two contigs; a copy that ends on a contig's last base and one that starts on a contig's first; an empty contig
    # and one of k - 1 bases between them
    contigs = [rnd(rng, 150) + orig + rnd(rng, 150), b"", rnd(rng, 200) + cp, rnd(rng, k - 1), cq + rnd(rng, 200)]
    out.append(_case("edge_two_contigs_ends", contigs, [(k, m), (k, 0), (24, 1)],
                     near=[(k, m, 0, 150), (k, m, 2, 200), (k, m, 4, 0)], total={(k, 0): 0}))
    # starts on either side of the pack's tiles of 4 096 starts: the last start of tile 0 and the first of tile 2
    rng = np.random.default_rng(1104)
    o1, o2 = rnd(rng, k), rnd(rng, k)
    s = rnd(rng, 4095) + o1
    s += rnd(rng, 8192 - len(s)) + o2
    s += rnd(rng, 100) + mutate(o1, [16]) + rnd(rng, 100) + rc(mutate(o2, [15])) + rnd(rng, 50)
    out.append(_case("edge_pack_tiles", [s], [(k, m), (k, 0)],
                     near=[(k, m, 0, 4095), (k, m, 0, 8192), (k, m, 0, 8192 + k + 100), (k, m, 0, 8192 + 2 * k + 200)], total={(k, 0): 0}))
    return out


# ---- mono_*: one genome at m = 0, 1, 2, 3

def mono_genome(seed=1201):
    """copies at 0 to 4 mismatches, forward and reverse-complemented, on two contigs"""
    rng = np.random.default_rng(seed)
    g = Genome(rng)
    starts = {}
    for d in range(5):
        for reverse in (False, True):
            pos = tuple(int(p) for p in sorted(rng.choice(32, d, replace=False)))
            starts[(d, reverse)] = g.pair(32, pos, reverse)
    return [g.done(), rnd(rng, 500)], starts


def mono_case():
    contigs, starts = mono_genome()
    near, clean = [], []
    for (d, _), (a, b) in starts.items():
        for m in range(4):
            (near if d <= m else clean).extend([(32, m, 0, a), (32, m, 0, b)])
    return _case("mono_k32", contigs, [(32, 0), (32, 1), (32, 2), (32, 3)], near=near, clean=clean, total={(32, 0): 4})


MONO_M0_K = (8, 16, 31, 32)


def all_cases():
    out = [pos_case(k, m, 100 + 7 * k + m) for k, m in POS]
    out += [over_case(k, m, 300 + 7 * k + m) for k, m in POS]
    out += self_cases() + shift_cases() + run_cases() + strand_cases() + edge_cases() + [mono_case()]
    return out
