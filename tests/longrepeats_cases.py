"""Inputs of tests/test_gpu_longrepeats.py, built without a GPU so that tests/test_longrepeats_model.py can check on the CPU that
they hold what the GPU tests are about (tests/longrepeats_model.py is the specification of both).

Every case is a small seeded genome (random contigs of 4 kb or more, so that no 33-mer repeats by chance) into which words are
planted, and it declares the tracts (slop 0) the plants must give.  The bases next to a plant are set so that no copy is a base
longer by chance: the declared tracts are exact."""
import numpy as np

from vcfdist_amd import _abi as A

K = (33, 40, 63, 64, 65, 100, 127, 128, 129, 250, 256)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
BASE = 32                                              # the base level of the rank doubling (include/vcfdist_longrepeats.h)


def revcomp(s):
    return s.translate(COMP)[::-1]


def rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))


def levels(k):
    """[(a, b)] of the schedule 32 -> 64 -> 128 -> k without the levels above k"""
    out, a = [], BASE
    while 2 * a < k:
        out.append((a, 2 * a))
        a *= 2
    return out + [(a, k)]


def hairpin_deltas(k):
    """The lengths k + delta of the reverse palindromes of the hairpin case: every level's d = b - a, and every delta at which the
    palindromic a-mer in the middle of the palindrome is one of the halves that the k-mer at its first base is built from (the
    a-mer at offset o is the middle one iff 2 o + a == k + delta).  A reverse palindrome has an even length."""
    lv = levels(k)
    out = {b - a for a, b in lv}
    words = {k: {0}}                                   # length -> offsets of the words of that length under the k-mer at 0
    for a, b in reversed(lv):
        words[a] = {o + x for o in words[b] for x in (0, b - a)}
    for a, _ in lv:
        out |= {2 * o + a - k for o in words[a]}
    return sorted(d for d in out if 1 <= d <= k and (k + d) % 2 == 0)


class Genome:
    """contigs under construction, and the tracts their plants declare"""

    def __init__(self, seed, lengths):
        self.rng = np.random.RandomState(seed)
        self.ctg = [bytearray(rand(self.rng, n)) for n in lengths]
        self.tracts = [[] for _ in lengths]

    def r(self, n):
        return rand(self.rng, n)

    def put(self, c, at, w, before=None, after=None):
        """w at [at, at + len(w)) of contig c; the base in front and the base behind are set where given"""
        s = self.ctg[c]
        assert 0 <= at and at + len(w) <= len(s)
        s[at:at + len(w)] = w
        if before is not None and at > 0:
            s[at - 1:at] = before
        if after is not None and at + len(w) < len(s):
            s[at + len(w):at + len(w) + 1] = after

    def declare(self, c, a, b):
        self.tracts[c].append((a, b))

    def case(self, empty=False):
        rows = []
        for t in self.tracts:
            merged = []
            for a, b in sorted(t):
                if merged and a <= merged[-1][1]:
                    merged[-1] = (merged[-1][0], max(merged[-1][1], b))
                else:
                    merged.append((a, b))
            rows.append(merged)
        assert empty == (not any(rows))
        return {"contigs": [bytes(s) for s in self.ctg], "tracts": rows, "empty": empty}

    # a forward copy cannot grow: the bases in front differ, and so do the bases behind
    def forward(self, k, c1, p1, c2, p2, w):
        self.put(c1, p1, w, b"A", b"A")
        self.put(c2, p2, w, b"C", b"C")
        if len(w) >= k:
            self.declare(c1, p1, p1 + len(w)); self.declare(c2, p2, p2 + len(w))

    # a reverse-complemented copy grows iff the base in front of one is the complement of the base behind the other
    def reverse(self, k, c1, p1, c2, p2, w):
        self.put(c1, p1, w, b"A", b"A")
        self.put(c2, p2, revcomp(w), b"A", b"A")
        if len(w) >= k:
            self.declare(c1, p1, p1 + len(w)); self.declare(c2, p2, p2 + len(w))


def palindrome(rng, n):
    """a word of n bases (n even) that is its own reverse complement"""
    assert n % 2 == 0
    half = rand(rng, n // 2)
    return half + revcomp(half)


def cases(k):
    """{name: {"contigs": [bytes], "tracts": [[(start, stop)] per contig], "empty": bool}} for a k-mer length k"""
    out = {}
    step = k + 300                                     # plants lie a slot apart: none is longer than 2 k

    # forward copies of k - 1 (none repeated), k and k + 1 bases, a copy with an N in it, reverse-complemented copies on the second
    # contig, a copy on another contig
    g = Genome(1000 + k, (4200 + 8 * step, 4200 + 7 * step))
    for i, n in enumerate((k - 1, k, k + 1)):
        g.forward(k, 0, 100 + 2 * i * step, 0, 100 + (2 * i + 1) * step, g.r(n))
        g.reverse(k, 1, 100 + 2 * i * step, 1, 100 + (2 * i + 1) * step, g.r(n))
    w = g.r(k + 20)                                    # the second copy has an N at offset 10: the starts 11..20 are left in both
    p1, p2 = 100 + 6 * step, 100 + 7 * step
    g.put(0, p1, w, b"A", b"A")
    g.put(0, p2, w[:10] + b"N" + w[11:], b"C", b"C")
    g.declare(0, p1 + 11, p1 + k + 20); g.declare(0, p2 + 11, p2 + k + 20)
    g.forward(k, 0, 4150 + 7 * step, 1, 100 + 6 * step, g.r(k + 7))
    out["copies"] = g.case()

    # overlapping occurrences: a homopolymer of k + 1 bases (both starts), a period-3 tract of k + 5 bases (all six starts)
    g = Genome(2000 + k, (4200 + 2 * step,))
    g.put(0, 500, b"A" * (k + 1), b"C", b"C")
    g.declare(0, 500, 500 + k + 1)
    g.put(0, 500 + step, (b"ACG" * (k // 3 + 3))[:k + 5], b"T", b"T")
    g.declare(0, 500 + step, 500 + step + k + 5)
    out["overlap"] = g.case()

    # the hairpin: a reverse palindrome of k + delta bases placed once.  Its k-mers at x and delta - x are reverse complements of
    # each other at different starts -- repeated, all but the middle one -- and the a-mer they share is its own reverse complement
    # and occurs nowhere else.  One case per delta, so that a failure names it.
    for d in hairpin_deltas(k):
        g = Genome(3000 + 7 * k + d, (4200 + 2 * k,))
        g.put(0, 2000, palindrome(g.rng, k + d), b"A", b"A")
        g.declare(0, 2000, 2000 + k + d)
        out[f"hairpin_{d}"] = g.case()
    if k % 2 == 0:                                     # a palindromic k-mer placed once is not repeated (odd k has none)
        g = Genome(4000 + k, (4200 + k,))
        g.put(0, 2000, palindrome(g.rng, k), b"A", b"A")
        out["palindrome_once"] = g.case(empty=True)

    # a copy cut by a contig seam: its halves u (k + 3 bases, the end of contig 0) and v (k + 2 bases, the start of contig 1) are
    # copies of the halves of the whole word further on; the k-mers across the seam do not exist
    g = Genome(5000 + k, (4200 + k, 4600 + 3 * k))
    u, v = g.r(k + 3), g.r(k + 2)
    L0 = len(g.ctg[0])
    g.put(0, L0 - len(u), u, b"A")
    g.put(1, 0, v, None, b"A")
    g.put(1, 2000, u + v, b"C", b"C")
    g.declare(0, L0 - len(u), L0); g.declare(1, 0, len(v)); g.declare(1, 2000, 2000 + len(u) + len(v))
    out["seam"] = g.case()
    # the a-mer that ends exactly at the seam, in front of a level with d == a: u (a bases) ends contig 0, v (k - a bases) begins
    # contig 1, and u + v is one k-mer further on.  Both halves are kept (they occur twice), the k-mer across the seam does not
    # exist, and the whole word occurs once: nothing is repeated.
    for a, b in levels(k):
        if b - a == a:
            g = Genome(6000 + 3 * k + a, (4200, 4600 + k))
            u, v = g.r(a), g.r(k - a)
            g.put(0, 4200 - a, u, b"A")
            g.put(1, 0, v, None, b"A")
            g.put(1, 2000, u + v, b"C", b"C")
            out[f"seam_exact_{a}"] = g.case(empty=True)

    # contigs shorter than 32, empty, shorter than k, of exactly k bases (its one k-mer has a copy: the tract is the whole contig)
    g = Genome(7000 + k, (20, 0, k - 1, k, 4200 + k, 31))
    g.put(4, 1000, bytes(g.ctg[3]), b"A", b"A")
    g.declare(3, 0, k); g.declare(4, 1000, 1000 + k)
    out["lengths"] = g.case()

    # copies that straddle the global positions 4096 and 8192 (tiles of the pack and of the pair kernels)
    g = Genome(8000 + k, (12400,))
    n = k + 9
    g.forward(k, 0, 4096 - n // 2, 0, 1000, g.r(n))
    g.reverse(k, 0, 8192 - n // 2, 0, 11000, g.r(n))
    out["tiles"] = g.case()
    return out


def specs_of(k, name):
    """the entries of the GPU call on a case: slop 0 and 5 at k, and on the case "copies" six other lengths in front of them, in
    falling order -- VPR_LREP_MAX_SPEC entries that share the base level and the levels 64 and 128"""
    own = [A.rep_kmer(k, 0), A.rep_kmer(k, 5)]
    if name != "copies":
        return own
    others = [x for x in K if x != k]
    return [A.rep_kmer(x, 0) for x in sorted((others[i] for i in (0, 2, 4, 6, 8, 9)), reverse=True)] + own


# ---- the command lines: a small planted FASTA and a handful of variants

CLI_SITES = {"chrA": (500, 1100, 3100, 5050, 6500), "chrB": (200, 1600, 3600)}        # 0-based SNP positions of the truth set
CLI_MISSED, CLI_EXTRA = ("chrA", 3100), ("chrA", 2000)                                 # not in the query set / only in it


def cli_inputs():
    """-> (contig names, contigs) of a two-contig FASTA of about 12 kb with forward and reverse-complemented copies of 300 bases,
    so that every default stratum (k = 64, 100, 250) has intervals on both contigs, and two copies of 120 bases (none at 250).  The
    sites at 1100, 3100, 1600 and 3600 lie inside a copy of 300 bases, the one at 5050 inside a copy of 120, the others in none."""
    g = Genome(99, (7000, 5000))
    g.forward(250, 0, 1000, 1, 1500, g.r(300))
    g.reverse(250, 0, 3000, 1, 3500, g.r(300))
    g.forward(250, 0, 5000, 0, 6000, g.r(120))
    return ["chrA", "chrB"], [bytes(s) for s in g.ctg]


def cli_vcf(names, contigs, query):
    """the text of the truth (query false) or the query VCF: heterozygous phased SNPs at the sites"""
    out = ["##fileformat=VCFv4.2"] + [f"##contig=<ID={n},length={len(c)}>" for n, c in zip(names, contigs)]
    out += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1"]
    for n, c in zip(names, contigs):
        sites = set(CLI_SITES[n])
        if query:
            sites = (sites - {CLI_MISSED[1]} if CLI_MISSED[0] == n else sites) | ({CLI_EXTRA[1]} if CLI_EXTRA[0] == n else set())
        for p in sorted(sites):
            ref = chr(c[p])
            out.append(f"{n}\t{p + 1}\t.\t{ref}\t{'ACGT'['ACGT'.index(ref) - 3]}\t30\tPASS\t.\tGT\t0|1")
    return "\n".join(out) + "\n"
