"""Inputs of tests/test_gpu_repeats.py, built without a GPU so that tests/test_repeats_model.py can check on the CPU that they
hold what the GPU tests are about (tests/repeats_model.py is the specification of both)."""
import os

import numpy as np

import repeats_model as RM
from vcfdist_amd import _abi as A

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))


# ---- 1. hand genomes (a few contigs of up to ~200 bases), built for one k each

HAND_K = (4, 5, 31, 32)
HAND_SPECS = [A.rep_kmer(k, slop) for k in HAND_K for slop in (0, 3)]          # VPR_REP_MAX_SPEC entries


def hand_cases(k):
    """{name: contigs (bytes)} for a k-mer length k; what each one is about is asserted in tests/test_repeats_model.py"""
    rng = np.random.RandomState(100 + k)
    r = lambda n: rand(rng, n)
    cases = {}
    w = r(k)
    # a contig shorter than k, one of exactly k bases (whose one k-mer has a forward copy on another contig: its tract is the whole
    # contig), and an empty contig between two others
    cases["lengths"] = [r(k - 1), w, b"", r(k + 5) + w + r(7)]
    cases["n_invalidates_k"] = [r(2 * k) + b"N" + r(2 * k)]
    w = r(k + 3)
    cases["forward"] = [r(9) + w + r(k + 1) + w + r(5), r(k) + w + r(11)]
    cases["revcomp"] = [r(9) + w + r(6), r(k + 2) + revcomp(w) + r(k)]
    half = r((k + 1) // 2)
    pal = half + revcomp(half)[k % 2:]                 # even k: a palindrome (its own reverse complement); odd k has none
    cases["palindrome_once"] = [r(k + 3) + pal + r(k + 2)]
    cases["palindrome_twice"] = [r(k + 3) + pal + r(k + 2) + pal + r(4)]
    cases["poly_t"] = [b"T" * (k + 8)]                 # fwd is all ones (k = 32: all 64 bits), rc is 0
    cases["poly_a"] = [b"A" * (k + 8)]                 # fwd is 0
    cases["poly_t_and_a"] = [b"G" + b"T" * k + b"G", b"G" + b"A" * k]       # one k-mer each: the reverse complement of the other
    w = r(k + 6)
    cases["ends_on_last_base"] = [r(k + 4) + w, w + r(k + 1)]               # a tract to a contig's last base, one from a contig's first
    s = r(2 * k + 8)
    # the starts 0..2 and 4..6 of s have a copy on the other contig, start 3 has none: two runs one start apart, which merge
    cases["runs_one_apart"] = [r(5) + s + r(5), s[0:k + 2] + b"N" + s[4:k + 6]]
    for _ in range(1000):                              # a genome with no repeat at all
        c = [r(k + 6), r(k + 2)]
        if RM.repeated(c, k)[2] == 0:
            break
    cases["none"] = c
    return cases


# ---- 2. seams

SEAM_SPECS = [A.rep_kmer(12), A.rep_kmer(16, 2), A.rep_kmer(20), A.rep_kmer(24), A.rep_kmer(31, 5), A.rep_kmer(32)]
SEAM_LENGTHS = (100_000, 120_007, 80_000)
SEAM_PLANT_LENGTHS = (20, 33, 64, 100, 257, 1000, 3000, 31, 32, 45, 500, 2048)


def seam_case(bases_per_workgroup):
    """Three contigs of random bases, about 300 kb.  Plant i (SEAM_PLANT_LENGTHS[i] bases) lies with its middle on the global
    position (4 i + 1) * bpw -- a seam of the per-base kernels -- and again (odd i: reverse-complemented) on 4 (i + 1) * bpw -- a
    seam of the run kernels, whose tile is four times as large; even plants have a third copy on the last contig.  One word ends
    with the first contig and begins the second; another is cut in two by the start of the third contig (its halves end the
    second and begin the third: the k-mers across the cut are no repeat of the whole word, planted inside the third).  A few runs
    of N, one of them inside a copy.  -> (contigs, specs, plants), plants: (global start, length) of every copy that lies on a seam"""
    bpw = bases_per_workgroup
    rng = np.random.RandomState(31)
    off = np.concatenate(([0], np.cumsum(SEAM_LENGTHS)))
    g = np.frombuffer(rand(rng, int(off[-1])), np.uint8).copy()
    put = lambda at, w: g.__setitem__(slice(at, at + len(w)), np.frombuffer(w, np.uint8))
    plants = []
    for i, n in enumerate(SEAM_PLANT_LENGTHS):
        w = rand(rng, n)
        a, b = (4 * i + 1) * bpw - n // 2, 4 * (i + 1) * bpw - n // 2
        put(a, w)
        put(b, revcomp(w) if i % 2 else w)
        plants += [(a, n), (b, n)]
        if i % 2 == 0:
            put(int(off[2]) + 1000 + 5000 * i, revcomp(w) if i % 4 else w)
    w = rand(rng, 500)
    put(int(off[1]) - 500, w)
    put(int(off[1]), w)
    u, v = rand(rng, 300), rand(rng, 300)
    put(int(off[2]) - 300, u)
    put(int(off[2]), v)
    put(int(off[2]) + 70000, u + v)
    for at, n in ((50_000, 1), (60_000, 5), (150_000, 50), (int(off[2]) + 75_000, 3), (4 * 6 * bpw, 2)):     # (the last: inside a copy of plant 5)
        g[at:at + n] = ord("N")
    contigs = [g[off[c]:off[c + 1]].copy() for c in range(3)]
    return contigs, SEAM_SPECS, plants


# ---- 5. the command lines: the demo callsets on a surrogate FASTA with planted copies at demo variant positions

DEMO_WINDOW = 400


def demo_fasta(length=5_100_000):
    """tests/demo_pipeline.surrogate_fasta with two planted copies of DEMO_WINDOW bases around isolated SNP records of the demo truth
    set that lie inside the demo BED: one forward (between two sites with the same base) and one reverse-complemented (between
    two sites with complementary bases), so that the bytes under every VCF record stay what they were -> (sequence, the four sites)"""
    import demo_pipeline as D
    seq = np.array(D.surrogate_fasta(length), np.uint8)
    recs = []
    for name in ("nist-v4.2.1_chr1_5Mb.vcf.gz", "query.vcf"):
        recs += [(int(f[1]) - 1, f[3].upper().encode()) for f in D.read_vcf_records(os.path.join(D.DEMO, name))]
    pos = np.array(sorted({p for p, _ in recs}))
    bed = [l.split("\t") for l in open(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")).read().split("\n") if l]
    truth = {int(f[1]) - 1 for f in D.read_vcf_records(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"))
             if len(f[3]) == 1 and len(f[4]) == 1 and f[4].upper() in "ACGT"}
    sites = []
    for _, a, b in bed:
        a, b = int(a), int(b)
        for p in sorted(truth):
            if a + 300 <= p < b - 300 and (not sites or p - sites[-1] > 2000):
                near = pos[np.searchsorted(pos, p - 300):np.searchsorted(pos, p + 300)]
                if len(near) == 1:
                    sites.append(p)
    half = DEMO_WINDOW // 2
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    src_f = sites[0]
    dst_f = next(p for p in sites[1:] if seq[p] == seq[src_f])
    rest = [p for p in sites if p not in (src_f, dst_f)]
    src_r = rest[0]
    dst_r = next(p for p in rest[1:] if seq[p] == comp[int(seq[src_r])])
    seq[dst_f - half:dst_f + half] = seq[src_f - half:src_f + half].copy()
    w = np.frombuffer(revcomp(bytes(seq[src_r - half:src_r + half])), np.uint8)
    seq[dst_r - (half - 1):dst_r + half + 1] = w       # (base src_r, at offset half of its window, lands at offset half - 1)
    for p, ref in recs:                                # the bytes under every record are what they were
        if p + len(ref) <= length:
            assert bytes(seq[p:p + len(ref)]) == ref, (p, ref)
    return seq, [src_f, dst_f, src_r, dst_r]
