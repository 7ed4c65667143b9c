"""Inputs of tests/test_gpu_strata_context.py, built without a GPU so that tests/test_context_model.py can check on the CPU that
they hold what the GPU tests are about (tests/context_model.py is the specification of both)."""
import os

import numpy as np

import context_model as CM
from vcfdist_amd import _abi as A

# ---- 1. hand contigs (1 - 200 bases) and small strata of both kinds

HAND_SPECS = [
    A.ctx_period(1, 4, 6, 0),        # 0: homopolymers of 4..6: lengths min_len - 1, min_len, max_len, max_len + 1
    A.ctx_period(1, 4, 0, 2),        # 1: slop 2: padded neighbours that overlap, abut and miss by one; slop clipped at both ends
    A.ctx_period(2, 5, 0, 0),        # 2: dinucleotides: two tracts that share a base; a homopolymer is not one
    A.ctx_period(4, 9, 0, 0),        # 3: ACAC... is not a period-4 tract
    A.ctx_period(3, 7, 0, 1),
    A.ctx_gc(40, 60, 5, 0),          # 5: W odd
    A.ctx_gc(50, 75, 4, 1),          # 6: W even; 100 g == lo W at g = 2 (flagged) and == hi W at g = 3 (not flagged)
    A.ctx_gc(0, 101, 1, 0),          # 7: every called base: the flags of two contigs touch at every contig seam
    A.ctx_period(6, 13, 0, 0),
    A.ctx_gc(0, 101, 50, 0),         # 9: contigs shorter than W
]
PAD_CONTIG = "AAAA" + "CGT" + "CCCC" + "GTAT" + "GGGG" + "ACTCA" + "TTTT" + "C"     # hp at 0-4, 7-11, 15-19, 24-28; L = 29
GC_CONTIG = "ATGCGCGATATGCNATGCGGGCATATTTAGCGCGCCCGATATATGCATGCNNGGCCATAT"
HAND_CONTIGS = [
    "AAAACGTNNAAAAACACACACACGTTTT",                       # 0: tracts at the first and at the last base
    "GGACACACACACTT",                                     # 1: no period-4 tract
    "GGACGTACGTACGTT",                                    # 2: period 4 at [2, 14)
    "",                                                   # 3: length 0
    "A",                                                  # 4: length 1
    "CGTAAA",                                             # 5: ends in AAA ...
    "AAACGT",                                             # 6: ... and the next one starts in AAA: no run across the seam
    "CAAANAAAC" + "GAAAAAAT" + "CAAAAAAAG" + "TAAAG" + "CAAAAC",     # 7: N inside a run; lengths 3, 4, 6, 7
    PAD_CONTIG,                                           # 8
    "ACACAGAGAG" + "T" + "CCCCCCCC" + "T",                # 9: period-2 tracts that share a base; C x 8 is not primitive
    GC_CONTIG,                                            # 10
    "ACGTTGCAAGCTTGACCATGGTACGATCGA",                     # 11: 30 called bases: shorter than W = 50
    "ACGACGACGACGT" + "TTGACTGACTGACTGAC" + "N" + "ACGTACACGTACACGTACA" + "GG",      # 12: periods 3, 4 (primitive) and 6
    "ACGT" * 16,                                          # 13: 64 called bases: the W = 50 windows of bases 25..39 fit
]


def hand_random_contig():
    rng = np.random.RandomState(11)
    return bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=200, p=[0.3, 0.2, 0.2, 0.28, 0.02])).decode()


def hand_case():
    """(contigs, specs)"""
    return HAND_CONTIGS + [hand_random_contig()], HAND_SPECS


# ---- 2. seams

SEAM_SPECS = [
    A.ctx_period(1, 8, 0, 0),        # 0: planted homopolymers: a tract START at every seam position
    A.ctx_period(2, 8, 0, 0),        # 1: planted dinucleotide tracts: a tract END at every seam position
    A.ctx_period(1, 3, 5, 3),
    A.ctx_period(3, 7, 0, 1),
    A.ctx_gc(65, 101, 10, 0),        # 4: the all-G/C stretch is one run longer than a workgroup tile
    A.ctx_gc(0, 30, 7, 2),
]
SEAM_BELOW = 20000


def seam_case(bases_per_workgroup, bases_per_lane):
    """Three contigs of about 70 000 random bases.  The first two start on a workgroup seam of the concatenation, so that their
    coordinates are the kernels' (the third does not, for the other alignments).  In contig c, d = c - 1, every multiple x of
    bases_per_lane in [0, SEAM_BELOW) carries GGGGGGGG (or TTTTTTTT) from x + d and ACACACAC (or CACACACA)
    behind it up to the next multiple + d: stratum 0 has a tract start and stratum 1 a tract stop at x + d."""
    bpw, bpl = bases_per_workgroup, bases_per_lane
    assert bpl == 16 and bpw % bpl == 0, "the planted unit is 8 + 8 bases"
    rng = np.random.RandomState(23)
    lengths = [17 * bpw, 18 * bpw, 70001]
    contigs = []
    for c, L in enumerate(lengths):
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L)
        d = c - 1
        for i in range(0, SEAM_BELOW // bpl):
            unit = np.frombuffer(b"GGGGGGGGACACACAC" if i % 2 == 0 else b"TTTTTTTTCACACACA", np.uint8)
            a = i * bpl + d
            if a < 0:                     # (unit 0 of contig 0: its first base falls in front of the contig)
                unit, a = unit[-a:], 0
            s[a:a + len(unit)] = unit
        s[SEAM_BELOW + d:SEAM_BELOW + d + 2] = np.frombuffer(b"GT", np.uint8)       # the last unit ends here
        s[rng.choice(np.arange(SEAM_BELOW + 100, L), size=20, replace=False)] = ord("N")
        contigs.append(s)
    contigs[0][30000:30000 + 2 * bpw + 900] = ord("A")            # a homopolymer longer than two workgroup tiles
    contigs[1][25000:25000 + 40000] = ord("T")                    # and one longer than two tiles of the run passes
    contigs[2][30000:30000 + bpw + 1900] = rng.choice(np.frombuffer(b"GC", np.uint8), size=bpw + 1900)   # a GC run longer than a tile
    return contigs, SEAM_SPECS


def seam_positions(bpw, bpl):
    return sorted({m * k + d for m in (bpl, bpw) for k in range(1, SEAM_BELOW // m + 1) if m * k < SEAM_BELOW for d in (-1, 0, 1)})


# ---- 3. words: planted tracts for the default set at variant positions

def periodic_gc(rng, percent, n=400):
    """n bases whose every window of 100 holds exactly `percent` G/C (a shuffled word of 100, repeated)"""
    word = np.array(list(b"GC" * 50)[:percent] + list(b"AT" * 50)[:100 - percent], np.uint8)
    rng.shuffle(word)
    return np.tile(word, n // 100)


PLANTS = [b"CAAAAAG", b"CAAAAAAAAAG", b"CAAAAAAAAAAAAAAAG", b"GACACACACACACT", b"TACGACGACGACGACGT", b"GACGTACGTACGTACGTACGTT"]
GC_PERCENT = [15, 27, 45, 60, 80]


def plant_defaults(seq, sites, rng):
    """Overwrites `seq` (uint8 array) around eleven positions, one per default stratum: the six low-complexity words of PLANTS
    centred on sites[0..5], and 400 bases of fixed GC content around sites[6..10]."""
    for w, p in zip(PLANTS, sites[:6]):
        a = int(p) - len(w) // 2
        seq[a:a + len(w)] = np.frombuffer(w, np.uint8)
    for pc, p in zip(GC_PERCENT, sites[6:11]):
        a = int(p) - 200
        seq[a:a + 400] = periodic_gc(rng, pc)


def spread_sites(pos, n, lo, hi, gap):
    """n of the sorted positions `pos` inside [lo, hi), at least `gap` apart"""
    out = []
    for p in np.unique(pos):
        if lo <= p < hi and (not out or p - out[-1] >= gap):
            out.append(int(p))
    assert len(out) >= n, (len(out), n)
    step = len(out) // n
    return out[::step][:n]


def intervals_cover(rows, positions, what):
    """positions that are a `what` ('start' or 'stop') of some interval of rows[contig]"""
    return set(np.concatenate([r[0 if what == "start" else 1] for r in rows]).tolist()) & set(positions)


def model_rows(contigs, specs):
    return CM.all_intervals(contigs, specs)


def random_rows(rng, ctg, length):
    """0 - 200 sorted non-overlapping regions of one contig, about one gap in twenty closed (the generator of
    tests/test_gpu_strata.py)"""
    n = int(rng.choice([0, 0, 1, 2, 17, 200, rng.randint(0, 201)]))
    if n == 0:
        return []
    cuts = np.sort(rng.choice(np.arange(1, length), size=2 * n, replace=False))
    st, sp = cuts[0::2].copy(), cuts[1::2].copy()
    close = np.nonzero(rng.rand(n - 1) < 0.05)[0]
    sp[close] = st[close + 1]
    return [(ctg, int(a), int(b)) for a, b in zip(st, sp)]


def words_case(tmp):
    """A 600-supercluster synthetic workload on one contig with the default set's tracts planted at variant positions, 70
    random BED strata, and the model: the intervals of the eleven defaults, written as BEDs behind the 70, and the location of
    every variant in all 81 (strata_model.locations)."""
    import strata_model as M
    from vcfdist_amd import api, io as IO
    syn = api.Synth(n_sc=600, len_a=10, len_b=300, len_max=300, seed=7, var_per_base=0.02)
    v = syn.variants()
    length = int(v.ctg_off[1])
    rng = np.random.RandomState(41)
    seq = np.array(v.ctg_seq, np.uint8)
    sub = np.concatenate([v.var_pos[h][v.var_type[h] == A.TYPE_SUB] for h in range(4)])
    sites = spread_sites(sub, 11, 1000, length - 1000, 1500)
    plant_defaults(seq, sites, rng)
    v.ctg_seq = np.ascontiguousarray(seq)
    names, specs = api.context_default()
    rows = CM.all_intervals([seq], specs)
    rng = np.random.RandomState(5)
    bed_strata = [(f"s{k}", random_rows(rng, "c0", length)) for k in range(70)]
    ctx_strata = [(n, CM.bed_rows(r, ["c0"])) for n, r in zip(names, rows)]
    got_names, beds = IO.read_strata(M.write_strata(tmp, bed_strata + ctx_strata))
    assert got_names == [n for n, _ in bed_strata] + names
    loc = M.locations(beds, ["c0"], v)
    return dict(syn=syn, v=v, names=names, specs=specs, rows=rows, beds=beds, loc=loc, sites=sites)


# ---- 6. the command lines: the demo callsets on a surrogate FASTA with planted tracts at demo variant positions

def plant_at(seq, pos, k, rng):
    """plants the tract of default stratum k around position `pos`, keeping the base at `pos` (a record's REF)"""
    ref = int(seq[pos])
    others = [b for b in b"ACGT" if b != ref]
    if k < 3:                                    # homopolymers of 5, 9 and 15 of the REF base, flanked by another base
        n = (5, 9, 15)[k]
        a = pos - n // 2
        seq[a:a + n] = ref
        seq[a - 1] = seq[a + n] = others[0]
    elif k < 6:                                  # period 2, 3, 4: a primitive word that starts with the REF base
        p, n = k - 1, (6, 5, 5)[k - 3]
        word = np.array([ref] + others[:p - 1], np.uint8)
        a = pos - p * (n // 2)
        seq[a:a + p * n] = np.tile(word, n)
        seq[a - 1] = seq[a + p * n] = others[-1] if p < 4 else ref       # (not the base the period would continue with)
    else:                                        # 400 bases of fixed GC content (the REF base may move it by one base in a hundred)
        seq[pos - 200:pos + 200] = periodic_gc(rng, GC_PERCENT[k - 6])
        seq[pos] = ref


def demo_fasta(length=5_100_000):
    """tests/demo_pipeline.surrogate_fasta with the default set's tracts planted at eleven isolated SNP records of the demo
    truth set that lie inside the demo BED -> (sequence, sites)"""
    import demo_pipeline as D
    seq = np.array(D.surrogate_fasta(length), np.uint8)
    recs = []
    for name in ("nist-v4.2.1_chr1_5Mb.vcf.gz", "query.vcf"):
        recs += [(int(f[1]) - 1, f[3].upper(), f[4].upper()) for f in D.read_vcf_records(os.path.join(D.DEMO, name))]
    pos = np.array(sorted({p for p, _, _ in recs}))
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
    assert len(sites) >= 11, len(sites)
    sites = sites[::len(sites) // 11][:11]
    rng = np.random.RandomState(77)
    for k, p in enumerate(sites):
        plant_at(seq, p, k, rng)
    return seq, sites
