"""Inputs of the error-class tests (include/vcfdist_errclass.h), shared by tests/test_errclass_model.py (which pins the model on
them with the CPU oracle and checks that no GPU test passes vacuously) and tests/test_gpu_errclass.py.  Every supercluster here is
built to be evaluated: the REF bytes are the contig's, variants of a haplotype do not overlap."""
import numpy as np

import varstrata_cases as VC
from vcfdist_amd import _abi as A

SUB, INS, DEL = A.TYPE_SUB, A.TYPE_INS, A.TYPE_DEL
GT, SYNC, PHASE, SITE, NEAR, ALONE, LOWQ, NONE = (A.EC_GT, A.EC_SYNC, A.EC_PHASE, A.EC_SITE, A.EC_NEAR, A.EC_ALONE, A.EC_LOWQ, A.EC_NONE)
_NEXT = {"A": "C", "C": "G", "G": "T", "T": "A"}
_PREV = {v: k for k, v in _NEXT.items()}


def hand_case():
    """-> (A.Variants, cases).  One contig; cases: {name: supercluster index}; expect(): the classes the definitions give."""
    rng = np.random.RandomState(41)
    ref = "".join(rng.choice(list("ACGT"), 4000))
    snp = lambda p, q=30.0: (p, SUB, ref[p], _NEXT[ref[p]], q)
    snp2 = lambda p, q=30.0: (p, SUB, ref[p], _PREV[ref[p]], q)            # another allele at the same site
    scs, cases = [], {}
    cur = [50]

    def add(name, span, q1, q2, t1, t2):
        """a supercluster [cur, cur + span); the variants' positions are relative to its start"""
        b = cur[0]
        mv = lambda vs: [(b + p,) + tuple(rest) for p, *rest in vs]
        cases[name] = len(scs)
        scs.append(dict(ctg=0, beg=b, end=b + span - 1, vars=[mv(q1), mv(q2), mv(t1), mv(t2)]))
        cur[0] = b + span + 30

    def rel(fn, p, *a):
        """the variant fn makes at contig position cur + p, with its position made relative again"""
        v = fn(cur[0] + p, *a)
        return (p,) + v[1:]
    s, s2 = (lambda p, *a: rel(snp, p, *a)), (lambda p, *a: rel(snp2, p, *a))
    # zygosity: query hom / truth het, and the reverse (both leave sc_phase NONE: either phasing costs the same)
    add("gt_query", 40, [s(20)], [s(20)], [s(20)], [])
    add("gt_truth", 40, [s(20)], [], [s(20)], [s(20)])
    # the same het allele on opposite haplotypes; three hets on query 1 / truth 1 and one on query 2 / truth 2 fix the phasing
    add("phase_orig", 200, [s(20), s(50), s(80), s(150)], [s(110)], [s(20), s(50), s(80)], [s(110), s(150)])
    # the same sites with the query haplotypes exchanged: phased SWAP, the compared slot of query 2 is truth 1
    add("phase_swap", 200, [s(110)], [s(20), s(50), s(80), s(150)], [s(20), s(50), s(80)], [s(110), s(150)])
    # a correct allele behind a wrong insertion at its position: one sync group, both fail; the partner's copy is FP too, so
    # this is no gt
    wrong = lambda: [(20, INS, "", "T", 30.0), s(20)]
    add("sync", 40, wrong(), wrong(), [s(20)], [s(20)])
    # a different allele at the same position
    add("site", 40, [s(20)], [s(20)], [s2(20)], [s2(20)])
    # the only truth variant exactly 50, 51, 1 and 10 bases from the call
    add("dist_50", 100, [s(70)], [s(70)], [s(20)], [s(20)])
    add("dist_51", 100, [s(71)], [s(71)], [s(20)], [s(20)])
    add("dist_1", 40, [s(21)], [s(21)], [s(20)], [s(20)])
    add("dist_10", 60, [s(30)], [s(30)], [s(20)], [s(20)])
    # no truth variant in the supercluster (quality 5: below a min_qual of 15); an empty partner slot; a truth variant alone
    add("no_truth", 40, [s(20, 5.0)], [s(20, 5.0)], [], [])
    add("lone_query", 40, [s(20)], [], [], [])
    add("lone_truth", 40, [], [], [], [s(20)])
    # a run of four variants at one position (three insertions and a SNP) with the copy last
    run4 = lambda: [(20, INS, "", "T", 30.0), (20, INS, "", "GG", 30.0), (20, INS, "", "C", 30.0), s(20)]
    add("run_of_four", 40, [s(20)], [s(20)], run4(), run4())
    # the 301-byte allele pair that differs in the last byte only, on opposite haplotypes of a supercluster that a het insertion
    # of 1 200 bases phases; beside it the same with the true copy
    big = (50, INS, "", "".join(rng.choice(list("ACGT"), 1200)), 30.0)
    add("long_tail", 200, [big], [(150, INS, "", VC.LONG_TAIL, 30.0)], [big, (150, INS, "", VC.LONG, 30.0)], [])
    add("long_copy", 200, [big], [(150, INS, "", VC.LONG, 30.0)], [big, (150, INS, "", VC.LONG, 30.0)], [])
    # a matched truth variant of low quality
    add("lowq", 40, [s(20, 10.0)], [s(20, 10.0)], [s(20)], [s(20)])
    return A.Variants.from_sites([ref], scs), cases


def index_of(v, cases, name, slot, k=0):
    """index in the slot of the k-th variant of a named supercluster"""
    return int(v.var_off[slot][cases[name]]) + k


# (name, slot, k-th variant of the supercluster in that slot) -> class at window 50 / 10 / 0 (one value: at every window)
EXPECT = [
    ("phase_orig", 0, 3, PHASE), ("phase_orig", 3, 1, PHASE), ("phase_orig", 0, 0, NONE), ("phase_orig", 2, 0, LOWQ),
    ("phase_swap", 1, 3, PHASE), ("phase_swap", 3, 1, PHASE), ("phase_swap", 0, 0, NONE), ("phase_swap", 3, 0, LOWQ),
    ("sync", 0, 1, SYNC), ("sync", 1, 1, SYNC), ("sync", 2, 0, SYNC), ("sync", 3, 0, SYNC), ("sync", 0, 0, SITE),
    ("site", 0, 0, SITE), ("site", 1, 0, SITE), ("site", 2, 0, SITE), ("site", 3, 0, SITE),
    ("dist_50", 0, 0, (NEAR, ALONE, ALONE)), ("dist_50", 2, 0, (NEAR, ALONE, ALONE)),
    ("dist_51", 0, 0, ALONE), ("dist_51", 3, 0, ALONE),
    ("dist_1", 1, 0, (NEAR, NEAR, ALONE)), ("dist_1", 2, 0, (NEAR, NEAR, ALONE)),
    ("dist_10", 0, 0, (NEAR, NEAR, ALONE)), ("dist_10", 3, 0, (NEAR, NEAR, ALONE)),
    ("no_truth", 0, 0, ALONE), ("no_truth", 1, 0, ALONE), ("lone_query", 0, 0, ALONE), ("lone_truth", 3, 0, ALONE),
    ("run_of_four", 0, 0, SYNC), ("run_of_four", 1, 0, SYNC),
    ("long_tail", 1, 0, SITE), ("long_tail", 2, 1, SITE), ("long_copy", 1, 0, PHASE), ("long_copy", 2, 1, PHASE), ("long_copy", 2, 0, LOWQ),
    ("lowq", 2, 0, LOWQ), ("lowq", 3, 0, LOWQ), ("lowq", 0, 0, NONE),
]
WINDOWS = (50, 10, 0)


def expect(window):
    """[(name, slot, k, class)] at one of WINDOWS"""
    return [(n, s, k, c[WINDOWS.index(window)] if isinstance(c, tuple) else c) for n, s, k, c in EXPECT]


# ---- the random shape of varstrata_cases, evaluable: about 300 superclusters on one contig

def random_variants(targets=(513, 257, 640, 300), seed=11, n_sc=300):
    """Superclusters 260 - 600 bases apart, two to five sites each; a site is a SNP, a second allele, or a short insertion or
    deletion; the truth mostly repeats the query's site, now and then on the other haplotype or with another allele.  Hap slot s
    keeps its first targets[s] variants (the superclusters behind them are empty in that slot), as in varstrata_cases."""
    rng = np.random.RandomState(seed)
    ref = "".join(rng.choice(list("ACGT"), 600 * n_sc + 1000))

    def allele(pos):
        u = rng.rand()
        if u < 0.6:
            return (pos, SUB, ref[pos], (_NEXT if rng.rand() < 0.5 else _PREV)[ref[pos]])
        n = int(rng.choice((1, 2, 5, 9)))
        return (pos, INS, "", "".join(rng.choice(list("ACGT"), n))) if u < 0.8 else (pos, DEL, ref[pos:pos + n], "")

    def place(a, how, haps, q):
        for h in ((0, 1) if how == "hom" else (0,) if how == "het0" else (1,)):
            haps[h].append(a + (q,))
    scs, beg = [], 100
    for _ in range(n_sc):
        vars_ = [[] for _ in range(4)]
        for pos in np.sort(rng.choice(np.arange(beg + 10, beg + 180, 16), size=rng.randint(2, 6), replace=False)).tolist():
            a, how, q = allele(pos), str(rng.choice(["hom", "het0", "het1"], p=[0.4, 0.3, 0.3])), float(rng.randint(1, 61))
            # now and then an insertion in front of a SNP at its position: a run of equal pos within a slot
            ins = (pos, INS, "", "".join(rng.choice(list("ACGT"), 2))) if a[1] == SUB and rng.rand() < 0.15 else None
            if ins:
                place(ins, how, vars_[0:2], q)
            place(a, how, vars_[0:2], q)
            u = rng.rand()
            if u < 0.6:
                if ins and rng.rand() < 0.5:
                    place(ins, how, vars_[2:4], q)
                place(a, how, vars_[2:4], q)                                      # the truth has the call
            elif u < 0.7:
                place(a, {"hom": "het0", "het0": "het1", "het1": "het0"}[how], vars_[2:4], q)      # other genotype / other haplotype
            elif u < 0.8:
                place(allele(pos), how, vars_[2:4], q)                            # something else at the site
            elif u < 0.9:
                place(allele(pos + 5), "hom", vars_[2:4], q)                      # something else near it
        scs.append(dict(ctg=0, beg=beg, end=beg + 199, vars=vars_))
        beg += int(rng.randint(260, 601))
    v = A.Variants.from_sites([ref], scs)
    for s, t in enumerate(targets):
        assert v.n_vars(s) >= t, (s, v.n_vars(s), t)
        v.var_off[s] = np.minimum(v.var_off[s], t)
        for name in ("var_pos", "var_type", "var_qual", "var_ref_off", "var_ref_len", "var_alt_off", "var_alt_len"):
            getattr(v, name)[s] = np.ascontiguousarray(getattr(v, name)[s][:t])
    return v


# the classes random_variants() populates under the CPU oracle (tests/test_errclass_model.py holds them to this)
RANDOM_POPULATED_QUERY = [GT, SYNC, PHASE, SITE, NEAR, ALONE]
RANDOM_POPULATED_TRUTH = [GT, SYNC, PHASE, SITE, NEAR, ALONE, LOWQ]
# and the classes the demo callsets populate (query, truth): what the command-line test may assert non-vacuity for
DEMO_POPULATED_QUERY = [PHASE, ALONE]
DEMO_POPULATED_TRUTH = [PHASE, NEAR, ALONE, LOWQ]


def edge_variants():
    """one query variant (its partner slot empty) and 513 truth variants on one hap (its partner slot empty)"""
    return random_variants(targets=(1, 0, 513, 0))


def synth():
    """an evaluable batch for the invariant (the library's generator; homozygous sites are copies on both haps)"""
    return VC.synth()


# ---- the demo callsets (tests/demo_pipeline.py)

def demo_variants(det):
    """the variant tables of demo_pipeline.run()'s details as an A.Variants, and the variant classes of its four slots"""
    import demo_pipeline as D
    from vcfdist_amd import cluster as K, summary as S
    sc, slots, fasta = det["sc"], det["slots"], det["fasta"]
    haps = [K.HapSeq(s["pos"], s["type"], s["ref"], s["alt"]) for s in slots]
    v = A.Variants(np.array([0, len(fasta)], np.int64), fasta, np.zeros(sc.n, np.int32), sc.beg, sc.end, [sc.var_off(i) for i in range(4)],
                   [h.pos for h in haps], [h.type for h in haps], [np.asarray(s["qual"], np.float32) for s in slots], [h.ref_off for h in haps],
                   [h.ref_len for h in haps], [h.alt_off for h in haps], [h.alt_len for h in haps], [h.pool for h in haps])
    return v, [S.var_class(h.type, h.ref_len, h.alt_len, D.G["sv_threshold"]) for h in haps]


def populated(cls_bytes):
    """(classes with a query member, classes with a truth member) of per-slot class bytes"""
    q, t = np.concatenate(cls_bytes[:2]), np.concatenate(cls_bytes[2:])
    return [c for c in range(A.EC_CLASSES) if (q == c).any()], [c for c in range(A.EC_CLASSES) if (t == c).any()]
