"""Inputs of the match-kind tests (include/vcfdist_matchkind.h), shared by tests/test_matchkind_model.py (which pins the model on
them with the CPU oracle and checks that no GPU test passes vacuously) and tests/test_gpu_matchkind.py.  Every supercluster here is
built to be evaluated: the REF bytes are the contig's, variants of a haplotype do not overlap.  The indel cases stand in planted
homopolymer runs: `T8` is a run of eight T between an A and a G, where a one-base deletion or insertion has eight placements."""
import numpy as np

import errclass_cases as EC
from vcfdist_amd import _abi as A

SUB, INS, DEL = A.TYPE_SUB, A.TYPE_INS, A.TYPE_DEL
EXACT, SHIFTED, REGROUPED, PARTIAL, NONE = A.MK_EXACT, A.MK_SHIFTED, A.MK_REGROUPED, A.MK_PARTIAL, A.MK_NONE
_NEXT = {"A": "C", "C": "G", "G": "T", "T": "A"}
_PREV = {v: k for k, v in _NEXT.items()}


def _plant_t8(ref, at):
    """A, eight T, G at ref[at - 1 .. at + 8] (ref: a list of bases)"""
    ref[at - 1:at + 9] = list("A" + "T" * 8 + "G")


def _near_miss(rng):
    """a random 10-base insertion and the same with its fifth base changed"""
    ins = "".join(rng.choice(list("ACGT"), 10))
    return ins, ins[:4] + _NEXT[ins[4]] + ins[5:]


def hand_case():
    """-> (A.Variants, cases).  One contig; cases: {name: supercluster index}; EXPECT: the kinds the definitions give."""
    rng = np.random.RandomState(43)
    ref = list(rng.choice(list("ACGT"), 4000))
    scs, cases = [], {}
    cur = [50]

    def add(name, span, q1, q2, t1, t2, t8=True):
        """a supercluster [cur, cur + span) with T8 at its relative positions 20..27; the variants' positions are relative to its
        start, a SNP is given as (pos, quality) and gets the next base"""
        b = cur[0]
        if t8:
            _plant_t8(ref, b + 20)

        def mv(vs):
            out = []
            for x in vs:
                if len(x) == 2:
                    p, q = x
                    out.append((b + p, SUB, ref[b + p], _NEXT[ref[b + p]], q))
                else:
                    out.append((b + x[0],) + tuple(x[1:]))
            return out
        cases[name] = len(scs)
        scs.append(dict(ctg=0, beg=b, end=b + span - 1, vars=[mv(q1), mv(q2), mv(t1), mv(t2)]))
        cur[0] = b + span + 30
    s = lambda p, q=30.0: (p, q)
    dl = lambda p, n=1: (p, DEL, "T" * n, "", 30.0)
    it = lambda p, a: (p, INS, "", a, 30.0)
    add("exact", 60, [s(40)], [s(40)], [s(40)], [s(40)])
    add("shifted", 60, [dl(24)], [dl(24)], [dl(20)], [dl(20)])
    add("regrouped", 60, [it(20, "T"), it(24, "T")], [it(20, "T"), it(24, "T")], [it(20, "TT")], [it(20, "TT")])
    t_ins, q_ins = _near_miss(rng)
    add("partial", 60, [it(20, q_ins)], [it(20, q_ins)], [it(20, t_ins)], [it(20, t_ins)], t8=False)
    inter = lambda: [dl(20), it(22, "G"), dl(24)]
    add("interleaved", 60, inter(), inter(), [dl(20, 2)], [dl(20, 2)])
    add("het_shift", 200, [dl(24), s(60), s(90)], [s(120)], [s(120)], [dl(20), s(60), s(90)])
    # a matched pair of low quality (the thresholds), a call and a truth variant alone
    add("lowq", 60, [s(40, 10.0)], [s(40, 10.0)], [s(40)], [s(40)])
    add("lone_fp", 60, [s(40)], [s(40)], [], [])
    add("lone_fn", 60, [], [], [s(40)], [s(40)])
    # a run of four variants at one position (three insertions and a SNP) with the copy of the SNP last
    run4 = lambda: [it(40, "C"), it(40, "GG"), it(40, "A"), s(40)]
    add("run_of_four", 60, run4(), run4(), run4(), run4())
    return A.Variants.from_sites(["".join(ref)], scs), cases


def index_of(v, cases, name, slot, k=0):
    """index in the slot of the k-th variant of a named supercluster"""
    return int(v.var_off[slot][cases[name]]) + k


# (name, slot, k-th variant of the supercluster in that slot) -> kind
EXPECT = (
    [("exact", sl, 0, EXACT) for sl in range(4)] + [("shifted", sl, 0, SHIFTED) for sl in range(4)]
    + [("regrouped", sl, k, REGROUPED) for sl in (0, 1) for k in (0, 1)] + [("regrouped", sl, 0, REGROUPED) for sl in (2, 3)]
    + [("partial", sl, 0, PARTIAL) for sl in range(4)]
    + [("interleaved", sl, k, kd) for sl in (0, 1) for k, kd in ((0, REGROUPED), (1, NONE), (2, REGROUPED))]
    + [("interleaved", sl, 0, REGROUPED) for sl in (2, 3)]
    + [("het_shift", 0, 0, SHIFTED), ("het_shift", 3, 0, SHIFTED), ("het_shift", 0, 1, EXACT), ("het_shift", 0, 2, EXACT),
       ("het_shift", 3, 1, EXACT), ("het_shift", 3, 2, EXACT), ("het_shift", 1, 0, EXACT), ("het_shift", 2, 0, EXACT)]
    + [("lowq", sl, 0, EXACT) for sl in range(4)] + [("lone_fp", 0, 0, NONE), ("lone_fp", 1, 0, NONE), ("lone_fn", 2, 0, NONE), ("lone_fn", 3, 0, NONE)]
    + [("run_of_four", sl, k, EXACT) for sl in range(4) for k in range(4)]
)


# ---- shapes for a 256-thread block: about 300 superclusters on one contig

def random_variants(targets=(513, 257, 640, 300), seed=12, n_sc=300):
    """The superclusters of errclass_cases.random_variants (two to five sites each: a SNP, a second allele, a short insertion or
    deletion; the truth mostly repeats the query's site), each followed by a planted T8 that now and then carries a shifted
    deletion, a split insertion, a deletion split around a REF-plane FP, and a near-miss insertion behind it.  Hap slot s keeps its
    first targets[s] variants (the superclusters behind them are empty in that slot)."""
    rng = np.random.RandomState(seed)
    ref = list(rng.choice(list("ACGT"), 700 * n_sc + 1000))

    def allele(pos):
        u = rng.rand()
        if u < 0.6:
            return (pos, SUB, ref[pos], (_NEXT if rng.rand() < 0.5 else _PREV)[ref[pos]])
        n = int(rng.choice((1, 2, 5, 9)))
        return (pos, INS, "", "".join(rng.choice(list("ACGT"), n))) if u < 0.8 else (pos, DEL, "".join(ref[pos:pos + n]), "")

    def place(a, how, haps, q):
        for h in ((0, 1) if how == "hom" else (0,) if how == "het0" else (1,)):
            haps[h].append(tuple(a) + (q,))
    scs, beg = [], 100
    for _ in range(n_sc):
        vars_ = [[] for _ in range(4)]
        for pos in np.sort(rng.choice(np.arange(beg + 10, beg + 180, 16), size=rng.randint(2, 6), replace=False)).tolist():
            a, how, q = allele(pos), str(rng.choice(["hom", "het0", "het1"], p=[0.4, 0.3, 0.3])), float(rng.randint(1, 61))
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
        # the planted run at beg + 210 .. 217 and the near miss at beg + 240
        p = beg + 210
        _plant_t8(ref, p)
        how, q, u = str(rng.choice(["hom", "het0", "het1"], p=[0.5, 0.25, 0.25])), float(rng.randint(1, 61)), rng.rand()
        if u < 0.25:        # shifted
            place((p + 4, DEL, "T", ""), how, vars_[0:2], q)
            place((p, DEL, "T", ""), how, vars_[2:4], q)
        elif u < 0.45:      # split
            place((p, INS, "", "T"), how, vars_[0:2], q)
            place((p + 4, INS, "", "T"), how, vars_[0:2], q)
            place((p, INS, "", "TT"), how, vars_[2:4], q)
        elif u < 0.6:       # split around a REF-plane FP
            place((p, DEL, "T", ""), how, vars_[0:2], q)
            place((p + 2, INS, "", "G"), how, vars_[0:2], q)
            place((p + 4, DEL, "T", ""), how, vars_[0:2], q)
            place((p, DEL, "TT", ""), how, vars_[2:4], q)
        if rng.rand() < 0.3:
            t_ins, q_ins = _near_miss(rng)
            how = str(rng.choice(["hom", "het0", "het1"], p=[0.5, 0.25, 0.25]))
            place((beg + 240, INS, "", q_ins), how, vars_[0:2], q)
            place((beg + 240, INS, "", t_ins), how, vars_[2:4], q)
        scs.append(dict(ctg=0, beg=beg, end=beg + 259, vars=vars_))
        beg += int(rng.randint(320, 661))
    v = A.Variants.from_sites(["".join(ref)], scs)
    for s, t in enumerate(targets):
        assert v.n_vars(s) >= t, (s, v.n_vars(s), t)
        v.var_off[s] = np.minimum(v.var_off[s], t)
        for name in ("var_pos", "var_type", "var_qual", "var_ref_off", "var_ref_len", "var_alt_off", "var_alt_len"):
            getattr(v, name)[s] = np.ascontiguousarray(getattr(v, name)[s][:t])
    return v


def edge_variants():
    """one query variant (its partner slot empty) and 513 truth variants on one hap (its partner slot empty)"""
    return random_variants(targets=(1, 0, 513, 0))


LONG_PLANTS = (200, 440, 680, 920, 1160)      # T8 runs of long_variants(); the last one holds the split around a REF-plane FP
LONG_FP = (302, 562, 822, 1082)               # query-only SNPs: REF-plane FPs


def long_variants():
    """ONE supercluster of 1 320 bases: a SNP every four bases on every haplotype (about 300 per slot, so that a slot's range
    crosses a 256-thread block's edge and the member scans are long), shifted one-base deletions in planted T8 runs, one
    deletion split around a REF-plane FP, and query-only SNPs between the sites."""
    rng = np.random.RandomState(5)
    ref = list(rng.choice(list("ACGT"), 1400))
    for p in LONG_PLANTS:
        _plant_t8(ref, p)
    snp = lambda p: (p, SUB, ref[p], _NEXT[ref[p]], float(rng.randint(1, 61)))
    vars_ = [[] for _ in range(4)]
    for p in range(12, 1310, 4):
        if any(P - 8 <= p <= P + 12 for P in LONG_PLANTS):
            continue
        a, u = snp(p), rng.rand()
        for h in ((0, 1) if u < 0.8 else (0,) if u < 0.9 else (1,)):            # het sites sit on the same haplotype in both callsets
            vars_[h].append(a)
            vars_[2 + h].append(a)
    for P in LONG_PLANTS[:-1]:
        for h in (0, 1):
            vars_[h].append((P + 4, DEL, "T", "", 30.0))
            vars_[2 + h].append((P, DEL, "T", "", 30.0))
    P = LONG_PLANTS[-1]
    for h in (0, 1):
        vars_[h] += [(P, DEL, "T", "", 30.0), (P + 2, INS, "", "G", 30.0), (P + 4, DEL, "T", "", 30.0)]
        vars_[2 + h].append((P, DEL, "TT", "", 30.0))
    for p in LONG_FP:
        for h in (0, 1):
            vars_[h].append(snp(p)[:4] + (30.0,))
    for h in range(4):
        vars_[h].sort(key=lambda x: x[0])
    return A.Variants.from_sites(["".join(ref)], [dict(ctg=0, beg=4, end=1323, vars=vars_)])


# the kinds the demo callsets populate under the CPU oracle chain (query, truth): what the command-line test may assert
# non-vacuity for (tests/test_matchkind_model.py holds them to this)
DEMO_POPULATED_QUERY = [EXACT]
DEMO_POPULATED_TRUTH = [EXACT]


def synth():
    """the synthetic batch of the error classes' tests"""
    return EC.synth()


def demo_variants(det):
    return EC.demo_variants(det)


def populated(kind_bytes):
    """(kinds with a query member, kinds with a truth member) of per-slot kind bytes"""
    q, t = np.concatenate(kind_bytes[:2]), np.concatenate(kind_bytes[2:])
    return [c for c in range(A.MK_KINDS) if (q == c).any()], [c for c in range(A.MK_KINDS) if (t == c).any()]
