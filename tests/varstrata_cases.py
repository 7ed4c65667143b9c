"""Inputs of the variant-strata tests (include/vcfdist_varstrata.h), shared by tests/test_varstrata_model.py (which pins the
model on them and checks that no GPU test passes vacuously) and tests/test_gpu_varstrata.py."""
import numpy as np

from vcfdist_amd import _abi as A
from vcfdist_amd import api

SUB, INS, DEL = A.TYPE_SUB, A.TYPE_INS, A.TYPE_DEL
LONG = "ACGGTCA" * 43                      # 301 bytes
LONG_TAIL = LONG[:-1] + "C"                # the same but for the last byte


def hand_specs():
    """the default set and entries around the hand cases' distances"""
    names, specs = api.varstrata_default()
    extra = [("same_pos", A.vs_near(0, 1)), ("alone_at_pos", A.vs_near(0, 0, 0)), ("one_in_10", A.vs_near(10, 1, 1)), ("two_in_11", A.vs_near(11, 2)),
             ("two_in_10", A.vs_near(10, 2, 2)), ("ins_2", A.vs_size(INS, 2, 2)), ("del_any", A.vs_size(DEL, 1)), ("ins_300", A.vs_size(INS, 300, 301))]
    return names + [n for n, _ in extra], specs + [s for _, s in extra]


def hand_case():
    """Two contigs of 300 bases, two superclusters each, as an A.Variants (find() names a variant by slot, contig and pos).
    The tables are made for the membership call alone (they are no input of an evaluation)."""
    v0 = [[] for _ in range(4)]     # contig 0, supercluster 0 [0, 100)
    v1 = [[] for _ in range(4)]     # contig 0, supercluster 1 [100, 300)
    v2 = [[] for _ in range(4)]     # contig 1, supercluster 2 [0, 150)
    v3 = [[] for _ in range(4)]     # contig 1, supercluster 3 [150, 300)
    q = 30.0
    # a SNP and an insertion at the same pos of one hap: each the other's neighbour at W 0, no copies
    v0[0] += [(10, SUB, "A", "G", q), (10, INS, "", "TT", q)]
    # two alleles equal except for the last ALT byte: no copy, both het
    v0[0] += [(30, INS, "", "ACGTA", q)]
    v0[1] += [(30, INS, "", "ACGTC", q)]
    # a DEL copy (alt_len 0): hom; the REF bytes are no part of a copy's definition, the lengths are
    v0[0] += [(50, DEL, "ACG", "", q), (60, DEL, "AAA", "", q), (64, DEL, "AAA", "", q)]
    v0[1] += [(50, DEL, "ACG", "", q), (60, DEL, "CCC", "", q), (64, DEL, "AAAA", "", q)]
    # transitions, transversions, and a SUB whose bytes are equal
    v0[1] += [(70, SUB, "A", "G", q), (72, SUB, "C", "T", q), (74, SUB, "A", "C", q), (76, SUB, "G", "T", q), (78, SUB, "T", "C", q),
              (80, SUB, "A", "A", q), (82, SUB, "G", "C", q), (84, SUB, "T", "A", q)]
    # truth: an N base on either side, lower case, an MNP
    v0[2] += [(20, SUB, "N", "A", q), (25, SUB, "A", "N", q), (35, SUB, "a", "g", q), (40, SUB, "AC", "GT", q)]
    # neighbours at exactly W = 10 and at W + 1
    v1[0] += [(120, SUB, "C", "T", q), (141, SUB, "T", "A", q)]
    v1[1] += [(130, SUB, "G", "A", q)]
    # a hom pair: neither is the other's neighbour, the insertion at 203 is, and it counts the pair twice
    v1[0] += [(200, SUB, "A", "C", q)]
    v1[1] += [(200, SUB, "A", "C", q), (203, INS, "", "G", q)]
    # a 301-byte allele: a hom pair, and on the query a pair that differs in the last byte alone
    v3[2] += [(200, INS, "", LONG, q)]
    v3[3] += [(200, INS, "", LONG, q)]
    v3[0] += [(200, INS, "", LONG, q)]
    v3[1] += [(200, INS, "", LONG_TAIL, q)]
    # contig ends: the same variant at the last bases of contig 0 (truth hap 1) and of contig 1 (truth hap 2) -- no copy, no
    # neighbour; a hom pair at the start of contig 1; truth hap 2 has nothing on contig 0
    v1[2] += [(295, SUB, "A", "G", q)]
    v2[2] += [(2, SUB, "A", "G", q)]
    v2[3] += [(2, SUB, "A", "G", q)]
    v3[3] += [(295, SUB, "A", "G", q)]
    # every size bin's limits, insertions on truth hap 1 and deletions on truth hap 2 of contig 1
    for k, n in enumerate((1, 5, 6, 15, 16, 49, 50, 51)):
        v2[2] += [(20 + 3 * k, INS, "", "ACGT"[k % 4] * n, q)]
        v2[3] += [(60 + 3 * k, DEL, "ACGT"[k % 4] * n, "", q)]
    rng = np.random.RandomState(3)
    contigs = ["".join(rng.choice(list("ACGT"), 300)) for _ in range(2)]
    scs = [dict(ctg=0, beg=0, end=99, vars=v0), dict(ctg=0, beg=100, end=299, vars=v1), dict(ctg=1, beg=0, end=149, vars=v2),
           dict(ctg=1, beg=150, end=299, vars=v3)]
    return A.Variants.from_sites(contigs, scs)


def find(v, slot, ctg, pos, type=None):
    """index in the slot of the (first) variant of a contig at pos (and of a type)"""
    c = np.repeat(np.asarray(v.sc_ctg), np.diff(v.var_off[slot]))
    m = (c == ctg) & (v.var_pos[slot] == pos)
    if type is not None:
        m &= v.var_type[slot] == type
    return int(np.nonzero(m)[0][0])


# ---- the random batch: about 300 superclusters over two contigs

INDEL_LENS = (1, 1, 1, 2, 3, 5, 6, 9, 15, 16, 30, 49, 50, 80)


def _allele(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def _random_allele(rng):
    """(type, ref, alt) of one random allele: mostly SNPs (now and then with an N), else an indel of a length around the bins' limits"""
    u = rng.rand()
    if u < 0.6:
        r = rng.choice(list("ACGTN"), p=[0.24, 0.24, 0.24, 0.24, 0.04])
        a = rng.choice([b for b in "ACGT" if b != r])
        return SUB, str(r), str(a)
    n = int(rng.choice(INDEL_LENS))
    return (INS, "", _allele(rng, n)) if u < 0.8 else (DEL, _allele(rng, n), "")


def _site(rng, pos, hap_vars, planted=None):
    """one site of a callset's two haps: hom, het on either hap, or two different alleles; now and then an insertion joins a SNP"""
    a = planted[0] if planted else _random_allele(rng)
    how = planted[1] if planted else rng.choice(["hom", "het0", "het1", "alt"], p=[0.35, 0.25, 0.25, 0.15])
    q = float(rng.randint(1, 61))
    if how in ("hom", "het0", "alt"):
        hap_vars[0].append((pos, a[0], a[1], a[2], q))
    if how in ("hom", "het1"):
        hap_vars[1].append((pos, a[0], a[1], a[2], q))
    if how == "alt":
        b = _random_allele(rng)
        hap_vars[1].append((pos, b[0], b[1], b[2], q))
    if not planted and a[0] == SUB and rng.rand() < 0.1:
        hap_vars[0].append((pos, INS, "", _allele(rng, 2), q))


PLANTED = [   # one isolated site per supercluster, the same in both callsets: every size bin, a transition, a transversion, hom and het
    [((SUB, "A", "G"), "hom")], [((SUB, "C", "A"), "het0")], [((INS, "", "ACG"), "het1")], [((INS, "", "ACGTACGTAC"), "hom")],
    [((INS, "", "ACGTA" * 6), "het0")], [((INS, "", LONG), "hom")], [((DEL, "AC", ""), "het1")], [((DEL, "ACGTACGTAC", ""), "hom")],
    [((DEL, "ACGTA" * 6, ""), "het0")], [((DEL, "ACGTAC" * 10, ""), "hom")],
    [((SUB, "G", "T"), "het0"), ((SUB, "T", "C"), "het1")],           # two sites four bases apart: near_10
]


def random_variants(targets=(513, 257, 640, 300), seed=11, n_sc=(150, 150)):
    """Superclusters 210 - 600 bases apart on two contigs, two to five sites each, truth mostly the query's sites; the first eleven
    superclusters of contig 0 hold PLANTED.  Hap slot s keeps its first targets[s] variants (the superclusters behind them are
    empty in that slot), so that slot sizes can be chosen: the tail of a workgroup, one variant, none."""
    rng = np.random.RandomState(seed)
    scs = []
    for ctg, n in enumerate(n_sc):
        beg = 100
        for k in range(n):
            span = 200
            vars_ = [[] for _ in range(4)]
            plant = PLANTED[k] if ctg == 0 and k < len(PLANTED) else None
            if plant:
                for j, p in enumerate(plant):
                    for callset in (0, 1):
                        _site(rng, beg + 80 + 4 * j, vars_[2 * callset:2 * callset + 2], planted=p)
                gap = 600
            else:
                for pos in np.sort(rng.choice(np.arange(beg + 5, beg + span - 5), size=rng.randint(2, 6), replace=False)):
                    same = rng.rand() < 0.7
                    st = rng.get_state()
                    _site(rng, int(pos), vars_[0:2])
                    if same:
                        rng.set_state(st)           # (the truth draws what the query drew)
                    if same or rng.rand() < 0.7:
                        _site(rng, int(pos), vars_[2:4])
                gap = int(rng.randint(210, 601))
            scs.append(dict(ctg=ctg, beg=beg, end=beg + span - 1, vars=vars_))
            beg += gap
    contigs = ["".join(rng.choice(list("ACGT"), 1000)) + "A" * 99000 for _ in n_sc]
    v = A.Variants.from_sites(contigs, scs)
    for s, t in enumerate(targets):
        assert v.n_vars(s) >= t, (s, v.n_vars(s), t)
        v.var_off[s] = np.minimum(v.var_off[s], t)
        for name in ("var_pos", "var_type", "var_qual", "var_ref_off", "var_ref_len", "var_alt_off", "var_alt_len"):
            getattr(v, name)[s] = np.ascontiguousarray(getattr(v, name)[s][:t])
    return v


def edge_variants():
    """the random batch with one query variant (its partner slot empty) and 513 truth variants on one hap (its partner slot empty)"""
    return random_variants(targets=(1, 0, 513, 0))


def synth(snp_only=False):
    """an evaluable batch for the counter tests (the library's generator; homozygous sites are copies on both haps)"""
    kw = dict(n_sc=300, len_a=10, len_b=300, len_max=300, seed=19, var_per_base=0.03, p_hom=0.4)
    if snp_only:
        kw.update(p_snp=1.0, seed=23)
    return api.Synth(**kw)
