"""The table of tests/long_haplotype_cases.py is what it claims (no GPU).

Every case has the post-trim lengths it declares and a deferred section; lev_banded equals lev wherever it answers and raises where
its band is too small; the kernel each batch is expected to take follows from the job lengths -- the oracle's own sections where
the oracle can take the case, the one-flank-base rule (asserted here on those) elsewhere -- through the restated selection; the
ballast and the spacer superclusters have the haplotype lengths they declare; and the oracle's answer for a spacer case does not
depend on the spacer's length, which is what tests/test_gpu_long_haplotype.py builds on."""
import functools
import time

import numpy as np
import pytest

import long_haplotype_cases as LH
import oracle_lib as O
import section_ed_cases as SC
from test_section_ed_cases import sections_of
from vcfdist_amd import _abi as A
from vcfdist_amd import api


@functools.lru_cache(maxsize=None)
def built(group, k):
    return SC.build(LH.GROUPS[group].cases[k])


@functools.lru_cache(maxsize=None)
def oracle_jobs(group, k):
    """(ref_len, tru_len) of the deferred sections of one case, as the oracle's walk cuts them"""
    b = built(group, k)
    batch = O.generate(A.Variants.from_sites([b.contig], [b.sc]))
    ex = O.Extra(batch, want=(0, 0))
    res = O.run(batch, extra=ex)
    assert (res.aln_status == 0).all(), b.case.name
    secs, _, _ = sections_of(batch, ex)
    return tuple((rl, tl) for _, rl, _, tl in secs if not SC.is_inline(rl, tl))


def jobs_of(group, k):
    if k not in LH.GROUPS[group].no_oracle:
        return oracle_jobs(group, k)
    b = built(group, k)
    return tuple(j for j in (LH.job_lens_same(X, Y) for X, Y in b.pairs) if not SC.is_inline(*j))


def test_lev_banded_equals_lev_where_it_answers_and_raises_where_it_cannot():
    assert LH.TYPE_SUB == A.TYPE_SUB
    assert LH.lev_banded(b"", b"", 0) == 0 and LH.lev_banded(b"kitten", b"sitting", 3) == 3 and LH.lev_banded(b"ACGT", b"", 4) == 4
    rng = np.random.RandomState(11)
    n_pairs = 0
    for it in range(220):
        a = bytes(SC._rand(rng, rng.randint(0, 601)))
        kind = it % 4
        if kind == 0 or len(a) < 20:
            b = bytes(SC._rand(rng, rng.randint(0, 601)))                   # unrelated: the distance is most of the length
        elif kind == 1:
            b = bytes(SC._mutate(rng, a, len(a) + rng.randint(-10, 11)))
        elif kind == 2:
            b = bytes(SC._plant(rng, a, rng.randint(0, 16)))
        else:
            b = a[:rng.randint(0, len(a))] + bytes(SC._rand(rng, rng.randint(0, 30)))
        d = SC.lev(a, b)
        for k in {d, d + 1, d + rng.randint(2, 40), max(len(a), len(b))}:
            if k >= abs(len(a) - len(b)):
                assert LH.lev_banded(a, b, k) == d, (it, k, d)
        if d > 0:                           # one short of the distance: no answer, whatever the band holds
            with pytest.raises(ValueError):
                LH.lev_banded(a, b, d - 1)
        n_pairs += 1
    assert n_pairs >= 200
    for seed in (1, 2):                     # two pairs of 4 000 bases
        r = np.random.RandomState(seed)
        a = bytes(SC._rand(r, 4000))
        b = bytes(SC._plant(r, a, 120)) if seed == 1 else bytes(SC._mutate(r, a, 3990))
        d = SC.lev(a, b)
        assert 0 < d <= 250
        assert LH.lev_banded(a, b, 250) == d == LH.lev_banded(b, a, d)
        with pytest.raises(ValueError):
            LH.lev_banded(a, b, d - 1)
    with pytest.raises(ValueError):
        LH.lev_banded(b"A" * 10, b"A" * 20, 5)


@pytest.mark.parametrize("group", list(LH.GROUPS))
def test_cases_have_their_declared_lengths_and_a_deferred_section(group):
    t0 = time.time()
    g = LH.GROUPS[group]
    assert sorted({k for bt in g.batches for k in bt}) == list(range(len(g.cases)))
    for k, case in enumerate(g.cases):
        b = built(group, k)
        for (X, Y), trim in zip(b.pairs, case.trim):
            assert SC.trimmed(X, Y) == trim, (case.name, SC.trimmed(X, Y))
        jobs = jobs_of(group, k)
        assert len(jobs) == case.deferred > 0, (case.name, jobs)
        assert not any(SC.is_inline(rl, tl) for rl, tl in jobs)
        if k not in g.no_oracle and case.mode == "same":        # the rule the groups without the oracle rely on
            for (X, Y), j in zip(b.pairs, jobs):
                if X and Y and SC.trimmed(X, Y) == (len(X), len(Y)):
                    assert j == LH.job_lens_same(X, Y), (case.name, j)
        # the supercluster's haplotypes, from the host marshalling: below EDB_MAX_TEXT, so that the ballast alone decides
        lens = api.batch_from_variants(A.Variants.from_sites([b.contig], [b.sc])).lens(0)
        assert max(lens) <= LH.EDB_MAX_TEXT, (case.name, lens)
    print(f"{group}: {len(g.cases)} cases, {time.time() - t0:.2f} s")


def test_the_planted_pairs_are_within_the_band_and_fill_the_planes():
    g = LH.GROUPS["bits_full_planes"]
    assert not g.ballast and g.no_oracle == {0, 1, 2, 3, 4} and set(g.kernels) == {"k_ed_bits"}
    assert [g.cases[k].mode for k in range(5)] == ["same", "same", "same", "fn", "fn"] and LH.BITS_REFUSED == {0, 1}
    for k in (0, 1, 3, 4):
        b = built("bits_full_planes", k)
        (X, Y), = b.pairs
        assert (X, Y) == built("bits_full_planes", k % 3).pairs[0]              # the same strings in both modes
        d = LH.expected_distance(b.case, X, Y)
        assert 0 < d <= 200 and len(X) == len(Y) >= 65000
        rl, tl = LH.job_lens_same(X, Y)
        assert (rl + 4095) // 4096 == 16 and (tl - 1) // 32 >= 2031 and tl <= LH.EDB_MAX_TEXT
        batch = api.batch_from_variants(A.Variants.from_sites([b.contig], [b.sc]))
        assert batch.lens(0) == [len(X) + 2 * SC.SC_MARGIN + 1] * 5
        assert [batch.n_vars(h) for h in range(4)] == ([2] * 4 if b.case.mode == "same" else [0, 0, 2, 2])


@pytest.mark.parametrize("n,k", [(300, 20), (1500, 196)])
def test_the_oracle_on_short_twins_of_the_fn_cases(n, k):
    """what the GPU test asserts for the `fn` cases of 65 000 bases, where no oracle reaches: one section of X and Y plus one
    flank base, alignment distance == ref_ed == query_ed == lev(X, Y), both truth variants false negatives without credit"""
    b = SC.build(LH._planted(n, 6400, "fn", k))
    (X, Y), = b.pairs
    d = SC.lev(X, Y)
    assert d == LH.lev_banded(X, Y, LH.PLANTED_K) > 0
    batch = O.generate(A.Variants.from_sites([b.contig], [b.sc]))
    ex = O.Extra(batch, want=(0, 0))
    res = O.run(batch, extra=ex)
    secs, _, _ = sections_of(batch, ex)
    assert [(rl, tl) for _, rl, _, tl in secs] == [LH.job_lens_same(X, Y)]
    assert (res.aln_status == 0).all() and (res.aln_dist == d).all()
    for h in (2, 3):
        for w in range(2):
            assert res.errtype[h][w].tolist() == [A.ERRTYPE_FN] * 2 and res.credit[h][w].tolist() == [0.0] * 2
            assert res.ref_ed[h][w].tolist() == [d] * 2 == res.query_ed[h][w].tolist()


@pytest.mark.parametrize("group", list(LH.GROUPS))
def test_the_expected_kernel_follows_from_the_selection_arithmetic(group):
    g = LH.GROUPS[group]
    for bt, kernel in zip(g.batches, g.kernels):
        jobs = [j for k in bt for j in jobs_of(group, k)]
        got, launches = LH.select(jobs, LH.BALLAST_LEN if g.ballast else LH.EDB_MAX_TEXT)
        assert got == kernel, (group, bt, got)
        assert LH.select(jobs, LH.EDB_MAX_TEXT)[0] == "k_ed_bits"
        if group == "wf_classes":
            assert launches >= 3, launches
        print(f"{group} {bt}: {len(jobs)} jobs, longest {max(max(j) for j in jobs)}, largest sum {max(sum(j) for j in jobs)}: "
              f"{got} x {launches}")


def test_the_borders_sit_where_the_table_says():
    """the arithmetic of the table's comments, on the job lengths (one flank base on each side)"""
    assert LH.lds_wf(17001, 17001 + 41) == 153078 <= LH.LDS_LIMIT < LH.lds_wf(17101, 17101 + 41) == 153978
    assert LH.select([(17001, 41)], 65537) == ("k_ed_wf", 1) and LH.select([(17101, 41)], 65537) == ("k_ed_diag", 1)
    assert LH.select([(64698, 301)], 65537)[0] == "k_ed_diag" and LH.select([(64699, 301)], 65537)[0] == "k_ed"      # sums 64 999, 65 000
    assert LH.select([(301, 64698)], 65537)[0] == "k_ed_diag" and LH.select([(301, 64699)], 65537)[0] == "k_ed"
    assert LH.lds_wf(19301, 38602) > LH.LDS_LIMIT and LH.lds_diag(19301, 38602) == 154442 > LH.LDS_LIMIT
    assert LH.select([(19301, 19301)], 65537)[0] == "k_ed"
    assert LH.select([(28999, 41)], 65537)[0] == "k_ed_diag"            # (lds_wf is over the limit long before max_long reaches 29 000)
    assert LH.select([(34, 34), (258, 2)], 65536)[0] == "k_ed_bits" and LH.select([(34, 34), (258, 2)], 65537) == ("k_ed_wf", 2)
    name, edges = LH.SELECTION_EDGE
    assert name in SC.GROUPS and [n for n, _ in edges] == [LH.EDB_MAX_TEXT, LH.EDB_MAX_TEXT + 1]


@pytest.mark.parametrize("n", [300, 65536, 65537])
def test_the_ballast_has_its_declared_lengths_and_nothing_deferred(n):
    contig, sc = LH.ballast(n)
    v = A.Variants.from_sites([contig], [sc])
    batch = api.batch_from_variants(v)
    assert batch.lens(0) == [n] * 5
    assert [batch.n_vars(h) for h in range(4)] == [1] * 4
    if n == 300:            # what the GPU test asserts for the ballast's own variants, from the oracle on a 300-base twin
        res = O.run(O.generate(v))
        assert (res.aln_status == 0).all() and (res.aln_dist == 0).all()
        for h in range(4):
            for w in range(2):
                assert res.errtype[h][w].tolist() == [A.ERRTYPE_TP] and res.credit[h][w].tolist() == [1.0]
                assert res.ref_ed[h][w].tolist() == [1] and res.query_ed[h][w].tolist() == [0]


def test_spacer_cases_have_their_declared_lengths():
    contigs, scs, lts = LH.spacer_batch()
    assert tuple(lts) == LH.SPACER_LT == (64999, 65000, 65001, 65534, 65535, 65536, 65537)
    batch = api.batch_from_variants(A.Variants.from_sites(contigs, scs))
    assert [batch.lens(i)[2] for i in range(batch.n_sc)] == list(LH.SPACER_LT)
    assert all(abs(l - lt) <= 8 for i, lt in enumerate(lts) for l in batch.lens(i))
    # the variants do not depend on the spacer: the same clusters, the right one moved
    _, twins, _ = LH.spacer_batch(n=300)
    for a, b in zip(scs, twins):
        for h in range(4):
            assert [(v[1:]) for v in a["vars"][h]] == [(v[1:]) for v in b["vars"][h]]


def test_the_spacer_tie_case_ties_and_the_others_do_not():
    kl, kr, seed = LH.SPACER_TIE
    for n in (300, 3000):
        c, sc, _ = LH.spacer_case(kl, kr, n, seed=seed)
        res = O.run(O.generate(A.Variants.from_sites([c], [sc])))
        assert (res.aln_status == [A.ST_SWAP_TIE, 0, A.ST_SWAP_TIE, 0]).all(), res.aln_status
    contigs, scs, _ = LH.spacer_batch(n=300)
    assert (O.run(O.generate(A.Variants.from_sites(contigs, scs))).aln_status == 0).all()


def test_the_oracle_does_not_see_the_spacer():
    """the premise of the GPU test: every array compare() looks at is the same for a spacer of 300 and of 3 000 bases"""
    t0 = time.time()
    cols = []
    for n in (300, 3000):
        contigs, scs, _ = LH.spacer_batch(n=n)
        v = A.Variants.from_sites(contigs, scs)
        res = O.run(O.generate(v))
        cols.append(LH.result_columns(res, v.var_off))
        assert (res.aln_status == 0).all()
        assert 0 < res.aln_dist.max() < 16 and (res.aln_dist > 0).all()
        for h in range(4):          # the clusters make more than one kind of answer
            assert len(set(res.errtype[h][0].tolist())) >= 2
    assert not LH.differing_columns(cols[0], cols[1])
    print(f"spacer invariance: {time.time() - t0:.2f} s")
