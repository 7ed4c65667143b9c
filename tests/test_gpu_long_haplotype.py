"""Behind a haplotype longer than 65 536 bases: the fallback section-edit-distance kernels, their selection, and the 16-bit borders
of the alignment levels -- the table of tests/long_haplotype_cases.py, with no environment switch anywhere.

Fallback groups.  A batch is a group's superclusters followed by the ballast, one supercluster of 65 537 bases with one SNP: the
batch's ed_max_len passes EDB_MAX_TEXT and every deferred section leaves k_ed_bits for k_ed_wf (a launch per size class),
k_ed_diag or the row sweep k_ed, as deferred_edit_distances() selects.  Required: the expected kernel ran over at least the
deferred sections and none of the others did; every result array restricted to the group's superclusters is bit-identical to the
run WITHOUT the ballast (which goes through k_ed_bits and equals the CPU oracle wherever the oracle can take the case); ref_ed equals
the plain DP lev(X, Y) independently of both; the ballast's own SNP is TP with credit 1, ref_ed 1, query_ed 0.

k_ed_bits with nearly full planes (text of 65 001 columns, 16 pattern groups) against the banded DP, alone and behind other jobs.

Two refusals of legal input are asserted exactly, as README's known limits state them: VPR_ST_ERR_LIMIT on the four alignments of a
65 201-base supercluster whose query carries a 65 000-base deletion and insertion, and VPR_ERR_ARG for a call that holds a swap
tie in an alignment of 64 999 bases.

Spacer groups.  Seven superclusters whose truth haplotype 1 has 64 999 .. 65 537 bases: every array equals the CPU oracle's answer
for the 300-base twin (the oracle does not see the spacer: tests/test_long_haplotype_cases.py), through the host marshalling and
through the device generator.

Each test prints a line `LONGHAP {json}` with its kernel table (kernel, launches, units, ms) and wall time."""
import functools
import json
import time

import numpy as np
import pytest

import long_haplotype_cases as LH
import oracle_lib as O
import section_ed_cases as SC
from test_gpu_parity import compare
from test_gpu_section_ed import assert_ref_ed, kernels
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu
ED_KERNELS = ("k_ed_bits", "k_ed_wf", "k_ed_diag", "k_ed")


@functools.lru_cache(maxsize=None)
def built(group, k):
    return SC.build(LH.GROUPS[group].cases[k])


@functools.lru_cache(maxsize=None)
def lev(case, X, Y):
    return LH.expected_distance(case, X, Y)


def expected(blt):
    """the reference distance per truth variant, in batch order"""
    out = []
    for b in blt:
        d = [lev(b.case, X, Y) for X, Y in b.pairs]
        out += [d[k] for k in b.var_pair]
    return np.array(out, np.int32)


def variants_of(blt, ballast_n=0):
    """the cases as superclusters 0 .. n - 1 of one batch (a contig each), then the ballast if asked for"""
    contigs = [b.contig for b in blt]
    scs = [dict(b.sc, ctg=i) for i, b in enumerate(blt)]
    if ballast_n:
        c, sc = LH.ballast(ballast_n, ctg=len(blt))
        contigs.append(c)
        scs.append(sc)
    return A.Variants.from_sites(contigs, scs)


def ed_table(pr):
    """[(kernel, launches, units, ms)] of the section-edit-distance kernels of the handle's last execute"""
    out = {}
    for s in pr.launch_stats():
        k = s.kernel.decode()
        if k in ED_KERNELS:
            n, u, ms = out.get(k, (0, 0, 0.0))
            out[k] = (n + 1, u + int(s.n_units), ms + float(s.ms))
    return [(k, n, u, round(ms, 3)) for k, (n, u, ms) in out.items()]


def report(what, t0, **tables):
    print("LONGHAP " + json.dumps(dict(test=what, wall_s=round(time.time() - t0, 2), **tables)))


def assert_only(pr, kernel, n_deferred, what):
    ran = kernels(pr)
    assert ran.get(kernel, 0) >= n_deferred > 0, (what, ran)
    assert not (set(ED_KERNELS) - {kernel}) & set(ran), (what, ran)


def assert_ballast_answer(res, what):
    """the ballast is the batch's last supercluster: distance 0, its SNP a true positive everywhere"""
    assert (res.aln_dist[-4:] == 0).all(), (what, res.aln_dist[-4:])
    for h in range(4):
        for w in range(2):
            assert res.errtype[h][w][-1] == A.ERRTYPE_TP and res.credit[h][w][-1] == 1.0, (what, h, w)
            assert res.ref_ed[h][w][-1] == 1 and res.query_ed[h][w][-1] == 0, (what, h, w)


@functools.lru_cache(maxsize=None)
def run_without_ballast(group, bt):
    """-> (columns, handle, built cases) of the batch without the ballast, computed once per batch.  The cases the oracle takes must
    equal it bit for bit: compare() on the whole batch where that is every case, else compare() on their sub-batch and the same
    columns out of the whole batch's run."""
    g = LH.GROUPS[group]
    blt = [built(group, k) for k in bt]
    v = variants_of(blt)
    batch = api.batch_from_variants(v)
    with_oracle = [i for i, k in enumerate(bt) if k not in g.no_oracle]
    if len(with_oracle) == len(bt):
        got, want, _, pr = compare(batch)
        assert (want.aln_status == 0).all()
    else:
        pr = api.PrecisionRecall()
        got = pr.run(batch)
        if with_oracle:
            first, count = with_oracle[0], len(with_oracle)
            assert with_oracle == list(range(first, first + count))
            sub_v = variants_of(blt[first:first + count])
            sub_got, sub_want, _, _ = compare(api.batch_from_variants(sub_v))
            assert (sub_want.aln_status == 0).all()
            assert not LH.differing_columns(LH.result_columns(got, v.var_off, first, count), LH.result_columns(sub_want, sub_v.var_off))
        # query equal to truth: every variant of the cases left to the plain DP is a true positive with full credit
        for i, k in enumerate(bt):
            if k in g.no_oracle:
                for h in range(4):
                    lo, hi = int(v.var_off[h][i]), int(v.var_off[h][i + 1])
                    for w in range(2):
                        assert (got.errtype[h][w][lo:hi] == A.ERRTYPE_TP).all() and (got.credit[h][w][lo:hi] == 1.0).all(), (blt[i].case.name, h, w)
                assert (got.aln_dist[4 * i:4 * i + 4] == 0).all()
    assert (got.aln_status == 0).all(), (group, bt, got.aln_status)
    assert_ref_ed(got, expected(blt), (group, bt, "without ballast"))
    return LH.result_columns(got, v.var_off), pr, blt


def run_with_ballast(group, bt, kernel, pr=None, ballast_n=LH.BALLAST_LEN):
    blt = [built(group, k) for k in bt]
    v = variants_of(blt, ballast_n)
    pr = pr if pr is not None else api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    what = (group, bt, "with ballast")
    assert (res.aln_status == 0).all(), (what, res.aln_status)
    assert_ref_ed(res, np.append(expected(blt), np.int32(1)), what)
    assert_only(pr, kernel, sum(b.case.deferred for b in blt), what)
    assert_ballast_answer(res, what)
    return LH.result_columns(res, v.var_off, 0, len(blt)), pr


BALLAST_BATCHES = [(name, i) for name, g in LH.GROUPS.items() if g.ballast for i in range(len(g.batches))]


@pytest.mark.parametrize("group,bi", BALLAST_BATCHES, ids=[f"{g}-{i}" for g, i in BALLAST_BATCHES])
def test_behind_the_ballast_the_selected_kernel_gives_the_same_arrays(group, bi):
    t0 = time.time()
    g = LH.GROUPS[group]
    bt, kernel = g.batches[bi], g.kernels[bi]
    cols0, pr0, blt = run_without_ballast(group, bt)
    assert_only(pr0, "k_ed_bits", sum(b.case.deferred for b in blt), (group, bt, "without ballast"))
    t1 = time.time()
    cols1, pr1 = run_with_ballast(group, bt, kernel)
    assert not LH.differing_columns(cols1, cols0), (group, bt)
    table = ed_table(pr1)
    if group == "wf_classes":       # the size classes: a launch each, with an LDS size each
        assert table[0][1] >= 3, table
    report(f"{group}-{bi}", t0, cases=len(blt), without_ballast=ed_table(pr0), with_ballast=table, s_without=round(t1 - t0, 2))


def test_selection_edge_at_65536_and_65537():
    """the same small group behind a ballast of exactly EDB_MAX_TEXT bases stays with k_ed_bits, one base more and it leaves"""
    t0 = time.time()
    name, edges = LH.SELECTION_EDGE
    blt = [SC.build(c, ctg=i) for i, c in enumerate(SC.GROUPS[name])]
    v0 = variants_of(blt)
    got, want, _, pr0 = compare(api.batch_from_variants(v0))
    cols0 = LH.result_columns(got, v0.var_off)
    want_ed = expected(blt)
    n_deferred = sum(b.case.deferred for b in blt)
    tables = {}
    for n, kernel in edges:
        v = variants_of(blt, n)
        pr = api.PrecisionRecall()
        res = pr.run(api.batch_from_variants(v))
        assert (res.aln_status == 0).all()
        assert_only(pr, kernel, n_deferred, (name, n))
        assert_ref_ed(res, np.append(want_ed, np.int32(1)), (name, n))
        assert_ballast_answer(res, (name, n))
        assert not LH.differing_columns(LH.result_columns(res, v.var_off, 0, len(blt)), cols0), n
        tables[f"ballast_{n}"] = ed_table(pr)
    report("selection_edge", t0, **tables)


def test_the_row_sweep_scratch_grows_and_is_reused_through_one_handle():
    """k_ed runs through a global scratch buffer that the handle grows lazily: per * stride ints, 19 312 for row_sweep_square's one
    job, 23 * 64 704 for row_sweep's.  One handle: the square (allocates), row_sweep (grows), the square again (a larger buffer
    than it needs, full of row_sweep's rows), row_sweep again: each equal to what a fresh handle gives without the ballast."""
    t0 = time.time()
    pr = api.PrecisionRecall()
    fresh, tables = {}, []
    for group in ("row_sweep_square", "row_sweep"):
        fresh[group] = run_without_ballast(group, LH.GROUPS[group].batches[0])[0]
    for group in ("row_sweep_square", "row_sweep", "row_sweep_square", "row_sweep"):
        cols, _ = run_with_ballast(group, LH.GROUPS[group].batches[0], "k_ed", pr=pr)
        assert not LH.differing_columns(cols, fresh[group]), group
        tables.append(ed_table(pr))
    report("row_sweep_scratch", t0, runs=tables)


BITS_BATCHES = list(range(len(LH.GROUPS["bits_full_planes"].batches)))
ERR_LIMIT = 128         # VPR_ST_ERR_LIMIT


@pytest.mark.parametrize("bi", BITS_BATCHES)
def test_k_ed_bits_with_nearly_full_planes_equals_the_banded_dp(bi):
    """no ballast: a text of 65 001 columns fills the LDS planes up to word 2 031, the pattern has 16 groups.  Alone in its batch, and
    behind twelve jobs of 33 and 258 columns whose planes are still in LDS when the long job's block starts.  With a query that has
    no variant (`fn`) the library answers: distance, ref_ed and query_ed are the banded DP's, both truth variants false negatives.
    With the query equal to the truth (`same`) it refuses those four alignments, and only those, with VPR_ST_ERR_LIMIT
    (long_haplotype_cases.py says why)."""
    t0 = time.time()
    bt = LH.GROUPS["bits_full_planes"].batches[bi]
    blt = [built("bits_full_planes", k) for k in bt]
    v = variants_of(blt)
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    refused = [i for i, k in enumerate(bt) if k in LH.BITS_REFUSED]
    st = np.asarray(res.aln_status).reshape(-1, 4)
    assert np.flatnonzero((st & ERR_LIMIT).any(1)).tolist() == refused, (bt, st)
    assert all((st[i] == ERR_LIMIT).all() if i in refused else (st[i] == 0).all() for i in range(len(bt))), (bt, st)
    want_ed = expected(blt)
    n_deferred = 0
    for i, b in enumerate(blt):
        lo, hi = int(v.var_off[2][i]), int(v.var_off[2][i + 1])
        assert [int(v.var_off[3][i]), int(v.var_off[3][i + 1])] == [lo, hi]
        if i in refused:
            continue
        n_deferred += b.case.deferred
        d = want_ed[lo:hi]
        fn = b.case.mode == "fn"
        assert (res.aln_dist[4 * i:4 * i + 4] == (d[0] if fn else 0)).all(), (b.case.name, res.aln_dist[4 * i:4 * i + 4], d[0])
        for h in (2, 3):
            for w in range(2):
                assert np.array_equal(res.ref_ed[h][w][lo:hi], d), (b.case.name, h, w, res.ref_ed[h][w][lo:hi], d)
                assert np.array_equal(res.query_ed[h][w][lo:hi], d if fn else 0 * d), (b.case.name, h, w, res.query_ed[h][w][lo:hi])
                assert (res.errtype[h][w][lo:hi] == (A.ERRTYPE_FN if fn else A.ERRTYPE_TP)).all(), (b.case.name, h, w)
                assert (res.credit[h][w][lo:hi] == (0.0 if fn else 1.0)).all(), (b.case.name, h, w)
    if n_deferred:
        assert_only(pr, "k_ed_bits", n_deferred, bt)
    else:
        assert not set(ED_KERNELS) & set(kernels(pr)), kernels(pr)
    report(f"bits_full_planes-{bi}", t0, cases=[b.case.name for b in blt], refused=refused, table=ed_table(pr),
           kernels_ms=round(pr.timing().ms_total, 2))


def test_a_swap_tie_beyond_the_replay_index_is_refused_for_the_whole_call():
    """an alignment with several optimal swap predecessors (VPR_ST_SWAP_TIE) is replayed over (Lq + Lr + 2 Lt) * Lt cells numbered
    with 32 bits; at 64 999 bases that is 1.7e10 and vpr_execute refuses the call with VPR_ERR_ARG, naming the alignment.  The same
    clusters 300 bases apart equal the oracle, ties included."""
    kl, kr, seed = LH.SPACER_TIE
    c, sc, _ = LH.spacer_case(kl, kr, 300, seed=seed)
    got, want, _, _ = compare(api.batch_from_variants(A.Variants.from_sites([c], [sc])))
    assert (want.aln_status == [A.ST_SWAP_TIE, 0, A.ST_SWAP_TIE, 0]).all()
    c, sc, lt = LH.spacer_case(kl, kr, LH.spacer_n(kl, kr, 64999, seed), seed=seed)
    assert lt == 64999
    pr = api.PrecisionRecall()
    with pytest.raises(api.VprError, match=r"vpr_execute failed \(-1\): supercluster 0 alignment [02]: .* exceed the tie replay's 32-bit cell index"):
        pr.run(api.batch_from_variants(A.Variants.from_sites([c], [sc])))


def test_spacer_superclusters_at_the_16_bit_borders_equal_their_short_twins():
    """truth haplotype 1 of 64 999, 65 000, 65 001, 65 534, 65 535, 65 536 and 65 537 bases, in one batch: every array is the oracle's
    answer for the same clusters 300 bases apart"""
    t0 = time.time()
    contigs, scs, _ = LH.spacer_batch(n=300)
    tv = A.Variants.from_sites(contigs, scs)
    twin_got, twin_want, _, _ = compare(api.batch_from_variants(tv))       # (the twins themselves: library == oracle)
    want = LH.result_columns(twin_want, tv.var_off)
    contigs, scs, lts = LH.spacer_batch()
    v = A.Variants.from_sites(contigs, scs)
    batch = api.batch_from_variants(v)
    assert [batch.lens(i)[2] for i in range(batch.n_sc)] == list(LH.SPACER_LT)
    assert all(np.array_equal(v.var_off[h], tv.var_off[h]) for h in range(4))
    t1 = time.time()
    pr = api.PrecisionRecall()
    res = pr.run(batch)
    bad = LH.differing_columns(LH.result_columns(res, v.var_off), want)
    assert not bad, ("host marshalling", bad)
    t2 = time.time()
    pr2 = api.PrecisionRecall()
    pr2.upload_variants(v.as_struct(), batch)
    pr2.execute()
    bad = LH.differing_columns(LH.result_columns(pr2.download(), v.var_off), want)
    assert not bad, ("device generate", bad)
    report("spacer", t0, lt=list(lts), s_twins=round(t1 - t0, 2), s_host=round(t2 - t1, 2), s_device=round(time.time() - t2, 2),
           kernels_ms=round(pr.timing().ms_total, 2))
