"""The lane levels' tail kernels (k_zero_tail, pr_zl.hip; k_one_tail, pr_d1.hip): a wave walks its alignments and, behind one
wait for its own stores, runs their credit sections over the step records it has just written.  Every result array against
the oracle, bit for bit (test_gpu_parity.compare), at the smallest shapes at which the fusion can go wrong: partial last
waves and padding lanes, the shortest alignments the levels take, waves that mix finished and rejected lanes, every kind of
distance-1 landing, kept paths, and the same handle executed again and again.

Two things the shapes cannot be, and what stands in their place:
  * the work list of the zero level holds the alignments of fewer than 1 024 truth rows; the four alignments of a supercluster
    share their truth haplotypes in pairs, so its length is always even: lists of 2, 62, 64, 66 and 130 alignments (a
    supercluster whose second truth haplotype carries a 1 100-base insertion contributes two), not 1, 63, 64, 65 and 129;
  * k_zero_lane leaves an alignment of ONE truth row to the general kernels (it exists only where a region is cut at the
    contig's end, and it is no distance-1 input either): two rows are the fewest a tail kernel walks.  The one-row alignment
    is still in the wave -- as a lane the tail must leave alone -- beside alignments of 2 and of 60 rows."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import compare
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu

ERR = A.ST_ERR_NO_PTR | A.ST_ERR_UNFINISHED | A.ST_ERR_LIMIT
S, I, D = A.TYPE_SUB, A.TYPE_INS, A.TYPE_DEL
_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _ref(n, seed):
    return "".join(np.random.RandomState(seed).choice(list("ACGT"), n))


def _tail_units(pr, name):
    """work-list length of the level's tail launch (launch statistics), 0 if it did not run"""
    return sum(int(s_.n_units) for s_ in pr.launch_stats() if s_.kernel.decode() == name)


def _check_paths(pr, batch, got, dists):
    """vpr_download_path against the oracle's walk, step for step, for every alignment of the short part (fewer than 1 024
    truth rows) whose distance is in `dists`"""
    n = 0
    for a in np.flatnonzero(np.isin(got.aln_dist, dists)):
        sc, aln = int(a) // 4, int(a) % 4
        if batch.lens(sc)[2 + (aln & 1)] >= 1024:
            continue
        one = batch.subset(np.array([sc]))
        ex = O.Extra(one, want=(0, aln))
        O.run(one, extra=ex)
        pl, q, t, sy, ed = pr.path(sc, aln)
        opl, oq, ot, osy, oed = ex.path_arrays()
        assert np.array_equal(pl, opl) and np.array_equal(q, oq) and np.array_equal(t, ot), (sc, aln)
        assert np.array_equal(sy, osy[:len(sy)]) and np.array_equal(ed, oed[:len(ed)]), (sc, aln)
        n += 1
    return n


def _list_length_batch(n_list, seed):
    """superclusters of 4 - 40 bases whose short part is exactly n_list alignments: n_list // 4 superclusters of four short
    alignments and, for n_list % 4 == 2, one whose second truth haplotype is 1 100 bases longer (its two alignments are the
    long part).  Most sites are shared by all four haplotypes (distance 0), every fourth is heterozygous (two alignments of
    distance 1 beside two of distance 0)."""
    rng = np.random.RandomState(seed)
    ref = _ref(50 * (n_list // 4 + 2), seed + 1000)
    scs, cur = [], 3
    for k in range(n_list // 4):
        L = int(rng.randint(4, 41))
        p = cur + int(rng.randint(1, L - 1))
        v = (p, S, ref[p], _OTHER[ref[p]], 20.0)
        scs.append(dict(ctg=0, beg=cur, end=cur + L - 1, vars=[[v], [v] if k % 4 else [], [v], [v] if k % 4 else []]))
        cur += L + 5
    if n_list % 4:
        ins = (cur + 20, I, "", _ref(1100, seed + 2000), 30.0)
        scs.append(dict(ctg=0, beg=cur, end=cur + 39, vars=[[], [ins], [], [ins]]))
    return api.batch_from_variants(A.Variants.from_sites([ref], scs))


@pytest.mark.parametrize("n_list", [2, 62, 64, 66, 130])
def test_list_lengths_around_the_wave_size(n_list):
    """partial last waves and padding lanes; on the first shape with VPR_CFG_KEEP_PATHS, the kept paths against the oracle's"""
    batch = _list_length_batch(n_list, seed=n_list)
    keep = n_list == 2
    got, want, _, pr = compare(batch, A.default_config(flags=A.CFG_KEEP_PATHS) if keep else None)
    nz = _tail_units(pr, "k_zero_tail")
    print(f"n_list {n_list}: k_zero_tail over {nz} alignments, {int((want.aln_dist == 0).sum())} of distance 0, "
          f"{pr.timing().n_lane1_finished} finished at distance 1")
    assert nz == n_list and (want.aln_dist == 0).sum() >= 2
    assert not (got.aln_status & ERR).any()
    if keep:
        assert _check_paths(pr, batch, got, [0]) >= 2


def test_shortest_alignments_share_a_wave_with_long_ones():
    """alignments of two truth rows (one move, two records) and of 60 in one wave with a one-row alignment at the contig's
    end, which the lane levels leave to the general kernels"""
    ref = _ref(400, 5)
    n = len(ref)
    snp = lambda p: (p, S, ref[p], _OTHER[ref[p]], 20.0)
    scs = []
    for k in range(4):          # two rows: no variant at all / a site on the second base shared by all haplotypes
        b = 10 + 10 * k
        scs.append(dict(ctg=0, beg=b, end=b + 1, vars=[[], [], [], []] if k % 2 else [[snp(b + 1)]] * 4))
    for k in range(3):          # 60 rows
        b = 100 + 70 * k
        scs.append(dict(ctg=0, beg=b, end=b + 59, vars=[[snp(b + 7), snp(b + 41)]] * 4))
    scs.append(dict(ctg=0, beg=50, end=52, vars=[[snp(51)]] * 4))        # three rows
    # the contig's last base deleted on query 1 and truth 1: one base is left of their haplotypes
    scs.append(dict(ctg=0, beg=n - 2, end=n + 1, vars=[[(n - 1, D, ref[n - 1], "", 9.0)], [], [(n - 1, D, ref[n - 1], "", 9.0)], []]))
    batch = api.batch_from_variants(A.Variants.from_sites([ref], scs))
    assert batch.lens(0)[2] == 2 and batch.lens(4)[2] == 60 and batch.lens(len(scs) - 1)[2] == 1
    got, want, _, pr = compare(batch)
    assert _tail_units(pr, "k_zero_tail") == 4 * len(scs) and (want.aln_dist.reshape(-1, 4)[:8] == 0).all()
    assert not (got.aln_status & ERR).any()


def test_finished_and_rejected_lanes_in_one_wave():
    """tandem repeats: a wave of the zero level holds lanes it finished, lanes it rejected cleanly (the distance-1 level's
    input) and lanes it rejected for a tie or a fifth diagonal; the credit phase runs for the first kind only"""
    batch = api.Synth(n_sc=400, len_a=6, len_b=90, len_min=5, len_max=90, seed=57, var_per_base=0.02, p_snp=0.4, p_repeat=0.9).batch()
    got, want, _, pr = compare(batch)
    t = pr.timing()
    n0, n_tie = int((want.aln_dist == 0).sum()), int(((want.aln_status & A.ST_SWAP_TIE) != 0).sum())
    print(f"{batch.n_sc} sc: {n0} alignments of distance 0, {t.n_lane1_seen} clean rejects, {t.n_lane1_finished} finished at distance 1, "
          f"{n_tie} with a swap tie, {t.n_band_retries} retries")
    assert _tail_units(pr, "k_zero_tail") == 4 * batch.n_sc and n0 > 0
    assert t.n_lane1_seen > 0 and t.n_lane1_finished > 0 and n_tie > 0 and t.n_band_retries > t.n_lane1_finished
    assert not (got.aln_status & ERR).any()


def _d1_landing_batch():
    """one edit on both truth haplotypes, none on the query's: a SUB, a one-base INS and a one-base DEL as the first, a middle
    and the last move of alignments of 2, 3, 5, 40, 255 and 256 truth rows (VPR_D1_MAX_ROWS = 256; a region of n bases is
    beg .. beg + n - 1, and the truth has one row more behind an INS, one less behind a DEL)"""
    ref = _ref(9000, 77)
    scs, rows, cur = [], [], 5
    for R in (2, 3, 5, 40, 255, 256):
        for typ in (S, I, D):
            n = R - (typ == I) + (typ == D)
            if n < 2:
                continue
            last = n - 2 if typ == D else n - 1           # offset of the last landing (a deletion keeps one base behind it)
            for o in sorted({1, min(max(1, n // 2), last), last}):
                p, end = cur + o, cur + n - 1
                if typ == S:
                    v = (p, S, ref[p], _OTHER[ref[p]], 20.0)
                elif typ == I:
                    v = (p, I, "", _OTHER[ref[p]], 20.0)
                else:
                    v = (p, D, ref[p], "", 20.0)
                scs.append(dict(ctg=0, beg=cur, end=end, vars=[[], [], [v], [v]]))
                rows.append(R)
                cur = end + 8
    return api.batch_from_variants(A.Variants.from_sites([ref], scs)), rows


def test_distance_one_landings_with_kept_paths():
    """SUB, INS and DEL landings at the first and the last move of a path, at 2 - 256 rows; walks and results against the oracle"""
    batch, rows = _d1_landing_batch()
    assert [batch.lens(k)[2] for k in range(batch.n_sc)] == rows
    got, want, _, pr = compare(batch, A.default_config(flags=A.CFG_KEEP_PATHS))
    t = pr.timing()
    print(f"{batch.n_sc} sc: {int((want.aln_dist == 1).sum())} alignments of distance 1, {t.n_lane1_seen} clean rejects, "
          f"{t.n_lane1_finished} finished at the lane level")
    assert (want.aln_dist == 1).all() and t.n_lane1_finished > 0
    assert _tail_units(pr, "k_one_tail") > 0 and _tail_units(pr, "k_zero_tail") == 4 * batch.n_sc
    assert not (got.aln_status & ERR).any()
    assert _check_paths(pr, batch, got, [1]) == 4 * batch.n_sc


def test_distance_one_batch_of_mixed_edits():
    """a batch whose rejects are mostly of distance 1, indels as frequent as substitutions, up to 300 rows (beyond 256 the
    16-cell kernels take them)"""
    batch = api.Synth(n_sc=600, len_a=4, len_b=300, len_min=4, len_max=300, seed=45, var_per_base=0.02, p_snp=0.4, indel_mean=2.0).batch()
    got, want, _, pr = compare(batch)
    t = pr.timing()
    print(f"{batch.n_sc} sc: {int((want.aln_dist == 1).sum())} alignments of distance 1, {t.n_lane1_finished} finished at the lane level")
    assert t.n_lane1_finished > 50 and _tail_units(pr, "k_one_tail") > 0
    assert not (got.aln_status & ERR).any()


def test_twenty_executes_of_one_handle_are_identical():
    """the tail kernels read what they have just written: a missing wait between the phases, or a record left over from the
    execute before, would show as a difference between two executes of one batch"""
    batch = api.Synth(n_sc=2000, len_mode=1, len_a=20.0, len_b=1.2, len_min=4, len_max=1000, seed=19).batch()
    got, want, _, pr = compare(batch)
    t = pr.timing()
    assert _tail_units(pr, "k_zero_tail") > 0 and (want.aln_dist == 0).any() and t.n_lane1_finished > 0
    assert not (got.aln_status & ERR).any()
    for k in range(19):
        pr.execute()
        assert not got.diff(pr.download()), k
