"""The table of tests/section_ed_cases.py is what it claims, and the CPU oracle agrees with the plain DP on it (no GPU).

For every case, alone in a batch: the oracle's four alignments end with status 0; every truth variant of a section carries
ref_ed == lev(X, Y) on both truth haplotypes and in both swap slots; the section the oracle's walk cuts out (read off its path and
sync points, dist.cpp:1190-1199) is flank + X + flank on the reference and the SAME flank + Y + flank on the truth haplotype;
its post-trim lengths and its side of the inline rule are the declared ones."""
import time

import numpy as np
import pytest

import oracle_lib as O
import section_ed_cases as SC
from vcfdist_amd import _abi as A


def test_lev_on_known_pairs_and_against_the_textbook_matrix():
    assert SC.lev(b"", b"") == 0 and SC.lev(b"ACGT", b"") == 4 and SC.lev(b"", b"ACG") == 3
    assert SC.lev(b"kitten", b"sitting") == 3 and SC.lev(b"sunday", b"saturday") == 3 and SC.lev(b"flaw", b"lawn") == 2
    assert SC.lev(b"ACGT", b"ACGT") == 0 and SC.lev(b"N", b"N") == 0 and SC.lev(b"a", b"A") == 1
    rng = np.random.RandomState(5)
    for _ in range(60):                 # the full matrix, cell by cell
        a = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), rng.randint(0, 40)).tobytes())
        b = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), rng.randint(0, 40)).tobytes())
        D = [[i + j if i * j == 0 else 0 for j in range(len(b) + 1)] for i in range(len(a) + 1)]
        for i in range(1, len(a) + 1):
            for j in range(1, len(b) + 1):
                D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
        assert SC.lev(a, b) == D[-1][-1] == SC.lev(b, a)


def test_trimmed_and_the_inline_rule():
    assert SC.trimmed(b"ACGT", b"ACGT") == (0, 0) and SC.trimmed(b"ACGT", b"ACT") == (1, 0) and SC.trimmed(b"", b"ACG") == (0, 3)
    assert SC.trimmed(b"AAAA", b"AAA") == (1, 0) and SC.trimmed(b"ACGTA", b"AGGTA") == (1, 1) and SC.trimmed(b"CA", b"AC") == (2, 2)
    assert SC.trimmed(b"ACA", b"A") == (2, 0)            # the prefix first: the suffix only sees what is left
    assert (SC.TYPE_INS, SC.TYPE_DEL) == (A.TYPE_INS, A.TYPE_DEL)
    for rl, tl, inline in ((32, 32, 1), (32, 256, 1), (256, 32, 1), (33, 33, 0), (32, 257, 0), (257, 32, 0), (0, 9000, 1), (9000, 0, 1),
                           (1, 1, 1), (1, 257, 0), (2, 256, 1), (33, 256, 0)):
        assert SC.is_inline(rl, tl) == bool(inline), (rl, tl)


def test_the_table_holds_the_borders():
    """the lengths the kernels can go wrong at are in the table (post-trim, either side as the pattern)"""
    trims = {c.trim[0] for g in ("one_group", "multi_group") for c in SC.GROUPS[g]}
    longer = {max(t) for t in trims}
    assert {63, 64, 65, 127, 128, 4095, 4096, 4097, 8192, 8193} <= longer
    assert {(4097, n) for n in (1, 31, 32, 33, 63, 64, 65, 100)} <= trims
    assert {(128, 2000), (2000, 128), (64, 65), (65, 64), (40, 4096), (100, 4097), (8192, 200), (8193, 200)} <= trims
    assert {c.sec for c in SC.GROUPS["inline_borders"]} >= {(32, 32), (32, 33), (33, 32), (33, 33), (32, 256), (256, 32), (32, 257),
                                                            (257, 32), (33, 256), (256, 33), (33, 257)}
    assert {c.trim[0] for c in SC.GROUPS["empty_and_trim"]} >= {(0, 257), (257, 0), (0, 300), (300, 0), (0, 40), (40, 0), (1, 0), (1, 1)}
    assert all(max(max(len(X), len(Y)) for X, Y in SC.build(c).pairs) <= 12000 for g in SC.GROUPS.values() for c in g)
    names = [c.name for g in SC.GROUPS.values() for c in g]
    assert len(names) == len(set(names))


def sections_of(batch, res_extra):
    """the sections of alignment (supercluster 0, query hap 1 x truth hap 1) as the credit walk cuts them (assign_credit,
    oracle/pr_oracle.cpp; dist.cpp:1190-1199): between two sync points k1 < k2 of the path the reference segment is
    (refpos[k1], refpos[k2]] and the truth segment (ti[k1], ti[k2]]; behind the last one, the rest of both strings.
    -> [(ref_beg, rl, tru_beg, tl)] of the sections whose two segments differ"""
    pl, qri, ti, sy, _ = res_extra.path_arrays()
    hp = batch.hap_ptr[0][batch.hap_off[0][0]:batch.hap_off[0][1]]
    refpos = np.where(pl == A.PLANE_QUERY, hp[np.minimum(qri, len(hp) - 1)], qri).astype(np.int64)
    ks = np.flatnonzero(sy[:len(pl)])
    R = bytes(batch.ref_seq[batch.ref_off[0]:batch.ref_off[1]])
    T = bytes(batch.hap_seq[2][batch.hap_off[2][0]:batch.hap_off[2][1]])
    cuts = [(int(refpos[k]) + 1, int(ti[k]) + 1) for k in ks] + [(len(R), len(T))]
    out = []
    for (r0, t0), (r1, t1) in zip(cuts[:-1], cuts[1:]):
        if R[r0:r1] != T[t0:t1]:
            out.append((r0, r1 - r0, t0, t1 - t0))
    return out, R, T


@pytest.mark.parametrize("group", list(SC.GROUPS))
def test_oracle_equals_the_plain_dp_on_every_case(group):
    t_start = time.time()
    n_pairs = 0
    for case in SC.GROUPS[group]:
        b = SC.build(case)
        v = A.Variants.from_sites([b.contig], [b.sc])
        batch = O.generate(v)
        ex = O.Extra(batch, want=(0, 0))
        res = O.run(batch, extra=ex)
        assert (res.aln_status == 0).all(), (case.name, res.aln_status)
        want = [SC.lev(X, Y) for X, Y in b.pairs]
        n_pairs += len(want)
        per_var = np.array([want[k] for k in b.var_pair])
        assert (per_var > 0).all()
        for h in (2, 3):
            for w in range(2):
                assert np.array_equal(res.ref_ed[h][w], per_var), (case.name, h, w, res.ref_ed[h][w][:6], per_var[:6])
        for (X, Y), d, trim in zip(b.pairs, want, case.trim):
            assert O.edit_distance(X, Y) == d, case.name
            assert SC.trimmed(X, Y) == trim, (case.name, SC.trimmed(X, Y))
        # the sections the walk cut out: one per pair, in order; flank + X + flank against the same flank + Y + flank
        secs, R, T = sections_of(batch, ex)
        assert len(secs) == len(b.pairs), (case.name, secs)
        n_def = 0
        for (r0, rl, t0, tl), (X, Y), trim, p in zip(secs, b.pairs, case.trim, b.pos):
            segR, segT = R[r0:r0 + rl], T[t0:t0 + tl]
            a = p - b.sc["beg"] - r0            # (the supercluster's reference string begins at its `beg`)
            assert a >= 0 and segR[a:a + len(X)] == X and segT[a:a + len(Y)] == Y, case.name
            assert segR[:a] == segT[:a] and segR[a + len(X):] == segT[a + len(Y):], case.name          # the same flank on both sides
            assert SC.trimmed(segR, segT) == trim, (case.name, SC.trimmed(segR, segT))
            if case.sec is not None:
                assert (rl, tl) == case.sec, (case.name, rl, tl)
            n_def += not SC.is_inline(rl, tl)
        assert n_def == case.deferred, (case.name, secs)
    print(f"{group}: {len(SC.GROUPS[group])} cases, {n_pairs} pairs, {time.time() - t_start:.2f} s")
