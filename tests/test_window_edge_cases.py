"""The table of tests/window_edge_cases.py is what it claims, with the oracle alone (no GPU): every case's distances are the declared
ones, the declared ties are ties, the path runs u cells off the window centre, the slack cases have slack -- and every border of
every window level is covered from both sides by cases whose unit lengths differ by one.  These are the conditions that keep
tests/test_gpu_window_edges.py from passing vacuously."""
import time

import pytest

import window_edge_cases as WE
from vcfdist_amd import _abi as A

N_CASES = 564


@pytest.fixture(scope="module")
def needs():
    t0 = time.time()
    out = WE.needs(WE.TABLE)
    print(f"needed_level of {len(WE.TABLE)} cases: {time.time() - t0:.1f} s")
    return out


def test_no_case_is_dropped(needs):
    assert len(WE.TABLE) == N_CASES
    assert len({c.name for c in WE.TABLE}) == N_CASES == len(needs)
    fam = {}
    for c in WE.TABLE:
        fam[c.family] = fam.get(c.family, 0) + 1
    assert fam == {"shift": 246, "priced": 114, "there_back": 6, "phase": 51, "het": 12, "het_same": 24, "plane_end": 40, "short": 10, "slack": 8,
                   "slide": 38, "swap": 15}, fam


def test_distances_ties_and_offsets_are_the_declared_ones(needs):
    for c in WE.TABLE:
        n = needs[c.name]
        alns = (0, 1) if c.het else (0, 1, 2, 3)        # (a het case's second query haplotype is the reference: other distances)
        assert all(n[0].dists[a] == c.dist for a in alns), (c.name, n[0].dists, c.dist)
        tied = [bool(s & A.ST_SWAP_TIE) for s in n[0].statuses]
        if c.tie:
            assert all(tied), (c.name, n[0].statuses)
        assert not any(s & ~(A.ST_SWAP_TIE | A.ST_WARN_MASK) for s in n[0].statuses), (c.name, n[0].statuses)
        # the path runs u cells off the centre, on the side the sign and the form say (the priced cases only while the
        # shifted path is the cheaper one)
        if c.family not in ("slide", "swap") and (c.k == 0 or 2 * c.k < c.u):
            up = (c.sign > 0) == (c.form == "ins")
            if up or c.family == "there_back":
                assert n[0].off_hi == c.u, (c.name, n[0])
            if not up or c.family == "there_back":
                assert n[0].off_lo == -c.u, (c.name, n[0])
        assert (n[0].slack > 0) == (c.family == "slack"), (c.name, n[0].slack)
        if c.family == "short":
            assert 5 <= min(n[0].lens) and max(n[0].lens) <= 70, (c.name, n[0].lens)
        assert len(n) == (4 if c.het else 1)
        if c.family == "het_same":      # the four alignments of the supercluster need different levels
            assert len({x.level for x in n}) >= 2 and n[2].level == n[3].level == 16 < n[0].level == n[1].level, (c.name, [x.level for x in n])


def _borders(needs, pick):
    """{(W, sign): [(u, u + 1)]}: pairs of cases that `pick` selects, alike but for u, of which the first needs level W and the
    second the level above"""
    by = {}
    for c in WE.TABLE:
        if pick(c):
            by[(c.family, c.sign, c.form, c.snp, c.side, c.k, c.u)] = needs[c.name][0].level
    out = {}
    for (fam, sign, form, snp, side, k, u), lv in by.items():
        up = by.get((fam, sign, form, snp, side, k, u + 1))
        if lv in WE.LEVELS and up == WE.next_level(lv):
            out.setdefault((lv, sign), []).append((u, u + 1))
    return out


def test_every_border_is_covered_from_both_sides(needs):
    want = {(W, sign) for W in WE.LEVELS for sign in (1, -1)}
    shift = _borders(needs, lambda c: c.family == "shift" and c.snp == 0 and c.form == "ins")
    priced = _borders(needs, lambda c: c.family == "priced" and c.k == 1)
    priced_s = _borders(needs, lambda c: c.family == "shift" and c.snp > 0)
    print("borders (level, sign): [(u needing the level, u needing the next)]")
    for name, b in (("shift, s = 0", shift), ("priced, k = 1 (s = 2)", priced), ("shift with truth-only SNPs (s = 1, 2)", priced_s)):
        print(f"  {name}: {dict(sorted(b.items()))}")
    assert set(shift) == want, sorted(want - set(shift))
    assert set(priced) == want, sorted(want - set(priced))
    assert set(priced_s) == want, sorted(want - set(priced_s))
    # the window holds still for 4 or 8 rows: the last offset that fits lies inside W / 2, and differs by sign
    for (W, sign), pairs in shift.items():
        assert all(u < W // 2 for u, _ in pairs), (W, sign, pairs)


def test_the_zero_budget_families_reach_every_level(needs):
    """slide (and the het cases' alignments against the reference haplotype): no query variant, so the exit test's bound is exact;
    a case on either side of the 1024-cell level's border too"""
    lv = {needs[c.name][0].level for c in WE.TABLE if c.family == "slide"}
    assert lv == {16, 64, 256, 1024, WE.DENSE}, lv
    assert {needs[c.name][0].level for c in WE.TABLE if c.family == "swap"} == {256, 1024}


def test_ties_need_the_64_and_the_256_cell_level(needs):
    lv = {c.u: needs[c.name][0].level for c in WE.TABLE if c.tie}
    assert len(lv) >= 5 and {16, 64, 256} & set(lv.values()) >= {64, 256}, lv


def test_restated_origins_stay_inside_the_planes():
    """stripe 0 at the origin, every other stripe inside [0, L - min(W, L)], constant over the stripe by construction"""
    cases = [c for c in WE.TABLE if c.family in ("plane_end", "short", "slack")]
    _, batch, _ = WE.batch_of(cases)
    for sc in range(batch.n_sc):
        q2r, t2r, tflag, r2q, Lq, Lr, Lt = WE.arrays_of(batch, sc, 0)
        tj = WE.tj_of(t2r, tflag)
        assert ((tj > 0) <= ((tflag & A.PTR_VARIANT) != 0)).all()
        for W in WE.LEVELS:
            loQ, loR = WE.origins(W, t2r, tj, r2q, Lq, Lr)
            assert loQ[0] == 0 and loR[0] == 0 and len(loQ) == -(-Lt // WE.STRIPE_ROWS[W])
            assert (loQ >= 0).all() and (loQ <= Lq - min(W, Lq)).all() and (loR >= 0).all() and (loR <= Lr - min(W, Lr)).all()
            if Lq <= W and Lr <= W:
                assert not loQ.any() and not loR.any()
    # the clamp at the plane's end is reached: a case whose last stripes sit at L - W
    hit = 0
    for sc, c in enumerate(cases):
        q2r, t2r, tflag, r2q, Lq, Lr, Lt = WE.arrays_of(batch, sc, 0)
        for W in (16, 64, 256):
            if Lq > W:
                hit += int(WE.origins(W, t2r, WE.tj_of(t2r, tflag), r2q, Lq, Lr)[0][-1] == Lq - W)
    assert hit >= 10, hit
