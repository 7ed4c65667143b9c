"""tests/strip_cases.py is what it claims (no GPU): the table's declared expectations against the model of k_strip_plan, the
residues of the cuts, what the oracle's path does at the cut of every crossing case, that each of the planner's five conditions
decides some cut, and that the constants were found in the sources."""
import collections

import numpy as np
import pytest

import oracle_lib as O
import strip_cases as S
from vcfdist_amd import _abi as A


@pytest.fixture(scope="module")
def table():
    """(batch of the whole table, {case name: (plan of query hap 1, plan of query hap 2)})"""
    _, batch = S.batch_of(S.TABLE)
    plans = {c.name: (S.plan_strips(batch, i, 0), S.plan_strips(batch, i, 2)) for i, c in enumerate(S.TABLE)}
    return batch, plans


def test_constants_come_from_the_sources():
    assert S.ST_CAP == 1024 * 4 - 8 and S.slots_of(S.ST_CAP, 1) == 4 and S.slots_of(1, S.ST_CAP + 1) == 6
    assert "ST_CAP - 1) / ST_CAP" in S.SLOTS_TEXT
    assert S.L2 - S.ST_CAP in range(12, 213) and S.L3 - 2 * S.ST_CAP in range(12, 213)       # (the smallest regions that show a cut)


def test_names_and_families():
    names = [c.name for c in S.TABLE]
    assert len(set(names)) == len(names)
    assert set(c.family for c in S.TABLE) == set(S.FAMILIES)
    n = collections.Counter(c.family for c in S.TABLE)
    assert all(n[f] <= 8 for f in S.FAMILIES), n
    assert all(c.aim for c in S.TABLE)


def test_declared_expectations_against_the_model(table):
    batch, plans = table
    for i, c in enumerate(S.TABLE):
        lq1, lq2, _, _, lr = batch.lens(i)
        for plan, ok, n, lq in ((plans[c.name][0], c.ok, c.n_strips, lq1), (plans[c.name][1], c.ok2, c.n2, lq2)):
            assert max(lq, lr) >= S.STRIP_MIN, c.name        # (the planner sees it)
            assert max(lq, lr) <= 32768                      # (the one-workgroup kernels can hold it: a refusal is ok == 0, not 2)
            assert (plan is not None) == (ok == 1) and (0 if plan is None else len(plan)) == n, (c.name, plan)
            if plan is None:
                continue
            # a plan tiles both planes, within a strip's capacity
            assert plan[0][:2] == (0, 0) and plan[-1][2:] == (lq, lr)
            for a, b in zip(plan, plan[1:]):
                assert a[2:] == b[:2]
            assert all(0 < s[2] - s[0] <= S.ST_CAP and 0 < s[3] - s[1] <= S.ST_CAP for s in plan), (c.name, plan)


def test_widths(table):
    batch, plans = table
    w = {c.name: batch.lens(i)[4] for i, c in enumerate(S.TABLE) if c.family == "widths"}
    assert sorted(w.values()) == [S.STRIP_MIN, S.ST_CAP, S.ST_CAP + 1, 2 * S.ST_CAP - 1, 2 * S.ST_CAP + 1]
    assert plans["width_cap+1"][0][-1] == (S.ST_CAP, S.ST_CAP, S.ST_CAP + 1, S.ST_CAP + 1)      # a last strip of one column
    assert plans["width_2cap+1"][0][-1][0] == 2 * S.ST_CAP


def test_cut_residues_cover_both_planes(table):
    _, plans = table
    seen, differ = [set(), set()], 0
    for c in S.TABLE:
        if c.family != "residue":
            continue
        for plan in plans[c.name]:
            for s in plan[1:]:
                seen[0].add(s[0] % 4)
                seen[1].add(s[1] % 4)
                differ += s[0] % 4 != s[1] % 4
    assert seen == [{0, 1, 2, 3}, {0, 1, 2, 3}] and differ >= 1


def test_pushed_cuts_moved(table):
    _, plans = table
    natural = (S.ST_CAP, S.ST_CAP)
    moved = {c.name: plans[c.name][0][1][:2] for c in S.TABLE if c.family == "push"}
    for name in ("push_snp_on", "push_snp_before", "push_snp_behind"):      # a SNP keeps the planes 1:1: the cut stays
        assert moved.pop(name) == natural
    assert all(m[0] < natural[0] or m[1] < natural[1] for m in moved.values()), moved
    assert moved["push_cap_q"] == (S.ST_CAP, S.ST_CAP - 300)      # the QUERY plane is full 300 REF columns early
    assert plans["push_adjacent_dels"][1][1][:2] != plans["push_adjacent_dels"][0][1][:2]


def test_row_blocks(table):
    batch, _ = table
    rows = {2: set(), 3: set()}
    for i, c in enumerate(S.TABLE):
        if c.family == "rows":
            rows[c.n_strips] |= set(batch.lens(i)[2:4])
    assert rows[2] == {1, 2, 63, 64, 65, 127, 128, 129} and rows[3] == {64, 65}


@pytest.mark.parametrize("name", [c.name for c in S.TABLE if c.family == "cross"])
def test_the_oracles_path_crosses_the_cut_as_declared(table, name):
    batch, plans = table
    i = [c.name for c in S.TABLE].index(name)
    one = batch.subset([i])
    edges, dels = S.crossing_edges(one, 0, 0, plans[name][0])
    aim = S.TABLE[i].aim
    if aim == "DEL":
        assert dels == [3] and edges == ["MAT"]
    else:
        assert edges == [aim] and dels == [0]


def test_crossing_cases_cover_every_edge_type():
    assert {c.aim for c in S.TABLE if c.family == "cross"} == {"MAT", "SUB", "DEL", "INS", "SWAP_Q2R", "SWAP_R2Q"}


def test_tie_cases_tie_in_the_oracle():
    cases = [c for c in S.TABLE if c.family == "ties"]
    assert [c.n_strips for c in cases] == [2, 3]
    for c in cases:
        st = S.oracle_results([c])[c.name]["aln_status"]
        assert ((st & A.ST_SWAP_TIE) != 0).all(), (c.name, st)
        _, b = S.batch_of([c])
        plan = S.plan_strips(b, 0, 0)
        # the tract lies behind a cut: in strip 1 of two, in the middle strip of three
        first = int(np.flatnonzero(b.hap_flag[2][:] & A.PTR_VARIANT)[0])
        assert plan[1][1] < b.hap_ptr[2][first] < plan[1][3] and b.hap_ptr[2][first] - plan[1][1] < (20 if len(plan) == 2 else 1 << 30), c.name


@pytest.mark.parametrize("cond", S.CONDITIONS)
def test_every_condition_of_the_planner_decides_a_cut(table, cond):
    batch, plans = table
    without = S.model_without(cond)
    hit = [c.name for i, c in enumerate(S.TABLE) if without(batch, i, 0) != plans[c.name][0] or without(batch, i, 2) != plans[c.name][1]]
    if cond in S.EDITED:
        # (no array the generator writes separates these from the pointer equalities, strip_cases.py: a hand-made one does)
        assert not hit
        b = S.edited(cond)
        full, cut = S.plan_strips(b, 0, 0), without(b, 0, 0)
        assert cut[1][:2] == (S.ST_CAP, S.ST_CAP) and full[1][1] < S.ST_CAP and full != cut
        q2r, _, r2q, _ = S.hap_arrays(b, 0, 0)                      # (the equalities hold on the natural cut)
        c_ = S.ST_CAP
        assert r2q[c_] == c_ and r2q[c_ - 1] == c_ - 1 and q2r[c_] == c_ and q2r[c_ - 1] == c_ - 1
    else:
        assert hit, cond
    print(cond, hit)


def test_slot_limit():
    assert S.search_slot_overflow() == (S.OVERFLOW_N, 9, 8)
    c = [c for c in S.TABLE if c.family == "slots"][0]
    _, b = S.batch_of([c])
    lq, _, _, _, lr = b.lens(0)
    assert S.plan_strips(b, 0, 0) is None and len(S.plan_strips(b, 0, 0, slots=9)) == 9 and S.slots_of(lq, lr) == 8
    # and a case of the table that fits its slots is refused with one slot fewer
    _, b = S.batch_of([S.TABLE[2]])
    assert len(S.plan_strips(b, 0, 0)) == 2 and S.plan_strips(b, 0, 0, slots=1) is None
