"""The dense level's column strips (pr_strip.hip) on the cases of tests/strip_cases.py: every result array against the oracle, bit
for bit, under band_mode 0 and 1; the strip plan the library kept (VPR_CFG_KEEP_STRIP_PLAN) against the model of k_strip_plan,
for every alignment of every planner call -- an alignment the model cuts and the library left to the one-workgroup kernels is a
failure --; the same arrays from the one-workgroup kernels (VPR_NO_STRIPS), without the skipped blocks (VPR_NO_UB), through
vpr_upload_variants and from a second execute of the resident batch.  One test per family, and one with the whole table in one
batch, in table order and reversed: the planner's slot offsets, the strip-major ticket list and the workspace offsets then see
alignments of many sizes side by side.  The oracle runs once per case (strip_cases.oracle_results)."""
import time

import pytest

import strip_cases as S
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu


def _check_plan(pr, batch, cases, band_mode):
    """the kept plan against the model; -> the records"""
    recs = pr.strip_plan()
    wide = {(sc, aln) for sc in range(batch.n_sc) for aln in range(4)
            if max(batch.lens(sc)[aln >> 1], batch.lens(sc)[4]) >= S.STRIP_MIN}
    for r in recs:
        key = (r["sc"], r["aln"])
        assert key in wide, r                                    # (narrower alignments never reach the planner)
        model = S.plan_strips(batch, *key)
        assert r["ok"] == (1 if model is not None else 0), (cases[r["sc"]].name, r, model)
        assert r["strips"] == (model or []), (cases[r["sc"]].name, r, model)
        assert r["from_window"] == (1 if band_mode and not r["tie_round"] else 0), r
    first = [(r["sc"], r["aln"]) for r in recs if not r["tie_round"]]
    assert len(set(first)) == len(first)                         # one planner call per alignment outside the tie rounds
    if band_mode == 0:
        assert set(first) == wide                                # the dense plan of round 0 holds every wide alignment
    for sc, c in enumerate(cases):                               # what the table declares (the model agrees: test_strip_cases.py)
        for r in recs:
            if r["sc"] == sc:
                ok, n = ((c.ok, c.n_strips), (c.ok2, c.n2))[r["aln"] >> 1]
                assert (r["ok"], len(r["strips"])) == (ok, n), (c.name, r)
    return recs


def _run_all(cases, monkeypatch, no_ub=False, reverse=False):
    t0 = time.time()
    cases = list(reversed(cases)) if reverse else list(cases)
    v, batch = S.batch_of(cases)
    want = S.expected(cases, batch)
    n_tie = int(((want.aln_status & A.ST_SWAP_TIE) != 0).sum())
    t_oracle = time.time() - t0
    kept = {}
    for band_mode in (0, 1):
        pr = api.PrecisionRecall(A.default_config(band_mode=band_mode, flags=A.CFG_KEEP_STRIP_PLAN))
        got = pr.run(batch)
        assert not got.diff(want), (band_mode, got.diff(want)[:4])
        assert pr.timing().n_tie_replays >= n_tie
        recs = kept[band_mode] = _check_plan(pr, batch, cases, band_mode)
        names = {s.kernel.decode() for s in pr.launch_stats()}
        if any(r["ok"] == 1 for r in recs):
            assert "k_fwd_strip" in names and "k_bwd_strip" in names
        if any(r["ok"] == 0 for r in recs):                      # the one-workgroup names beside the strips'
            assert any(n.startswith("k_fwd<1024") for n in names) and any(n.startswith("k_bwd<1024") for n in names), names
        pr.execute()                                             # the resident batch again
        again = pr.download()
        assert not again.diff(want), (band_mode, "second execute", again.diff(want)[:4])
        assert pr.strip_plan() == recs
        for var in ("VPR_NO_STRIPS",) + (("VPR_NO_UB",) if no_ub and band_mode else ()):
            monkeypatch.setenv(var, "1")
            pr2 = api.PrecisionRecall(A.default_config(band_mode=band_mode, flags=A.CFG_KEEP_STRIP_PLAN))
            other = pr2.run(batch)
            monkeypatch.delenv(var)
            assert not other.diff(want), (band_mode, var, other.diff(want)[:4])
            if var == "VPR_NO_STRIPS":
                assert pr2.strip_plan() == [] and "k_fwd_strip" not in {s.kernel.decode() for s in pr2.launch_stats()}
            else:
                assert pr2.strip_plan() == recs
    pr = api.PrecisionRecall(A.default_config(flags=A.CFG_KEEP_STRIP_PLAN))
    pr.upload_variants(v.as_struct(), batch)                     # generate_ptrs_strs on the device
    pr.execute()
    got = pr.download()
    assert not got.diff(want), ("vpr_upload_variants", got.diff(want)[:4])
    assert pr.strip_plan() == kept[1]
    pr = api.PrecisionRecall(A.default_config(band_mode=0))      # without the flag: nothing kept
    assert not pr.run(batch).diff(want) and pr.strip_plan() == []
    print(f"{len(cases)} cases, {sum(len(k) for k in kept.values())} plan records, wall {time.time() - t0:.2f} s (oracle {t_oracle:.2f} s)")
    return want, kept


def _family(name):
    return [c for c in S.TABLE if c.family == name]


def test_widths(monkeypatch):
    _run_all(_family("widths"), monkeypatch)


def test_cut_residues(monkeypatch):
    _run_all(_family("residue"), monkeypatch)


@pytest.mark.parametrize("half", [0, 1])
def test_pushed_cuts(monkeypatch, half):
    cases = _family("push")
    _run_all(cases[:len(cases) // 2] if half == 0 else cases[len(cases) // 2:], monkeypatch)


def test_no_cut_and_more_cuts_than_slots(monkeypatch):
    cases = _family("nocut") + _family("slots")
    _, kept = _run_all(cases, monkeypatch)
    assert len(kept[0]) == 4 * len(cases) and all(r["ok"] == 0 for r in kept[0])


@pytest.mark.parametrize("strips", [2, 3])
def test_row_blocks(monkeypatch, strips):
    _run_all([c for c in _family("rows") if c.n_strips == strips], monkeypatch)


def test_what_crosses_the_cut(monkeypatch):
    _run_all(_family("cross"), monkeypatch)


def test_ties_behind_a_cut(monkeypatch):
    want, kept = _run_all(_family("ties"), monkeypatch)
    assert ((want.aln_status & A.ST_SWAP_TIE) != 0).all()
    assert any(r["tie_round"] for r in kept[0])                  # the dense tie round planned them again


def test_blocks_skipped_under_the_upper_bound(monkeypatch):
    cases = _family("ub")
    _, kept = _run_all(cases, monkeypatch, no_ub=True)
    for sc in range(len(cases)):                                 # the truth-only deletion sent (query 1, truth 1) through the windows
        assert any(r["sc"] == sc and r["aln"] == 0 and r["from_window"] and r["ok"] == 1 for r in kept[1]), cases[sc].name


def test_other_bytes(monkeypatch):
    _run_all(_family("bytes"), monkeypatch)


@pytest.mark.parametrize("reverse", [False, True])
def test_whole_table_in_one_batch(monkeypatch, reverse):
    _, kept = _run_all(S.TABLE, monkeypatch, reverse=reverse)
    sizes = {len(r["strips"]) for r in kept[0]}
    assert sizes >= {0, 1, 2, 3}
