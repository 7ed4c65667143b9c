"""tests/wfa_cluster_cases.py is what it claims, shown on the CPU: every case has the job shapes, size classes, scores, doubling
rounds, first-hit diagonals and iteration counts it declares -- by the module's own restated arithmetic, and by the CPU oracle
(oracle/wfa_oracle.cpp) where the oracle keeps a figure -- and the reference fixtures cluster_biwfa_edges_* hold exactly these cases.
That the oracle equals the fixtures' answers is tests/test_ref_pins.py's generic pin; here only that it picks them up."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_lib as O  # noqa: E402
import ref_pins as R  # noqa: E402
import wfa_cluster_cases as W  # noqa: E402
from wfa_cluster_helpers import DEFINED, hap_of, oracle_run  # noqa: E402
from vcfdist_amd import cluster as K  # noqa: E402

def test_the_table_covers_what_the_module_says():
    groups = {g: [c for c in W.TABLE if c.group == g] for g in W.GROUPS}
    assert all(groups[g] for g in W.GROUPS) and sum(map(len, groups.values())) == len(W.TABLE)
    assert all(c.aim and c.name.startswith(c.group + "_") for c in W.TABLE)
    # bucket: both sides of each of the four LDS borders, by a deletion and by an insertion; two cases well inside the global class
    for b in range(4):
        for kind in ("del", "ins"):
            sides = {c.declare["jobs"][0, "fwd"][1] for c in groups["bucket"] if c.name.startswith(f"bucket_{kind}") and f"_{W.LIM[b] >> 10}k_" in c.name}
            assert sides == {b, b + 1}, (b, kind, sides)
    assert len([c for c in groups["bucket"] if c.name.startswith("bucket_global")]) == 2
    assert any(nb in W.LIM for c in groups["bucket"] for nb in c.declare.get("need", {}).values()), "no job needs exactly a launch's LDS"
    # stride: 63 .. 129 diagonals for the align job and for a reach job; first hits on lane 63, on lane 0 of the next chunk, on diagonal 0,
    # and on diagonal mat_len - 1 in the first, second and third chunk
    for kind in ("align", "fwd"):
        assert sorted(c.declare["jobs"][0, kind][0] for c in groups["stride"] if (0, kind) in c.declare.get("jobs", {})) == [63, 64, 65, 127, 128, 129]
    assert {c.declare["hit"][0, "fwd"] for c in groups["stride"] if "hit" in c.declare and not c.declare.get("last_diagonal")} == {0, 63, 64}
    assert sorted(c.declare["hit"][0, "fwd"] // 64 for c in groups["stride"] if c.declare.get("last_diagonal")) == [0, 1, 2]
    # ring: every penalty set of the swg pins, x == o + e and -o 0, below and above the ring length each (and at it where a cluster can)
    import ast
    import re
    text = open(os.path.join(HERE, "golden", "make_ref_goldens.py")).read()
    assert tuple(ast.literal_eval(re.search(r"^PENALTIES = (\[.*?\])", text, re.M).group(1))) == W.PENALTIES
    for pen in W.PENALTIES + (W.PEN_EQ, W.PEN_OPEN0, W.PEN_EXACT):
        tags = {c.declare["ring"] for c in groups["ring"] if c.pen == pen}
        assert {"below", "above"} <= tags, pen
    assert W.PEN_EQ[0] == W.PEN_EQ[1] + W.PEN_EQ[2] and W.PEN_OPEN0[1] == 0
    assert any(c.pen[0] > c.pen[1] + c.pen[2] for c in groups["ring"]) and any(c.pen[0] < c.pen[2] for c in groups["ring"])
    # doubling: two, three and four calls of the sliding side, in a dinucleotide and in a homopolymer tract; both contig ends
    assert sorted(c.declare["calls"] for c in groups["doubling"] if "_dinuc_" in c.name) == [3, 4, 5]
    assert sorted(c.declare["calls"] for c in groups["doubling"] if "_homop_" in c.name) == [3, 4, 5]
    # merge: one, two and three merging iterations, each run at limits 1, 2 and 4
    assert [c.declare["iterations"][4] for c in groups["merge"]] == [2, 3, 4] and all(c.itrs == (1, 2, 4) for c in groups["merge"])


@pytest.mark.parametrize("case", W.TABLE, ids=lambda c: c.name)
def test_case_stays_clear_of_undefined_input(case):
    n = len(case.ctg)
    assert set(case.ctg) <= set("ACGT") and 40 <= n <= 7000
    last = 0
    for p, t, ref, alt in case.variants:
        assert t in (W.S, W.I, W.D) and case.ctg[p:p + len(ref)] == ref and ref != alt
        assert (len(ref), len(alt)) == {W.S: (1, 1), W.I: (0, len(alt)), W.D: (len(ref), 0)}[t] and len(ref) + len(alt) > 0
        assert p >= last, "records overlap"
        last = p + len(ref)
        if case.declare.get("undefined") != "pos0":
            assert p >= 1
        if not case.declare.get("last_base"):
            assert p + len(ref) <= n - 1
    if "clusters" in case.declare and not case.declare.get("undefined"):
        for cl in W.case_clusters(case):
            beg, end, _ = W.cluster_span(cl)
            assert len(W.apply_variants(case.ctg, cl, max(beg, 0), min(end, n))) > 0


@pytest.mark.parametrize("case", DEFINED, ids=lambda c: c.name)
def test_case_is_what_it_declares(case):
    d = case.declare
    n = len(case.ctg)
    it = max(case.itrs)
    got, st = oracle_run(case, it)
    # the final clusters
    assert got.var_beg.tolist() == [a for a, _ in d["clusters"]] + [len(case.variants)], (case.name, got.var_beg.tolist())
    clusters = W.case_clusters(case)
    scores = [W.cluster_score(case.ctg, cl, case.pen) for cl in clusters]
    # shapes and size classes of the jobs the case is aimed at
    for (c, kind), (mat_len, cls) in d.get("jobs", {}).items():
        j = W.align_job(clusters[c], n, case.pen) if kind == "align" else W.reach_job(clusters[c], n, case.pen, scores[c], kind == "rev", 1)
        assert j.mat_len == mat_len == j.q_len + j.r_len - 1, (case.name, kind, j)
        assert j.need_bytes == W.need_bytes(j.q_len, j.r_len, case.pen)
        if cls is not None:
            assert j.cls == cls and (cls == W.GLOBAL or j.need_bytes <= W.LIM[cls]) and (cls == 0 or j.need_bytes > W.LIM[cls - 1]), (case.name, j)
    for (c, kind), nb in d.get("need", {}).items():
        assert W.reach_job(clusters[c], n, case.pen, scores[c], kind == "rev", 1).need_bytes == nb
    # the ring's length against the score
    for c, sc in d.get("score", {}).items():
        assert scores[c] == sc, (case.name, c, scores[c], sc)
    if "ring" in d:
        rows = W.ring_rows(case.pen)
        assert all({"below": sc < rows, "at": sc == rows, "above": sc > rows}[d["ring"]] for sc in scores)
        if d["ring"] == "below":
            assert not any(rows > s > max(scores) for s in W._ring_recipes(case.pen)), "a score nearer to the ring length can be made"
        if d["ring"] == "above":
            assert not any(rows < s < min(scores) for s in W._ring_recipes(case.pen))
    # doubling rounds: the restated reach against what is declared and against the oracle's count
    single = st["iterations"] == 1
    if single:
        rounds = [(W.side_rounds(case.ctg, cl, case.pen, sc, True), W.side_rounds(case.ctg, cl, case.pen, sc, False)) for cl, sc in zip(clusters, scores)]
        assert sum(map(sum, rounds)) == st["reach_calls"], (case.name, rounds, st)
        assert st["align_calls"] == len(clusters)
        for c, r in d.get("rounds", {}).items():
            assert rounds[c] == r, (case.name, rounds)
    if "calls" in d:
        assert st["reach_calls"] == d["calls"], (case.name, st)
    if case.group == "doubling":
        assert "calls" in d and single and (d["calls"] > 2 or case.name == "doubling_reissue_1")          # (the counter-case: one base shorter)
    # first hits
    for (c, kind), hit_d in d.get("hit", {}).items():
        tr, j = W.side_trace(case.ctg, clusters[c], case.pen, scores[c], kind == "rev", 1)
        assert tr.d == hit_d and hit_d < j.mat_len, (case.name, tr, j)
        assert W.side_rounds(case.ctg, clusters[c], case.pen, scores[c], kind == "rev") == 1, "the side would be re-issued"
        if d.get("last_diagonal"):
            assert tr.d == j.mat_len - 1 and tr.reach == j.r_len - 1 and tr.s == case.pen[1] + (j.r_len - 1) * case.pen[2] <= scores[c], (case.name, tr, j)
        if d.get("two_values"):
            chunk = {v for k, v in tr.hits if k // 64 == tr.d // 64}
            assert len(chunk) > 1, (case.name, tr.hits)
    # iterations by limit
    for limit in case.itrs:
        want = d.get("iterations", {}).get(limit)
        if want is not None:
            assert oracle_run(case, limit)[1]["iterations"] == want, (case.name, limit)
    if case.group == "diag":
        md = [W.cluster_span(cl)[2] for cl in clusters]
        assert {"diag_positive": md[0] > 0, "diag_negative": md[0] < 0, "diag_cancel": md[0] == 0 and len(clusters[0]) == 2,
                "diag_sv_insertion": md[0] == -2000}[case.name]


def test_bucket_cases_predict_their_classes():
    """the class counts the GPU test holds vcl_wfa_last_classes to: every border case puts its reach jobs where it says, the mixed
    contig has jobs in all five classes, and its clusters stand in an order the stable sort has to change"""
    for c in (c for c in W.TABLE if c.group == "bucket"):
        pred = W.predicted_classes(c)
        _, st = oracle_run(c, max(c.itrs))
        assert sum(pred) == st["align_calls"] + st["reach_calls"], (c.name, pred, st)
        for (ci, kind), (_, cls) in c.declare.get("jobs", {}).items():
            assert pred[cls] >= 1
    mixed = W.BY_NAME["bucket_mixed"]
    assert all(k > 0 for k in W.predicted_classes(mixed)), W.predicted_classes(mixed)
    first = [W.reach_job(cl, len(mixed.ctg), mixed.pen, W.cluster_score(mixed.ctg, cl, mixed.pen), False, 1).cls for cl in W.case_clusters(mixed)]
    assert first != sorted(first) and set(first) == set(range(W.N_CLASSES)) and first[0] == first[-1] == W.GLOBAL, first


def test_the_restated_reach_equals_the_oracle_reaches():
    """reach_trace is a restatement of its own: on every single-iteration case its reaches, through the doubling rounds, give the
    oracle's left and right reach of every cluster"""
    n = 0
    for case in DEFINED:
        got, st = oracle_run(case, max(case.itrs))
        if st["iterations"] != 1 or case.name == "diag_sv_insertion":
            continue
        for c, cl in enumerate(W.case_clusters(case)):
            sc = W.cluster_score(case.ctg, cl, case.pen)
            beg, end, _ = W.cluster_span(cl)
            for rev in (True, False):
                rnd = W.side_rounds(case.ctg, cl, case.pen, sc, rev)
                tr, j = W.side_trace(case.ctg, cl, case.pen, sc, rev, rnd)
                if rev:
                    assert end - tr.reach == got.left_reach[c], (case.name, c, "left")
                else:
                    assert beg + tr.reach + 1 == got.right_reach[c], (case.name, c, "right")
                n += 1
    assert n > 250


# ---- the fixtures

def test_fixtures_hold_the_table():
    """one fixture per penalty set and iteration limit with exactly the table's cases, inputs included, and they are among the
    parameters of the generic pins (tests/test_ref_pins.py: oracle == reference; tests/test_gpu_ref_pins.py: kernel == reference)"""
    import test_ref_pins as TP
    sets = W.fixture_sets()
    assert len(sets) == len(W.PENALTIES) + 3 + 2          # every penalty set at limit 4; 5/6/2 also at 1 and 2
    pinned = [p.values[0] if hasattr(p, "values") else p for p in TP.test_cluster_oracles_equal_the_reference_clusters.pytestmark[0].args[1]]
    for (pen, itrs), cases in sets.items():
        name = W.fixture_name(pen, itrs)
        assert name in pinned and name in R.fixture_names("cluster_biwfa_edges_")
        fx = R.Fixture(name)
        assert fx.refused is None
        assert bytes(fx.extra["case_names"]).decode().split("\n") == [c.name for c in cases]
        o = R.case_args(fx.case)
        assert (o["sub"], o["open"], o["extend"], o["max_cluster_itrs"]) == pen + (itrs,) and o["cluster"][0] == "biwfa"
        for ctg, (c, (cname, seq)) in enumerate(zip(cases, R.case_contigs(fx.case))):
            s, _, _ = R.case_slot(fx.case, 0, ctg)
            assert cname == c.name and seq == c.ctg.encode()
            assert list(zip(s["pos"].tolist(), s["type"].tolist(), [r.decode() for r in s["ref"]], [a.decode() for a in s["alt"]])) == list(c.variants)
    assert {c.name for cs in sets.values() for c in cs} == {c.name for c in DEFINED}


def test_position_zero_is_refused_by_the_reference_and_by_us():
    """a variant at position 0: the region starts one base in front of the contig.  The reference's generate_str exits; the oracle
    and the library answer VCL_ERR_ARG (the library before it touches the device: tests/test_gpu_wfa_cluster_edges.py)"""
    assert [c.name for c in W.UNDEFINED] == ["edge_pos0"]
    fx = R.Fixture("cluster_biwfa_edges_pos0_refused")
    assert fx.refused is not None and "position out of range (generate_str)" in fx.refused, fx.refused
    case = W.BY_NAME["edge_pos0"]
    assert R.case_contigs(fx.case)[0][1] == case.ctg.encode() and R.case_slot(fx.case, 0, 0)[0]["pos"].tolist() == [0]
    with pytest.raises(ValueError):
        K.wfa_cluster(hap_of(case), case.ctg, L=O.lib(), prefix="vco")


def test_a_variant_past_the_contigs_end_is_refused_by_the_oracle_and_the_library():
    """the other half of the argument check: a deletion whose REF allele passes the contig's last base has no region to generate;
    the oracle and the library (before it touches a device: this runs without one) answer VCL_ERR_ARG.  Position 0 likewise."""
    ctg = W.BY_NAME["edge_pos1"].ctg
    n = len(ctg)
    for hap in (K.HapSeq([n - 2], [W.D], [ctg[n - 2:] + "A"], [""]), K.HapSeq([n], [W.S], ["A"], ["C"]), hap_of(W.BY_NAME["edge_pos0"])):
        with pytest.raises(ValueError, match="vco_wfa_cluster failed: -1$"):
            K.wfa_cluster(hap, ctg, L=O.lib(), prefix="vco")
        with pytest.raises(ValueError, match="vcl_wfa_cluster failed: -1$"):
            K.wfa_cluster(hap, ctg)
    # a deletion that ends on the last base is an input like any other for the oracle (the reference answers it too)
    K.wfa_cluster(K.HapSeq([n - 3], [W.D], [ctg[n - 3:]], [""]), ctg, L=O.lib(), prefix="vco")
