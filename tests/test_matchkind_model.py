"""The brute-force model of the match kinds (tests/matchkind_model.py) on the hand cases evaluated by the CPU oracle, the C ABI's
declarations, the writer of match-kinds*.tsv, the command lines' parse-time behaviour, and the conditions the GPU tests' inputs
(tests/matchkind_cases.py) have to meet for those tests not to pass vacuously."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import matchkind_cases as MC
import matchkind_model as MM
import oracle_lib as O
from vcfdist_amd import _abi as A
from vcfdist_amd import api, report as RP, summary as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def evaluated(v, sv_threshold=50):
    """a batch through the CPU oracle: results, phase-block phasing (one phase set) and the variant classes"""
    batch = O.generate(v)
    res = O.run(batch)
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32), L=O.lib(), prefix="vso")
    cls = [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold) for s in range(4)]
    return batch, res, pb, cls


def check_invariant(v, batch, res, pb, cls, kd, min_qual=0, max_qual=60):
    """for every type and threshold the query's kinds sum to the counters' query TP, the truth's to their truth TP"""
    cnt = MM.counts(v, res, pb, kd, cls, min_qual, max_qual)
    plain = O.oracle_pr_counts(O.lib(), batch.var_off, res, cls, pb, min_qual, max_qual)
    assert np.array_equal(cnt[0].sum(1), plain[0, :, A.ERRTYPE_TP]) and np.array_equal(cnt[1].sum(1), plain[1, :, A.ERRTYPE_TP])
    assert np.array_equal(cnt[:, 3], cnt[:, :3].sum(1))
    return cnt, plain


def test_header_and_library_agree():
    text = open(os.path.join(ROOT, "include", "vcfdist_matchkind.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b(v(?:pr|rp)_\w+)\s*\(", code)
    assert sorted(names) == sorted(api.MATCHKIND_EXPORTED) and len(names) == 6
    L = api.lib()
    for n in names:
        assert hasattr(L, n), n
    codes = [int(re.search(rf"#define VPR_MK_{k} (\d+)", text).group(1)) for k in ("EXACT", "SHIFTED", "REGROUPED", "PARTIAL", "KINDS", "NONE")]
    assert codes == [A.MK_EXACT, A.MK_SHIFTED, A.MK_REGROUPED, A.MK_PARTIAL, A.MK_KINDS, A.MK_NONE] == [0, 1, 2, 3, 4, 255]
    assert api.matchkind_names() == MM.NAMES == ["exact", "shifted", "regrouped", "partial"]
    # these are this project's definitions, and both the header and the README say so in bold
    assert re.search(r"\*\*These are this project's own definitions[^*]*NOT a reproduction[^*]*\*\*", text, re.S)
    assert re.search(r"\*\*[^*]*match kinds[^*]*this project's own definitions[^*]*\*\*", open(os.path.join(ROOT, "README.md")).read(), re.S)


# ---- the model on the definitions

@pytest.fixture(scope="module")
def hand():
    v, cases = MC.hand_case()
    batch, res, pb, cls = evaluated(v)
    return dict(v=v, cases=cases, batch=batch, res=res, pb=pb, cls=cls)


def test_hand_cases_literally(hand):
    v, cases, res, pb = hand["v"], hand["cases"], hand["res"], hand["pb"]
    kd = MM.kinds(v, res, pb)
    for name, slot, k, want in MC.EXPECT:
        assert kd[slot][MC.index_of(v, cases, name, slot, k)] == want, (name, slot, k)
    at = lambda name, slot, k=0: MC.index_of(v, cases, name, slot, k)
    col = lambda field, name, slot, k=0, w=0: getattr(res, field)[slot][w][at(name, slot, k)]
    # what the cases are built for, on the oracle's own results
    assert col("query_ed", "shifted", 0) == 0 and col("ref_ed", "shifted", 0) == 1
    assert col("sync_group", "shifted", 0) == col("sync_group", "shifted", 2)
    assert col("ref_ed", "regrouped", 0) == 2 and col("query_ed", "regrouped", 0) == 0
    assert col("query_ed", "partial", 0) == 1 and col("ref_ed", "partial", 0) == 10 and abs(col("credit", "partial", 0) - 0.9) < 1e-6
    # interleaved: the insertion is FP on the REF plane with a group of its own between two members of one group
    g = [int(col("sync_group", "interleaved", 0, k)) for k in range(3)]
    assert g[0] == g[2] != g[1] and col("errtype", "interleaved", 0, 1) == A.ERRTYPE_FP and col("ref_ed", "interleaved", 0, 1) == 0
    assert [f[:2] for f in MM.interleaved_groups(v, res, pb)] == [(0, cases["interleaved"]), (1, cases["interleaved"])]
    # het_shift: phased SWAP, so query 1 is compared with truth 2
    assert res.sc_phase[cases["het_shift"]] == A.PHASE_SWAP and res.sc_phase[cases["shifted"]] == A.PHASE_NONE
    assert col("sync_group", "het_shift", 0, 0, 1) == col("sync_group", "het_shift", 3, 0, 1)
    assert MC.populated(kd) == ([0, 1, 2, 3], [0, 1, 2, 3])
    assert set(np.unique(np.concatenate(kd))) == {0, 1, 2, 3, A.MK_NONE}


@pytest.mark.parametrize("pb_kind", ["null", "zeros", "ones"])
def test_hand_cases_under_either_phase_block_phasing(hand, pb_kind):
    """the superclusters left NONE follow pb_phase: the cases are symmetric in it, so the kinds do not depend on it"""
    v, cases, res = hand["v"], hand["cases"], hand["res"]
    pb = None if pb_kind == "null" else np.full(v.n_sc, pb_kind == "ones", np.int32)
    kd = MM.kinds(v, res, pb)
    for name, slot, k, want in MC.EXPECT:
        assert kd[slot][MC.index_of(v, cases, name, slot, k)] == want, (name, slot, k)


def test_invariant_and_thresholds(hand):
    v, batch, res, pb, cls = hand["v"], hand["batch"], hand["res"], hand["pb"], hand["cls"]
    kd = MM.kinds(v, res, pb)
    for mn, mx in ((0, 60), (15, 40), (30, 30), (7, 60), (0, 4)):
        cnt, plain = check_invariant(v, batch, res, pb, cls, kd, mn, mx)
        assert plain[0, 3, A.ERRTYPE_TP].any() and plain[1, 3, A.ERRTYPE_TP].any()
    # the low-quality pair: matched up to threshold 10 in both callsets, at no threshold from a min_qual of 15 on
    full, _ = check_invariant(v, batch, res, pb, cls, kd, 0, 60)
    cnt, _ = check_invariant(v, batch, res, pb, cls, kd, 15, 40)
    for cs in (0, 1):
        assert full[cs, 0, A.MK_EXACT, 10] - full[cs, 0, A.MK_EXACT, 11] == 2 and cnt[cs, 0, A.MK_EXACT, 0] == full[cs, 0, A.MK_EXACT, 15]
        assert (np.diff(full[cs], axis=-1) <= 0).all()                             # a TP counts up to its bin, in either callset
    # the query's split records count one each, the truth's record once
    assert full[0, 1, A.MK_REGROUPED, 0] == 8 and full[1, 1, A.MK_REGROUPED, 0] == 4


# ---- non-vacuity of the GPU tests' inputs

def test_random_edge_and_long_batches_are_not_vacuous():
    v = MC.random_variants()
    assert [v.n_vars(s) for s in range(4)] == [513, 257, 640, 300] and v.n_sc == 300
    batch, res, pb, cls = evaluated(v, sv_threshold=6)
    assert (res.sc_phase == A.PHASE_SWAP).any() and (res.sc_phase == A.PHASE_NONE).any()
    kd = MM.kinds(v, res, pb)
    assert MC.populated(kd) == ([0, 1, 2, 3], [0, 1, 2, 3])                         # all four kinds in both callsets
    assert len(MM.interleaved_groups(v, res, pb)) >= 1
    cnt, plain = check_invariant(v, batch, res, pb, cls, kd)
    assert all(plain[:, t, A.ERRTYPE_TP].any() for t in range(3))                   # SNP, INDEL and SV rows
    e = MC.edge_variants()
    assert [e.n_vars(s) for s in range(4)] == [1, 0, 513, 0]
    batch, res, pb, cls = evaluated(e)
    kd = MM.kinds(e, res, pb)
    assert kd[1].shape == (0,) and (kd[2] == A.MK_NONE).sum() > 500
    check_invariant(e, batch, res, pb, cls, kd)
    lg = MC.long_variants()
    assert lg.n_sc == 1 and all(270 <= lg.n_vars(s) <= 330 for s in range(4))       # a range that crosses a 256-thread block
    batch, res, pb, cls = evaluated(lg)
    kd = MM.kinds(lg, res, pb)
    cnt, _ = check_invariant(lg, batch, res, pb, cls, kd)
    assert cnt[0, 3, A.MK_SHIFTED, 0] == cnt[1, 3, A.MK_SHIFTED, 0] == 2 * (len(MC.LONG_PLANTS) - 1) and cnt[0, 3, A.MK_EXACT, 0] > 500
    assert len(MM.interleaved_groups(lg, res, pb)) == 2 and (kd[0] == A.MK_NONE).sum() == len(MC.LONG_FP) + 1
    # the group split around the REF-plane FP lies behind the first block's edge, its compared range in front of it
    i = int(np.nonzero(kd[0] == A.MK_REGROUPED)[0][0])
    assert 200 < i < 256 < lg.n_vars(0)


def test_demo_kinds():
    """the kinds the demo callsets populate: the command-line test may assert non-vacuity for these only"""
    import demo_pipeline as D
    rows, det = D.run(product=False)
    v, cls = MC.demo_variants(det)
    kd = MM.kinds(v, det["res"], det["pb"])
    assert MC.populated(kd) == (MC.DEMO_POPULATED_QUERY, MC.DEMO_POPULATED_TRUTH)
    cnt, plain = check_invariant(v, det["batch"], det["res"], det["pb"], cls, kd, D.G["min_qual"], D.G["max_qual"])
    assert np.array_equal(plain, det["counts"])


# ---- the writer

def test_writer_equals_the_model(hand, tmp_path):
    v, batch, res, pb, cls = hand["v"], hand["batch"], hand["res"], hand["pb"], hand["cls"]
    kd = MM.kinds(v, res, pb)
    for mn, mx in ((0, 60), (15, 40)):
        cnt, plain = check_invariant(v, batch, res, pb, cls, kd, mn, mx)
        pre = str(tmp_path / f"{mn}_{mx}_")
        RP.write_match_kinds(pre, cnt, plain, mn, mx)
        want_all, want_sum = MM.tsv_text(cnt, plain, mn, mx)
        assert open(pre + "match-kinds.tsv").read() == want_all and open(pre + "match-kinds-summary.tsv").read() == want_sum
        head = want_sum.split("\n")[0].split("\t")
        assert head[:3] == ["VAR_TYPE", "THRESHOLD", "MIN_QUAL"] and head[3:] == MM.COLUMNS and len(MM.COLUMNS) == 10
        assert MM.COLUMNS == "QUERY_TP QTP_EXACT QTP_SHIFTED QTP_REGROUPED QTP_PARTIAL TRUTH_TP TTP_EXACT TTP_SHIFTED TTP_REGROUPED TTP_PARTIAL".split()
        assert len(want_all.split("\n")) == 4 * (mx - mn + 1) + 2 and len(want_sum.split("\n")) == 10
        assert re.fullmatch(r"[0-9\t\n]*", re.sub(r"(?m)^[A-Z]+\t(?:[A-Z]+\t)?", "", want_all.split("\n", 1)[1]))      # integers only
    with pytest.raises(RP.ReportError):
        RP.write_match_kinds(str(tmp_path / "no" / "such") + "/", cnt, plain, 15, 40)
    with pytest.raises(RP.ReportError):
        RP.write_match_kinds(pre, cnt, plain, 0, 60)                                # counts of another number of thresholds


# ---- the command lines, up to where the inputs are read

GOOD_OPTIONS = (["--classify-matches"], ["--classify-matches", "-n"], ["--classify-matches", "--classify-errors", "--stratify-variants", "--bootstrap", "4"])


def test_cxx_command_line_parses_the_option(tmp_path):
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa"), "-p", str(tmp_path) + "/"]
    for opts in GOOD_OPTIONS:
        r = subprocess.run([cli] + missing + opts, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "unknown option" not in r.stderr and "no_query" in r.stderr, (opts, r.stderr)
    r = subprocess.run([cli] + missing + ["--classify-matchs"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "unknown option '--classify-matchs'" in r.stderr and r.stdout == ""


def test_python_command_line_parses_the_option(tmp_path, capsys):
    from vcfdist_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    out = capsys.readouterr().out
    assert e.value.code == 0 and "--classify-matches" in out and "match-kinds.tsv" in out
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa"), "-p", str(tmp_path) + "/"]
    for opts in GOOD_OPTIONS:
        with pytest.raises(Exception) as e:                                        # (the first input does not exist)
            main(missing + opts)
        assert "no_query" in str(e.value), (opts, e.value)
    r = subprocess.run([sys.executable, "-m", "vcfdist_amd"] + missing + ["--classify-matchs"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode != 0 and "--classify-matchs" in r.stderr
