"""The model of the label counts cut by stratum and resampled (tests/labelcut_model.py) on batches evaluated by the CPU oracle: hand
counts for three strata, the sum identities against the stratified and the replicate counters' models, the per-variant table the
GPU tests use against the literal statement, the percentile picks, the writers against the model's text, the header, and the
command lines' parse-time checks of --cut-classes."""
import os
import re
import subprocess

import numpy as np
import pytest

import bootstrap_model as BM
import errclass_cases as EC
import errclass_model as EM
import labelcut_model as LM
import matchkind_cases as MC
import matchkind_model as MM
import oracle_lib as O
import strata_model as SM
from vcfdist_amd import _abi as A
from vcfdist_amd import api, report as RP, summary as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def evaluated(v, sv_threshold=50):
    """a batch through the CPU oracle: results, phase-block phasing (one phase set) and the variant classes"""
    batch = O.generate(v)
    res = O.run(batch)
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32), L=O.lib(), prefix="vso")
    cls = [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold) for s in range(4)]
    return dict(v=v, batch=batch, res=res, pb=pb, cls=cls)


def labels_of(P, e):
    return EM.classes(e["v"], e["res"], e["pb"], 50) if P is LM.ERRCLASS else MM.kinds(e["v"], e["res"], e["pb"])


def words_from(members):
    """membership words per slot from members[k][slot] bool arrays"""
    out = []
    for s in range(4):
        w = np.zeros(((len(members) + 63) // 64, len(members[0][s])), np.uint64)
        for k, m in enumerate(members):
            w[k >> 6] |= np.asarray(m[s], np.uint64) << np.uint64(k & 63)
        out.append(w)
    return out


@pytest.fixture(scope="module")
def hand():
    v, cases = EC.hand_case()
    e = evaluated(v)
    e["cases"] = cases
    return e


@pytest.fixture(scope="module", params=["errclass", "matchkind"])
def rand(request):
    P = LM.PASSES[request.param]
    e = evaluated((EC if P is LM.ERRCLASS else MC).random_variants(), 6)
    e["P"], e["bytes"] = P, labels_of(P, e)
    rng = np.random.RandomState(5)
    e["members"] = [[rng.rand(e["v"].n_vars(s)) < p for s in range(4)] for p in (1.0, 0.0, 0.5, 0.1)]
    return e


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "vcfdist_labelcut.h")).read()
    names = re.findall(r"\b(v(?:pr|rp)_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert sorted(names) == sorted(api.LABELCUT_EXPORTED) and len(names) == 16
    for h in ("vcfdist_errclass.h", "vcfdist_matchkind.h"):
        body = open(os.path.join(ROOT, "include", h)).read()
        assert '#include "vcfdist_labelcut.h"' in body and "Cut by stratum and resampled" in body


def test_hand_counts_for_three_strata(hand):
    """everything, nothing, and a stratum that holds the `site` supercluster's first query FP (class site) and the lone truth FN
    (class alone) but not, for one, the query FP of `dist_51` (class alone)"""
    v, cases, res, pb, cls = hand["v"], hand["cases"], hand["res"], hand["pb"], hand["cls"]
    cl = EM.classes(v, res, pb, 50)
    i, j, other = EC.index_of(v, cases, "site", 0), EC.index_of(v, cases, "lone_truth", 3), EC.index_of(v, cases, "dist_51", 0)
    assert (cl[0][i], cl[3][j], cl[0][other]) == (A.EC_SITE, A.EC_ALONE, A.EC_ALONE) and res.callq[0][0][i] == 30.0
    two = [np.zeros(v.n_vars(s), bool) for s in range(4)]
    two[0][i] = two[3][j] = True
    members = [[np.ones(v.n_vars(s), bool) for s in range(4)], [np.zeros(v.n_vars(s), bool) for s in range(4)], two]
    words = words_from(members)
    got = LM.strata_counts(LM.ERRCLASS, v, res, pb, cl, cls, words, 3)
    assert got.shape == (3, 2, 4, 7, 61)
    # everything: the unstratified counts; at threshold 0 the 24 query FP of error-classes-summary.tsv, class by class
    assert np.array_equal(got[0], EM.counts(v, res, pb, cl, cls))
    assert got[0][0, 3, :, 0].tolist() == [1, 4, 3, 5, 6, 5, 0] and got[0][1, 3, :, 0].tolist() == [1, 4, 3, 9, 6, 3, 0]
    assert not got[1].any()
    want = np.zeros((2, 4, 7, 61), np.int64)
    want[0, 0, A.EC_SITE, :31] = want[0, 3, A.EC_SITE, :31] = 1          # a query FP of quality 30: thresholds 0..30
    want[1, 0, A.EC_ALONE, :] = want[1, 3, A.EC_ALONE, :] = 1            # a truth FN: every threshold
    assert np.array_equal(got[2], want)
    # and the same through a range with a min_qual: the FP counts at 15..30 of 15..40
    got = LM.strata_counts(LM.ERRCLASS, v, res, pb, cl, cls, words, 3, 15, 40)
    assert got[2][0, 0, A.EC_SITE].tolist() == [1] * 16 + [0] * 10 and got[2][1, 3, A.EC_ALONE].tolist() == [1] * 26


@pytest.mark.parametrize("mn,mx", [(0, 60), (15, 40)])
def test_sum_identities(rand, mn, mx):
    P, v, batch, res, pb, cls, b = (rand[k] for k in ("P", "v", "batch", "res", "pb", "cls", "bytes"))
    words = words_from(rand["members"])
    F = LM.fast(P, v, res, pb, b, cls, mn, mx)
    got = F.strata_counts(words, 4)
    assert np.array_equal(got[0], P.counts(v, res, pb, b, cls, mn, mx)) and not got[1].any() and got[3].any()
    for k, member in enumerate(rand["members"]):
        if k >= 2:                                                        # the table against the literal statement
            assert np.array_equal(got[k], P.counts(v, res, pb, LM.masked(b, member), cls, mn, mx)), k
        strat = SM.expected_counts(batch.var_off, res, cls, pb, member, mn, mx)
        for cs in range(2):                                               # every type, every threshold
            assert np.array_equal(got[k][cs].sum(1), strat[cs, :, P.sums[cs]]), (k, cs)
    keys = A.boot_keys(2, np.arange(v.n_sc))
    for member in (None, rand["members"][2]):
        rep = F.boot_counts(keys, 7, 5, member)
        if mx == 60:
            assert np.array_equal(rep[:2], LM.boot_counts(P, v, res, pb, b, cls, keys, 7, 2, mn, mx, member))
        boot = BM.expected_counts(batch.var_off, res, cls, pb, keys, 7, 5, mn, mx, member)
        for cs in range(2):
            assert np.array_equal(rep[:, cs].sum(2), boot[:, cs, :, P.sums[cs]]), cs
        assert rep.any() and len({tuple(x.ravel()) for x in rep}) == 5


def test_percentile_picks():
    assert LM.pick(1) == (0, 0) and LM.pick(20) == (0, 19) and LM.pick(1000) == (25, 974) and LM.pick(40) == (1, 38) and LM.pick(41) == (1, 39)
    for n in (1, 20, 1000):
        assert LM.pick(n) == BM.pick(n) == (int(np.floor(0.025 * n)), int(np.ceil(0.975 * n)) - 1)


@pytest.mark.parametrize("n_rep", [1, 20, 1000])
def test_writers_equal_the_model(rand, n_rep, tmp_path):
    P, v, batch, res, pb, cls, b = (rand[k] for k in ("P", "v", "batch", "res", "pb", "cls", "bytes"))
    mn, mx = (0, 60) if n_rep != 20 else (15, 40)
    F = LM.fast(P, v, res, pb, b, cls, mn, mx)
    point, plain = F.total(), O.oracle_pr_counts(O.lib(), batch.var_off, res, cls, pb, mn, mx)
    boot = F.boot_counts(A.boot_keys(0, np.arange(v.n_sc)), 3, n_rep)
    pre = str(tmp_path) + "/"
    stem = P.stem.replace("-", "_")
    getattr(RP, f"write_{stem}_bootstrap")(pre, point, plain, boot, mn, mx)
    text = open(pre + f"bootstrap-{P.stem}-summary.tsv").read()
    assert text == LM.bootstrap_text(P, point, plain, boot, mn, mx)
    head, rows = text.split("\n")[0].split("\t"), [l.split("\t") for l in text.split("\n")[1:-1]]
    assert head[:3] == ["VAR_TYPE", "THRESHOLD", "MIN_QUAL"] and head[3:6] == [P.columns[0], P.columns[0] + "_LO", P.columns[0] + "_HI"]
    assert len(head) == 3 + 3 * len(P.columns) and len(rows) == 8 and [r[1] for r in rows] == ["NONE", "BEST"] * 4
    for r in rows:                                                        # integers, LO <= HI, and both the point for one replicate
        cells = [int(x) for x in r[3:]]
        assert all(cells[j + 1] <= cells[j + 2] for j in range(0, len(cells), 3))
    if n_rep == 1:
        w1 = BM.weights(3, 1, A.boot_keys(0, np.arange(v.n_sc)))
        assert all(r[4] == r[5] for r in rows) and w1.min() == 0 and w1.max() > 1
    else:
        assert any(int(r[4]) < int(r[3]) < int(r[5]) for r in rows)
    if n_rep == 20:
        names = ["all", "none", "half", "tenth"]
        words = words_from(rand["members"])
        sc = F.strata_counts(words, 4)
        pr_strata = np.stack([SM.expected_counts(batch.var_off, res, cls, pb, m, mn, mx) for m in rand["members"]])
        getattr(RP, f"write_{stem}_stratified")(pre, names, sc, pr_strata, mn, mx)
        want = LM.stratified_text(P, names, sc, pr_strata, mn, mx)
        assert (open(pre + f"stratified-{P.stem}.tsv").read(), open(pre + f"stratified-{P.stem}-summary.tsv").read()) == want
        # the stratum that holds everything, without its STRATUM column, is the unstratified pair of files
        getattr(RP, f"write_{stem}")(pre, point, plain, mn, mx)
        for f, w in zip((f"{P.stem}.tsv", f"{P.stem}-summary.tsv"), want):
            lines = [l[4:] for l in w.split("\n") if l.startswith("all\t")]
            assert "\n".join([w.split("\n")[0][len("STRATUM\t"):]] + lines) + "\n" == open(pre + f).read(), f
        with pytest.raises(RP.ReportError):
            getattr(RP, f"write_{stem}_stratified")(pre, names[:3], sc, pr_strata, mn, mx)
        with pytest.raises(RP.ReportError):
            getattr(RP, f"write_{stem}_stratified")(str(tmp_path / "no" / "such") + "/", names, sc, pr_strata, mn, mx)
        with pytest.raises(RP.ReportError):
            getattr(RP, f"write_{stem}_bootstrap")(pre, point, plain, boot[:, :, :, :, :5], mn, mx)


# ---- the command lines, up to where the inputs are read

BAD_OPTIONS = ((["--cut-classes"], "--cut-classes needs --classify-errors or --classify-matches"),
               (["--cut-classes", "--classify-errors"], "--cut-classes needs --stratify"),
               (["--cut-classes", "--classify-matches"], "--cut-classes needs --stratify"),
               (["--cut-classes", "--stratify-variants"], "--cut-classes needs --classify-errors or --classify-matches"),
               (["--cut-classes", "--bootstrap", "4"], "--cut-classes needs --classify-errors or --classify-matches"))
GOOD_OPTIONS = (["--cut-classes", "--classify-errors", "--stratify-variants"], ["--cut-classes", "--classify-matches", "--bootstrap", "4"],
                ["--cut-classes", "--classify-errors", "--classify-matches", "--stratify-context", "--bootstrap", "4", "-n"])


def test_cxx_command_line_checks_the_option(tmp_path):
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa"), "-p", str(tmp_path) + "/"]
    for opts, text in BAD_OPTIONS:
        r = subprocess.run([cli] + missing + opts, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "ERROR: " + text in r.stderr and "no_query" not in r.stderr and r.stdout == "", (opts, r.stderr)
    for opts in GOOD_OPTIONS:
        r = subprocess.run([cli] + missing + opts, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "unknown option" not in r.stderr and "no_query" in r.stderr, (opts, r.stderr)


def test_python_command_line_checks_the_option(tmp_path):
    """python -m vcfdist_amd ends in an ERROR: line before it touches a device or an input"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="")
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa"), "-p", str(tmp_path / "out") + "/"]
    import sys
    for opts, text in BAD_OPTIONS[:3]:
        r = subprocess.run([sys.executable, "-m", "vcfdist_amd"] + missing + opts, capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
        assert r.returncode != 0 and r.stderr.strip().split("\n")[-1].startswith("ERROR: " + text) and r.stdout == "", (opts, r.stderr)
        assert "no_query" not in r.stderr and not (tmp_path / "out").exists()
    from vcfdist_amd.__main__ import main
    for opts, text in BAD_OPTIONS[3:]:
        with pytest.raises(SystemExit) as e:
            main(missing + opts)
        assert "ERROR: " + text in str(e.value), opts
    for opts in GOOD_OPTIONS:
        with pytest.raises(Exception) as e:                                # (the first input does not exist)
            main(missing + opts)
        assert "no_query" in str(e.value), (opts, e.value)
