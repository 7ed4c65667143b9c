"""Host side of the bootstrap replicates (include/vcfdist_bootstrap.h): the definition's check vectors, the weight table,
the exported symbols, the writers' bytes against the model and the command lines' option checks.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bootstrap_model as M
from vcfdist_amd import _abi as A
from vcfdist_amd import api, report as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported():
    text = open(os.path.join(ROOT, "include", "vcfdist_bootstrap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bint\s+(v[pr][rp]_\w+)\s*\(", code)
    assert sorted(names) == sorted(api.BOOT_EXPORTED) and len(names) == 5
    L = api.lib()
    for n in names:
        assert hasattr(L, n), n
    assert {"vrp_write_bootstrap", "vrp_write_bootstrap_stratified"} <= set(RP.EXPORTED)
    # the header's table and limits are the Python mirror's
    table = re.search(r"#define VPR_BOOT_T \{(.*?)\}", text, flags=re.S).group(1)
    assert tuple(int(x) for x in re.findall(r"(\d+)u", table)) == A.BOOT_T
    assert int(re.search(r"#define VPR_BOOT_MAX_REPLICATES (\d+)", text).group(1)) == A.BOOT_MAX_REPLICATES == 100000
    assert "conditional on the phasing" in text.lower()


def test_check_vectors():
    assert int(M.draw(1, 0, 0)) == 755968199
    assert int(M.draw(1, 0, 1)) == 1618525976
    assert int(M.draw(2, 3, (5 << 32) | 7)) == 2339623235
    # the same through the vectorised form the GPU tests use
    u = M.draw(1, np.zeros(2, np.uint64), np.array([0, 1], np.uint64))
    assert u.tolist() == [755968199, 1618525976]
    assert M.weights(1, 1, [0, 1]).tolist() == [[0, 1]]        # 755968199 < T[0] <= 1618525976 < T[1]


def test_table_is_the_poisson_cdf():
    assert tuple(M.table_from_cdf()) == A.BOOT_T
    assert len(A.BOOT_T) == A.BOOT_MAX_WEIGHT == 12 and list(A.BOOT_T) == sorted(set(A.BOOT_T)) and A.BOOT_T[-1] < 2 ** 32


def test_weights_at_the_table_edges():
    for k, t in enumerate(A.BOOT_T):
        assert int(M.weight_of_draw(t - 1)) == k and int(M.weight_of_draw(t)) == k + 1
    assert int(M.weight_of_draw(0)) == 0 and int(M.weight_of_draw(2 ** 32 - 1)) == 12


def test_weights_look_like_poisson_1():
    w = M.weights(1, 200, np.arange(1000, dtype=np.uint64))
    assert abs(w.mean() - 1) < 0.02 and abs(w.var() - 1) < 0.03 and w.min() == 0 and 4 <= w.max() <= 12


def test_pick_is_the_percentile_interval():
    assert M.pick(1) == (0, 0) and M.pick(2) == (0, 1) and M.pick(40) == (1, 38) and M.pick(1000) == (25, 974)
    for n in range(1, 2001):
        lo, hi = M.pick(n)
        assert 0 <= lo <= hi < n
        # floor(0.025 n) and ceil(0.975 n) - 1 in exact arithmetic
        assert lo == (25 * n) // 1000 and hi == -((-975 * n) // 1000) - 1


def test_fold_is_the_counters_fold():
    """the model's fold against a direct statement of the counters: a variant with last threshold index b counts at thresholds
    0..b; a truth variant is also FN at every threshold above b"""
    rng = np.random.RandomState(3)
    nq = 5
    hist = rng.randint(0, 9, size=(2, 3, 3, nq + 1))
    want = np.zeros((2, 4, 3, nq), np.int64)
    for cs in range(2):
        for t in range(3):
            for e in range(3):
                for b in range(nq + 1):
                    n = hist[cs, t, e, b]
                    last = -1 if b == nq else b
                    for k in range(nq):
                        if k <= last:
                            want[cs, t, e, k] += n
                        elif cs == 1:
                            want[cs, t, 2, k] += n
    want[:, 3] = want[:, :3].sum(axis=1)
    assert np.array_equal(M.fold(hist, nq), want)


def _hand_made(n_rep, nq, seed):
    rng = np.random.RandomState(seed)
    hist = rng.randint(0, 400, size=(2, 3, 3, nq + 1))
    hist[:, 2] = 0                      # no SV at all: precision and recall of an empty class are 1, F1 has no maximum
    counts = M.fold(hist, nq)
    boot = np.stack([M.fold(rng.poisson(hist), nq) for _ in range(n_rep)])
    return counts, boot


@pytest.mark.parametrize("n_rep", [1, 2, 40, 1000])
def test_writers_equal_the_model(tmp_path, n_rep):
    min_qual, max_qual = (0, 20) if n_rep < 1000 else (3, 9)
    nq = max_qual - min_qual + 1
    counts, boot = _hand_made(n_rep, nq, seed=n_rep)
    pre = str(tmp_path) + "/"
    seed = 2 ** 64 - 1 if n_rep == 2 else 7
    RP.write_bootstrap(pre, counts, boot, seed, min_qual, max_qual)
    want_sum, want_rep = M.bootstrap_files(counts, boot, seed, min_qual, max_qual)
    got_sum = open(pre + "bootstrap-precision-recall-summary.tsv").read()
    assert got_sum == want_sum
    assert open(pre + "bootstrap-replicates.tsv").read() == want_rep
    assert sorted(os.listdir(pre)) == ["bootstrap-precision-recall-summary.tsv", "bootstrap-replicates.tsv"]
    assert want_rep.count("\n") == 1 + 8 * n_rep
    # rows and point columns are those of precision-recall-summary.tsv
    RP.write_precision_recall(pre, counts, min_qual, max_qual)
    point = [l.split("\t") for l in open(pre + "precision-recall-summary.tsv").read().split("\n")[1:-1]]
    rows = [l.split("\t") for l in got_sum.split("\n")[1:-1]]
    assert len(rows) == len(point) == 8
    for b, p in zip(rows, point):
        assert b[:3] == p[:3] and [b[5], b[8], b[11]] == p[7:10] and b[3] == str(n_rep) and b[4] == str(seed)
        for j in (5, 8, 11):            # LO <= HI everywhere; with one replicate both are that replicate
            assert float(b[j + 1]) <= float(b[j + 2])
            if n_rep == 1:
                assert b[j + 1] == b[j + 2]
    if n_rep >= 40:
        assert any(float(b[6]) < float(b[5]) < float(b[7]) for b in rows)          # an interval that brackets its point estimate
    # the stratified table: the first table once per stratum behind the STRATUM column
    counts2, boot2 = _hand_made(n_rep, nq, seed=n_rep + 1)
    RP.write_bootstrap_stratified(pre, ["whole", "other one"], np.stack([counts, counts2]), np.stack([boot, boot2]), seed, min_qual, max_qual)
    got = open(pre + "stratified-bootstrap-precision-recall-summary.tsv").read()
    assert got == M.stratified_file(["whole", "other one"], [counts, counts2], [boot, boot2], seed, min_qual, max_qual)
    whole = "".join(l.split("\t", 1)[1] + "\n" for l in got.split("\n")[:-1] if l.startswith(("STRATUM\t", "whole\t")))
    assert whole == got_sum
    assert not os.path.exists(pre + "stratified-bootstrap-replicates.tsv")


def test_writers_refuse_bad_arguments(tmp_path):
    counts, boot = _hand_made(2, 3, seed=1)
    with pytest.raises(RP.ReportError):
        RP.write_bootstrap(str(tmp_path) + "/", counts, boot[:, :1], 1, 0, 2)
    with pytest.raises(RP.ReportError):
        RP.write_bootstrap(str(tmp_path / "missing" / "dir") + "/", counts, boot, 1, 0, 2)
    with pytest.raises(RP.ReportError):
        RP.write_bootstrap_stratified(str(tmp_path) + "/", ["a"], np.stack([counts, counts]), np.stack([boot, boot]), 1, 0, 2)


@pytest.mark.parametrize("bad", [["--bootstrap", "0"], ["--bootstrap", "100001"], ["--bootstrap", "ten"], ["--bootstrap", "40", "--bootstrap-seed", "-1"],
                                 ["--bootstrap", "40", "--bootstrap-seed", "x"], ["--bootstrap"]])
def test_command_lines_check_the_options_before_reading_anything(tmp_path, bad):
    """both options are checked when the arguments are parsed: the input files named here do not exist and are never opened"""
    inputs = [str(tmp_path / "no-query.vcf"), str(tmp_path / "no-truth.vcf"), str(tmp_path / "no-ref.fa")]
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    for cmd in ([cli], [sys.executable, "-m", "vcfdist_amd"]):
        r = subprocess.run(cmd + inputs + bad, capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode != 0 and "ootstrap" in r.stderr and "no-query" not in r.stderr, r.stderr[-500:]
