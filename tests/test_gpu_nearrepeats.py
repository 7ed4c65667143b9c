"""Near-repeat strata on the GPU (include/vcfdist_nearrepeats.h, pr_nearrepeats.hip): the intervals and the start counts against
the numpy model of tests/nearrepeats_model.py on every planted case of tests/nearrepeats_cases.py, determinism, the state machine
of the calls, m = 0 against vpr_repeat_intervals, and both command lines with --stratify-near-repeats."""
import ctypes as C
import functools
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import cli_paths_cases as PC
import nearrepeats_cases as NC
import nearrepeats_model as NM
from label_common import ROOT, _without_command
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu
STRAT_FILES = ("stratified-precision-recall-summary.tsv", "stratified-precision-recall.tsv")
NEAR_BED = "near-repeat-strata.bed"


@functools.lru_cache(maxsize=None)
def cases():
    return {c.name: c for c in NC.all_cases()}


def specs_of(case):
    """the case's entries, with a slop on every other one"""
    return [A.near_kmer(k, m, 3 * (e % 2)) for e, (k, m) in enumerate(case.specs)]


@functools.lru_cache(maxsize=None)
def model(name, backwards):
    """the model's answer for a case, computed once: (rows, n_valid, n_near)"""
    case = cases()[name]
    specs = specs_of(case)
    return NM.all_intervals(case.contigs, specs[::-1] if backwards else specs)


def check_rows(got, want):
    assert len(got) == len(want) and all(len(g) == len(w) for g, w in zip(got, want))
    bad = NM.same(got, want)
    assert not bad, [(k, c, [x.tolist()[:8] for x in got[k][c]], [x.tolist()[:8] for x in want[k][c]]) for k, c in bad[:3]]
    for row in (r for per in got for r in per):
        assert row[0].dtype == np.int32 and (row[1] > row[0]).all() and (row[0][1:] > row[1][:-1]).all()      # sorted, merged, non-empty


def check_case(pr, name):
    """a case in both orders of its entries against the model: intervals, valid and near-repeated starts, bit for bit"""
    case = cases()[name]
    for backwards in (False, True):
        specs = specs_of(case)[::-1] if backwards else specs_of(case)
        rows, n_valid, n_near = model(name, backwards)
        pr.nearrepeat_intervals(case.contigs, specs)
        check_rows(pr.download_nearrepeat_intervals(), rows)
        got_valid, got_near, compares, max_run = pr.nearrepeat_stats(cost=True)
        assert np.array_equal(got_valid, n_valid) and np.array_equal(got_near, n_near), (name, got_valid, n_valid, got_near, n_near)
        built_for = len(specs) - 1 if backwards else 0
        assert max_run[built_for] >= case.min_run, (name, max_run, case.min_run)
        assert (compares[built_for] > 0 or not case.near) and (max_run >= 1).all(), (name, compares, max_run)


GROUPS = ["pos_k16", "pos_k25", "pos_k31_m1", "pos_k32_m1", "pos_k24_m2", "pos_k31_m2", "pos_k32_m2", "pos_k32_m3", "over_", "self_", "shift_",
          "run_k32_m1_b0", "run_k32_m1_b1", "run_k24_m2_b0", "run_k24_m2_b1", "run_k24_m2_b2", "strand_", "seam_", "n_", "edge_", "mono_"]


def test_the_groups_cover_every_case():
    hit = [sum(n.startswith(g) for g in GROUPS) for n in cases()]
    assert hit and all(h == 1 for h in hit)


@pytest.mark.parametrize("group", GROUPS)
def test_cases_equal_the_model(group):
    pr = api.PrecisionRecall()
    names = [n for n in cases() if n.startswith(group)]
    assert names
    for name in names:
        check_case(pr, name)


def snapshot(pr):
    L = api.lib()
    n_spec, n_ctg = pr._nearrepeats
    off = np.zeros(n_spec * n_ctg + 1, np.int64)
    assert L.vpr_nearrepeat_interval_counts(pr._h, A._ptr(off, C.c_int64)) == 0
    st, sp = np.zeros(int(off[-1]) + 1, np.int32), np.zeros(int(off[-1]) + 1, np.int32)
    assert L.vpr_nearrepeat_download_intervals(pr._h, A._ptr(st, C.c_int32), A._ptr(sp, C.c_int32)) == 0
    return (off, st, sp) + pr.nearrepeat_stats(cost=True)


def test_two_calls_and_a_fresh_handle_give_identical_arrays():
    case = cases()["pos_k32_m2"]
    specs = specs_of(case) + [A.near_kmer(24, 1), A.near_kmer(32, 3, 5)]
    pr = api.PrecisionRecall()
    pr.nearrepeat_intervals(case.contigs, specs)
    one = snapshot(pr)
    assert all(t > 0 for t in pr.nearrepeat_timing())
    pr.nearrepeat_intervals(case.contigs, specs)
    two = snapshot(pr)
    other = api.PrecisionRecall()
    other.nearrepeat_intervals(case.contigs, specs)
    three = snapshot(other)
    assert len(one[1]) > 500
    for a, b, c in zip(one, two, three):                       # the compares and the longest run among them
        assert np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize("k", NC.MONO_M0_K)
def test_m0_equals_the_repeat_strata_on_the_same_handle(k):
    contigs, _ = NC.mono_genome()
    contigs = contigs + [contigs[0][100:400]]
    pr = api.PrecisionRecall()
    pr.repeat_intervals(contigs, [A.rep_kmer(k, 0), A.rep_kmer(k, 7)])
    pr.nearrepeat_intervals(contigs, [A.near_kmer(k, 0, 0), A.near_kmer(k, 0, 7)])
    a, b = pr.download_repeat_intervals(), pr.download_nearrepeat_intervals()
    assert not NM.same(a, b) and sum(len(r[0]) for r in a[0]) > 0
    assert all(np.array_equal(x, y) for x, y in zip(pr.repeat_stats(), pr.nearrepeat_stats()))


def test_state_and_arguments():
    pr = api.PrecisionRecall()
    L = api.lib()
    contigs = cases()["strand_alone"].contigs
    ok = [A.near_kmer(32, 1)]

    def refused(code, f, *a, **kw):
        with pytest.raises(api.VprError) as e:
            f(*a, **kw)
        assert f"({code})" in str(e.value), str(e.value)
        return str(e.value)
    off1 = np.zeros(2, np.int64)
    buf = np.zeros(4, np.int32)
    # before any call: VPR_ERR_STATE from the count, the download and the stats
    refused(-4, pr.download_nearrepeat_intervals)
    assert L.vpr_nearrepeat_interval_counts(pr._h, A._ptr(off1, C.c_int64)) == -4
    assert L.vpr_nearrepeat_download_intervals(pr._h, A._ptr(buf, C.c_int32), A._ptr(buf, C.c_int32)) == -4
    refused(-4, pr.nearrepeat_stats)
    assert pr.nearrepeat_timing() == (0, 0, 0, 0)
    pr.nearrepeat_intervals(contigs, ok)
    rows = pr.download_nearrepeat_intervals()
    assert sum(len(r[0]) for r in rows[0]) == 2
    assert L.vpr_nearrepeat_download_intervals(pr._h, None, None) == -1             # null pointers: VPR_ERR_ARG
    assert L.vpr_nearrepeat_interval_counts(pr._h, None) == -1
    bad_specs = ((A.near_kmer(32, 4), "m 4"), (A.near_kmer(32, -1), "m -1"), (A.near_kmer(33, 1), "k 33"), (A.near_kmer(15, 1), "k 15"),
                 (A.near_kmer(23, 2), "k 23"), (A.near_kmer(31, 3), "k 31"), (A.near_kmer(7, 0), "k 7"), (A.near_kmer(32, 1, -1), "slop -1"))
    for bad, what in bad_specs:
        msg = refused(-1, pr.nearrepeat_intervals, contigs, [ok[0], bad])
        assert "vpr_nearrepeat_intervals" in msg and "entry 1" in msg and what in msg, msg
        refused(-4, pr.download_nearrepeat_intervals)               # after a refused call the earlier intervals are gone
        refused(-4, pr.nearrepeat_stats)
        pr.nearrepeat_intervals(contigs, ok)
    msg = refused(-1, pr.nearrepeat_intervals, contigs, [A.near_kmer(32, 1), A.near_kmer(24, 1), A.near_kmer(32, 1)])
    assert "vpr_nearrepeat_intervals" in msg and "entries 0 and 2 are equal" in msg, msg
    refused(-4, pr.download_nearrepeat_intervals)
    for spec in ([], [A.near_kmer(32, 1, s) for s in range(5)]):
        msg = refused(-1, pr.nearrepeat_intervals, contigs, spec)
        assert "vpr_nearrepeat_intervals" in msg and "n_spec" in msg, msg
        refused(-4, pr.download_nearrepeat_intervals)
    pr.nearrepeat_intervals(contigs, [A.near_kmer(32, 1, s) for s in range(4)])        # the limit itself
    assert len(pr.download_nearrepeat_intervals()) == 4
    msg = refused(-1, pr.nearrepeat_intervals, contigs, None)
    assert "vpr_nearrepeat_intervals" in msg and "null spec" in msg, msg
    seq = np.frombuffer(b"".join(contigs), np.uint8)
    msg = refused(-1, pr.nearrepeat_intervals, (np.array([1, len(seq)], np.int64), seq), ok)
    assert "vpr_nearrepeat_intervals" in msg and "ctg_off[0]" in msg, msg
    refused(-4, pr.download_nearrepeat_intervals)
    # above 2^31 - 1 bases: refused before a byte of the sequence is read (the offsets describe more than the buffer holds)
    msg = refused(-1, pr.nearrepeat_intervals, (np.array([0, 2**31 - 1, 2**31], np.int64), seq), ok)
    assert "vpr_nearrepeat_intervals" in msg and "2147483648 bases in total" in msg, msg
    refused(-4, pr.download_nearrepeat_intervals)
    # after a refused call the handle still works, and the intervals outlive a call of the exact family
    pr.nearrepeat_intervals(contigs, ok)
    pr.repeat_intervals(contigs, [A.rep_kmer(32)])
    assert not NM.same(pr.download_nearrepeat_intervals(), rows)


# ---- the command lines, on the three contigs of tests/cli_paths_cases.py

NEAR_ARG = "32:1,24:2,16:0"
NEAR_SPECS = [A.near_kmer(32, 1), A.near_kmer(24, 2), A.near_kmer(16, 0)]
NEAR_NAMES = ["near_k32_m1", "near_k24_m2", "near_k16_m0"]
LINE = r"near repeat strata: (\d+) intervals of 3 strata, (\d+) valid and (\d+) near-repeated starts \(k=32, m=1\), (\d+) valid and (\d+) " \
       r"near-repeated starts \(k=24, m=2\), (\d+) valid and (\d+) near-repeated starts \(k=16, m=0\), (\d+) compares, longest run (\d+), " \
       r"([0-9.]+) ms on the device"
CLI, PY = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]


def run(cmd, args, **kw):
    """a driver under its own time limit"""
    return subprocess.run(["timeout", "-k", "10", "120"] + cmd + args, capture_output=True, text=True, cwd=ROOT, timeout=150, **kw)


def test_command_lines_on_three_contigs(tmp_path):
    w = PC.write(tmp_path)
    rows, n_valid, n_near = NM.all_intervals(w["contigs"], NEAR_SPECS)
    assert all(sum(len(r[c][0]) for c in range(3)) > 0 for r in rows)
    lst, _ = NM.write_model_strata(tmp_path, NEAR_NAMES, PC.NAMES, rows, "near.tsv")
    near = ["--stratify-near-repeats", NEAR_ARG]
    more = ["--bootstrap", "4", "--classify-errors", "--cut-classes"]
    runs = {}
    for name, cmd, extra in (("c", CLI, []), ("c-r", CLI, near + more), ("py-r", PY, near + more), ("c-l", CLI, ["--stratify", lst] + more),
                             ("c-n", CLI, near + ["-n"]), ("c-all", CLI, near + ["--stratify", w["list"], "--stratify-repeats", "--stratify-context"]),
                             ("py-all", PY, near + ["--stratify", w["list"], "--stratify-repeats", "--stratify-context"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = run(cmd, w["inputs"] + ["-p", pre] + extra)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    want_bed = NM.near_repeat_bed_text(NEAR_NAMES, PC.NAMES, rows).encode()
    assert rd(runs["c-r"][0] + NEAR_BED) == want_bed and rd(runs["py-r"][0] + NEAR_BED) == want_bed
    # both drivers write the same files, byte for byte; the stratified tables are those of --stratify over the model's BEDs
    files = sorted(os.listdir(runs["c-r"][0]))
    assert files == sorted(os.listdir(runs["py-r"][0])) and NEAR_BED in files
    for f in files:
        assert _without_command(runs["c-r"][0] + f) == _without_command(runs["py-r"][0] + f), f
    strat = [f for f in files if f.startswith("stratified-")]
    assert set(STRAT_FILES) <= set(strat) and len(strat) >= 4
    for f in strat:
        assert rd(runs["c-r"][0] + f) == rd(runs["c-l"][0] + f) and len(rd(runs["c-r"][0] + f)) > 200, f
    # the table order: behind --stratify FILE and --stratify-repeats, in front of --stratify-context
    for a, b in (("c-all", "py-all"),):
        assert sorted(os.listdir(runs[a][0])) == sorted(os.listdir(runs[b][0]))
        for f in os.listdir(runs[a][0]):
            assert _without_command(runs[a][0] + f) == _without_command(runs[b][0] + f), f
    order = []
    for l in open(runs["c-all"][0] + STRAT_FILES[0]).read().split("\n")[1:-1]:
        if l.split("\t")[0] not in order:
            order.append(l.split("\t")[0])
    rep_names, ctx_names = api.repeats_default()[0], api.context_default()[0]
    assert order == [n for n, _ in PC.STRATA] + rep_names + NEAR_NAMES + ctx_names, order
    # the run without the option is unchanged: the files of the plain run, both streams, no word of the option
    plain = sorted(os.listdir(runs["c"][0]))
    assert NEAR_BED not in plain and len(plain) > 8
    for f in plain:
        assert _without_command(runs["c"][0] + f) == _without_command(runs["c-r"][0] + f), f
    assert runs["c"][1] == runs["c-r"][1] == runs["py-r"][1] == runs["c-n"][1]
    assert "near" not in runs["c"][2] and "stratified" not in runs["c"][2]
    # stderr: one line with the intervals, the start counts, the cost and the device time (also under -n)
    n_iv = sum(len(r[c][0]) for r in rows for c in range(3))
    for name in ("c-r", "py-r", "c-n"):
        m = re.findall(LINE, runs[name][2])
        assert len(m) == 1 and int(m[0][0]) == n_iv and int(m[0][7]) > 0 and int(m[0][8]) >= 2 and float(m[0][9]) > 0, runs[name][2][-800:]
        assert [int(x) for x in m[0][1:7:2]] == n_valid.tolist() and [int(x) for x in m[0][2:7:2]] == n_near.tolist()
    assert os.listdir(runs["c-n"][0]) == []
    # a near-repeat name that is also a name of the list ends the run before anything is evaluated
    bad = tmp_path / "bad.tsv"
    (tmp_path / "whole.bed").write_text("chrA\t0\t3000\n")
    bad.write_text("whole\twhole.bed\nnear_k24_m2\twhole.bed\n")
    for cmd in (CLI, PY):
        r = run(cmd, w["inputs"] + ["-n", "--stratify", str(bad)] + near)
        assert r.returncode != 0 and "duplicate stratum name 'near_k24_m2' (a near repeat stratum of --stratify-near-repeats)" in r.stderr, r.stderr[-800:]
        assert "PRECISION-RECALL" not in r.stdout
    r = run(CLI, w["inputs"] + ["-n", "--stratify", str(bad)])
    assert r.returncode == 0, r.stderr[-500:]                                   # (the list alone is fine)


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("near_ranks")
    w = PC.write(tmp)
    base = w["inputs"] + ["--stratify", w["list"], "--stratify-near-repeats", NEAR_ARG, "--bootstrap", "4", "--classify-errors", "--cut-classes"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), VCFDIST_ONE_GPU="1")
    (tmp / "one").mkdir()
    r = run(PY, base + ["-p", str(tmp / "one") + "/"], env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return tmp, base, env


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_two_ranks_give_one_ranks_files(one_rank, how):
    tmp, base, env = one_rank
    out = tmp / how
    out.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # (the child runs under its own time limit: a rank that hangs in a collective is ended, not waited for)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vcfdist_amd"] + base +
                       ["-p", str(out) + "/", "--shard", how], capture_output=True, text=True, env=env, cwd=ROOT, timeout=330)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(tmp / "one"))
    assert files == sorted(os.listdir(out)) and NEAR_BED in files and len(files) > 10
    for f in files:
        assert _without_command(str(tmp / "one" / f)) == _without_command(str(out / f)), f
