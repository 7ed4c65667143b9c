"""Repeat strata on the GPU (include/vcfdist_repeats.h, pr_repeats.hip): the intervals and the start counts against the numpy model
of tests/repeats_model.py (hand genomes, kernel seams), determinism, the state machine of the calls, and both command lines with
--stratify-repeats."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import repeats_cases as RC
import repeats_model as RM
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_rows(got, want):
    assert len(got) == len(want) and all(len(g) == len(w) for g, w in zip(got, want))
    bad = RM.same(got, want)
    assert not bad, [(k, c, [x.tolist() for x in got[k][c]], [x.tolist() for x in want[k][c]]) for k, c in bad[:3]]
    for row in (r for per in got for r in per):
        assert row[0].dtype == np.int32 and (row[1] > row[0]).all() and (row[0][1:] > row[1][:-1]).all()      # sorted, merged, non-empty


def check_call(pr, contigs, specs, want=None):
    """one call against the model: intervals, valid and repeated starts, bit for bit"""
    rows, n_valid, n_rep = want or RM.all_intervals(contigs, specs)
    pr.repeat_intervals(contigs, specs)
    check_rows(pr.download_repeat_intervals(), rows)
    got_valid, got_rep = pr.repeat_stats()
    assert np.array_equal(got_valid, n_valid) and np.array_equal(got_rep, n_rep), (got_valid, n_valid, got_rep, n_rep)


# ---- 1. hand genomes

@pytest.mark.parametrize("k", RC.HAND_K)
def test_hand_cases_equal_the_model(k):
    """the genomes are built for k; every one runs with all of k in {4, 5, 31, 32} x slop in {0, 3}"""
    pr = api.PrecisionRecall()
    cases = RC.hand_cases(k)
    for name, contigs in cases.items():
        check_call(pr, contigs, RC.HAND_SPECS)
    rows, _, n_rep = RM.all_intervals(cases["none"], [A.rep_kmer(k)])
    assert n_rep[0] == 0 and all(len(r[0]) == 0 for r in rows[0])           # the genome with no repeat gives empty rows
    # all of them as one genome, in both orders: no state of a neighbour leaks, and copies across the cases are found
    every = [c for contigs in cases.values() for c in contigs]
    check_call(pr, every, RC.HAND_SPECS)
    check_call(pr, every[::-1], RC.HAND_SPECS)


# ---- 2. seams, 3. determinism

@pytest.fixture(scope="module")
def seams():
    bpw, _ = api.context_info()
    contigs, specs, _ = RC.seam_case(bpw)
    want = RM.all_intervals(contigs, specs)
    rows = want[0]
    assert all(len(rows[k][c][0]) > 0 for k in range(len(specs)) for c in range(3))
    assert all(not (len(rows[k][c][0]) == 1 and rows[k][c][1][0] - rows[k][c][0][0] == len(contigs[c])) for k in range(len(specs)) for c in range(3))
    return contigs, specs, want


def snapshot(pr):
    L = api.lib()
    n_spec, n_ctg = pr._repeats
    off = np.zeros(n_spec * n_ctg + 1, np.int64)
    assert L.vpr_repeat_interval_counts(pr._h, A._ptr(off, C.c_int64)) == 0
    st, sp = np.zeros(int(off[-1]) + 1, np.int32), np.zeros(int(off[-1]) + 1, np.int32)
    assert L.vpr_repeat_download_intervals(pr._h, A._ptr(st, C.c_int32), A._ptr(sp, C.c_int32)) == 0
    return (off, st, sp) + pr.repeat_stats()


def test_seams_equal_the_model(seams, monkeypatch):
    contigs, specs, want = seams
    pr = api.PrecisionRecall()
    check_call(pr, contigs, specs, want)
    whole = snapshot(pr)
    ms = pr.repeat_timing()
    assert all(t > 0 for t in ms)
    # the run passes over pieces of one contig each (the sort stays genome-wide): the same rows
    monkeypatch.setenv("VPR_CONTEXT_PIECE_BASES", "100000")
    check_call(pr, contigs, specs, want)
    assert all(np.array_equal(a, b) for a, b in zip(snapshot(pr), whole))


def test_two_calls_and_a_fresh_handle_give_identical_arrays(seams):
    contigs, specs, _ = seams
    pr = api.PrecisionRecall()
    pr.repeat_intervals(contigs, specs)
    one = snapshot(pr)
    pr.repeat_intervals(contigs, specs)
    two = snapshot(pr)
    other = api.PrecisionRecall()
    other.repeat_intervals(contigs, specs)
    three = snapshot(other)
    assert len(one[1]) > 1000
    for a, b, c in zip(one, two, three):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- 4. state and arguments

def test_state_and_arguments():
    pr = api.PrecisionRecall()
    L = api.lib()
    contigs = RC.hand_cases(5)["forward"]
    ok = [A.rep_kmer(5)]

    def refused(code, f, *a, **kw):
        with pytest.raises(api.VprError) as e:
            f(*a, **kw)
        assert f"({code})" in str(e.value), str(e.value)
        return str(e.value)
    off1 = np.zeros(2, np.int64)
    buf = np.zeros(4, np.int32)
    # before any call: VPR_ERR_STATE from the count, the download and the stats
    refused(-4, pr.download_repeat_intervals)
    assert L.vpr_repeat_interval_counts(pr._h, A._ptr(off1, C.c_int64)) == -4
    assert L.vpr_repeat_download_intervals(pr._h, A._ptr(buf, C.c_int32), A._ptr(buf, C.c_int32)) == -4
    assert L.vpr_repeat_download_intervals(pr._h, None, None) == -4
    refused(-4, pr.repeat_stats)
    pr.repeat_intervals(contigs, ok)
    rows = pr.download_repeat_intervals()
    assert sum(len(r[0]) for r in rows[0]) > 0
    assert L.vpr_repeat_download_intervals(pr._h, None, None) == -1             # null pointers: VPR_ERR_ARG
    assert L.vpr_repeat_interval_counts(pr._h, None) == -1
    for bad, what in ((A.rep_kmer(3), "k 3"), (A.rep_kmer(33), "k 33"), (A.rep_kmer(8, -1), "slop -1")):
        msg = refused(-1, pr.repeat_intervals, contigs, [ok[0], bad])
        assert "vpr_repeat_intervals" in msg and "entry 1" in msg and what in msg, msg
        refused(-4, pr.download_repeat_intervals)                   # after a refused call the earlier intervals are gone
        pr.repeat_intervals(contigs, ok)
    for spec in ([], ok * 9):
        msg = refused(-1, pr.repeat_intervals, contigs, spec)
        assert "vpr_repeat_intervals" in msg and "n_spec" in msg, msg
    pr.repeat_intervals(contigs, ok * 8)                            # the limit itself
    assert not RM.same(pr.download_repeat_intervals(), rows * 8)
    msg = refused(-1, pr.repeat_intervals, contigs, None)
    assert "vpr_repeat_intervals" in msg and "null spec" in msg, msg
    seq = np.frombuffer(b"".join(contigs), np.uint8)
    off = np.array([1, len(contigs[0]), len(seq)], np.int64)
    msg = refused(-1, pr.repeat_intervals, (off, seq), ok)
    assert "vpr_repeat_intervals" in msg and "ctg_off[0]" in msg, msg
    refused(-4, pr.download_repeat_intervals)
    refused(-4, pr.repeat_stats)
    # (no test of a total above UINT32_MAX bases: that check, like all of these, precedes any read of the sequence, but the call
    # that reaches it needs offsets that describe 4 GiB of sequence, and a test must not hand the library a pointer to less)
    # after a refused call the handle still works, and evaluates a batch
    pr.repeat_intervals(contigs, ok)
    assert not RM.same(pr.download_repeat_intervals(), rows)
    batch = api.Synth(n_sc=16, len_a=8, len_b=100, len_max=100, seed=3).batch()
    res = pr.run(batch)
    assert not res.diff(api.PrecisionRecall().run(batch))
    assert not RM.same(pr.download_repeat_intervals(), rows)       # the intervals outlive an evaluation on the handle


# ---- 5. the command lines

from test_gpu_strata_context import STRAT_BOOT, STRAT_FILES, _without_command, _write_fasta     # noqa: E402 -- the helpers of the context twin

REPEAT_BED = "repeat-strata.bed"
LINE = r"repeat strata: (\d+) intervals of 3 strata, (\d+) valid and (\d+) repeated starts \(k=16\), (\d+) valid and (\d+) repeated starts \(k=24\), " \
       r"(\d+) valid and (\d+) repeated starts \(k=32\), ([0-9.]+) ms on the device"


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """the surrogate FASTA with the planted copies, and the model's intervals of the default set on it"""
    tmp = tmp_path_factory.mktemp("repeats_demo")
    seq, sites = RC.demo_fasta()
    names, specs = api.repeats_default()
    rows, n_valid, n_rep = RM.all_intervals([seq], specs)
    assert all(len(r[0][0]) > 0 for r in rows)                 # every default stratum has an interval
    return dict(tmp=tmp, seq=seq, sites=sites, names=names, specs=specs, rows=rows, n_valid=n_valid, n_rep=n_rep)


def test_command_lines_on_demo_files(demo, tmp_path):
    import demo_pipeline as D
    names, rows = demo["names"], demo["rows"]
    fa = _write_fasta(tmp_path / "surrogate.fa", demo["seq"], ("chr1",))
    lst, _ = RM.write_model_strata(tmp_path, names, ["chr1"], rows, "repeats.tsv")
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    boot = ["--bootstrap", "16"]
    runs = {}
    for name, cmd, extra in (("c", cli, []), ("c-r", cli, ["--stratify-repeats"] + boot), ("py-r", py, ["--stratify-repeats"] + boot),
                             ("c-l", cli, ["--stratify", lst] + boot), ("c-n", cli, ["--stratify-repeats", "-n"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    # repeat-strata.bed equals the model; the C++ and the Python files are byte-identical
    want_bed = RM.repeat_bed_text(names, ["chr1"], rows).encode()
    assert rd(runs["c-r"][0] + REPEAT_BED) == want_bed and rd(runs["py-r"][0] + REPEAT_BED) == want_bed
    for f in STRAT_FILES + (STRAT_BOOT,):
        assert rd(runs["c-r"][0] + f) == rd(runs["py-r"][0] + f), f
        # the end-to-end check: the same tables as --stratify LIST over the model's BEDs under the same names
        assert rd(runs["c-r"][0] + f) == rd(runs["c-l"][0] + f) and len(rd(runs["c-r"][0] + f)) > 500, f
    assert not os.path.exists(runs["c-l"][0] + REPEAT_BED) and not os.path.exists(runs["c"][0] + REPEAT_BED)
    # every default stratum has a member
    summary = [l.split("\t") for l in open(runs["c-r"][0] + STRAT_FILES[0]).read().split("\n")[1:-1]]
    none_all = {r[0]: [int(x) for x in r[4:8]] for r in summary if r[1] == "ALL" and r[2] == "NONE"}
    assert list(none_all) == names and all(sum(v) > 0 for v in none_all.values()), none_all
    # the run without the option is unchanged: every file of the plain run, and stdout
    plain = sorted(os.listdir(runs["c"][0]))
    extra = {f for f in os.listdir(runs["c-r"][0]) if f not in plain}
    assert set(STRAT_FILES) | {STRAT_BOOT, REPEAT_BED} <= extra and all("strat" in f or "bootstrap" in f for f in extra), extra
    for f in plain:
        assert _without_command(runs["c"][0] + f) == _without_command(runs["c-r"][0] + f), f
    assert runs["c"][1] == runs["c-r"][1] == runs["py-r"][1] == runs["c-n"][1]
    assert "stratified" not in runs["c"][2] and "repeat" not in runs["c"][2]
    # stderr: the stratified line, and the line with the intervals, the start counts and the device time (also under -n)
    n_iv = sum(len(r[0][0]) for r in rows)
    for name in ("c-r", "py-r", "c-n"):
        m = re.findall(r"stratified: (\d+) strata, (\d+) of (\d+) hap-variants in none of them", runs[name][2])
        assert len(m) == 1 and int(m[0][0]) == 3 and 0 < int(m[0][1]) < int(m[0][2]), runs[name][2][-500:]
        m = re.findall(LINE, runs[name][2])
        assert len(m) == 1 and int(m[0][0]) == n_iv and float(m[0][7]) > 0, runs[name][2][-500:]
        assert [int(x) for x in m[0][1:7:2]] == demo["n_valid"].tolist() and [int(x) for x in m[0][2:7:2]] == demo["n_rep"].tolist()
    assert os.listdir(runs["c-n"][0]) == []                                   # -n: no file appears
    # a repeat name that is also a name of the list ends the run before anything is evaluated
    bad = tmp_path / "bad.tsv"
    bad.write_text("whole\trep_k16.bed\nrep_k24\trep_k32.bed\n")
    for cmd in (cli, py):
        r = subprocess.run(cmd + inputs + ["-n", "--stratify", str(bad), "--stratify-repeats"], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode != 0 and "duplicate stratum name 'rep_k24'" in r.stderr and "PRECISION-RECALL" not in r.stdout
        r = subprocess.run(cmd + inputs + ["-n", "--stratify", str(bad)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-500:]                             # (the list alone is fine)


# ---- 6. two ranks on one GPU

@pytest.fixture(scope="module")
def two_contigs(demo):
    """the demo callsets twice, as chr1 and chr2, on a FASTA whose chr2 is a copy of chr1 -- every valid start is then repeated
    across contigs; a list of BED strata made of the model's intervals on that genome (under names of their own), and the one-rank
    run with --stratify, --stratify-repeats, --bootstrap and --cut-classes"""
    import gzip
    import demo_pipeline as D
    tmp = demo["tmp"]
    fa = _write_fasta(tmp / "two.fa", demo["seq"], ("chr1", "chr2"))
    rows, n_valid, n_rep = RM.all_intervals([demo["seq"], demo["seq"]], demo["specs"])
    assert np.array_equal(n_valid, n_rep) and n_valid[0] > 2 * 5_000_000

    def twice(lines):
        head = [l for l in lines if l.startswith("#")]
        body = [l for l in lines if l and not l.startswith("#")]
        head = [l for l in head if not l.startswith("##contig")] or head
        ctg = ["##contig=<ID=chr1,length=5100000>", "##contig=<ID=chr2,length=5100000>"]
        return "\n".join(head[:1] + ctg + head[1:] + body + ["chr2" + l[4:] for l in body if l.startswith("chr1\t")]) + "\n"
    qv, tv, bed = tmp / "q.vcf", tmp / "t.vcf", tmp / "r.bed"
    qv.write_text(twice(open(os.path.join(D.DEMO, "query.vcf")).read().split("\n")))
    tv.write_text(twice(gzip.open(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), "rt").read().split("\n")))
    b = [l for l in open(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")).read().split("\n") if l]
    bed.write_text("\n".join(b + ["chr2" + l[4:] for l in b]) + "\n")
    model_names = [n.replace("rep_", "model_") for n in demo["names"]]
    lst, _ = RM.write_model_strata(tmp, model_names, ["chr1", "chr2"], rows, "two.tsv")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), VCFDIST_ONE_GPU="1")
    base = [str(qv), str(tv), fa, "-b", str(bed), "--stratify", lst, "--stratify-repeats", "--bootstrap", "8", "--classify-errors", "--cut-classes"]
    (tmp / "one").mkdir()
    subprocess.run([sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL, timeout=600)
    return tmp, base, env, rows, model_names


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_command_line_two_ranks(two_contigs, demo, how):
    tmp, base, env, rows, model_names = two_contigs
    out = tmp / how
    out.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # (the child runs under its own time limit: a rank that hangs in a collective is ended, not waited for)
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vcfdist_amd"] + base + ["-p", str(out) + "/", "--shard", how],
                   check=True, env=env, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=660)
    for name in STRAT_FILES + (STRAT_BOOT, REPEAT_BED, "precision-recall.tsv", "precision-recall-summary.tsv", "stratified-error-classes-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 60, name
    assert (out / REPEAT_BED).read_text() == RM.repeat_bed_text(demo["names"], ["chr1", "chr2"], rows)
    # the repeat strata's rows of the stratified summary equal those of the BED strata made of the model's intervals
    lines = (out / STRAT_FILES[0]).read_text().split("\n")[1:-1]
    for rep, model in zip(demo["names"], model_names):
        got = [l.split("\t", 1)[1] for l in lines if l.startswith(rep + "\t")]
        want = [l.split("\t", 1)[1] for l in lines if l.startswith(model + "\t")]
        assert got == want and len(got) >= 8 and any(int(x) > 0 for l in got for x in l.split("\t")[3:7]), rep
