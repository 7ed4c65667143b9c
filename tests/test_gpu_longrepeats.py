"""Long repeat strata on the GPU (include/vcfdist_longrepeats.h, pr_longrepeats.hip): the intervals and the start counts against the
model of tests/longrepeats_model.py on the planted cases of tests/longrepeats_cases.py, determinism, the state machine of the
calls, the independence from vpr_repeat_intervals on the same handle, and both command lines with --stratify-long-repeats."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import longrepeats_cases as LC
import longrepeats_model as LM
import repeats_model as RM
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_rows(got, want, what):
    assert len(got) == len(want) and all(len(g) == len(w) for g, w in zip(got, want)), what
    bad = LM.same(got, want)
    assert not bad, (what, [(k, c, [x.tolist() for x in got[k][c]], [x.tolist() for x in want[k][c]]) for k, c in bad[:3]])
    for row in (r for per in got for r in per):
        assert row[0].dtype == np.int32 and (row[1] > row[0]).all() and (row[0][1:] > row[1][:-1]).all()      # sorted, merged, non-empty


def check_call(pr, contigs, specs, what, want=None):
    """one call against the model: intervals, valid and repeated starts, bit for bit"""
    rows, n_valid, n_rep = want or LM.all_intervals(contigs, specs)
    pr.longrepeat_intervals(contigs, specs)
    got_valid, got_rep = pr.longrepeat_stats()
    print(what, [(s.k, s.slop) for s in specs], got_valid.tolist(), n_valid.tolist(), got_rep.tolist(), n_rep.tolist())
    check_rows(pr.download_longrepeat_intervals(), rows, what)
    assert np.array_equal(got_valid, n_valid) and np.array_equal(got_rep, n_rep), (what, got_valid, n_valid, got_rep, n_rep)


# ---- 1. the planted cases

@pytest.mark.parametrize("k", LC.K)
def test_cases_equal_the_model(k):
    """every case at (k, 0) and (k, 5); "copies" with six other lengths in front, VPR_LREP_MAX_SPEC entries in one call"""
    pr = api.PrecisionRecall()
    failed = []                          # every case runs, so that a failure names all the cases that catch it
    for name, case in LC.cases(k).items():
        specs = LC.specs_of(k, name)
        want = LM.all_intervals(case["contigs"], specs)
        own = len(specs) - 2
        assert [(int(a), int(b)) for a, b in zip(*want[0][own][0])] == case["tracts"][0], name       # (the declared tracts, once more)
        try:
            check_call(pr, case["contigs"], specs, (k, name), want)
        except AssertionError as e:
            failed.append((name, str(e)[:300]))
    assert not failed, failed


def edge_inputs(name):
    """(contigs, short specs, long specs) at the edges of what the two entries share: an entry without a valid start between two that
    have some, a genome without a called base, a genome of whole tiles"""
    rng = np.random.RandomState(11)
    if name == "no valid start":         # three contigs of 20 called bases, the third the first one's reverse complement
        a = LC.rand(rng, 20)
        return [a, LC.rand(rng, 20), LC.revcomp(a)], [A.rep_kmer(16), A.rep_kmer(24), A.rep_kmer(16, 3)], [A.rep_kmer(33)]
    if name == "all N":                  # (and an empty contig between the two)
        return [b"N" * 5000, b"", b"N" * 4096], api.repeats_default()[1], api.longrepeats_default()[1]
    s = bytearray(LC.rand(rng, 8192))    # "whole tiles": 8192 called bases, 2 tiles of the pack and 4 of the pair kernel, one 300-base copy
    s[5000:5300] = s[1000:1300]
    return [bytes(s)], [A.rep_kmer(32)], api.longrepeats_default()[1]


@pytest.mark.parametrize("name", ["no valid start", "all N", "whole tiles"])
def test_edges_of_the_shared_tail_equal_the_models(name):
    contigs, short, long_ = edge_inputs(name)
    want_short, want_long = RM.all_intervals(contigs, short), LM.all_intervals(contigs, long_)
    empty = lambda rows: all(len(r[0]) == 0 and len(r[1]) == 0 for r in rows)
    # (what the inputs are about, on the model)
    if name == "no valid start":
        assert want_short[1].tolist() == [15, 0, 15] and want_short[2].tolist() == [10, 0, 10] and empty(want_short[0][1])
        assert not empty(want_short[0][0]) and not empty(want_short[0][2]) and want_long[1].tolist() == [0] and empty(want_long[0][0])
    elif name == "all N":
        for want in (want_short, want_long):
            assert not want[1].any() and not want[2].any() and all(empty(rows) for rows in want[0])
    else:
        assert len(contigs[0]) == 8192 and all(n > 0 for n in want_long[2]) and want_short[2][0] >= 2 * (300 - 31)
    pr = api.PrecisionRecall()
    for _ in range(2):                   # (the second round meets the first one's buffers)
        pr.repeat_intervals(contigs, short)
        check_rows(pr.download_repeat_intervals(), want_short[0], (name, "short"))
        got = pr.repeat_stats()
        assert np.array_equal(got[0], want_short[1]) and np.array_equal(got[1], want_short[2]), (name, got, want_short[1:])
        check_call(pr, contigs, long_, (name, "long"), want_long)


# ---- 2. determinism

def snapshot(pr):
    L = api.lib()
    n_spec, n_ctg = pr._longrepeats
    off = np.zeros(n_spec * n_ctg + 1, np.int64)
    assert L.vpr_longrepeat_interval_counts(pr._h, A._ptr(off, C.c_int64)) == 0
    st, sp = np.zeros(int(off[-1]) + 1, np.int32), np.zeros(int(off[-1]) + 1, np.int32)
    assert L.vpr_longrepeat_download_intervals(pr._h, A._ptr(st, C.c_int32), A._ptr(sp, C.c_int32)) == 0
    return (off, st, sp) + pr.longrepeat_stats(levels=True)


def test_two_calls_and_a_fresh_handle_give_identical_arrays(monkeypatch):
    case = LC.cases(100)["copies"]
    specs = LC.specs_of(100, "copies")
    pr = api.PrecisionRecall()
    pr.longrepeat_intervals(case["contigs"], specs)
    one = snapshot(pr)
    assert all(t > 0 for t in pr.longrepeat_timing())
    pr.longrepeat_intervals(case["contigs"], specs)
    two = snapshot(pr)
    other = api.PrecisionRecall()
    other.longrepeat_intervals(case["contigs"], specs)
    three = snapshot(other)
    assert one[0][-1] >= 8 * 6 and (one[6][:2] > 0).all() and one[6][0] > 8000       # the base level sorted every valid 32-mer start
    assert one[6][1] < one[6][0] / 4 and one[6][2] <= one[6][1]                  # the upper levels sort candidates only
    for a, b, c in zip(one, two, three):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # the run passes over pieces of one contig each: the same rows
    monkeypatch.setenv("VPR_CONTEXT_PIECE_BASES", "5000")
    pr.longrepeat_intervals(case["contigs"], specs)
    assert all(np.array_equal(a, b) for a, b in zip(snapshot(pr), one))


# ---- 3. state and arguments

def test_state_and_arguments():
    pr = api.PrecisionRecall()
    L = api.lib()
    case = LC.cases(40)["copies"]
    contigs = case["contigs"]
    ok = [A.rep_kmer(40)]

    def refused(code, f, *a, **kw):
        with pytest.raises(api.VprError) as e:
            f(*a, **kw)
        assert f"({code})" in str(e.value), str(e.value)
        return str(e.value)
    off1 = np.zeros(3, np.int64)
    buf = np.zeros(64, np.int32)
    # before any call: VPR_ERR_STATE from the count, the download and the stats
    refused(-4, pr.download_longrepeat_intervals)
    assert L.vpr_longrepeat_interval_counts(pr._h, A._ptr(off1, C.c_int64)) == -4
    assert L.vpr_longrepeat_download_intervals(pr._h, A._ptr(buf, C.c_int32), A._ptr(buf, C.c_int32)) == -4
    assert L.vpr_longrepeat_download_intervals(pr._h, None, None) == -4
    refused(-4, pr.longrepeat_stats)
    pr.longrepeat_intervals(contigs, ok)
    rows = pr.download_longrepeat_intervals()
    assert [[(int(a), int(b)) for a, b in zip(*r)] for r in rows[0]] == case["tracts"]
    assert L.vpr_longrepeat_download_intervals(pr._h, None, None) == -1         # null pointers: VPR_ERR_ARG
    assert L.vpr_longrepeat_interval_counts(pr._h, None) == -1
    for bad, what in ((A.rep_kmer(32), "k 32"), (A.rep_kmer(257), "k 257"), (A.rep_kmer(64, -1), "slop -1")):
        msg = refused(-1, pr.longrepeat_intervals, contigs, [ok[0], bad])
        assert "vpr_longrepeat_intervals" in msg and "entry 1" in msg and what in msg, msg
        refused(-4, pr.download_longrepeat_intervals)               # after a refused call the earlier intervals are gone
        refused(-4, pr.longrepeat_stats)
        pr.longrepeat_intervals(contigs, ok)
    for spec in ([], ok * 9):
        msg = refused(-1, pr.longrepeat_intervals, contigs, spec)
        assert "vpr_longrepeat_intervals" in msg and "n_spec" in msg, msg
    pr.longrepeat_intervals(contigs, ok * 8)                        # the limit itself
    assert not LM.same(pr.download_longrepeat_intervals(), rows * 8)
    msg = refused(-1, pr.longrepeat_intervals, contigs, None)
    assert "vpr_longrepeat_intervals" in msg and "null spec" in msg, msg
    seq = np.frombuffer(b"".join(contigs), np.uint8)
    off = np.array([1, len(contigs[0]), len(seq)], np.int64)
    msg = refused(-1, pr.longrepeat_intervals, (off, seq), ok)
    assert "vpr_longrepeat_intervals" in msg and "ctg_off[0]" in msg, msg
    refused(-4, pr.download_longrepeat_intervals)
    refused(-4, pr.longrepeat_stats)
    # after a refused call the handle still works
    pr.longrepeat_intervals(contigs, ok)
    assert not LM.same(pr.download_longrepeat_intervals(), rows)


def test_both_repeat_entries_on_one_handle():
    """vpr_repeat_intervals and vpr_longrepeat_intervals keep their intervals apart: either survives the other's calls and refusals"""
    pr = api.PrecisionRecall()
    contigs = LC.cases(64)["copies"]["contigs"]
    short, long_ = [A.rep_kmer(32), A.rep_kmer(20, 2)], [A.rep_kmer(64), A.rep_kmer(33, 1)]
    want_short, want_long = RM.all_intervals(contigs, short), LM.all_intervals(contigs, long_)
    assert not LM.same(LM.all_intervals(contigs, [A.rep_kmer(32)])[0], want_short[0][:1])         # (one family: the models agree at 32)
    pr.repeat_intervals(contigs, short)
    pr.longrepeat_intervals(contigs, long_)
    check_rows(pr.download_repeat_intervals(), want_short[0], "short after long")
    check_rows(pr.download_longrepeat_intervals(), want_long[0], "long")
    pr.repeat_intervals(contigs, short[:1])
    check_rows(pr.download_longrepeat_intervals(), want_long[0], "long after short")
    assert np.array_equal(pr.longrepeat_stats()[1], want_long[2]) and np.array_equal(pr.repeat_stats()[1], want_short[2][:1])
    with pytest.raises(api.VprError):
        pr.longrepeat_intervals(contigs, [A.rep_kmer(32)])
    check_rows(pr.download_repeat_intervals(), want_short[0][:1], "short after a refused long")
    with pytest.raises(api.VprError):
        pr.download_longrepeat_intervals()
    pr.longrepeat_intervals(contigs, long_)
    with pytest.raises(api.VprError):
        pr.repeat_intervals(contigs, [A.rep_kmer(33)])
    check_rows(pr.download_longrepeat_intervals(), want_long[0], "long after a refused short")


# ---- 4. the command lines

from test_gpu_varstrata import STRAT_BOOT, STRAT_FILES, _without_command     # noqa: E402 -- the helpers of the variant-strata twin

LONG_BED = "long-repeat-strata.bed"
LINE = r"long repeat strata: (\d+) intervals of 3 strata, (\d+) valid and (\d+) repeated starts \(k=64\), (\d+) valid and (\d+) repeated starts " \
       r"\(k=100\), (\d+) valid and (\d+) repeated starts \(k=250\), ([0-9.]+) ms on the device"


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the small planted FASTA, its two VCFs and the model's intervals of the default set on it"""
    tmp = tmp_path_factory.mktemp("longrepeats_cli")
    ctg_names, contigs = LC.cli_inputs()
    fa = tmp / "planted.fa"
    fa.write_text("".join(f">{n}\n{c.decode()}\n" for n, c in zip(ctg_names, contigs)))
    (tmp / "truth.vcf").write_text(LC.cli_vcf(ctg_names, contigs, False))
    (tmp / "query.vcf").write_text(LC.cli_vcf(ctg_names, contigs, True))
    names, specs = api.longrepeats_default()
    rows, n_valid, n_rep = LM.all_intervals(contigs, specs)
    inputs = [str(tmp / "query.vcf"), str(tmp / "truth.vcf"), str(fa)]
    return dict(tmp=tmp, inputs=inputs, ctg_names=ctg_names, names=names, rows=rows, n_valid=n_valid, n_rep=n_rep)


def _list_of_bed(tmp, bed_path, names, list_name):
    """a --stratify list over the rows of a strata BED, one BED per name"""
    text = open(bed_path).read().split("\n")[:-1]
    lines = []
    for n in names:
        (tmp / f"{list_name}.{n}.bed").write_text("".join(l.rsplit("\t", 1)[0] + "\n" for l in text if l.endswith("\t" + n)))
        lines.append(f"{n}\t{list_name}.{n}.bed\n")
    (tmp / list_name).write_text("".join(lines))
    return str(tmp / list_name)


def test_command_lines_on_a_planted_fasta(planted, tmp_path):
    names, rows, inputs = planted["names"], planted["rows"], planted["inputs"]
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    boot = ["--bootstrap", "8"]
    runs = {}

    def run(name, cmd, extra):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    for name, cmd, extra in (("c", cli, []), ("c-l", cli, ["--stratify-long-repeats"] + boot), ("py-l", py, ["--stratify-long-repeats"] + boot),
                             ("c-n", cli, ["--stratify-long-repeats", "-n"]), ("c-ro", cli, ["--stratify-long-repeats", "-rq", "-ro"]),
                             ("c-all", cli, ["--stratify-repeats", "--stratify-long-repeats", "--stratify-context", "--stratify-variants"]),
                             ("py-all", py, ["--stratify-repeats", "--stratify-long-repeats", "--stratify-context", "--stratify-variants"])):
        run(name, cmd, extra)
    rd = lambda p: open(p, "rb").read()
    # long-repeat-strata.bed equals the model; the C++ and the Python files are byte-identical
    want_bed = LM.long_repeat_bed_text(names, planted["ctg_names"], rows).encode()
    assert rd(runs["c-l"][0] + LONG_BED) == want_bed and rd(runs["py-l"][0] + LONG_BED) == want_bed and len(want_bed) > 200
    # the end-to-end check: the same tables as --stratify LIST over long-repeat-strata.bed under the same names
    lst = _list_of_bed(tmp_path, runs["c-l"][0] + LONG_BED, names, "long.tsv")
    run("c-list", cli, ["--stratify", lst] + boot)
    for f in STRAT_FILES + (STRAT_BOOT,):
        assert rd(runs["c-l"][0] + f) == rd(runs["py-l"][0] + f), f
        assert rd(runs["c-l"][0] + f) == rd(runs["c-list"][0] + f) and len(rd(runs["c-l"][0] + f)) > 500, f
    assert not os.path.exists(runs["c-list"][0] + LONG_BED) and not os.path.exists(runs["c"][0] + LONG_BED)
    # every default stratum has a member, and rep_k250 (no 120-base copy) fewer than rep_k64
    summary = [l.split("\t") for l in open(runs["c-l"][0] + STRAT_FILES[0]).read().split("\n")[1:-1]]
    none_all = {r[0]: [int(x) for x in r[4:8]] for r in summary if r[1] == "ALL" and r[2] == "NONE"}
    assert list(none_all) == names and all(sum(v) > 0 for v in none_all.values()), none_all
    assert sum(none_all["rep_k250"]) < sum(none_all["rep_k64"])
    # behind the strata of --stratify-repeats, in front of those of --stratify-context and --stratify-variants; both drivers alike
    order = []
    for l in open(runs["c-all"][0] + STRAT_FILES[0]).read().split("\n")[1:-1]:
        if l.split("\t")[0] not in order:
            order.append(l.split("\t")[0])
    a = order.index("rep_k64")
    assert order[a - 1] == "rep_k32" and order[a:a + 3] == names and len(order) > a + 3 + 4, order
    for f in os.listdir(runs["c-all"][0]):
        assert _without_command(runs["c-all"][0] + f) == _without_command(runs["py-all"][0] + f), f
    assert rd(runs["c-all"][0] + LONG_BED) == want_bed and os.path.exists(runs["c-all"][0] + "repeat-strata.bed")
    # the run without the option is unchanged: every file of the plain run, and stdout
    plain = sorted(os.listdir(runs["c"][0]))
    extra = {f for f in os.listdir(runs["c-l"][0]) if f not in plain}
    assert set(STRAT_FILES) | {STRAT_BOOT, LONG_BED} <= extra and all("strat" in f or "bootstrap" in f for f in extra), extra
    for f in plain:
        assert _without_command(runs["c"][0] + f) == _without_command(runs["c-l"][0] + f), f
    assert runs["c"][1] == runs["c-l"][1] == runs["py-l"][1] == runs["c-n"][1]
    assert "stratified" not in runs["c"][2] and "repeat" not in runs["c"][2]
    # stderr: the line with the intervals, the start counts and the device time (also under -n, not under -ro)
    n_iv = sum(len(r[c][0]) for r in rows for c in range(2))
    for name in ("c-l", "py-l", "c-n", "c-all", "py-all"):
        m = re.findall(LINE, runs[name][2])
        assert len(m) == 1 and int(m[0][0]) == n_iv and float(m[0][7]) > 0, runs[name][2][-800:]
        assert [int(x) for x in m[0][1:7:2]] == planted["n_valid"].tolist() and [int(x) for x in m[0][2:7:2]] == planted["n_rep"].tolist()
    assert os.listdir(runs["c-n"][0]) == []                                   # -n: no file appears
    assert "long repeat strata" not in runs["c-ro"][2] and not os.path.exists(runs["c-ro"][0] + LONG_BED)
    # a long repeat name that is also a name of the list ends the run before anything is evaluated
    bad = tmp_path / "bad.tsv"
    bad.write_text("whole\tlong.tsv.rep_k64.bed\nrep_k100\tlong.tsv.rep_k250.bed\n")
    for cmd in (cli, py):
        r = subprocess.run(cmd + inputs + ["-n", "--stratify", str(bad), "--stratify-long-repeats"], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode != 0 and "duplicate stratum name 'rep_k100'" in r.stderr and "PRECISION-RECALL" not in r.stdout
        r = subprocess.run(cmd + inputs + ["-n", "--stratify", str(bad)], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]                             # (the list alone is fine)


# ---- 5. two ranks on one GPU

@pytest.fixture(scope="module")
def one_rank(planted):
    tmp = planted["tmp"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), VCFDIST_ONE_GPU="1")
    base = planted["inputs"] + ["--stratify-long-repeats", "--bootstrap", "8", "--classify-errors", "--cut-classes"]
    (tmp / "one").mkdir()
    subprocess.run([sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL, timeout=300)
    return tmp, base, env


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_command_line_two_ranks(one_rank, planted, how):
    tmp, base, env = one_rank
    out = tmp / how
    out.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # (the child runs under its own time limit: a rank that hangs in a collective is ended, not waited for)
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vcfdist_amd"] + base + ["-p", str(out) + "/", "--shard", how],
                   check=True, env=env, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=330)
    for name in STRAT_FILES + (STRAT_BOOT, LONG_BED, "precision-recall.tsv", "precision-recall-summary.tsv", "stratified-error-classes-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 60, name
    assert (out / LONG_BED).read_text() == LM.long_repeat_bed_text(planted["names"], planted["ctg_names"], planted["rows"])
