"""Error classes on the GPU (include/vcfdist_errclass.h, pr_errclass.hip): the class bytes and the counts against the brute-force
model of tests/errclass_model.py (hand cases, random and edge shapes, a synthetic batch with the counters' invariant and the
all-reduce entry), the state machine of the calls, and both command lines with --classify-errors on one and on two ranks.
tests/test_errclass_model.py checks on the CPU that none of this passes vacuously."""
import copy
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import errclass_cases as EC
import errclass_model as EM
from label_common import _without_command, _write_fasta, two_contig_run, var_classes
from vcfdist_amd import _abi as A
from vcfdist_amd import api, summary as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(pr, v, res, cls, pb, window=50, min_qual=0, max_qual=60, first=False):
    """one vpr_errclass call: bytes and counts equal the model's on the downloaded results -> (bytes, counts)"""
    got = pr.errclass(v, cls if first else None, pb, window, min_qual, max_qual)
    cl = pr.errclass_download()
    want = EM.classes(v, res, pb, window)
    for s in range(4):
        assert cl[s].shape == want[s].shape and np.array_equal(cl[s], want[s]), (s, window, np.nonzero(cl[s] != want[s]))
    assert np.array_equal(got, EM.counts(v, res, pb, want, cls, min_qual, max_qual)), (window, min_qual, max_qual)
    return cl, got


# ---- 1. the hand batch

@pytest.fixture(scope="module")
def hand():
    v, cases = EC.hand_case()
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32))
    return dict(v=v, cases=cases, pr=pr, res=res, pb=pb, cls=var_classes(v))


def test_hand_batch_equals_the_model(hand):
    v, cases, pr, res, pb, cls = (hand[k] for k in ("v", "cases", "pr", "res", "pb", "cls"))
    cl, got = check(pr, v, res, cls, pb, first=True)
    assert pr.errclass_timing() > 0
    assert EC.populated(cl) == (list(range(6)), list(range(7)))
    for name, slot, k, want in EC.expect(50):                                      # and literally, as on the CPU
        assert cl[slot][EC.index_of(v, cases, name, slot, k)] == want, (name, slot, k)
    again = pr.errclass(v, None, pb)                                               # a second call gives identical bytes
    assert np.array_equal(again, got) and all(np.array_equal(a, b) for a, b in zip(pr.errclass_download(), cl))
    for window in (0, 10, 2 ** 31 - 1):
        check(pr, v, res, cls, pb, window)
    rng = np.random.RandomState(4)
    for other in (None, np.zeros(v.n_sc, np.int32), np.ones(v.n_sc, np.int32), rng.randint(0, 2, v.n_sc).astype(np.int32)):
        check(pr, v, res, cls, other)
    for mn, mx in ((30, 30), (15, 40), (7, 60)):                                   # nq = 1, and a min_qual above 0
        check(pr, v, res, cls, pb, 50, mn, mx)


# ---- 2. random and edge shapes

@pytest.mark.parametrize("shape", ["random", "edge"])
def test_random_and_edge_shapes_equal_the_model(shape):
    v = EC.random_variants() if shape == "random" else EC.edge_variants()
    assert [v.n_vars(s) for s in range(4)] == ([513, 257, 640, 300] if shape == "random" else [1, 0, 513, 0])
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32))
    cls = var_classes(v, 6)
    cl, got = check(pr, v, res, cls, pb, first=True)
    if shape == "random":
        assert EC.populated(cl) == (EC.RANDOM_POPULATED_QUERY, EC.RANDOM_POPULATED_TRUTH)
    else:
        assert (cl[2] == A.EC_ALONE).sum() > 400 and cl[1].shape == (0,)
    plain = S.pr_counts(pr, None, pb)
    assert np.array_equal(got[0].sum(1), plain[0, :, A.ERRTYPE_FP]) and np.array_equal(got[1].sum(1), plain[1, :, A.ERRTYPE_FN])
    check(pr, v, res, cls, None, 3, 10, 50)


# ---- 3. the synthetic batch: the counters' invariant, the all-reduce entry

def test_synth_batch_invariant_and_allreduce():
    from vcfdist_amd import rccl
    v = EC.synth().variants()
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    pb, _, _ = S.phase(res.sc_phase, np.ones(v.n_sc, np.int32))
    cls = var_classes(v, 6)
    plain = S.pr_counts(pr, cls, pb)
    got = pr.errclass(v, None, pb)
    assert plain.any() and plain[0, 3, A.ERRTYPE_FP].any() and plain[1, 3, A.ERRTYPE_FN].any()
    for t in range(4):                                                             # every type, every threshold
        assert np.array_equal(got[0, t].sum(0), plain[0, t, A.ERRTYPE_FP]) and np.array_equal(got[1, t].sum(0), plain[1, t, A.ERRTYPE_FN]), t
    assert not got[0, :, A.EC_LOWQ].any() and np.array_equal(got[:, 3], got[:, :3].sum(1))
    assert np.array_equal(got, EM.counts(v, res, pb, pr.errclass_download(), cls))
    if not rccl.available():
        pytest.skip("no RCCL library in this process")
    torch.cuda.set_device(0)
    comm = rccl.Comm(1, 0, rccl.unique_id())
    try:
        assert np.array_equal(rccl.allreduce_errclass(pr, comm, v, None, pb), got)
    finally:
        comm.destroy()


# ---- 4. state and arguments

def test_state_and_arguments(hand):
    v, res, pb, cls = hand["v"], hand["res"], hand["pb"], hand["cls"]
    pr = api.PrecisionRecall()

    def refused(code, call=None, *a, **kw):
        with pytest.raises(api.VprError) as e:
            (call or pr.errclass)(*a, **kw)
        assert f"({code})" in str(e.value) and "vpr_errclass" in str(e.value), str(e.value)
        return str(e.value)
    batch = api.batch_from_variants(v)
    pr.upload(batch)
    assert "before vpr_execute" in refused(-4, None, v, cls, pb)                   # a call before vpr_execute
    refused(-4, pr.errclass_download)                                              # a download before a call
    pr.execute()
    res = pr.download()
    # other variant counts: the slot and both numbers
    other = EC.edge_variants()
    msg = refused(-4, None, other, cls, pb)
    assert "300 superclusters" in msg and f"batch {v.n_sc}" in msg, msg
    short = copy.deepcopy(v)
    short.var_off[2] = np.minimum(short.var_off[2], v.n_vars(2) - 1)
    msg = refused(-4, None, short, cls, pb)
    assert "hap slot 2" in msg and f"{v.n_vars(2) - 1} variants" in msg and f"batch {v.n_vars(2)}" in msg, msg
    # var_pos unsorted inside a supercluster: the slot and the variant
    bad = copy.deepcopy(v)
    i = EC.index_of(v, hand["cases"], "phase_orig", 0)
    bad.var_pos[0][[i, i + 1]] = bad.var_pos[0][[i + 1, i]]
    msg = refused(-1, None, bad, cls, pb)
    assert "hap slot 0" in msg and "var_pos is unsorted" in msg and f"variant {i + 1} " in msg, msg
    bad = copy.deepcopy(v)
    bad.var_alt_len[3][0] = -1
    assert "hap slot 3" in refused(-1, None, bad, cls, pb)
    assert "window -1" in refused(-1, None, v, cls, pb, -1)
    assert "max_qual 10 is below min_qual 20" in refused(-1, None, v, cls, pb, 50, 20, 10)
    assert "more than 779 thresholds" in refused(-1, None, v, cls, pb, 50, 0, 779)
    refused(-4, pr.errclass_download)                                              # no refused call left bytes behind
    # no order between superclusters is required, and after the refusals the handle gives the right bytes
    check(pr, v, res, cls, pb, first=True)
    pr.upload(batch)                                                               # the bytes go with the next upload
    refused(-4, pr.errclass_download)


# ---- 5. the command lines

EC_FILES = ("error-classes.tsv", "error-classes-summary.tsv")
OTHER = ("stratified-precision-recall-summary.tsv", "stratified-precision-recall.tsv", "variant-strata.tsv",
         "stratified-bootstrap-precision-recall-summary.tsv", "bootstrap-precision-recall-summary.tsv", "bootstrap-replicates.tsv")


@pytest.fixture(scope="module")
def demo():
    """the demo callsets through the CPU oracle chain (tests/demo_pipeline.py) and the model's text of the two files"""
    import demo_pipeline as D
    rows, det = D.run(product=False)
    v, cls = EC.demo_variants(det)
    cl = EM.classes(v, det["res"], det["pb"], 50)
    cnt = EM.counts(v, det["res"], det["pb"], cl, cls, D.G["min_qual"], D.G["max_qual"])
    text = EM.tsv_text(cnt, det["counts"], D.G["min_qual"], D.G["max_qual"])
    return dict(populated=EC.populated(cl), counts=cnt, files=dict(zip(EC_FILES, text)))


def test_command_lines_on_demo_files(demo, tmp_path):
    import demo_pipeline as D
    from vcfdist_amd.__main__ import main
    assert demo["populated"] == (EC.DEMO_POPULATED_QUERY, EC.DEMO_POPULATED_TRUTH)
    for c in EC.DEMO_POPULATED_QUERY:
        assert demo["counts"][0, 3, c, 0] > 0 and f"\t{int(demo['counts'][0, 3, c, 0])}\t" in demo["files"][EC_FILES[1]]
    for c in EC.DEMO_POPULATED_TRUTH:
        assert demo["counts"][1, 3, c].max() > 0
    fa = _write_fasta(tmp_path / "surrogate.fa", D.surrogate_fasta(5_100_000), ("chr1",))
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    others = ["--stratify-variants", "--bootstrap", "16"]
    runs = {}
    for name, cmd, extra in (("c", cli, []), ("c-e", cli, ["--classify-errors"]), ("py-all", py, others + ["--classify-errors", "--error-window", "50"]),
                             ("c-others", cli, others), ("c-n", cli, ["--classify-errors", "-n"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    # the two files: byte-identical from both drivers, alone or beside the other features, and the model's text on the oracle chain
    for f in EC_FILES:
        assert rd(runs["c-e"][0] + f) == rd(runs["py-all"][0] + f), f
        assert rd(runs["c-e"][0] + f).decode() == demo["files"][f], f
    # the other features' files are what they are without the option
    for f in OTHER:
        assert rd(runs["py-all"][0] + f) == rd(runs["c-others"][0] + f) and len(rd(runs["c-others"][0] + f)) > 100, f
    # the run without the option is unchanged: every file of the plain run, and stdout
    plain = sorted(os.listdir(runs["c"][0]))
    assert not set(EC_FILES) & set(plain) and sorted(set(os.listdir(runs["c-e"][0])) - set(EC_FILES)) == plain
    assert sorted(set(os.listdir(runs["py-all"][0])) - set(EC_FILES) - set(OTHER)) == plain
    for name in ("c-e", "py-all"):
        for f in plain:
            assert _without_command(runs["c"][0] + f) == _without_command(runs[name][0] + f), (name, f)
    assert runs["c"][1] == runs["c-e"][1] == runs["py-all"][1] == runs["c-others"][1] == runs["c-n"][1]
    assert "error classes" not in runs["c"][2] and "error classes" not in runs["c-others"][2]
    # stderr: the window, the classified query FP and truth FN at threshold NONE, the device time
    n_fp, n_fn = int(demo["counts"][0, 3, :, 0].sum()), int(demo["counts"][1, 3, :, 0].sum())
    for name in ("c-e", "py-all", "c-n"):
        m = re.findall(r"error classes: window 50, (\d+) query FP and (\d+) truth FN classified, ([0-9.]+) ms on the device", runs[name][2])
        assert len(m) == 1 and (int(m[0][0]), int(m[0][1])) == (n_fp, n_fn) and float(m[0][2]) > 0, runs[name][2][-500:]
    assert n_fp > 0 and n_fn > 0 and os.listdir(runs["c-n"][0]) == []            # -n: no file appears
    # the window is checked when the arguments are parsed: nothing is read, nothing is evaluated
    for extra, text in ((["--error-window", "10"], "--error-window needs --classify-errors"), (["--classify-errors", "--error-window", "-1"], "error window"),
                        (["--classify-errors", "--error-window", "x"], "error window")):
        out = tmp_path / "bad"
        with pytest.raises(SystemExit):
            main(inputs + ["-p", str(out) + "/"] + extra)
        assert not out.exists()


@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    """the demo callsets twice, as chr1 and chr2, and the one-rank run with --classify-errors"""
    return two_contig_run(tmp_path_factory.mktemp("errclass_two"), ["--classify-errors", "--error-window", "20"])


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_command_line_two_ranks(two_contigs, how):
    tmp, base, env = two_contigs
    out = tmp / how
    out.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # (the child runs under its own time limit: a rank that hangs in a collective is ended, not waited for)
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vcfdist_amd"] + base + ["-p", str(out) + "/", "--shard", how],
                   check=True, env=env, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=660)
    for name in EC_FILES + ("precision-recall.tsv", "precision-recall-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 60, name
    text = (out / EC_FILES[1]).read_text().split("\n")
    cells = [int(x) for x in text[[l.split("\t")[:2] for l in text].index(["ALL", "NONE"])].split("\t")[3:]]
    assert cells[0] == sum(cells[1:7]) > 0 and cells[7] == sum(cells[8:]) > 0 and cells[0] % 2 == 0 and cells[7] % 2 == 0     # both contigs hold the demo
