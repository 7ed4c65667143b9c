"""Match kinds on the GPU (include/vcfdist_matchkind.h, pr_matchkind.hip): the kind bytes and the counts against the brute-force
model of tests/matchkind_model.py (hand cases, shapes built for a 256-thread block, a synthetic batch with the counters' invariant
and the all-reduce entry), the state machine of the calls, and both command lines with --classify-matches on one and on two ranks.
tests/test_matchkind_model.py checks on the CPU that none of this passes vacuously."""
import copy
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import matchkind_cases as MC
import matchkind_model as MM
from label_common import _without_command, _write_fasta, two_contig_run, var_classes
from vcfdist_amd import _abi as A
from vcfdist_amd import api, summary as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(pr, v, res, cls, pb, min_qual=0, max_qual=60, first=False):
    """one vpr_matchkind call: bytes and counts equal the model's on the downloaded results -> (bytes, counts)"""
    got = pr.matchkind(v, cls if first else None, pb, min_qual, max_qual)
    kd = pr.matchkind_download()
    want = MM.kinds(v, res, pb)
    for s in range(4):
        assert kd[s].shape == want[s].shape and np.array_equal(kd[s], want[s]), (s, np.nonzero(kd[s] != want[s]))
    assert np.array_equal(got, MM.counts(v, res, pb, want, cls, min_qual, max_qual)), (min_qual, max_qual)
    return kd, got


def sums_equal_the_counters(got, plain):
    """for every type and threshold the four kinds of a callset sum to vpr_pr_counts' TP of that callset"""
    for t in range(4):
        assert np.array_equal(got[0, t].sum(0), plain[0, t, A.ERRTYPE_TP]) and np.array_equal(got[1, t].sum(0), plain[1, t, A.ERRTYPE_TP]), t
    assert np.array_equal(got[:, 3], got[:, :3].sum(1))


# ---- 1. the hand batch

@pytest.fixture(scope="module")
def hand():
    v, cases = MC.hand_case()
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32))
    return dict(v=v, cases=cases, pr=pr, res=res, pb=pb, cls=var_classes(v))


def test_hand_batch_equals_the_model(hand):
    v, cases, pr, res, pb, cls = (hand[k] for k in ("v", "cases", "pr", "res", "pb", "cls"))
    kd, got = check(pr, v, res, cls, pb, first=True)
    assert pr.matchkind_timing() > 0
    assert MC.populated(kd) == ([0, 1, 2, 3], [0, 1, 2, 3])
    for name, slot, k, want in MC.EXPECT:                                          # and literally, as on the CPU
        assert kd[slot][MC.index_of(v, cases, name, slot, k)] == want, (name, slot, k)
    again = pr.matchkind(v, None, pb)                                              # a second call gives identical bytes
    assert np.array_equal(again, got) and all(np.array_equal(a, b) for a, b in zip(pr.matchkind_download(), kd))
    rng = np.random.RandomState(4)
    for other in (None, np.zeros(v.n_sc, np.int32), np.ones(v.n_sc, np.int32), rng.randint(0, 2, v.n_sc).astype(np.int32)):
        check(pr, v, res, cls, other)
    for mn, mx in ((30, 30), (15, 40), (7, 60)):                                   # nq = 1, and a min_qual above 0
        check(pr, v, res, cls, pb, mn, mx)


# ---- 2. shapes built for a 256-thread block

@pytest.mark.parametrize("shape", ["random", "edge", "long"])
def test_block_shapes_equal_the_model(shape):
    v = {"random": MC.random_variants, "edge": MC.edge_variants, "long": MC.long_variants}[shape]()
    if shape != "long":
        assert [v.n_vars(s) for s in range(4)] == ([513, 257, 640, 300] if shape == "random" else [1, 0, 513, 0])
    else:
        assert v.n_sc == 1 and all(v.n_vars(s) > 256 for s in range(4))
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32))
    cls = var_classes(v, 50 if shape == "long" else 6)
    kd, got = check(pr, v, res, cls, pb, first=True)
    if shape == "random":
        assert MC.populated(kd) == ([0, 1, 2, 3], [0, 1, 2, 3]) and len(MM.interleaved_groups(v, res, pb)) >= 1
    elif shape == "edge":
        assert kd[1].shape == (0,) and (kd[2] == A.MK_NONE).sum() > 500
    else:
        assert got[0, 3, A.MK_SHIFTED, 0] == 2 * (len(MC.LONG_PLANTS) - 1) and len(MM.interleaved_groups(v, res, pb)) == 2
    sums_equal_the_counters(got, S.pr_counts(pr, None, pb))
    check(pr, v, res, cls, None, 10, 50)


# ---- 3. the synthetic batch: the counters' invariant, the all-reduce entry

def test_synth_batch_invariant_and_allreduce():
    from vcfdist_amd import rccl
    v = MC.synth().variants()
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    pb, _, _ = S.phase(res.sc_phase, np.ones(v.n_sc, np.int32))
    cls = var_classes(v, 6)
    plain = S.pr_counts(pr, cls, pb)
    got = pr.matchkind(v, None, pb)
    assert plain[0, 3, A.ERRTYPE_TP].any() and plain[1, 3, A.ERRTYPE_TP].any()
    sums_equal_the_counters(got, plain)                                            # every type, every threshold
    assert np.array_equal(got, MM.counts(v, res, pb, pr.matchkind_download(), cls))
    if not rccl.available():
        pytest.skip("no RCCL library in this process")
    torch.cuda.set_device(0)
    comm = rccl.Comm(1, 0, rccl.unique_id())
    try:
        assert np.array_equal(rccl.allreduce_matchkind(pr, comm, v, None, pb), got)
    finally:
        comm.destroy()


# ---- 4. state and arguments

def test_state_and_arguments(hand):
    v, res, pb, cls = hand["v"], hand["res"], hand["pb"], hand["cls"]
    pr = api.PrecisionRecall()

    def refused(code, call=None, *a, **kw):
        with pytest.raises(api.VprError) as e:
            (call or pr.matchkind)(*a, **kw)
        assert f"({code})" in str(e.value) and "vpr_matchkind" in str(e.value), str(e.value)
        return str(e.value)
    batch = api.batch_from_variants(v)
    pr.upload(batch)
    assert "before vpr_execute" in refused(-4, None, v, cls, pb)                   # a call before vpr_execute
    refused(-4, pr.matchkind_download)                                             # a download before a call
    pr.execute()
    res = pr.download()
    # other supercluster or variant counts: the slot and both numbers
    other = MC.edge_variants()
    msg = refused(-4, None, other, cls, pb)
    assert "300 superclusters" in msg and f"batch {v.n_sc}" in msg, msg
    short = copy.deepcopy(v)
    short.var_off[2] = np.minimum(short.var_off[2], v.n_vars(2) - 1)
    msg = refused(-4, None, short, cls, pb)
    assert "hap slot 2" in msg and f"{v.n_vars(2) - 1} variants" in msg and f"batch {v.n_vars(2)}" in msg, msg
    # var_pos unsorted inside a supercluster: the slot and the variant
    bad = copy.deepcopy(v)
    i = MC.index_of(v, hand["cases"], "het_shift", 0)
    bad.var_pos[0][[i, i + 1]] = bad.var_pos[0][[i + 1, i]]
    msg = refused(-1, None, bad, cls, pb)
    assert "hap slot 0" in msg and "var_pos is unsorted" in msg and f"variant {i + 1} " in msg, msg
    bad = copy.deepcopy(v)
    bad.var_alt_len[3][0] = -1
    assert "hap slot 3" in refused(-1, None, bad, cls, pb)
    assert "max_qual 10 is below min_qual 20" in refused(-1, None, v, cls, pb, 20, 10)
    assert "more than 1364 thresholds" in refused(-1, None, v, cls, pb, 0, 1364)
    # null counts, through the C entry itself
    vs = v.as_struct()
    assert api.lib().vpr_matchkind(pr._h, C.byref(vs), None, None, 0, 60, None) == -1
    assert "vpr_matchkind: null argument" in api.lib().vpr_last_error(pr._h).decode()
    refused(-4, pr.matchkind_download)                                             # no refused call left bytes behind
    # after the refusals the handle gives the right bytes
    check(pr, v, res, cls, pb, first=True)
    pr.upload(batch)                                                               # the bytes go with the next upload
    refused(-4, pr.matchkind_download)


# ---- 5. the command lines

MK_FILES = ("match-kinds.tsv", "match-kinds-summary.tsv")
OTHER = ("stratified-precision-recall-summary.tsv", "stratified-precision-recall.tsv", "variant-strata.tsv",
         "stratified-bootstrap-precision-recall-summary.tsv", "bootstrap-precision-recall-summary.tsv", "bootstrap-replicates.tsv",
         "error-classes.tsv", "error-classes-summary.tsv")
STDERR = (r"match kinds: query TP (\d+) exact, (\d+) shifted, (\d+) regrouped, (\d+) partial; truth TP (\d+) exact, (\d+) shifted, (\d+) regrouped, "
          r"(\d+) partial, ([0-9.]+) ms on the device")


@pytest.fixture(scope="module")
def demo():
    """the demo callsets through the CPU oracle chain (tests/demo_pipeline.py) and the model's text of the two files"""
    import demo_pipeline as D
    rows, det = D.run(product=False)
    v, cls = MC.demo_variants(det)
    kd = MM.kinds(v, det["res"], det["pb"])
    cnt = MM.counts(v, det["res"], det["pb"], kd, cls, D.G["min_qual"], D.G["max_qual"])
    text = MM.tsv_text(cnt, det["counts"], D.G["min_qual"], D.G["max_qual"])
    return dict(populated=MC.populated(kd), counts=cnt, files=dict(zip(MK_FILES, text)))


def test_command_lines_on_demo_files(demo, tmp_path):
    import demo_pipeline as D
    assert demo["populated"] == (MC.DEMO_POPULATED_QUERY, MC.DEMO_POPULATED_TRUTH)
    fa = _write_fasta(tmp_path / "surrogate.fa", D.surrogate_fasta(5_100_000), ("chr1",))
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    others = ["--classify-errors", "--stratify-variants", "--bootstrap", "20"]
    runs = {}
    for name, cmd, extra in (("c", cli, []), ("c-m", cli, ["--classify-matches"]), ("py-all", py, others + ["--classify-matches"]),
                             ("c-all", cli, ["--classify-matches"] + others), ("c-others", cli, others), ("c-n", cli, ["--classify-matches", "-n"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(["timeout", "-k", "10", "600"] + cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=660)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    # the two files: byte-identical from both drivers, alone or beside the other features, and the model's text on the oracle chain
    for f in MK_FILES:
        assert rd(runs["c-m"][0] + f) == rd(runs["py-all"][0] + f) == rd(runs["c-all"][0] + f), f
        assert rd(runs["c-m"][0] + f).decode() == demo["files"][f], f
    # the other features' files are what they are without the option
    for f in OTHER:
        assert rd(runs["py-all"][0] + f) == rd(runs["c-others"][0] + f) == rd(runs["c-all"][0] + f) and len(rd(runs["c-others"][0] + f)) > 100, f
    # the option adds exactly the two files; every file of the plain run, and stdout, are unchanged
    plain = sorted(os.listdir(runs["c"][0]))
    assert not set(MK_FILES) & set(plain)
    assert sorted(os.listdir(runs["c-m"][0])) == sorted(plain + list(MK_FILES))
    assert sorted(os.listdir(runs["py-all"][0])) == sorted(plain + list(MK_FILES) + list(OTHER))
    assert sorted(os.listdir(runs["c-all"][0])) == sorted(plain + list(MK_FILES) + list(OTHER))
    assert sorted(os.listdir(runs["c-others"][0])) == sorted(plain + list(OTHER))
    for name in ("c-m", "py-all", "c-all"):
        for f in plain:
            assert _without_command(runs["c"][0] + f) == _without_command(runs[name][0] + f), (name, f)
    assert len({runs[name][1] for name in runs}) == 1 and len(runs["c"][1]) > 100
    assert "match kinds" not in runs["c"][2] and "match kinds" not in runs["c-others"][2]
    # stderr: the eight counts at threshold NONE and the device time
    want = tuple(int(x) for x in demo["counts"][:, 3, :, 0].ravel())
    for name in ("c-m", "py-all", "c-all", "c-n"):
        m = re.findall(STDERR, runs[name][2])
        assert len(m) == 1 and tuple(int(x) for x in m[0][:8]) == want and float(m[0][8]) > 0, runs[name][2][-500:]
    assert want[0] > 0 and want[4] > 0 and os.listdir(runs["c-n"][0]) == []      # -n: no file appears


@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    """the demo callsets twice, as chr1 and chr2, and the one-rank run with --classify-matches"""
    return two_contig_run(tmp_path_factory.mktemp("matchkind_two"), ["--classify-matches"])


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
    for name in MK_FILES + ("precision-recall.tsv", "precision-recall-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 60, name
    text = (out / MK_FILES[1]).read_text().split("\n")
    cells = [int(x) for x in text[[l.split("\t")[:2] for l in text].index(["ALL", "NONE"])].split("\t")[3:]]
    assert cells[0] == sum(cells[1:5]) > 0 and cells[5] == sum(cells[6:]) > 0 and cells[0] % 2 == 0 and cells[5] % 2 == 0     # both contigs hold the demo
