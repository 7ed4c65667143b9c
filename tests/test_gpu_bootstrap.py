"""Bootstrap replicates of the precision/recall counters on the GPU (include/vcfdist_bootstrap.h, pr_cut.hip): every
replicate against the numpy definition (tests/bootstrap_model.py), exact integer equality throughout; the launch shapes
(replicate groups, variant spans, quality slices), the weight algebra (equal keys, split and permuted batches), the stratum
cut, seeds, the native collective, the state machine of the calls, and both command lines with --bootstrap (one rank and
two)."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import bootstrap_model as M
import strata_model as SM
from vcfdist_amd import _abi as A
from vcfdist_amd import api, io as IO, shard, summary as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1


@pytest.fixture(scope="module")
def counted(tmp_path_factory):
    """the batch of the strata tests' `counted` fixture, executed once, with three strata: the whole contig, the first third
    of a tiling, a random one"""
    syn = api.Synth(n_sc=4000, len_mode=1, len_a=25.0, len_b=1.0, len_min=4, len_max=2000, seed=31, p_keep=0.8, p_drop=0.1)
    v = syn.variants()
    batch = syn.batch()
    pr = api.PrecisionRecall()
    res = pr.run(batch)
    cls = [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold=6) for s in range(4)]
    pb, _, _ = S.phase(res.sc_phase, np.ones(batch.n_sc, np.int32))
    length = int(v.ctg_off[1])
    rng = np.random.RandomState(9)
    cuts = np.sort(rng.choice(np.arange(1, length), size=400, replace=False))
    strata = [("whole", [("c0", 0, length)]), ("tile0", [("c0", 0, length // 3)]),
              ("random", [("c0", int(a), int(b)) for a, b in zip(cuts[0::2], cuts[1::2])])]
    names, beds = IO.read_strata(SM.write_strata(tmp_path_factory.mktemp("boot_strata"), strata))
    loc = SM.locations(beds, ["c0"], v)
    keys = A.boot_keys(0, np.arange(batch.n_sc))
    return dict(v=v, batch=batch, pr=pr, res=res, cls=cls, pb=pb, beds=beds, loc=loc, keys=keys)


def _three_contigs():
    """the three-contig 600-supercluster batch of the strata tests (supercluster k lies on contig k % 3) and its keys"""
    syn = api.Synth(n_sc=600, len_a=10, len_b=300, len_max=300, seed=7, var_per_base=0.02)
    v = syn.variants()
    n = int(v.ctg_off[1])
    v.ctg_off = np.array([0, n, 2 * n, 3 * n], np.int64)
    v.ctg_seq = np.ascontiguousarray(np.tile(v.ctg_seq, 3))
    v.sc_ctg = (np.arange(v.n_sc) % 3).astype(np.int32)
    keys = A.boot_keys(np.arange(v.n_sc) % 3, np.arange(v.n_sc) // 3)
    return v, keys


def _classes(v):
    return [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold=6) for s in range(4)]


# ---- 1. every replicate against the definition, over the launch shapes

@pytest.mark.parametrize("quals", [(0, 60), (30, 30), (0, 400)])
@pytest.mark.parametrize("n_rep", [1, 64, 65, 130])
def test_replicates_equal_the_model(counted, n_rep, quals):
    c = counted
    pr, batch, res, cls, pb, keys = c["pr"], c["batch"], c["res"], c["cls"], c["pb"], c["keys"]
    min_qual, max_qual = quals
    nq = max_qual - min_qual + 1
    got = pr.pr_counts_boot(cls, pb, keys, n_rep, SEED, min_qual, max_qual)
    assert got.shape == (n_rep, 2, 4, 3, nq) and got.dtype == np.int64
    want = M.expected_counts(batch.var_off, res, cls, pb, keys, SEED, n_rep, min_qual, max_qual)
    assert np.array_equal(got, want), np.nonzero((got != want).reshape(n_rep, -1).any(axis=1))[0][:8]
    assert got[:, :, 3].sum() > 0
    (spans, groups, slices), ms = pr.boot_info()
    assert groups == (n_rep + 63) // 64 and ms > 0
    # some slot ran in at least two spans: a span edge and 64-variant edges inside superclusters are exercised
    assert spans >= 2 and max(batch.n_vars(s) for s in range(4)) >= 2048
    bins = np.concatenate([b % (nq + 1) for _, b in M.variant_bins(batch.var_off, res, cls, pb, min_qual, max_qual)])
    if quals == (0, 400):
        assert slices > 1
        edge = -(-(nq + 1) // slices)                 # first quality bin of the second slice
        assert (bins == edge - 1).any() and (bins == edge).any(), edge         # callq on both sides of a slice edge
    else:
        assert slices == 1
    if quals == (30, 30):
        assert (bins == nq).any() and (bins == 0).any()                        # below the only threshold: the bin of no threshold


def test_point_estimate_is_untouched_and_sizes_are_awkward(counted):
    c = counted
    assert any(c["batch"].n_vars(s) % 64 for s in range(4))                    # n_var no multiple of 64
    total = S.pr_counts(c["pr"], c["cls"], c["pb"])
    assert np.array_equal(total, SM.O.oracle_pr_counts(SM.O.lib(), c["batch"].var_off, c["res"], c["cls"], c["pb"], 0, 60))
    # the fold of an unweighted histogram is the counters': the model at weight 1 for everybody
    ones = M.fold(np.stack([sum(np.bincount(b, minlength=9 * 62) for s, (_, b) in enumerate(M.variant_bins(c["batch"].var_off, c["res"], c["cls"], c["pb"]))
                                if s >> 1 == cs) for cs in range(2)]), 61)
    assert np.array_equal(ones, total)


def test_empty_hap_slot():
    v, keys = _three_contigs()
    for name in ("var_pos", "var_type", "var_qual", "var_ref_off", "var_ref_len", "var_alt_off", "var_alt_len"):
        getattr(v, name)[1] = getattr(v, name)[1][:0]
    v.var_off[1] = np.zeros_like(v.var_off[1])
    batch = api.batch_from_variants(v)
    assert batch.n_vars(1) == 0 and batch.n_vars(0) > 0 and any(batch.n_vars(s) % 64 for s in range(4))
    pr = api.PrecisionRecall()
    res = pr.run(batch)
    cls = _classes(v)
    pb, _, _ = S.phase(res.sc_phase, np.ones(batch.n_sc, np.int32))
    got = pr.pr_counts_boot(cls, pb, keys, 65, SEED)
    assert np.array_equal(got, M.expected_counts(batch.var_off, res, cls, pb, keys, SEED, 65)) and got.any()


# ---- 2. the weight algebra

def test_equal_keys_scale_the_point_counts(counted):
    c = counted
    pr, cls, pb = c["pr"], c["cls"], c["pb"]
    key, n_rep = (5 << 32) | 7, 130
    total = S.pr_counts(pr, cls, pb)
    got = pr.pr_counts_boot(cls, pb, np.full(c["batch"].n_sc, key, np.uint64), n_rep, SEED)
    w = M.weights(SEED, n_rep, [key])[:, 0]
    assert (w == 0).any() and (w >= 2).any() and total.any()
    for r in range(n_rep):
        assert np.array_equal(got[r], int(w[r]) * total), (r, int(w[r]))


def test_split_and_permuted_batches_draw_the_same_weights():
    v, keys = _three_contigs()
    whole = api.batch_from_variants(v)
    cls = _classes(v)
    pr = api.PrecisionRecall()
    res = pr.run(whole)
    pb, _, _ = S.phase(res.sc_phase, np.ones(whole.n_sc, np.int32))
    n_rep = 65
    want = pr.pr_counts_boot(cls, pb, keys, n_rep, SEED)
    assert np.array_equal(want, M.expected_counts(whole.var_off, res, cls, pb, keys, SEED, n_rep)) and want.any()

    def part(idx):
        pr.run(whole.subset(idx))
        cls_p = [shard.subset_per_variant(cls[s], whole.var_off[s], idx) for s in range(4)]
        return pr.pr_counts_boot(cls_p, pb[idx], keys[idx], n_rep, SEED)
    even, odd = part(np.arange(0, whole.n_sc, 2)), part(np.arange(1, whole.n_sc, 2))
    assert even.any() and odd.any() and np.array_equal(even + odd, want)
    perm = np.random.RandomState(4).permutation(whole.n_sc)
    assert np.array_equal(part(perm), want)
    # (the keys carry the weights: the same batch under other keys counts otherwise)
    assert not np.array_equal(pr.pr_counts_boot(None, pb[perm], keys, n_rep, SEED), want)


def test_seeds(counted):
    c = counted
    pr, cls, pb, keys = c["pr"], c["cls"], c["pb"], c["keys"]
    one = pr.pr_counts_boot(cls, pb, keys, 64, 1)
    assert np.array_equal(one, pr.pr_counts_boot(None, pb, keys, 64, 1))
    two = pr.pr_counts_boot(None, pb, keys, 64, 2)
    assert not np.array_equal(one, two)
    assert np.array_equal(two, M.expected_counts(c["batch"].var_off, c["res"], cls, pb, keys, 2, 64))
    big = 2 ** 64 - 3
    assert np.array_equal(pr.pr_counts_boot(None, pb, keys, 3, big), M.expected_counts(c["batch"].var_off, c["res"], cls, pb, keys, big, 3))


# ---- 3. the stratum cut

def test_stratum_cut(counted):
    c = counted
    pr, v, batch, res, cls, pb, keys, loc = c["pr"], c["v"], c["batch"], c["res"], c["cls"], c["pb"], c["keys"], c["loc"]
    pr.strata_masks(v, SM.strata_of(c["beds"], ["c0"]))
    n_rep = 65
    plain = pr.pr_counts_boot(cls, pb, keys, n_rep, SEED)
    got = [pr.pr_counts_boot(None, pb, keys, n_rep, SEED, stratum=k) for k in range(3)]
    for k in range(3):
        member = [loc[s][k] == SM.INSIDE for s in range(4)]
        assert np.array_equal(got[k], M.expected_counts(batch.var_off, res, cls, pb, keys, SEED, n_rep, member=member)), k
    assert all((loc[s][0] == SM.INSIDE).all() for s in range(4)) and np.array_equal(got[0], plain)
    assert got[1].any() and got[2].any() and (got[1] <= plain).all() and not np.array_equal(got[1], got[2])
    # the replicates of a stratum at weight 1 are the stratified counters
    ones = pr.pr_counts_boot(None, pb, np.full(batch.n_sc, 1, np.uint64), 1, SEED, stratum=2)
    assert int(M.weights(SEED, 1, [1])[0, 0]) == 1
    assert np.array_equal(ones[0], S.pr_counts_strata(pr, None, pb)[2])


# ---- 4. native collective

def test_native_collective_on_a_one_rank_communicator(counted):
    from vcfdist_amd import rccl
    if not rccl.available():
        pytest.skip("no RCCL library in this process")
    torch.cuda.set_device(0)
    c = counted
    comm = rccl.Comm(1, 0, rccl.unique_id())
    try:
        want = c["pr"].pr_counts_boot(c["cls"], c["pb"], c["keys"], 65, SEED)
        got = rccl.allreduce_counts_boot(c["pr"], comm, c["cls"], c["pb"], c["keys"], 65, SEED)
        assert want.sum() > 0 and np.array_equal(got, want)
    finally:
        comm.destroy()


# ---- 5. state and arguments

def test_state_and_arguments(counted):
    c = counted
    cls, pb, keys, batch = c["cls"], c["pb"], c["keys"], c["batch"]

    def refused(code, f, *a, **kw):
        with pytest.raises(api.VprError) as e:
            f(*a, **kw)
        assert f"({code})" in str(e.value) and len(str(e.value).split("): ", 1)[1]) > 10, str(e.value)      # every error carries a message
    pr = api.PrecisionRecall()
    pr.upload(batch)
    refused(-4, pr.pr_counts_boot, cls, pb, keys, 8)                          # before vpr_execute: VPR_ERR_STATE
    with pytest.raises(api.VprError, match=r"\(-1\)"):                         # (nothing has run)
        pr.boot_info()
    pr.execute()
    refused(-1, pr.pr_counts_boot, cls, pb, None, 8)                          # null sc_key
    for n_rep in (0, -1, A.BOOT_MAX_REPLICATES + 1):
        refused(-1, pr.pr_counts_boot, cls, pb, keys, n_rep)
    refused(-1, pr.pr_counts_boot, cls, pb, keys, 8, min_qual=5, max_qual=4)
    L = api.lib()
    key = np.ascontiguousarray(keys, np.uint64)
    assert L.vpr_pr_counts_boot(pr._h, None, None, 0, 60, A._ptr(key, api.C.c_uint64), 1, 8, -1, None) == -1       # null counts
    assert b"null" in L.vpr_last_error(pr._h)
    refused(-4, pr.pr_counts_boot, cls, pb, keys, 8, stratum=0)               # no membership words
    other = api.Synth(n_sc=50, len_a=10, len_b=300, len_max=300, seed=3, var_per_base=0.02).variants()
    pr.strata_masks(other, A.Strata([[([10], [2000])]], 1))
    refused(-4, pr.pr_counts_boot, cls, pb, keys, 8, stratum=0)               # words of another batch
    pr.strata_masks(c["v"], SM.strata_of(c["beds"], ["c0"]))
    refused(-1, pr.pr_counts_boot, cls, pb, keys, 8, stratum=3)               # stratum >= n_strata
    good = pr.pr_counts_boot(cls, pb, keys, 8, stratum=2)
    assert good.any() and pr.boot_info()[0][1] == 1
    # a further execute of the same batch keeps everything; the next upload ends it
    pr.execute()
    assert np.array_equal(good, pr.pr_counts_boot(None, pb, keys, 8, stratum=2))
    pr.upload(batch)
    refused(-4, pr.pr_counts_boot, cls, pb, keys, 8)


# ---- 6, 7. the command lines

BOOT_FILES = ("bootstrap-precision-recall-summary.tsv", "bootstrap-replicates.tsv")
STRAT_BOOT = "stratified-bootstrap-precision-recall-summary.tsv"


def test_command_lines_on_demo_files(tmp_path, monkeypatch):
    import demo_pipeline as D
    import test_gpu_strata as TS
    from vcfdist_amd import __main__ as CLI, report as RP
    fa = TS._surrogate(tmp_path)
    lst = TS._demo_strata(tmp_path)
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    boot = ["--bootstrap", "40", "--bootstrap-seed", "5"]
    runs = {}
    for name, cmd, extra in (("c", [cli], []), ("c-b", [cli], boot), ("py-b", [sys.executable, "-m", "vcfdist_amd"], boot),
                             ("c-sb", [cli], boot + ["--stratify", lst]), ("c-n", [cli], boot + ["-n"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    for f in BOOT_FILES:
        assert rd(runs["c-b"][0] + f) == rd(runs["py-b"][0] + f) == rd(runs["c-sb"][0] + f), f       # C++ and Python: the same bytes
        assert not os.path.exists(runs["c"][0] + f)
    # the model's writers, fed the driver's counts, write the same bytes (the Python driver once more, in this process)
    seen = {}
    real = RP.write_bootstrap
    monkeypatch.setattr(RP, "write_bootstrap", lambda prefix, counts, cb, seed, mn, mx: (seen.update(a=(counts.copy(), cb.copy(), seed, mn, mx)),
                                                                                         real(prefix, counts, cb, seed, mn, mx))[1])
    os.makedirs(str(tmp_path / "in-process"))
    CLI.main(inputs + ["-p", str(tmp_path / "in-process") + "/"] + boot)
    counts, cb, seed, mn, mx = seen["a"]
    assert cb.shape == (40, 2, 4, 3, 61) and seed == 5 and (mn, mx) == (0, 60)
    for f, text in zip(BOOT_FILES, M.bootstrap_files(counts, cb, seed, mn, mx)):
        assert rd(runs["c-b"][0] + f) == text.encode() == rd(str(tmp_path / "in-process") + "/" + f), f
    rows = [l.split("\t") for l in open(runs["c-b"][0] + BOOT_FILES[0]).read().split("\n")[1:-1]]
    assert len(rows) == 8 and all(r[3] == "40" and r[4] == "5" for r in rows)
    assert all(float(r[j + 1]) <= float(r[j + 2]) for r in rows for j in (5, 8, 11))
    assert any(float(r[6]) < float(r[7]) for r in rows if r[0] == "ALL")                       # an interval with some width
    # every other output file, and stdout, equal the run without the option
    plain = sorted(os.listdir(runs["c"][0]))
    assert sorted(set(os.listdir(runs["c-b"][0])) - set(BOOT_FILES)) == plain
    for f in plain:
        assert TS._without_command(runs["c"][0] + f) == TS._without_command(runs["c-b"][0] + f), f
    assert runs["c"][1] == runs["c-b"][1] == runs["py-b"][1] == runs["c-n"][1]
    # one line on stderr: replicates, seed, device milliseconds
    for name in ("c-b", "py-b", "c-sb", "c-n"):
        m = re.findall(r"bootstrap: 40 replicates, seed 5, ([0-9.]+) ms on the device", runs[name][2])
        assert len(m) == 1 and float(m[0]) > 0, runs[name][2][-500:]
    assert "bootstrap" not in runs["c"][2]
    assert os.listdir(runs["c-n"][0]) == []                                                    # -n: no file appears
    # with --stratify: the whole-contig stratum's rows are the unstratified table's; no stratified replicate file
    lines = open(runs["c-sb"][0] + STRAT_BOOT).read().split("\n")
    whole = "".join(l.split("\t", 1)[1] + "\n" for l in lines[:-1] if l.startswith(("STRATUM\t", "whole\t")))
    assert whole == open(runs["c-sb"][0] + BOOT_FILES[0]).read()
    assert {l.split("\t", 1)[0] for l in lines[1:-1]} == {"whole", "even", "odd"} and len(lines) == 1 + 24 + 1
    assert not os.path.exists(runs["c-b"][0] + STRAT_BOOT)
    assert sorted(set(os.listdir(runs["c-sb"][0])) - set(BOOT_FILES) - set(TS.STRAT_FILES) - {STRAT_BOOT}) == plain


@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    """the inputs of the strata tests' two-rank runs (the demo callsets twice, as chr1 and chr2, and a strata list over both)
    and the one-rank run with --bootstrap"""
    import gzip
    import demo_pipeline as D
    import test_gpu_strata as TS
    tmp = tmp_path_factory.mktemp("two_contigs_boot")
    fa = TS._surrogate(tmp, ("chr1", "chr2"))

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
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), VCFDIST_ONE_GPU="1")
    base = [str(qv), str(tv), fa, "-b", str(bed), "--stratify", TS._demo_strata(tmp, ("chr1", "chr2")), "--bootstrap", "40"]
    (tmp / "one").mkdir()
    subprocess.run([sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL, timeout=600)
    return tmp, base, env


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
    for name in BOOT_FILES + (STRAT_BOOT, "precision-recall-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 60, name
    text = (out / STRAT_BOOT).read_text()
    assert "whole\tALL\tNONE\t0\t40\t1\t" in text and "odd\tSNP\tBEST" in text
    # chr2 repeats chr1 under other keys: its superclusters draw their own weights, so the replicates are not chr1's doubled
    rep = [l.split("\t") for l in (out / BOOT_FILES[1]).read_text().split("\n")[1:-1] if l.split("\t")[1:3] == ["ALL", "NONE"]]
    assert len(rep) == 40 and any(int(r[4]) % 2 for r in rep)
