"""The label counts cut by stratum and resampled on the GPU (include/vcfdist_labelcut.h, pr_cut.hip), for both label passes:
k_label_hist_strata and k_label_boot bit for bit against tests/labelcut_model.py on the downloaded label bytes (hand batches, the
random shapes under 70 random strata, replicate-group edges, quality slices, a permuted batch), the sums against the stratified
and the replicate counters, a synthetic batch with the all-reduce entries, the state machine of the calls, and both command lines
with --cut-classes on one and on two ranks.  tests/test_labelcut_model.py holds the model to its literal statement on the CPU."""
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
import labelcut_model as LM
import matchkind_cases as MC
import matchkind_model as MM
from label_common import _without_command, _write_fasta, two_contig_run, var_classes
from vcfdist_amd import _abi as A
from vcfdist_amd import api, shard, summary as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ("errclass", "matchkind")


def label(pr, name, v, cls, pb, min_qual=0, max_qual=60):
    """the label call of a pass -> (its counts, its bytes)"""
    got = pr.errclass(v, cls, pb, 50, min_qual, max_qual) if name == "errclass" else pr.matchkind(v, cls, pb, min_qual, max_qual)
    return got, (pr.errclass_download() if name == "errclass" else pr.matchkind_download())


def cut(pr, name, what):
    return getattr(pr, f"{name}_{what}")


def random_words(v, n_strata, seed, ones=(), zeros=()):
    """membership words [n_words, n_var] per slot: random bits, strata `ones` hold every variant, strata `zeros` none; the bits
    above n_strata of the last word are set (a kernel that counted them would show)"""
    rng = np.random.RandomState(seed)
    nw = (n_strata + 63) // 64
    out = []
    for s in range(4):
        w = rng.randint(0, 2 ** 62, (nw, v.n_vars(s))).astype(np.uint64) ^ (rng.randint(0, 4, (nw, v.n_vars(s))).astype(np.uint64) << np.uint64(62))
        for k in ones:
            w[k >> 6] |= np.uint64(1) << np.uint64(k & 63)
        for k in zeros:
            w[k >> 6] &= ~(np.uint64(1) << np.uint64(k & 63))
        if n_strata & 63:
            w[-1] |= ~np.uint64((1 << (n_strata & 63)) - 1)
        out.append(w)
    return out


def evaluated(v, sv_threshold=50):
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32))
    return dict(v=v, pr=pr, res=res, pb=pb, cls=var_classes(v, sv_threshold))


# ---- 1. the hand batches

@pytest.mark.parametrize("name", PASSES)
def test_hand_batch_equals_the_model(name):
    P = LM.PASSES[name]
    v, _ = (EC if name == "errclass" else MC).hand_case()
    e = evaluated(v)
    pr, res, pb, cls = e["pr"], e["res"], e["pb"], e["cls"]
    plain, b = label(pr, name, v, cls, pb)
    assert plain.any()
    words = random_words(v, 5, 3, ones=(0,), zeros=(1,))
    pr.upload_strata_masks(5, words)
    got = cut(pr, name, "strata")()
    assert got.shape == (5,) + plain.shape
    assert np.array_equal(got, LM.strata_counts(P, v, res, pb, b, cls, words, 5))           # the literal statement
    assert np.array_equal(got[0], plain) and not got[1].any() and got[2].any() and not np.array_equal(got[2], plain)
    keys = A.boot_keys(0, np.arange(v.n_sc))
    for stratum in (-1, 2):
        member = None if stratum < 0 else LM.member_of(words, stratum)
        rep = cut(pr, name, "boot")(keys, 3, seed=5, stratum=stratum)
        assert np.array_equal(rep, LM.boot_counts(P, v, res, pb, b, cls, keys, 5, 3, member=member)) and rep.any()
    ms = cut(pr, name, "cut_timing")()
    assert ms[0] > 0 and ms[1] > 0
    # the cut uses the phasing the bytes were made under, whatever a later counters call passes
    other = 1 - np.asarray(pb)
    S.pr_counts(pr, None, other)
    assert np.array_equal(cut(pr, name, "strata")(), got)


# ---- 2. the random shapes: 70 strata, the three threshold ranges, the replicate groups

@pytest.fixture(scope="module", params=PASSES)
def rand(request):
    name = request.param
    v = (EC if name == "errclass" else MC).random_variants()
    assert [v.n_vars(s) for s in range(4)] == [513, 257, 640, 300]                          # straddle the 256-lane blocks
    e = evaluated(v, 6)
    words = random_words(v, 70, 17, ones=(5, 66), zeros=(6, 69))                            # two words, a partial last chunk
    e.update(name=name, P=LM.PASSES[name], words=words, fast={})
    e["pr"].upload_strata_masks(70, words)
    return e


def labelled(e, mn, mx):
    """the label call at a range, and the model's table of it (once per range)"""
    plain, b = label(e["pr"], e["name"], e["v"], e["cls"], e["pb"], mn, mx)
    if (mn, mx) not in e["fast"]:
        e["fast"][(mn, mx)] = LM.fast(e["P"], e["v"], e["res"], e["pb"], b, e["cls"], mn, mx)
        assert np.array_equal(e["fast"][(mn, mx)].total(), plain)
    return plain, e["fast"][(mn, mx)]


@pytest.mark.parametrize("mn,mx", [(0, 0), (0, 60), (0, 300), (0, 500)])
def test_random_shapes_strata(rand, mn, mx):
    pr, name, P = rand["pr"], rand["name"], rand["P"]
    plain, F = labelled(rand, mn, mx)
    got = cut(pr, name, "strata")(mn, mx)
    info = cut(pr, name, "cut_info")()
    nq = mx - mn + 1
    per = 3 * P.labels * (nq + 1) * 4                                                       # LDS bytes of a stratum's bins
    want_chunk = max(c for c in (1, 2, 4, 8, 16, 32, 64) if c == 1 or c * per <= 40 * 1024)
    assert info["chunk"] == want_chunk and info["chunks"] == -(-70 // want_chunk) and info["lds"] == min(want_chunk, 70) * per
    if (mn, mx) == (0, 60):
        assert info["chunk"] == (4 if name == "errclass" else 8)
    if (mx == 300 and name == "errclass") or mx == 500:
        assert info["chunk"] == 1 and info["chunks"] == 70                                  # one stratum per workgroup
    assert np.array_equal(got, F.strata_counts(rand["words"], 70))
    assert np.array_equal(got[5], plain) and np.array_equal(got[66], plain) and not got[6].any() and not got[69].any()
    strat = S.pr_counts_strata(pr, None, rand["pb"], mn, mx)                                # the class sums
    for cs in range(2):
        assert np.array_equal(got[:, cs].sum(2), strat[:, cs, :, P.sums[cs]]), cs
    assert strat[:, 0, 3, P.sums[0]].any() and len({tuple(x.ravel()) for x in got}) > 60


@pytest.mark.parametrize("n_rep", [1, 64, 65, 130])
def test_random_shapes_replicates(rand, n_rep):
    pr, name, P, v = rand["pr"], rand["name"], rand["P"], rand["v"]
    plain, F = labelled(rand, 0, 60)
    keys = A.boot_keys(3, np.arange(v.n_sc))
    for stratum in (-1, 3, 67):                                                             # the first and the second word
        member = None if stratum < 0 else LM.member_of(rand["words"], stratum)
        got = cut(pr, name, "boot")(keys, n_rep, seed=9, stratum=stratum)
        info = cut(pr, name, "cut_info")()
        assert info["groups"] == (n_rep + 63) // 64 and info["slices"] == (3 if name == "errclass" else 2) and info["spans"] >= 1
        assert got.shape == (n_rep,) + plain.shape and np.array_equal(got, F.boot_counts(keys, 9, n_rep, member)), stratum
        boot = S.pr_counts_boot(pr, None, rand["pb"], keys, n_rep, 9, 0, 60, stratum)       # the label sums, per replicate
        for cs in range(2):
            assert np.array_equal(got[:, cs].sum(2), boot[:, cs, :, P.sums[cs]]), (stratum, cs)
        assert got.any() and (n_rep == 1 or len({tuple(x.ravel()) for x in got}) > 1)
    if n_rep == 65:                                                                         # a range of one slice, and a min_qual above 0
        plain2, F2 = labelled(rand, 15, 30)
        assert np.array_equal(cut(pr, name, "boot")(keys, n_rep, 9, 15, 30), F2.boot_counts(keys, 9, n_rep))
        assert cut(pr, name, "cut_info")()["slices"] == 1


@pytest.mark.parametrize("name", PASSES)
def test_permuted_batch_gives_the_same_replicates(name):
    """the superclusters in another order, the keys permuted with them: every replicate's counts are the same"""
    v = (EC if name == "errclass" else MC).random_variants()
    order = np.random.RandomState(8).permutation(v.n_sc)
    keys = A.boot_keys(1, np.arange(v.n_sc))
    out, pb = [], None
    for vv, kk in ((v, keys), (shard.subset_variants(v, order), keys[order])):
        e = evaluated(vv, 6)
        pb = e["pb"] if pb is None else pb[order]                                           # (the phasing goes with its supercluster)
        label(e["pr"], name, vv, e["cls"], pb)
        out.append(cut(e["pr"], name, "boot")(kk, 70, seed=2))
    assert np.array_equal(out[0], out[1]) and out[0].any()


# ---- 3. the synthetic batch: the fourteen variant strata, repeated calls, the all-reduce entries

def test_synth_batch_repeats_and_allreduce():
    from vcfdist_amd import rccl
    syn = api.Synth(n_sc=3000, len_a=10, len_b=300, len_max=300, seed=19, var_per_base=0.03, p_hom=0.4)
    v = syn.variants()
    e = evaluated(v, 6)
    pr, pb, cls = e["pr"], e["pb"], e["cls"]
    names, spec = api.varstrata_default()
    assert len(names) == 14
    pr.varstrata_masks(v, spec)
    keys = A.boot_keys(0, np.arange(v.n_sc))
    strat, boot = S.pr_counts_strata(pr, cls, pb), S.pr_counts_boot(pr, None, pb, keys, 100, 4)
    comm = None
    if rccl.available():
        torch.cuda.set_device(0)
        comm = rccl.Comm(1, 0, rccl.unique_id())
    try:
        for name in PASSES:
            P = LM.PASSES[name]
            plain, _ = label(pr, name, v, None, pb)
            a, b = cut(pr, name, "strata")(), cut(pr, name, "boot")(keys, 100, seed=4)
            assert a.shape[0] == 14 and a.any() and b.any()
            assert np.array_equal(a, cut(pr, name, "strata")()) and np.array_equal(b, cut(pr, name, "boot")(keys, 100, seed=4))
            for cs in range(2):
                assert np.array_equal(a[:, cs].sum(2), strat[:, cs, :, P.sums[cs]]) and np.array_equal(b[:, cs].sum(2), boot[:, cs, :, P.sums[cs]])
            assert (a <= plain[None]).all()
            if comm is not None:
                assert np.array_equal(cut(pr, name, "strata")(comm=comm._c), a)
                assert np.array_equal(cut(pr, name, "boot")(keys, 100, seed=4, comm=comm._c), b)
    finally:
        if comm is not None:
            comm.destroy()
    if comm is None:
        pytest.skip("no RCCL library in this process: the all-reduce entries were not compared")


# ---- 4. state and arguments

@pytest.mark.parametrize("name", PASSES)
def test_state_and_arguments(name):
    v, _ = EC.hand_case()
    cls = var_classes(v)
    pr = api.PrecisionRecall()
    keys = A.boot_keys(0, np.arange(v.n_sc))
    strata, boot = cut(pr, name, "strata"), cut(pr, name, "boot")

    def refused(code, entry, call, *a, **kw):
        with pytest.raises(api.VprError) as e:
            call(*a, **kw)
        assert f"({code})" in str(e.value) and f"vpr_{name}_{entry}" in str(e.value), str(e.value)
        return str(e.value)
    batch = api.batch_from_variants(v)
    pr.upload(batch)
    assert "before vpr_execute" in refused(-4, "strata", strata)
    assert "before vpr_execute" in refused(-4, "boot", boot, keys, 4)
    pr.execute()
    res = pr.download()
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32))
    words = random_words(v, 5, 1)
    pr.upload_strata_masks(5, words)
    # before the label call of THIS pass (the other pass's bytes do not count)
    other = "matchkind" if name == "errclass" else "errclass"
    label(pr, other, v, cls, pb)
    assert f"before vpr_{name}" in refused(-4, "strata", strata)
    assert f"before vpr_{name}" in refused(-4, "boot", boot, keys, 4)
    _, b = label(pr, name, v, None, pb)
    P = LM.PASSES[name]
    good = strata()
    assert np.array_equal(good, LM.strata_counts(P, v, res, pb, b, cls, words, 5))
    # arguments
    assert "max_qual 10 is below min_qual 20" in refused(-1, "strata", strata, 20, 10)
    assert "max_qual 10 is below min_qual 20" in refused(-1, "boot", boot, keys, 4, 1, 20, 10)
    cap = 779 if name == "errclass" else 1364
    assert f"more than {cap} thresholds" in refused(-1, "strata", strata, 0, cap)
    assert f"more than {cap} thresholds" in refused(-1, "boot", boot, keys, 4, 1, 0, cap)
    for n_rep in (0, -1, A.BOOT_MAX_REPLICATES + 1):
        assert "replicates" in refused(-1, "boot", boot, keys, n_rep)
    assert "stratum 5 of 5" in refused(-1, "boot", boot, keys, 4, stratum=5)
    refused(-1, "boot", boot, keys, 4, stratum=-2)
    assert "null" in refused(-1, "boot", boot, None, 4)
    L, h = api.lib(), pr._h
    assert getattr(L, f"vpr_{name}_strata")(h, 0, 60, None) == -1 and f"vpr_{name}_strata: null" in L.vpr_last_error(h).decode()
    assert getattr(L, f"vpr_{name}_boot")(h, 0, 60, keys.ctypes.data_as(api.C.POINTER(api.C.c_uint64)), 1, 4, -1, None) == -1
    assert getattr(L, f"vpr_allreduce_{name}_strata")(h, None, 0, 60, None) == -1
    assert getattr(L, f"vpr_{name}_cut_timing")(h, None, None) == -1
    # words of another batch: the per-slot counts differ
    nv = [v.n_vars(s) for s in range(4)]
    pr.upload_strata_masks(5, [np.zeros((1, n + 1), np.uint64) for n in nv])
    assert "membership words hold" in refused(-4, "strata", strata)
    assert "membership words hold" in refused(-4, "boot", boot, keys, 4, stratum=0)
    assert boot(keys, 4).any()                                                              # (without a stratum no words are needed)
    pr.upload_strata_masks(5, words)
    assert np.array_equal(strata(), good)                                                   # after the refusals the handle is right
    # a fresh upload: the bytes go, and the words with them
    pr.upload(batch)
    pr.execute()
    assert f"before vpr_{name}" in refused(-4, "strata", strata)
    label(pr, name, v, cls, pb)
    assert "no membership words" in refused(-4, "strata", strata)
    assert "no membership words" in refused(-4, "boot", boot, keys, 4, stratum=0)


# ---- 5. the command lines

def cut_files(stem):
    return (f"stratified-{stem}.tsv", f"stratified-{stem}-summary.tsv", f"bootstrap-{stem}-summary.tsv")


ALL_CUT_FILES = cut_files("error-classes") + cut_files("match-kinds")


@pytest.fixture(scope="module")
def demo():
    """the demo callsets through the CPU oracle chain (tests/demo_pipeline.py) and the model's text of the six files for the strata
    `whole` (a BED over every variant) and the fourteen variant strata, and 16 replicates of seed 1"""
    import demo_pipeline as D
    import strata_model as SM
    import varstrata_model as VM
    rows, det = D.run(product=False)
    v, cls = EC.demo_variants(det)
    res, pb, mn, mx = det["res"], det["pb"], D.G["min_qual"], D.G["max_qual"]
    names, specs = api.varstrata_default()
    bits = VM.members(v, specs)
    members = [[np.ones(v.n_vars(s), bool) for s in range(4)]] + [[np.asarray(bits[s][k], bool) for s in range(4)] for k in range(len(names))]
    words = []
    for s in range(4):
        w = np.zeros((1, v.n_vars(s)), np.uint64)
        for k, m in enumerate(members):
            w[0] |= m[s].astype(np.uint64) << np.uint64(k)
        words.append(w)
    pr_strata = np.stack([SM.expected_counts(det["batch"].var_off, res, cls, pb, m, mn, mx) for m in members])
    keys = A.boot_keys(0, np.arange(v.n_sc))
    files, points = {}, {}
    for P, b in ((LM.ERRCLASS, EM.classes(v, res, pb, 50)), (LM.MATCHKIND, MM.kinds(v, res, pb))):
        F = LM.fast(P, v, res, pb, b, cls, mn, mx)
        point = F.total()
        assert np.array_equal(point, P.counts(v, res, pb, b, cls, mn, mx))
        a, s = LM.stratified_text(P, ["whole"] + names, F.strata_counts(words, len(members)), pr_strata, mn, mx)
        files.update(zip(cut_files(P.stem), (a, s, LM.bootstrap_text(P, point, det["counts"], F.boot_counts(keys, 1, 16), mn, mx))))
        points[P.name] = point
    return dict(names=["whole"] + names, files=files, points=points)


def test_command_lines_on_demo_files(demo, tmp_path):
    import demo_pipeline as D
    import strata_model as SM
    assert demo["points"]["errclass"][0, 3, :, 0].sum() > 0 and demo["points"]["matchkind"][1, 3, :, 0].sum() > 0
    fa = _write_fasta(tmp_path / "surrogate.fa", D.surrogate_fasta(5_100_000), ("chr1",))
    beds = SM.write_strata(tmp_path, [("whole", [("chr1", 0, 5_000_000)])], "beds.tsv")
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    others = ["--classify-errors", "--classify-matches", "--stratify", beds, "--stratify-context", "--stratify-variants", "--bootstrap", "16"]
    runs = {}
    for name, cmd, extra in (("c-all", cli, others), ("c-cut", cli, others + ["--cut-classes"]), ("py-cut", py, ["--cut-classes"] + others),
                             ("c-n", cli, others + ["--cut-classes", "-n"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(["timeout", "-k", "10", "600"] + cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=660)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    ctx_names = api.context_default()[0]
    for f in ALL_CUT_FILES:
        # byte-identical from both drivers
        assert rd(runs["c-cut"][0] + f) == rd(runs["py-cut"][0] + f) and len(rd(runs["c-cut"][0] + f)) > 300, f
        lines = open(runs["c-cut"][0] + f).read().split("\n")
        if f.startswith("bootstrap-"):
            assert "\n".join(lines) == demo["files"][f], f                                  # the model's text on the oracle chain
            continue
        order = [l.split("\t", 1)[0] for l in lines[1:-1]]
        assert [n for i, n in enumerate(order) if i == 0 or order[i - 1] != n] == ["whole"] + ctx_names + demo["names"][1:], f
        assert [l for l in lines[:-1] if l.split("\t", 1)[0] in ["STRATUM"] + demo["names"]] == demo["files"][f].split("\n")[:-1], f
        # the stratum that holds every variant, without its STRATUM column, is the unstratified table byte for byte
        whole = "".join(l.split("\t", 1)[1] + "\n" for l in lines[:-1] if l.startswith(("STRATUM\t", "whole\t")))
        assert whole.encode() == rd(runs["c-cut"][0] + f.replace("stratified-", "")), f
    # without the option: the file set and every byte of every file are what they are beside all the other options
    without = sorted(os.listdir(runs["c-all"][0]))
    assert not set(ALL_CUT_FILES) & set(without) and len(without) > 20
    for name in ("c-cut", "py-cut"):
        assert sorted(set(os.listdir(runs[name][0])) - set(ALL_CUT_FILES)) == without, name
        for f in without:
            assert _without_command(runs["c-all"][0] + f) == _without_command(runs[name][0] + f), (name, f)
    assert runs["c-all"][1] == runs["c-cut"][1] == runs["py-cut"][1] == runs["c-n"][1]
    assert " cut: " not in runs["c-all"][2]
    drop = lambda err: [l for l in err.split("\n") if " cut: " not in l and " ms " not in l]
    assert drop(runs["c-all"][2]) == drop(runs["c-cut"][2])
    # stderr: one more line per pass with the strata, the replicates and the device time
    n_strata = 1 + len(ctx_names) + 14
    for name in ("c-cut", "py-cut", "c-n"):
        for noun in ("error classes", "match kinds"):
            m = re.findall(rf"{noun} cut: (\d+) strata, (\d+) replicates, ([0-9.]+) ms on the device", runs[name][2])
            assert len(m) == 1 and (int(m[0][0]), int(m[0][1])) == (n_strata, 16) and float(m[0][2]) > 0, runs[name][2][-800:]
    assert os.listdir(runs["c-n"][0]) == []                                                 # -n: no file appears


@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    """the demo callsets twice, as chr1 and chr2, and the one-rank run with both passes cut and resampled"""
    return two_contig_run(tmp_path_factory.mktemp("labelcut_two"),
                          ["--classify-errors", "--classify-matches", "--stratify-variants", "--bootstrap", "8", "--cut-classes"])


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
    for name in ALL_CUT_FILES + ("error-classes.tsv", "match-kinds-summary.tsv", "stratified-precision-recall-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 300, name
    # both contigs hold the demo: hom and het partition the variants, so their classes add up to the unstratified table's
    text = [l.split("\t") for l in (out / "stratified-error-classes-summary.tsv").read_text().split("\n")[1:-1]]
    row = lambda s: [int(x) for x in next(l for l in text if l[:3] == [s, "ALL", "NONE"])[4:]]
    plain = [l.split("\t") for l in (out / "error-classes-summary.tsv").read_text().split("\n")[1:-1]]
    total = [int(x) for x in next(l for l in plain if l[:2] == ["ALL", "NONE"])[3:]]
    assert [a + b for a, b in zip(row("hom"), row("het"))] == total and total[0] > 0 and total[0] % 2 == 0
