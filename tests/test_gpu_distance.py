"""The distance mode (-d) on the GPU: vpr_distance's jobs, per-quality totals and every edit record against the CPU model
(tests/distance_model.cpp), on seeded synthetic batches, with the round budget forced small, over two executes, and through
both command lines on the demo files."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import distance_helpers as DH  # noqa: E402

pytestmark = pytest.mark.gpu
ERR = 32 | 64 | 128      # VPR_ST_ERR_NO_PTR | _UNFINISHED | _LIMIT


def _expected(v, res, max_qual=60, **pen):
    skip = np.zeros(v.n_sc, np.uint8)
    bad = np.nonzero(res.aln_status & np.uint32(ERR))[0] // 4
    skip[bad] = 1
    jobs, recs = DH.run(v, res.sc_phase, skip, max_qual=max_qual, **pen)
    qd = np.zeros(max_qual + 2, np.int64)
    for sc, hap, lo, hi, d in jobs:
        qd[max(lo, 0):min(hi, max_qual + 2)] += d
    return jobs, recs, qd, skip


def _check(got, jobs, recs, qd):
    assert got["info"].n_limit == 0 and got["info"].n_error == 0
    assert (got["job_status"] == 0).all()
    g_jobs = np.stack([got["job_sc"], got["job_hap"].astype(np.int32), got["job_min_qual"], got["job_max_qual"], got["job_dist"]], 1)
    assert g_jobs.shape == jobs.shape and (g_jobs == jobs).all(), "jobs / distances differ from the model"
    g_recs = np.stack([got["edit_sc"], got["edit_hap"].astype(np.int32), got["edit_pos"], got["edit_type"].astype(np.int32), got["edit_len"],
                       got["edit_min_qual"], got["edit_max_qual"]], 1) if len(got["edit_sc"]) else np.zeros((0, 7), np.int32)
    assert g_recs.shape == recs.shape, (g_recs.shape, recs.shape)
    if len(recs):
        diff = np.nonzero((g_recs != recs).any(1))[0]
        assert len(diff) == 0, f"record {diff[0]}: {g_recs[diff[0]]} vs model {recs[diff[0]]}"
    assert (got["qual_dists"] == qd).all()


def _run(syn, level_b=False, **kw):
    from vcfdist_amd import api
    pr = api.PrecisionRecall()
    if level_b:
        batch = syn.batch()
        pr.upload_variants(syn.struct, batch)
        pr.execute()
        res = pr.download()
    else:
        res = pr.run(syn.batch())
    return pr, res, pr.distance(syn.variants(), **kw)


def _synth(**p):
    from vcfdist_amd import api
    return api.Synth(**p)


@pytest.mark.parametrize("which", ["PARAMS", "PARAMS_JOINT"])
def test_regression_batches_equal_the_model(which):
    import make_regression as MR
    syn = _synth(**getattr(MR, which))
    pr, res, got = _run(syn)
    jobs, recs, qd, _ = _expected(syn.variants(), res)
    assert len(jobs) > 2 * syn.params.n_sc - 1
    _check(got, jobs, recs, qd)


def test_wgs_slice_level_b_upload_and_other_penalties():
    syn = _synth(n_sc=3000, seed=3, len_mode=1, len_a=20.0, len_b=1.2, len_min=4, len_max=10000)
    pr, res, got = _run(syn, level_b=True)
    jobs, recs, qd, _ = _expected(syn.variants(), res)
    _check(got, jobs, recs, qd)
    got = pr.distance(syn.variants(), eval_sub=4, eval_open=3, eval_extend=2, max_qual=40)
    jobs, recs, qd, _ = _expected(syn.variants(), res, max_qual=40, x=4, o=3, e=2)
    _check(got, jobs, recs, qd)


JOINT = dict(n_sc=300, seed=11, len_mode=1, len_a=20.0, len_b=1.2, len_min=4, len_max=10002, p_sv=0.1, sv_min=50, sv_max=3000)


# JOINT with 500 superclusters: the CPU model gives 1 249 edit records with every supercluster in its original phasing, 1 475 with every
# one swapped, and 1 249 as the sum of the per-supercluster minima -- above the record buffer's first 1 024 whatever the phasing
JOINT_EDITS = dict(JOINT, n_sc=500)


def test_joint_batch_with_sv_indels_and_small_rounds():
    syn = _synth(**JOINT_EDITS)
    pr, res, got = _run(syn)
    v = syn.variants()
    assert max(int(np.max(v.var_ref_len[s], initial=0)) for s in range(4)) >= 50      # SV-sized indels are there
    jobs, recs, qd, _ = _expected(v, res)
    _check(got, jobs, recs, qd)
    assert got["info"].n_rounds == 1
    small = pr.distance(v, round_bytes=1 << 16)
    assert small["info"].n_rounds > 1 and small["info"].n_hist_rounds > small["info"].n_rounds
    _check(small, jobs, recs, qd)
    # a handle whose record buffer starts empty: it grows between sub-rounds and has to keep what it holds
    _, _, fresh = _run(syn, round_bytes=1 << 16)
    assert fresh["info"].n_edits > 1024 and fresh["info"].n_hist_rounds >= 2
    _check(fresh, jobs, recs, qd)


def test_two_executes_give_identical_output():
    syn = _synth(**JOINT)
    from vcfdist_amd import api
    pr = api.PrecisionRecall()
    batch = syn.batch()
    outs = []
    for _ in range(2):
        pr.run(batch)
        outs.append(pr.distance(syn.variants()))
    for k, a in outs[0].items():
        if k != "info":
            assert np.array_equal(a, outs[1][k]), k


def _limit_batch():
    """three superclusters; the middle one holds nine directly adjacent one-base deletion records on query hap 1 -- more allowed
    swap sources on one position than the precision/recall path keeps (eight): its alignments come back with VPR_ST_ERR_LIMIT"""
    from vcfdist_amd import _abi as A
    rng = np.random.RandomState(23)
    ref = "".join(rng.choice(list("ACGT"), 400))
    S, I, D = A.TYPE_SUB, A.TYPE_INS, A.TYPE_DEL
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    run9 = [(200 + k, D, ref[200 + k], "", 30.0) for k in range(9)]
    scs = [dict(ctg=0, beg=40, end=70, vars=[[(50, S, ref[50], other(ref[50]), 20.0)], [], [(50, S, ref[50], other(ref[50]), 40.0)],
                                             [(60, I, "", "GT", 9.0)]]),
           dict(ctg=0, beg=190, end=220, vars=[run9, [], [(200, D, ref[200:209], "", 50.0)], []]),
           dict(ctg=0, beg=300, end=340, vars=[[(310, D, ref[310:313], "", 20.0)], [(320, S, ref[320], other(ref[320]), 5.0)],
                                               [(310, D, ref[310:313], "", 40.0)], [(320, S, ref[320], other(ref[320]), 7.0)]])]
    return A.Variants.from_sites([ref], scs)


def test_superclusters_with_error_alignments_produce_no_jobs():
    from vcfdist_amd import api
    v = _limit_batch()
    pr = api.PrecisionRecall()
    res = pr.run(api.batch_from_variants(v))
    st = res.aln_status.reshape(-1, 4) & np.uint32(ERR)
    assert st[1].all() and not st[[0, 2]].any()
    got = pr.distance(v)
    assert set(got["job_sc"].tolist()) == {0, 2} and 1 not in set(got["edit_sc"].tolist())
    jobs, recs, qd, skip = _expected(v, res)
    assert skip.tolist() == [0, 1, 0]
    _check(got, jobs, recs, qd)


def test_calls_that_return_err_arg():
    import ctypes as C
    from vcfdist_amd import _abi as A, api
    syn = _synth(n_sc=20, seed=5, len_a=8, len_b=200, len_max=200)
    pr = api.PrecisionRecall()
    L = api.lib()
    cfg = A.VprDistConfig(eval_sub=3, eval_open=2, eval_extend=1, min_qual=0, max_qual=60, flags=0, round_bytes=0)
    v = syn.variants()          # (kept alive: the struct points into its arrays)
    vs = v.as_struct()
    assert L.vpr_distance(pr._h, C.byref(vs), C.byref(cfg)) == -1          # before any execute
    pr.run(syn.batch())
    ov = _synth(n_sc=21, seed=5, len_a=8, len_b=200, len_max=200).variants()
    other = ov.as_struct()
    assert L.vpr_distance(pr._h, C.byref(other), C.byref(cfg)) == -1       # n_sc differs from the executed batch
    assert L.vpr_distance(pr._h, C.byref(vs), C.byref(cfg)) == 0
    info = A.VprDistInfo()
    assert L.vpr_distance_info(pr._h, C.byref(info)) == 0 and info.n_jobs > 0
    # a later execute (or upload) retires the distance results: no earlier batch's records come back
    pr.run(syn.batch())
    r = A.VprDistResults()
    assert L.vpr_distance_info(pr._h, C.byref(info)) == -1
    assert L.vpr_distance_download(pr._h, C.byref(r)) == -1
    assert L.vpr_distance(pr._h, C.byref(vs), C.byref(cfg)) == 0 and L.vpr_distance_info(pr._h, C.byref(info)) == 0
    pr.upload(syn.batch())
    assert L.vpr_distance_download(pr._h, C.byref(r)) == -1


# ---- the command lines on the demo files

def _surrogate(tmp_path):
    import demo_pipeline as D
    fa = tmp_path / "surrogate.fa"
    seq = D.surrogate_fasta(5_100_000)
    with open(fa, "w") as fh:
        fh.write(">chr1 surrogate\n")
        s = bytes(seq).decode()
        for i in range(0, len(s), 100000):
            fh.write(s[i:i + 100000] + "\n")
    return str(fa)


def test_command_lines_on_demo_files(tmp_path):
    import demo_pipeline as D
    from vcfdist_amd import _abi as A, cluster as K
    fa = _surrogate(tmp_path)
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    runs = {}
    for name, cmd in (("c", [cli]), ("py", [sys.executable, "-m", "vcfdist_amd"])):
        for d in ("", "-d"):
            pre = str(tmp_path / f"{name}{d}") + "/"
            os.makedirs(pre)
            r = subprocess.run(cmd + inputs + ["-p", pre] + ([d] if d else []), capture_output=True, text=True, cwd=ROOT, timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            runs[name + d] = (pre, r.stdout)
    files = ("distance.tsv", "distance-summary.tsv", "edits.tsv")
    rd = lambda p: open(p, "rb").read()
    for f in files:
        assert rd(runs["c-d"][0] + f) == rd(runs["py-d"][0] + f), f
        assert not os.path.exists(runs["c"][0] + f) and not os.path.exists(runs["py"][0] + f)
    for name in ("c", "py"):
        plain = sorted(os.listdir(runs[name][0]))
        assert sorted(set(os.listdir(runs[name + "-d"][0])) - set(files)) == plain
        for f in plain:
            if f == "parameters.txt":
                continue
            a, b = rd(runs[name][0] + f), rd(runs[name + "-d"][0] + f)
            if f == "summary.vcf":      # the ##fileDate / ##CL lines differ
                a = b"\n".join(l for l in a.split(b"\n") if not l.startswith((b"##fileDate", b"##CL")))
                b = b"\n".join(l for l in b.split(b"\n") if not l.startswith((b"##fileDate", b"##CL")))
            assert a == b, f
        par = rd(runs[name + "-d"][0] + "parameters.txt").decode()
        assert "eval_sub = 3\neval_open = 2\neval_extend = 1\ndistance = true" in par
        # stdout: the ALIGNMENT DISTANCE SUMMARY in front of the unchanged PRECISION-RECALL SUMMARY
        out_d, out = runs[name + "-d"][1], runs[name][1]
        assert out_d.endswith(out) and out_d.startswith("ALIGNMENT DISTANCE SUMMARY\n")
    assert runs["c-d"][1] == runs["py-d"][1]
    # the model's writers fed with the CPU oracle chain's superclusters and phases
    rows, det = D.run(product=False)
    slots, sc, res = det["slots"], det["sc"], det["res"]
    haps = [K.HapSeq(s["pos"], s["type"], s["ref"], s["alt"]) for s in slots]
    v = A.Variants(np.array([0, len(det["fasta"])], np.int64), det["fasta"], np.zeros(sc.n, np.int32), sc.beg, sc.end,
                   [sc.var_off(i) for i in range(4)], [h.pos for h in haps], [h.type for h in haps],
                   [np.asarray(s["qual"], np.float32) for s in slots], [h.ref_off for h in haps], [h.ref_len for h in haps],
                   [h.alt_off for h in haps], [h.alt_len for h in haps], [h.pool for h in haps])
    skip = np.zeros(sc.n, np.uint8)
    skip[np.nonzero(np.asarray(res.aln_status) & np.uint32(ERR))[0] // 4] = 1
    jobs, recs = DH.run(v, np.asarray(res.sc_phase, np.int32), skip)
    mp = str(tmp_path / "model") + "/"
    os.makedirs(mp)
    text = DH.write(mp, ["chr1"] * len(recs), recs, 0, 60)
    for f in files:
        assert rd(mp + f) == rd(runs["c-d"][0] + f), f
    assert runs["c-d"][1].startswith(text + "\n")
    # -d -n: the summary, no files
    pre = str(tmp_path / "n") + "/"
    os.makedirs(pre)
    r = subprocess.run([cli] + inputs + ["-p", pre, "-d", "-n"], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith(text + "\n") and os.listdir(pre) == []
