"""The HIP paths pinned on the reference's own compiled functions, from the fixtures under tests/golden/ref/ alone (no oracle, no
model and no reference binary in the comparison; tests/ref_pins.py and tests/golden/README.md describe the fixtures):

  vpr_execute (Level A upload and vpr_upload_variants' device generate)  == precision_recall_threads_wrapper: sc_phase, both phase
                                                                            distances, the six per-variant columns bit for bit
  vpr_distance (one round, and many with a small round_bytes)            == edits_wrapper's editData records, order included
  vrl_realign                                                            == wf_swg_realign + left_shift, every column
  wfa_cluster.hip                                                        == wf_swg_cluster's cluster starts and reaches"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_pins as R  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_LIMIT = 128          # VPR_ST_ERR_LIMIT

CHAIN = [n for n in R.fixture_names("chain_") + R.fixture_names("demo_") if R.Fixture(n).refused is None]
REALIGN = R.fixture_names("realign_")
BIWFA = [n for n in CHAIN + [n for n in R.fixture_names("cluster_") if not n.endswith("_refused")] if R.case_args(R.Fixture(n).case)["cluster"][0] == "biwfa" and not n.endswith("_d")]
# _limit_batch's run of k directly adjacent one-base deletion records (it starts at position 200).  A position keeps up to eight
# allowed swap sources (pr_device.h); behind a run of k records there are k + 1, so k = 7 is the most the library evaluates and
# k = 8, 9, 12 come back with VPR_ST_ERR_LIMIT: that refusal is what is asserted here, the fixture's answer for those superclusters
# is asserted on the oracle only (tests/test_ref_pins.py).  The reference itself has no such bound.
LIMITED = ("chain_limit8", "chain_limit9", "chain_limit12")
TWIN = {n: n + "_d" for n in R.fixture_names("demo_") if not n.endswith("_d")}          # the same case recorded without -d


def _compare(name, res, want, v, skip_sc=()):
    keep_sc = np.ones(v.n_sc, bool)
    keep_sc[list(skip_sc)] = False
    for f, key in (("sc_phase", "sc_phase"), ("orig_phase_dist", "orig"), ("swap_phase_dist", "swap")):
        got = np.asarray(getattr(res, f)).astype(np.int64)
        assert np.array_equal(got[keep_sc], want[key][keep_sc]), (name, f, np.flatnonzero(got != want[key])[:8])
    got = R.results_per_variant(res)
    for key, w in want["cols"].items():
        k = key[1]
        keep = np.ones(len(w), bool)
        for sc in skip_sc:
            keep[int(v.var_off[k][sc]):int(v.var_off[k][sc + 1])] = False
        bad = np.flatnonzero((got[key] != w) & keep)
        assert len(bad) == 0, f"{name}: {key[0]} of slot {k}, phasing {key[2]}: {len(bad)} differ, first at variant {bad[0]}: {got[key][bad[0]]} vs reference {w[bad[0]]}"


def _records(got):
    if not len(got["edit_sc"]):
        return np.zeros((0, 7), np.int64)
    return np.stack([got["edit_sc"], got["edit_hap"], got["edit_pos"], got["edit_type"], got["edit_len"], got["edit_min_qual"],
                     got["edit_max_qual"]], 1).astype(np.int64)


@pytest.mark.parametrize("name", CHAIN)
def test_precision_recall_and_distance_equal_the_reference(name):
    from vcfdist_amd import api
    fx = R.Fixture(name)
    o = R.case_args(fx.case)
    if name in TWIN:         # without -d the reference answers what it answers with -d, less the edit records: nothing more to run
        twin = R.Fixture(TWIN[name])
        assert sorted(fx.out) == sorted(k for k in twin.out if not k.startswith("ed_"))
        assert all(np.array_equal(fx.out[k], twin.out[k]) for k in fx.out)
        return
    v, want = R.ref_batch(fx)
    if v is None:
        assert "no_variants" in name
        return
    skip = [sc for sc in range(v.n_sc) if v.sc_beg[sc] <= 200 <= v.sc_end[sc]] if name in LIMITED else []
    assert len(skip) == (1 if name in LIMITED else 0)
    batch = api.batch_from_variants(v)
    pr = api.PrecisionRecall()
    res = pr.run(batch)
    st = np.asarray(res.aln_status).reshape(-1, 4) & np.uint32(ERR_LIMIT)
    assert np.flatnonzero(st.any(1)).tolist() == skip, (name, "superclusters refused with VPR_ST_ERR_LIMIT")
    _compare(name, res, want, v, skip)
    if o["distance"]:
        pen = dict(eval_sub=o["eval_sub"], eval_open=o["eval_open"], eval_extend=o["eval_extend"], max_qual=o["max_qual"])
        w = want["edits"][~np.isin(want["edits"][:, 0], skip)]
        for kw in (dict(), dict(round_bytes=1 << 16)):
            got = pr.distance(v, **pen, **kw)
            assert got["info"].n_error == 0 and (got["job_status"] == 0).all()
            g = _records(got)
            assert g.shape == w.shape, (name, kw, g.shape, w.shape)
            bad = np.flatnonzero((g != w).any(1))
            assert len(bad) == 0, f"{name} {kw}: edit record {bad[0]}: {g[bad[0]]} vs reference {w[bad[0]]}"
    # the same through vpr_upload_variants: generate_ptrs_strs on the device
    vs = v.as_struct()
    pr2 = api.PrecisionRecall()
    pr2.upload_variants(vs, batch)
    pr2.execute()
    _compare(name + " (device generate)", pr2.download(), want, v, skip)


def test_small_round_bytes_really_takes_many_rounds():
    from vcfdist_amd import api
    fx = R.Fixture("chain_joint61")
    v, want = R.ref_batch(fx)
    pr = api.PrecisionRecall()
    pr.run(api.batch_from_variants(v))
    assert pr.distance(v, round_bytes=1 << 16)["info"].n_rounds > 1


@pytest.mark.parametrize("name", REALIGN)
def test_realign_equals_the_reference(name):
    from vcfdist_amd import api, cluster as K
    import realign_model as RM
    fx = R.Fixture(name)
    o = R.case_args(fx.case)
    if fx.refused is not None:
        # the reference exits on a cluster whose region starts in front of the contig; vrl_realign keeps it and says so
        assert name == "realign_hand_pos0"
        s, _, _ = R.case_slot(fx.case, 0, 0)
        hap = R.hap_columns(s)
        cl = K.simple_cluster(K.Hap(hap["pos"], hap["rlen"], hap["type"], hap["ref_len"], hap["alt_len"]), 0, 50, 10)
        cols, status, info = api.realign(hap, cl, R.case_contigs(fx.case)[0][1])
        assert status.tolist() == [RM.ST_EDGE] and cols["pos"].tolist() == s["pos"].tolist()
        return
    n_rec = 0
    for ctg, (cname, seq) in enumerate(R.case_contigs(fx.case)):
        s, a, b = R.case_slot(fx.case, 0, ctg)
        if b == a:
            continue
        cl = R.ref_cluster_objects(fx, ctg)[0]
        cols, status, info = api.realign(R.hap_columns(s), cl, seq, sub=o["sub"], open=o["open"], extend=o["extend"], max_qual=o["max_qual"])
        assert not status.any(), (name, ctg, np.flatnonzero(status)[:8])
        ra, rb = int(fx.out["r0_off"][ctg]), int(fx.out["r0_off"][ctg + 1])
        assert len(cols["pos"]) == rb - ra, (name, ctg)
        for f in ("pos", "rlen", "type", "phase_set", "orig_gt", "ref_len", "alt_len"):
            assert np.array_equal(cols[f].astype(np.int64), fx.out["r0_" + f][ra:rb]), (name, ctg, f)
        for f in ("var_qual", "gt_qual"):
            assert np.array_equal(cols[f].view(np.uint32).astype(np.int64), fx.out["r0_" + f][ra:rb]), (name, ctg, f)
        ro = np.concatenate([[0], np.cumsum(fx.out["r0_ref_len"])])
        ao = np.concatenate([[0], np.cumsum(fx.out["r0_alt_len"])])
        pool = bytes(cols["pool"])
        got_ref = b"".join(pool[int(p):int(p) + int(n)] for p, n in zip(cols["ref_off"], cols["ref_len"]))
        got_alt = b"".join(pool[int(p):int(p) + int(n)] for p, n in zip(cols["alt_off"], cols["alt_len"]))
        assert got_ref == bytes(fx.out["r0_refs"][ro[ra]:ro[rb]].astype(np.uint8)), (name, ctg, "ref alleles")
        assert got_alt == bytes(fx.out["r0_alts"][ao[ra]:ao[rb]].astype(np.uint8)), (name, ctg, "alt alleles")
        n_rec += rb - ra
    assert n_rec > 0


@pytest.mark.parametrize("name", BIWFA)
def test_wfa_cluster_kernel_equals_the_reference(name):
    from vcfdist_amd import cluster as K
    fx = R.Fixture(name)
    o = R.case_args(fx.case)
    n = 0
    for ctg, (cname, seq) in enumerate(R.case_contigs(fx.case)):
        for k in range(4):
            s, a, b = R.case_slot(fx.case, k, ctg)
            if a == b:
                continue
            got = K.wfa_cluster(K.HapSeq(s["pos"], s["type"], s["ref"], s["alt"]), bytes(seq), sub=o["sub"], open=o["open"], extend=o["extend"],
                                max_cluster_itrs=o["max_cluster_itrs"], reach_min_gap=10)[0]
            st, le, ri = (x.tolist() for x in R.ref_clusters(fx.out, k, ctg))
            nc = len(st) - 1
            assert got.var_beg.tolist() == st, (name, ctg, k)
            assert got.left_reach.tolist()[:nc] == le[:nc] and got.right_reach.tolist()[:nc] == ri[:nc], (name, ctg, k)
            n += nc
    assert n > 0
