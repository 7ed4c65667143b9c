"""The CPU restatements pinned on the reference's own compiled functions.  tests/golden/ref/ holds cases and what
oracle/_ref/ref_harness (vcfdist's translation units, compiled unmodified; oracle/Makefile, target `ref`) answered for them;
here the models and oracles that every GPU parity test trusts are compared with those answers:

  tests/distance_model.cpp (dm_steps, dm_job, dm_run)      == wf_swg_align + wf_swg_backtrack + count_dist, edits_wrapper
  oracle_lib.edit_distance                                 == wf_ed
  oracle/cluster_oracle.cpp, wfa_oracle.cpp, host cluster.cpp == simple_cluster, wf_swg_cluster, superclusterData
  oracle/pr_oracle.cpp                                     == precision_recall_threads_wrapper (sc_phase, distances, six columns)
  oracle/summary_oracle.cpp                                == phaseblockData (pb_phase, switches, flips)
  tests/realign_model.py                                   == wf_swg_realign + left_shift

Where the harness is built, every fixture is also regenerated from its inputs and must equal what is committed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import distance_helpers as DH  # noqa: E402
import oracle_lib as O  # noqa: E402
import ref_pins as R  # noqa: E402

ALL = R.fixture_names()
SWG = R.fixture_names("swg_")
ED = R.fixture_names("ed_")
CHAIN = R.fixture_names("chain_") + R.fixture_names("demo_")
REALIGN = R.fixture_names("realign_")
# (a refused cluster case, cluster_biwfa_edges_pos0_refused, is held by tests/test_wfa_cluster_cases.py)
CLUSTER = [n for n in R.fixture_names("cluster_") if not n.endswith("_refused")]


def test_the_fixture_sets_are_there():
    """every set of tests/golden/README.md: a missing directory must not turn the parametrised pins below into nothing"""
    assert len(SWG) >= 6 + 8 + 2 and len(ED) >= 4 and len(REALIGN) >= 3 + 5 and len(CLUSTER) >= 7 + 11
    assert len([n for n in CHAIN if n.startswith("chain_")]) >= 6 + 1 + 6 + 4 + 2 + 6 and len([n for n in CHAIN if n.startswith("demo_")]) == 6
    for pen in ("562", "321", "432", "111", "921", "132"):
        assert f"swg_hand_{pen}" in SWG


def test_cigar_mapping_on_the_hand_case():
    """the reference writes a diagonal move twice and a gap step once; "ACAC" / "CCCAACA" at 3/2/1 (the hand case of
    tests/test_distance_model.py): score 12, distance 6, CIGAR 4 4 4 4 1 2 2 2 2 8 8 in forward order"""
    fx = R.Fixture("swg_hand_321")
    k = R.case_pairs(fx.case).index((b"ACAC", b"CCCAACA"))
    cig = fx.out["cigar"][fx.out["cigar_off"][k]:fx.out["cigar_off"][k + 1]].tolist()
    assert cig == [4, 4, 4, 4, 1, 2, 2, 2, 2, 8, 8] and fx.out["score"][k] == 12 and fx.out["dist"][k] == 6
    assert R.steps_from_cigar(cig) == [R.F_MAT, R.F_MAT, R.F_INS] + [R.F_DEL] * 4 + [R.F_SUB]
    with pytest.raises(AssertionError):
        R.steps_from_cigar([4, 4, 4, 1])


@pytest.mark.parametrize("name", SWG)
def test_distance_model_equals_the_reference_alignment(name):
    """dm_steps == wf_swg_backtrack's CIGAR step for step, dm_job's distance == count_dist, on every pair"""
    fx = R.Fixture(name)
    assert fx.refused is None, fx.refused
    x, o, e = (int(v) for v in fx.case["pen"])
    pairs = R.case_pairs(fx.case)
    assert len(pairs) == len(fx.out["score"]) > 0
    for k, (q, t) in enumerate(pairs):
        want = R.steps_from_cigar(fx.out["cigar"][fx.out["cigar_off"][k]:fx.out["cigar_off"][k + 1]])
        got = DH.steps(q.decode(), t.decode(), x, o, e)
        if got != want:
            first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            raise AssertionError(f"pair {k} (|q| {len(q)}, |t| {len(t)}, {x}/{o}/{e}): step {first}: model {got[first:first + 6]} reference {want[first:first + 6]}")
        if len(q) + len(t) < 4000:
            d, rec = DH.job(q.decode(), t.decode(), x, o, e, beg=11)
            assert d == fx.out["dist"][k] == sum(s != R.F_MAT for s in want), k
    # the model's score is not exported.  The reference's is at least the cost of its own CIGAR (gap runs o + n e, substitutions
    # x): a cell that carries several flags lets the backtrack walk a mismatch as a match (test_ored_ins_flag... of
    # tests/test_distance_model.py), so the CIGAR can cost less than the score, never more
    for k in range(len(pairs)):
        st = R.steps_from_cigar(fx.out["cigar"][fx.out["cigar_off"][k]:fx.out["cigar_off"][k + 1]])
        cost = sum(x for s in st if s == R.F_SUB) + sum(e for s in st if s in (R.F_INS, R.F_DEL)) + \
            sum(o for i, s in enumerate(st) if s in (R.F_INS, R.F_DEL) and (i == 0 or st[i - 1] != s))
        assert cost <= fx.out["score"][k], k


@pytest.mark.parametrize("name", ED)
def test_oracle_edit_distance_equals_wf_ed(name):
    fx = R.Fixture(name)
    assert fx.refused is None, fx.refused
    pairs = R.case_pairs(fx.case)
    assert len(pairs) == len(fx.out["score"]) > 0
    for k, (q, t) in enumerate(pairs):
        assert O.edit_distance(q, t) == fx.out["score"][k], (k, len(q), len(t))


# ---- the chain

def _cluster_arrays(c):
    return c.var_beg.tolist(), c.left_reach.tolist(), c.right_reach.tolist()


def check_clusters(fx, ctg, lib, prefix):
    """our clusters of contig index ctg (ref_pins.our_clusters) == the reference's: starts and both reaches of every cluster"""
    haps, cl = R.our_clusters(fx.case, ctg, lib, prefix)
    for k in range(4):
        want = tuple(a.tolist() for a in R.ref_clusters(fx.out, k, ctg))
        got = _cluster_arrays(cl[k])
        if len(haps[k].pos) == 0:
            assert want == ([], [], []) and cl[k].n == 0, (fx.name, ctg, k)
            continue
        assert got[0] == want[0], (fx.name, prefix, "cluster starts", ctg, k)
        # the sentinel reach behind the last cluster is not part of the comparison
        nc = len(want[0]) - 1
        assert got[1][:nc] == want[1][:nc] and got[2][:nc] == want[2][:nc], (fx.name, prefix, "reaches", ctg, k)
    return haps, cl


def check_chain(fx, cluster_libs, run_pr, check_edits=True):
    """one chain fixture, contig by contig in the reference's order.  cluster_libs: [(lib, prefix)] to cluster and
    supercluster with (each must equal the reference); run_pr(variants) -> A.Results or None (skip the precision/recall part)"""
    from vcfdist_amd import cluster as K, summary as S
    assert fx.refused is None, fx.refused
    o = R.case_args(fx.case)
    n_sc_total = 0
    for ci, ctg in enumerate(fx.out["out_ctgs"].tolist()):
        rs = R.ref_superclusters(fx, ci)
        n_sc_total += rs["n"]
        sc = None
        for lib, prefix in cluster_libs:
            if prefix == "vcl" and o["cluster"][0] == "biwfa":
                continue                                    # the library's biWFA clustering is a GPU kernel (tests/test_gpu_ref_pins.py)
            haps, cl = check_clusters(fx, ctg, lib, prefix)
            sc = K.supercluster(haps, cl, o["max_supercluster_size"], L=lib, prefix=prefix)
            assert sc.n == rs["n"], (fx.name, prefix, ctg, sc.n, rs["n"])
            assert sc.beg.tolist() == rs["beg"].tolist() and sc.end.tolist() == rs["end"].tolist(), (fx.name, prefix, ctg)
            for k in range(4):
                if len(haps[k].pos):
                    assert sc.brk[k].tolist() == rs["brk"][k].tolist(), (fx.name, prefix, ctg, k)
        if sc is None or sc.n == 0 or run_pr is None:
            continue
        v = R.our_variants(fx.case, ctg, haps, sc)
        res = run_pr(v)
        assert np.asarray(res.sc_phase).tolist() == rs["sc_phase"].tolist(), (fx.name, ctg, "sc_phase")
        assert np.asarray(res.orig_phase_dist).tolist() == rs["orig"].tolist(), (fx.name, ctg, "orig_phase_dist")
        assert np.asarray(res.swap_phase_dist).tolist() == rs["swap"].tolist(), (fx.name, ctg, "swap_phase_dist")
        want, got = R.ref_per_variant(fx, ctg, ci), R.results_per_variant(res)
        for key in want:
            if not np.array_equal(want[key], got[key]):
                bad = np.flatnonzero(want[key] != got[key])
                raise AssertionError(f"{fx.name} contig {ctg}: {key[0]} of slot {key[1]}, phasing {key[2]}: {len(bad)} differ, first at variant "
                                     f"{bad[0]}: ours {got[key][bad[0]]} reference {want[key][bad[0]]}")
        pb, sw, fl = S.phase(res.sc_phase, rs["phase_set"], L=O.lib(), prefix="vso")
        assert pb.tolist() == rs["pb_phase"].tolist(), (fx.name, ctg, "pb_phase")
        assert sw.tolist() == rs["switches"].tolist() and fl.tolist() == rs["flips"].tolist(), (fx.name, ctg, "switches / flips")
        if o["distance"] and check_edits:
            jobs, recs = DH.run(v, np.asarray(res.sc_phase, np.int32), np.zeros(sc.n, np.uint8), x=o["eval_sub"], o=o["eval_open"], e=o["eval_extend"],
                                max_qual=o["max_qual"])
            want = R.ref_edits(fx, ctg)
            assert recs.shape == want.shape, (fx.name, ctg, recs.shape, want.shape)
            bad = np.flatnonzero((recs != want).any(1))
            assert len(bad) == 0, f"{fx.name} contig {ctg}: edit record {bad[0]}: model {recs[bad[0]]} reference {want[bad[0]]}"
    return n_sc_total


def oracle_pr(v):
    return O.run(O.generate(v))


@pytest.mark.parametrize("name", CLUSTER)
def test_cluster_oracles_equal_the_reference_clusters(name):
    """simple_cluster (gap and size) and wf_swg_cluster on whole synthetic contigs, other penalties and iteration limits, and on the
    edge cases of tests/wfa_cluster_cases.py (cluster_biwfa_edges_*)"""
    from vcfdist_amd import api
    fx = R.Fixture(name)
    assert fx.refused is None, fx.refused
    n = 0
    for ctg in range(len(R.case_contigs(fx.case))):
        libs = [(O.lib(), "vco")] + ([] if R.case_args(fx.case)["cluster"][0] == "biwfa" else [(api.lib(), "vcl")])
        for lib, prefix in libs:
            haps, cl = check_clusters(fx, ctg, lib, prefix)
            n += sum(c.n for c in cl)
    assert n >= 20


REFUSED = [n for n in CHAIN if R.Fixture(n).refused is not None]
# hand cases the reference refuses, and what our side does with them (tests/golden/README.md, "refused cases")
OURS_REFUSES = {"chain_edges_pos0": "Contig 'chr1' not present in reference FASTA"}
OURS_EVALUATES = {"chain_edges_last_base": "exit -11"}


@pytest.mark.parametrize("name", [n for n in CHAIN if n not in REFUSED])
def test_oracles_equal_the_reference_chain(name):
    """clusters, reaches, superclusters (cluster_oracle.cpp / wfa_oracle.cpp and the library's host cluster.cpp), then
    pr_oracle.cpp's phases, phase distances and six per-variant columns bit for bit, summary_oracle.cpp's phasing, and the
    distance model's edit records in order -- all against the reference's chain on the same variant tables"""
    from vcfdist_amd import api
    fx = R.Fixture(name)
    if name.startswith("demo_") and not name.endswith("_d"):
        # the demo without -d: the reference answers what it answers with -d, less the edit records (checked there)
        twin = R.Fixture(name + "_d")
        assert sorted(fx.out) == sorted(k for k in twin.out if not k.startswith("ed_"))
        assert all(np.array_equal(fx.out[k], twin.out[k]) for k in fx.out)
        return
    n = check_chain(fx, [(O.lib(), "vco"), (api.lib(), "vcl")], oracle_pr)
    if "no_variants" not in name:
        assert n > 0


def test_cases_the_reference_refuses():
    """a variant at position 0: the reference's generate_ptrs_strs reads the base in front of the region and exits; the oracle and
    the library's host marshalling refuse the region too.  A SNP on a contig's last base: the reference's region passes the
    contig's end and calc_prec_recall_path writes outside its matrices (dist.cpp:539-546; here it dies of it) -- no defined
    answer to pin; the oracle and the library cut the region at the last base (include/vcfdist_pr.h) and evaluate it"""
    from vcfdist_amd import _abi as A, api, cluster as K
    assert sorted(REFUSED) == sorted(list(OURS_REFUSES) + list(OURS_EVALUATES))
    for name in REFUSED:
        fx = R.Fixture(name)
        want = OURS_REFUSES.get(name) or OURS_EVALUATES[name]
        assert want in fx.refused, (name, fx.refused)
        haps, cl = R.our_clusters(fx.case, 0, O.lib(), "vco")
        sc = K.supercluster(haps, cl, 10000, L=O.lib(), prefix="vco")
        v = R.our_variants(fx.case, 0, haps, sc)
        if name in OURS_REFUSES:
            with pytest.raises(ValueError):
                O.generate(v)
            with pytest.raises(api.VprError):
                api.batch_from_variants(v)
        else:
            res = O.run(O.generate(v))
            assert res.errtype[0][0].tolist() == [A.ERRTYPE_TP] and res.errtype[2][0].tolist() == [A.ERRTYPE_TP]
            assert bytes(api.batch_from_variants(v).ref_seq) == bytes(O.generate(v).ref_seq)


@pytest.mark.parametrize("name", [n for n in CHAIN if n.startswith("chain_ties")])
def test_tie_fixtures_hold_ties_decided_other_than_largest_source(name):
    """the fixtures the tie replay exists for: the oracle's containers keep a swap predecessor other than the highest index"""
    from vcfdist_amd import cluster as K
    fx = R.Fixture(name)
    o = R.case_args(fx.case)
    n_nonmax = 0
    for ci, ctg in enumerate(fx.out["out_ctgs"].tolist()):
        haps, cl = R.our_clusters(fx.case, ctg, O.lib(), "vco")
        sc = K.supercluster(haps, cl, o["max_supercluster_size"], L=O.lib(), prefix="vco")
        if sc.n:
            b = O.generate(R.our_variants(fx.case, ctg, haps, sc))
            ex = O.Extra(b)
            O.run(b, extra=ex)
            n_nonmax += int((ex.swap_used_conflict_nonmax > 0).sum())
    assert n_nonmax > 0


@pytest.mark.parametrize("name", REALIGN)
def test_realign_model_equals_the_reference(name):
    """realign_model.py == wf_swg_realign + left_shift: every column of every (contig, hap), floats bit for bit"""
    import realign_model as RM
    fx = R.Fixture(name)
    o = R.case_args(fx.case)
    if fx.refused is not None:
        # a cluster whose region would start in front of the contig: the reference's generate_str exits; the model (and
        # vrl_realign, tests/test_gpu_ref_pins.py) keeps that cluster's variants and says so with ST_EDGE
        assert name == "realign_hand_pos0" and "position out of range (generate_str)" in fx.refused, fx.refused
        haps, cl = R.our_clusters(fx.case, 0, O.lib(), "vco", slots=[0])
        s, _, _ = R.case_slot(fx.case, 0, 0)
        got, status = RM.realign(np.frombuffer(R.case_contigs(fx.case)[0][1], np.uint8), R.hap_columns(s), cl[0].var_beg)
        assert status.tolist() == [RM.ST_EDGE] and [r["pos"] for r in got] == s["pos"].tolist()
        return
    n_rec = 0
    for ctg, (cname, seq) in enumerate(R.case_contigs(fx.case)):
        s, a, b = R.case_slot(fx.case, 0, ctg)
        if b == a:
            continue
        hap = R.hap_columns(s)
        var_beg = R.ref_clusters(fx.out, 0, ctg)[0]
        got, status = RM.realign(np.frombuffer(seq, np.uint8), hap, var_beg.astype(np.int32), o["sub"], o["open"], o["extend"], o["max_qual"])
        assert not np.any(status), (name, ctg)
        ra, rb = int(fx.out["r0_off"][ctg]), int(fx.out["r0_off"][ctg + 1])
        assert len(got) == rb - ra, (name, ctg, len(got), rb - ra)
        ro = np.concatenate([[0], np.cumsum(fx.out["r0_ref_len"])])
        ao = np.concatenate([[0], np.cumsum(fx.out["r0_alt_len"])])
        for k, rec in enumerate(got):
            i = ra + k
            want = dict(pos=fx.out["r0_pos"][i], rlen=fx.out["r0_rlen"][i], type=fx.out["r0_type"][i], phase_set=fx.out["r0_phase_set"][i],
                        orig_gt=fx.out["r0_orig_gt"][i], ref=bytes(fx.out["r0_refs"][ro[i]:ro[i + 1]].astype(np.uint8)),
                        alt=bytes(fx.out["r0_alts"][ao[i]:ao[i + 1]].astype(np.uint8)))
            for f, w in want.items():
                g = rec[f].encode() if isinstance(rec[f], str) else rec[f]
                assert g == w, (name, ctg, k, f, g, w)
            for f in ("var_qual", "gt_qual"):
                assert int(np.float32(rec[f]).view(np.uint32)) == fx.out["r0_" + f][i], (name, ctg, k, f)
        n_rec += len(got)
    assert n_rec > 0


# ---- the fixtures themselves

@pytest.mark.skipif(not R.have_harness(), reason="oracle/_ref/ref_harness is not built here (no reference sources): the fixtures cannot be regenerated")
@pytest.mark.parametrize("name", ALL)
def test_fixture_is_what_the_reference_answers(name):
    """the harness on the fixture's inputs gives exactly the fixture's outputs: a stale or hand-edited fixture fails here"""
    fx = R.Fixture(name)
    out = fx.rerun()
    if fx.refused is not None:
        assert out == fx.refused
        return
    assert not isinstance(out, str), out
    assert sorted(out) == sorted(fx.out)
    for k in out:
        assert np.array_equal(out[k], fx.out[k]), (name, k)


def test_no_fixture_is_larger_than_the_largest_earlier_one():
    for name in ALL:
        assert os.path.getsize(os.path.join(R.GOLDEN, name + ".npz")) <= 543_000, name


def test_random_sets_dropped_at_most_two_percent():
    for name in SWG + ED:
        fx = R.Fixture(name)
        if "n_pairs" in fx.extra:
            assert int(fx.extra["n_dropped"]) <= 0.02 * int(fx.extra["n_pairs"]), name
