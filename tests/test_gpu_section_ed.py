"""The section edit distances (ref_ed) of the HIP path at their edges: the table of tests/section_ed_cases.py, a group per batch so
that one launch carries many jobs of very different lengths.  Every array against the CPU oracle bit for bit (compare() of
test_gpu_parity.py), and -- independently of the oracle -- ref_ed of every truth variant against the plain DP lev(X, Y).  By
default the deferred sections go through k_ed_bits (pr_ed.hip); VPR_ED_WF / VPR_ED_DIAG force k_ed_wf / k_ed_diag
(pr_kernels.hip), which must have run and must give the same arrays.  The inline sections (small_ed in credit_walk) are the
group inline_borders' first half.  The row sweep k_ed and the kernel selection for batches with a haplotype above 65 536 bases are
in tests/test_gpu_long_haplotype.py (the table of tests/long_haplotype_cases.py, behind a ballast supercluster)."""
import functools
import time

import numpy as np
import pytest

import section_ed_cases as SC
from test_gpu_parity import compare
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def group(name):
    """-> (the built cases, the group's batch, lev(X, Y) per truth variant in batch order)"""
    contigs, scs, built = SC.build_group(SC.GROUPS[name])
    batch = api.batch_from_variants(A.Variants.from_sites(contigs, scs))
    return built, batch, expected(built)


@functools.lru_cache(maxsize=None)
def lev(X, Y):
    return SC.lev(X, Y)


def expected(built):
    out = []
    for b in built:
        d = [lev(X, Y) for X, Y in b.pairs]
        out += [d[k] for k in b.var_pair]
    return np.array(out, np.int32)


def kernels(pr):
    """{kernel name: units summed over its launches} of the handle's last execute"""
    out = {}
    for s in pr.launch_stats():
        out[s.kernel.decode()] = out.get(s.kernel.decode(), 0) + int(s.n_units)
    return out


def assert_ref_ed(res, want, what):
    for h in (2, 3):
        for w in range(2):
            got = res.ref_ed[h][w]
            assert np.array_equal(got, want), (what, h, w, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])


@pytest.mark.parametrize("name", list(SC.GROUPS))
def test_group_equals_the_oracle_and_the_plain_dp(name, monkeypatch):
    t0 = time.time()
    built, batch, want_ed = group(name)
    got, want, _, pr = compare(batch)
    t_oracle_and_default = time.time() - t0
    assert (want.aln_status == 0).all()
    assert_ref_ed(got, want_ed, name)
    ran = kernels(pr)
    n_deferred = sum(b.case.deferred for b in built)
    assert ran.get("k_ed_bits", 0) >= n_deferred > 0, ran
    assert not {"k_ed_wf", "k_ed_diag", "k_ed"} & set(ran), ran
    if name == "inline_borders":
        # the inline cases alone: small_ed in both orientations, no deferred kernel at all
        inl = [b for b in built if not b.case.deferred]
        assert len(inl) >= 5
        b2 = api.batch_from_variants(A.Variants.from_sites([b.contig for b in inl], [dict(b.sc, ctg=i) for i, b in enumerate(inl)]))
        pr2 = api.PrecisionRecall()
        assert_ref_ed(pr2.run(b2), expected(inl), "inline alone")
        assert not [k for k in kernels(pr2) if k.startswith("k_ed")], kernels(pr2)
    if name in ("one_group", "multi_group", "packed"):
        for var, kernel in (("VPR_ED_WF", "k_ed_wf"), ("VPR_ED_DIAG", "k_ed_diag")):
            monkeypatch.setenv(var, "1")
            pr2 = api.PrecisionRecall()
            other = pr2.run(batch)
            monkeypatch.delenv(var)
            ran2 = kernels(pr2)
            assert ran2.get(kernel, 0) >= n_deferred and "k_ed_bits" not in ran2, (var, ran2)
            assert not got.diff(other), var
    print(f"{name}: {len(built)} cases, {n_deferred} deferred sections, k_ed_bits over {ran['k_ed_bits']} jobs; "
          f"oracle + default run {t_oracle_and_default:.2f} s, all {time.time() - t0:.2f} s")


ALONE = 8       # deferred cases per parametrised case below
ALONE_PARTS = [(g, k) for g, cases in SC.GROUPS.items() for k in range(0, sum(1 for c in cases if c.deferred), ALONE)]


@pytest.mark.parametrize("name,first", ALONE_PARTS, ids=[f"{g}-{k}" for g, k in ALONE_PARTS])
def test_a_deferred_case_alone_in_its_batch_gives_the_same_distance(name, first):
    """one batch per deferred case: ref_ed is lev(X, Y) as it is inside the group's batch -- whatever block the job lands in and
    whatever the job before it left in the LDS planes.  A handle per batch: through ONE handle vpr_upload took 1.2 s and 8.0 s
    (measured) for two of one_group's batches that follow a tiny batch with retries, against 3 ms through a fresh handle."""
    t0 = time.time()
    cases = [c for c in SC.GROUPS[name] if c.deferred][first:first + ALONE]
    assert cases
    for case in cases:
        b = SC.build(case)
        pr = api.PrecisionRecall()
        res = pr.run(api.batch_from_variants(A.Variants.from_sites([b.contig], [b.sc])))
        assert (res.aln_status == 0).all(), case.name
        assert_ref_ed(res, expected([b]), case.name)
        assert kernels(pr).get("k_ed_bits", 0) >= case.deferred, (case.name, kernels(pr))
    print(f"{name} from {first}: {len(cases)} batches of one case, {time.time() - t0:.2f} s")
