"""One handle taking different batches one after another: what vpr_upload's free_batch, the kept device and page-locked blocks
and the handle's K0 timing events are about.  The sequence goes large -> tiny -> large -> small, through both upload entries,
so the kept blocks are reused, outgrown and reused again; after every upload the handle's results equal the oracle's bit for
bit (the rules of test_gpu_parity.compare) and a fresh handle's download."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # VPR_ERR_ARG (include/vcfdist_pr.h)
REF = "ACGTTGCAACGT"


def _tiny_sites():
    """the five hand-made superclusters of test_gpu_parity.test_minimum_sizes_and_empty_haps"""
    S, I, D = A.TYPE_SUB, A.TYPE_INS, A.TYPE_DEL
    return [
        dict(ctg=0, beg=2, end=4, vars=[[(3, S, "T", "A", 9.0)], [], [], []]),
        dict(ctg=0, beg=2, end=4, vars=[[], [], [(3, S, "T", "A", 9.0)], []]),
        dict(ctg=0, beg=4, end=6, vars=[[(5, I, "", "GG", 5.0)], [(5, I, "", "GG", 5.0)],
                                         [(5, I, "", "GG", 7.0)], [(5, I, "", "G", 7.0)]]),
        dict(ctg=0, beg=5, end=9, vars=[[(6, D, "CA", "", 5.0)], [], [(6, D, "CA", "", 7.0)], [(6, D, "C", "", 7.0)]]),
        dict(ctg=0, beg=1, end=10, vars=[[], [], [], []]),
    ]


@functools.lru_cache(maxsize=None)
def _steps():
    """the four uploads: (entry, batch, variant tables or None, the oracle's results); computed once, never written to"""
    big = api.Synth(n_sc=300, len_a=8, len_b=2500, len_min=5, len_max=2500, seed=6)
    small = api.Synth(n_sc=64, len_a=8, len_b=300, len_max=300, seed=7)
    tiny_v = A.Variants.from_sites([REF], _tiny_sites())
    b_big, b_tiny, b_small = big.batch(), api.batch_from_variants(tiny_v), small.batch()
    w_big, w_tiny, w_small = (O.run(b, extra=O.Extra(b)) for b in (b_big, b_tiny, b_small))
    return (("upload", b_big, None, w_big),
            ("upload_variants", b_tiny, tiny_v, w_tiny),
            ("upload_variants", b_big, big, w_big),              # (the generator owns its tables)
            ("upload", b_small, None, w_small))


def _equals_oracle(got, want, pr):
    for f in ("aln_dist", "aln_end_plane", "aln_beg_plane", "aln_status", "sc_phase", "orig_phase_dist", "swap_phase_dist"):
        a, b = getattr(got, f), getattr(want, f)
        assert np.array_equal(a, b), (f, np.flatnonzero(a != b)[:8])
    for h in range(4):
        for w in range(2):
            for name, dt in A.Results.PER_VAR:
                x, y = getattr(got, name)[h][w], getattr(want, name)[h][w]
                if dt == np.float32:
                    x, y = x.view(np.uint32), y.view(np.uint32)
                assert np.array_equal(x, y), (name, h, w, np.flatnonzero(x != y)[:8])
    assert pr.timing().n_tie_replays >= int(((want.aln_status & A.ST_SWAP_TIE) != 0).sum())


def _upload(pr, entry, batch, tables):
    if entry == "upload":
        pr.upload(batch)
    else:
        pr.upload_variants(tables.struct if isinstance(tables, api.Synth) else tables.as_struct(), batch)


def _sequence(cfg):
    pr = api.PrecisionRecall(cfg)
    fresh = {}                                  # a fresh handle's download per batch (the third upload repeats the first batch)
    for k, (entry, batch, tables, want) in enumerate(_steps()):
        _upload(pr, entry, batch, tables)
        pr.execute()
        got = pr.download()
        _equals_oracle(got, want, pr)
        if id(batch) not in fresh:
            fresh[id(batch)] = api.PrecisionRecall(cfg).run(batch)
        assert not got.diff(fresh[id(batch)]), (k, entry)


def test_one_handle_takes_four_batches_through_both_uploads():
    _sequence(A.default_config())


@pytest.mark.parametrize("kw", [dict(band_mode=0), dict(band_mode=2), dict(band_mode=3), dict(flags=A.CFG_HAP_DEDUP),
                                dict(workspace_bytes=8 << 20)],
                         ids=["dense", "c64", "q16", "hap_dedup", "workspace_8MB"])
def test_the_same_sequence_at_other_configurations(kw):
    """dense only, 64-cell and general 16-cell round 0; identical alignments computed once (the work list is a subset: host
    planner); an 8 MB workspace (several chunks: host planner)"""
    _sequence(A.default_config(**kw))


def test_the_same_sequence_with_the_host_planner(monkeypatch):
    monkeypatch.setenv("VPR_HOST_PLAN", "1")
    _sequence(A.default_config())


def test_a_refused_upload_leaves_the_handle_usable():
    """a supercluster whose truth haplotype is empty (a deletion of its whole region) passes the host marshalling and is refused
    by vpr_upload behind the K0 kernels -- with their timing events recorded and the batch's blocks taken; the next upload on the
    same handle is a good one"""
    sites = _tiny_sites()
    sites.insert(1, dict(ctg=0, beg=4, end=6, vars=[[], [], [(4, A.TYPE_DEL, REF[4:7], "", 7.0)], []]))
    bad = api.batch_from_variants(A.Variants.from_sites([REF], sites))
    assert bad.lens(1)[2] == 0
    pr = api.PrecisionRecall()
    with pytest.raises(api.VprError) as e:
        pr.upload(bad)
    assert str(e.value) == f"vpr_upload failed ({ERR_ARG}): supercluster 1 has an empty string"
    entry, batch, tables, want = _steps()[3]
    for _ in range(2):          # (twice: the refused upload's blocks are kept ones by then)
        _upload(pr, entry, batch, tables)
        pr.execute()
        _equals_oracle(pr.download(), want, pr)
