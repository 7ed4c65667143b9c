"""The window ladder's exit test on paths at a window's edge: the table of tests/window_edge_cases.py through the kernels.

  parity      every array against the CPU oracle bit for bit (compare() of test_gpu_parity.py) under band_mode 1, 3, 2 and 0, a batch
              per family and level; and, asserted directly, the dense results (band_mode 0) equal to each windowed run's.
  soundness   a batch per case under band_mode 3 and 2, where every alignment enters the window levels: from launch_stats(), the
              alignments that reached each level above the first (the n_units of the level's forward launches) must be at least
              those whose needed_level is that level or above (needed_level: the cells on optimal paths, window_edge_cases.py).  A
              case accepted below its needed level fails even if its arrays are right: the lower bound is unsound there and equal
              arrays are luck.  The counts are list lengths, not capacities: a
              retry round's plan is made from the host's fail list (lad_start, pr_api.hip), round 0 of band_mode 3 / 2 runs its
              short and long part with n_short / n_long; the one capacity (cap_ip, the in-place 16-cell round behind the lane
              levels) exists under band_mode 1 only, which is not read here.  A tie round re-runs the forward sweep of the level
              that ACCEPTED an alignment under the same kernel name, so in a batch of one homozygous case -- four times the same
              alignment -- the count of the needed level is exact from below: it is 0 if a lower level accepted.
  ties        the 2k == u cases: n_tie_replays at least the oracle's tie count (inside compare()), and the same arrays through
              vpr_upload and vpr_upload_variants.
  tightness   measured, not asserted: per family and level, how many cases were accepted at needed_level and how many climbed
              further, and how many were accepted below the level their forward reach would need (printed as one JSON line when
              the module is done; profiles/window_edges_gpu.json is a recording of it)."""
import json
import time

import numpy as np
import pytest

import window_edge_cases as WE
from test_gpu_parity import compare
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu

PART = 12       # cases per parametrised case of the per-case tests


def _groups():
    out = {}
    for c in WE.TABLE:
        out.setdefault(f"{c.family if c.family in ('shift', 'priced') else 'other'}_w{c.W}", []).append(c)
    return out


GROUPS = _groups()
PARTS = [(g, k) for g, cases in GROUPS.items() for k in range(0, len(cases), PART)]
TIGHT = {}      # {(family, needed level, band_mode): {accepted level: cases, "below_fwd": cases accepted below Need.level_fwd}}


def level_of_kernel(name):
    if name == "k_fwd_q16":
        return 16
    if name == "k_fwd_stripe":
        return 64
    if name.startswith("k_fwd_wide<"):
        return {"k_fwd_wide<4>": 256, "k_fwd_wide<16>": 1024}[name]
    if name.startswith("k_fwd<") or name == "k_fwd_strip":
        return WE.DENSE
    return None


def reached(pr):
    """{level: alignments its forward launches of the handle's last execute held}"""
    out = {}
    for s in pr.launch_stats():
        lv = level_of_kernel(s.kernel.decode()) if s.kind == 1 else None
        if lv is not None:
            out[lv] = out.get(lv, 0) + int(s.n_units)
    return out


@pytest.fixture(scope="module", autouse=True)
def tightness_table():
    yield
    rows = [dict(family=f, needed=("dense" if n == WE.DENSE else n), band_mode=m, below_forward_reach=acc.pop("below_fwd", 0),
                 accepted={("dense" if k == WE.DENSE else str(k)): v for k, v in sorted(acc.items())})
            for (f, n, m), acc in sorted(TIGHT.items())]
    print("\nwindow_edges_tightness " + json.dumps(rows))


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_equals_the_oracle_in_every_band_mode_and_the_dense_sweep(name):
    t0 = time.time()
    _, batch, _ = WE.batch_of(GROUPS[name])
    needs = WE.needs(GROUPS[name])
    need = [n.level for c in GROUPS[name] for n in needs[c.name] * (1 if c.het else 4)]         # per alignment
    got = {}
    for mode in (1, 3, 2, 0):
        got[mode], want, _, pr = compare(batch, A.default_config(band_mode=mode))
        r = reached(pr)
        if mode == 0:
            assert set(r) == {WE.DENSE}, r
        for L in WE.LEVELS[1:] + (WE.DENSE,):       # (weak in a batch: a tie round's re-run counts too; the test below is exact)
            if mode in (3, 2) and L > (16 if mode == 3 else 64):
                assert r.get(L, 0) >= sum(1 for n in need if n >= L), (name, mode, L, r)
    assert not (want.aln_status & ~np.uint32(A.ST_SWAP_TIE | A.ST_WARN_MASK)).any()
    for mode in (1, 3, 2):      # dense as the arbiter: implied by the parity above, asserted so that a failure names the mode
        assert not got[mode].diff(got[0]), (name, mode, got[mode].diff(got[0])[:4])
    print(f"{name}: {len(GROUPS[name])} cases, four band modes against the oracle in {time.time() - t0:.2f} s")


@pytest.mark.parametrize("name,first", PARTS, ids=[f"{g}-{k}" for g, k in PARTS])
def test_no_level_below_the_needed_one_accepts(name, first):
    t0 = time.time()
    cases = GROUPS[name][first:first + PART]
    needs = WE.needs(cases)
    slowest = (0.0, "")
    for c in cases:
        t1 = time.time()
        need = needs[c.name] * (1 if c.het else 4)          # per alignment
        _, batch, _ = WE.batch_of([c])
        for mode, lowest in ((3, 16), (2, 64)):
            if mode == 2 and max(n.level for n in need) <= 64:
                continue            # (no level below the needed one in this mode: nothing that the run could show)
            pr = api.PrecisionRecall(A.default_config(band_mode=mode))
            res = pr.run(batch)
            assert tuple(int(d) for d in res.aln_dist[:4]) == need[0].dists, (c.name, mode)
            r = reached(pr)
            pr.close()          # (a handle per case and band mode: released at once, not when the collector comes by)
            for L in WE.LEVELS[1:] + (WE.DENSE,):
                if L > lowest:
                    n_need = sum(1 for n in need if n.level >= L)
                    assert r.get(L, 0) >= n_need, \
                        f"{c.name}, band_mode {mode}: {n_need} alignments need level {L} or above, {r.get(L, 0)} reached it ({r}): accepted below the needed level"
            if not c.het:
                acc = TIGHT.setdefault((c.family, max(need[0].level, lowest), mode), {})
                acc[max(r)] = acc.get(max(r), 0) + 1
                acc["below_fwd"] = acc.get("below_fwd", 0) + int(max(r) < need[0].level_fwd)
        slowest = max(slowest, (time.time() - t1, c.name))
    print(f"{name} from {first}: {len(cases)} batches of one case under band_mode 3 and 2, {time.time() - t0:.2f} s "
          f"(the slowest: {slowest[1]}, {slowest[0]:.2f} s)")


def test_ties_at_the_edge_through_both_uploads():
    cases = [c for c in WE.TABLE if c.tie]
    assert len(cases) >= 5
    v, batch, _ = WE.batch_of(cases)
    got_a, want, _, pr_a = compare(batch)
    n_tie = int(((want.aln_status & A.ST_SWAP_TIE) != 0).sum())
    assert n_tie >= 4 * len(cases) and pr_a.timing().n_tie_replays >= n_tie
    got_v, _, _, pr_v = compare(batch, variants_struct=v.as_struct())
    assert pr_v.timing().n_tie_replays >= n_tie
    assert not got_a.diff(got_v), got_a.diff(got_v)[:4]
    for mode in (3, 2):
        got_m, _, _, pr_m = compare(batch, A.default_config(band_mode=mode), variants_struct=v.as_struct())
        assert pr_m.timing().n_tie_replays >= n_tie and not got_a.diff(got_m), mode
