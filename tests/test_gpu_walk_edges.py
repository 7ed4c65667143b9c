"""The walks of the window and dense levels on the oracle's path, entry for entry: the table of tests/walk_edge_cases.py through the
kernels (k_walk_q16, k_walk_rows, the segment walk k_walk_seg, k_walk<wave>, k_walk<lane>).

  paths       a batch per case with CFG_KEEP_PATHS under band_mode 1, 3, 2 and 0, and under band_mode 2 with VPR_SEQ_WALK: the five
              arrays of vpr_download_path of EVERY alignment equal the oracle's, and the lengths agree.  A homozygous case is four
              times the same alignment, all four finish in the same, last round, so nothing is skipped and a VprError on the
              download fails the test.  Of a heterozygous case an alignment may be skipped only where the launch stats show that
              an earlier round accepted some (the last level's forward launches held fewer than four).  A failure names the case,
              the band mode, the alignment and the first path index that differs.
  kernels     the level that accepted a case is the highest whose forward launches ran (reached() of test_gpu_window_edges.py);
              the walk kernel for that level, band mode and launch size follows from the rules of enqueue_part / walk_launch
              (expected_walk below, with LONG_LT, VPR_WSEG_MIN_ROWS' default and the lane walk's 2 048 read out of the sources), and
              its name must be among the walk launches.  Over the whole table every pair of REQUIRED_PAIRS (walk kernel, feature)
              must have occurred: a case that does not reach the kernel it is aimed at fails that test, not the list.
  agreement   k_walk_seg's and k_walk_rows' paths of the same batch are equal, asserted directly.
  lanes       the small cases repeated to 512 superclusters or more: one dense launch of 2 048 alignments (k_walk<lane>) under
              band_mode 0, every case's first and last copy compared path by path; the same batch under band_mode 2 (the segment
              walk's slot accounting with thousands of one-segment alignments).  Both runs are one round by the stats, and no
              download may fail.
  results     compare()'s arrays on a batch per family under the four band modes through vpr_upload and vpr_upload_variants.

Every comparison is equality.  Measured times, the accepted level per case and the (kernel, feature) coverage are printed as one
JSON line when the module is done; profiles/walk_edges_gpu.json is a recording of it."""
import json
import time

import numpy as np
import pytest

import oracle_lib as O
import walk_edge_cases as WK
import window_edge_cases as WE
from test_gpu_window_edges import reached
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu

PART = 6        # cases per parametrised case of the per-case tests (five handles each; about one handle in thirty takes 2 to 3 s)
RUNS = ((1, False), (3, False), (2, False), (0, False), (2, True))       # (band_mode, VPR_SEQ_WALK)
FAMILIES = sorted({c.family for c in WK.TABLE})
PARTS = [(f, k) for f in FAMILIES for k in range(0, len([c for c in WK.HOM if c.family == f]), PART)]
RECORD = dict(levels={}, pairs={}, seconds={})       # levels: {case: {run: level}}; pairs: {(kernel, feature): a case}

SEG = [("enter", WK.WSEG_ROWS, m, "at") for m in WK.ROW_MOVES] + [("ins_row", WK.WSEG_ROWS, s) for s in ("before", "after")] + [("run_end", "INS", 0), ("end_plane", 1)]
REQUIRED_PAIRS = (
    # the 128-row segment border of k_wseg_map, its 256 staged columns and other(); the 64-segment chunk of k_wseg_compose
    [("k_walk_seg", f) for f in SEG + [("enter", WK.CHUNK_STRIPES, m, "at") for m in WK.ROW_MOVES]
     + [("el", "first", 0), ("el", "first", 1), ("el", "last", WK.FS_W - 1), ("el", "last", WK.FS_W - 2), ("r2q_off", WK.WSEG_COLS - 1),
        ("r2q_off", WK.WSEG_COLS), ("other_fallback", "r2q"), ("segments", 65), ("last_seg_rows", 1)]]
    # the 64-stripe and 64-row chunks of walk_rows_range
    + [("k_walk_rows", f) for f in SEG + [("enter", b, m, "at") for b in (WK.FS_W, WK.CHUNK_STRIPES) for m in WK.ROW_MOVES]
       + [("ins_row", b, s) for b in (WK.FS_W, WK.CHUNK_STRIPES) for s in ("before", "after")] + [("segments", 65), ("last_seg_rows", 1)]]
    # k_walk<wave>: its runs of 2 and of 64, row_get and col_get, the direct read, the dense tile and its keep mask, the tile's rows
    + [("k_walk<wave>", f) for f in [("wave_run", k, n) for k in ("MS", "INS", "DEL") for n in (2, WK.FS_W)] + [("wave_run_cut", k) for k in ("MS", "INS", "DEL")]
       + [("row_get", "next"), ("row_get", "skip"), ("col_get", "recentre"), ("direct",), ("tile", 0, "right"), ("tile", 0, "inner"), ("tile", 1, "right"),
          ("tile_rows",), ("long_run_single_run", "INS"), ("long_run_single_run", "DEL"), ("ref_run_swap", 2), ("sync101",)]
       + [("keep", p, r) for p in (0, 1) for r in (1, 2, 3)] + [("last4", p, r) for p in (0, 1) for r in (0, 1, 2, 3)]
       + [("enter", WK.WALK_TR, m, "at") for m in WK.ROW_MOVES] + [("Lq", n) for n in WK.PLANES] + [("Lr", n) for n in WK.PLANES]]
    # ... on window rows (the 256- and 1024-cell levels: the 32-row tile, and the tile around the walk of the 1024-cell level)
    + [("k_walk<wave>@256", ("run", "INS", n)) for n in (63, 64, 65, 127)] + [("k_walk<wave>@1024", ("run", "INS", 300))]
    + [("k_walk_q16", ("Lt", n)) for n in WK.LTS[:11]]
)


def expected_walk(level, mode, seq, Lt, n_aln):
    """the walk kernel of enqueue_part / walk_launch for an alignment of Lt truth rows that `level` accepted in a launch of n_aln
    alignments (None: the lane levels of band_mode 1, tests/test_gpu_lane_tail.py's)"""
    if not level or (level == 16 and mode == 1):
        return None
    if level == 16:
        return "k_walk_q16"
    long_part = mode in (1, 3) and Lt >= WK.K["LONG_LT"]         # round 0's long part starts at the 64-cell level
    wave = long_part or n_aln < WK.K["LANE_WALK_MIN"]
    if level == 64:
        if seq:
            return "k_walk_rows" if wave else "k_walk<lane>"
        return "k_walk_rows" if long_part and Lt < WK.K["WSEG_MIN_ROWS"] else "k_walk_seg"
    return "k_walk<wave>" if wave else "k_walk<lane>"


def first_difference(got, want):
    """None, or a text naming the first path index at which the kernel's five arrays differ from the oracle's"""
    n = min(len(got[0]), len(want[0]))
    bad = np.zeros(n, bool)
    for g, w in zip(got, want):
        bad |= np.asarray(g[:n]) != np.asarray(w[:n])
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        ent = lambda p: tuple(int(a[i]) for a in p)
        return f"path index {i}: (plane, qri, ti, sync, edit) {ent(got)} from the kernel, {ent(want)} from the oracle"
    if len(got[0]) != len(want[0]):
        return f"path index {n}: path_len {len(got[0])} from the kernel, {len(want[0])} from the oracle"
    return None


def run_case(case, fe, mode, seq, monkeypatch, batch):
    """one batch of one case -> (accepted level, walk kernels, {aln: path}); asserts every path against the oracle's"""
    tag = f"{case.name}, band_mode {mode}{', VPR_SEQ_WALK' if seq else ''}"
    if seq:
        monkeypatch.setenv("VPR_SEQ_WALK", "1")
    pr = api.PrecisionRecall(A.default_config(band_mode=mode, flags=A.CFG_KEEP_PATHS))
    if seq:
        monkeypatch.delenv("VPR_SEQ_WALK")
    res = pr.run(batch)
    r = reached(pr)
    level = max(r) if r else 0
    walks = {s.kernel.decode() for s in pr.launch_stats() if s.kind == 3}
    paths, skipped = {}, []
    for aln in range(4):
        try:
            paths[aln] = pr.path(0, aln)
        except api.VprError as e:
            assert WK.is_het(case), f"{tag}, alignment {aln}: no path ({e})"
            skipped.append(aln)
            continue
        diff = first_difference(paths[aln], WK.path_of(case, fe, aln))
        assert diff is None, f"{tag}, alignment {aln}, level {level}, walks {sorted(walks)}: {diff}"
    pr.close()
    # (behind the paths: a walk that gave up is first told by the path index at which its path ends)
    assert not (res.aln_status[:4] & ~np.uint32(A.ST_SWAP_TIE | A.ST_WARN_MASK)).any(), (tag, res.aln_status[:4])
    if skipped:         # an earlier round accepted some: the last level's forward launches held fewer than four
        assert r and len(skipped) <= 4 - min(4, r[level]) and paths, (tag, skipped, r)
    want = expected_walk(level, mode, seq, max(fe[0].lens[2:4]), 4)
    if want is not None and not skipped:
        assert want in walks, f"{tag}: level {level} accepted, {want} expected, the walk launches were {sorted(walks)}"
    return level, walks, paths, want


@pytest.fixture(scope="module")
def feats():
    t0 = time.time()
    out = WK.feats(WK.TABLE)
    RECORD["seconds"]["oracle_features"] = round(time.time() - t0, 2)
    return out


@pytest.fixture(scope="module", autouse=True)
def recording():
    yield
    lv = lambda x: "dense" if x == WE.DENSE else x
    out = dict(seconds=RECORD["seconds"],
               levels={c: {k: lv(v) for k, v in d.items()} for c, d in sorted(RECORD["levels"].items())},
               pairs=sorted(f"{k} {f}: {c}" for (k, f), c in RECORD["pairs"].items() if (k, f) in set(REQUIRED_PAIRS)),
               n_pairs_seen=len(RECORD["pairs"]))
    print("\nwalk_edges_gpu " + json.dumps(out))


WAVE_TRACE = ("wave_run", "wave_run_cut", "wave_run_end", "row_get", "col_get", "direct", "tile", "tile_rows", "keep", "last4")


def _note(case, F, run, level, want):
    RECORD["levels"].setdefault(case.name, {})[f"{run[0]}{'s' if run[1] else ''}"] = level
    if want is None:
        return
    for f in F:
        if f[0] in WAVE_TRACE and not (want == "k_walk<wave>" and level == WE.DENSE):
            continue        # (wave_trace restates k_walk<wave> on dense rows: shown only where the dense level accepted)
        RECORD["pairs"].setdefault((want, f), case.name)
        if want == "k_walk<wave>" and level in (256, 1024):
            RECORD["pairs"].setdefault((f"{want}@{level}", f), case.name)


@pytest.mark.parametrize("family,first", PARTS, ids=[f"{f}-{k}" for f, k in PARTS])
def test_every_path_entry_equals_the_oracles(family, first, feats, monkeypatch):
    t0 = time.time()
    cases = [c for c in WK.HOM if c.family == family][first:first + PART]
    for c in cases:
        fe = feats[c.name]
        _, batch = WK.batch_of([c])
        got = {}
        for run in RUNS:
            level, walks, paths, want = run_case(c, fe, run[0], run[1], monkeypatch, batch)
            got[run] = (want, paths)
            _note(c, fe[0].features, run, level, want)
        # agreement: the segment walk and the row walk on the same batch
        (ka, pa), (kb, pb) = got[(2, False)], got[(2, True)]
        if {ka, kb} == {"k_walk_seg", "k_walk_rows"}:
            for aln in range(4):
                diff = first_difference(pa[aln], pb[aln])
                assert diff is None, f"{c.name}, alignment {aln}: {ka} against {kb}: {diff.replace('oracle', kb)}"
    RECORD["seconds"][f"{family}-{first}"] = round(time.time() - t0, 2)
    print(f"{family} from {first}: {len(cases)} batches of one case, five runs each, {time.time() - t0:.2f} s")


def test_heterozygous_cases(feats, monkeypatch):
    t0 = time.time()
    for c in WK.HET:
        fe = feats[c.name]
        _, batch = WK.batch_of([c])
        for run in RUNS:
            level, walks, paths, want = run_case(c, fe, run[0], run[1], monkeypatch, batch)
            assert paths, (c.name, run)
            RECORD["levels"].setdefault(c.name, {})[f"{run[0]}{'s' if run[1] else ''}"] = level
    RECORD["seconds"]["het"] = round(time.time() - t0, 2)


def test_every_required_pair_of_walk_kernel_and_feature_occurred(feats):
    """(after the per-case tests of this module: it reads what they recorded)"""
    if not all(c.name in RECORD["levels"] and len(RECORD["levels"][c.name]) == len(RUNS) for c in WK.HOM):
        pytest.fail("the per-case tests of this module did not all run before this one: run the module as a whole")
    missing = [p for p in REQUIRED_PAIRS if p not in RECORD["pairs"]]
    assert not missing, missing


def _small(feats):
    """the cases whose planes fit the smallest dense kernel class (64 cells): one launch holds them all"""
    return [c for c in WK.HOM if c.family in ("rows", "runs", "planes") and max(feats[c.name][0].lens) <= WK.FS_W]


def test_lane_walk_of_a_dense_launch_and_one_segment_slots(feats):
    t0 = time.time()
    cases = _small(feats)
    repeat = -(-512 // len(cases))
    _, batch = WK.batch_of(cases, repeat=repeat)
    assert batch.n_sc >= 512 and 4 * batch.n_sc >= WK.K["LANE_WALK_MIN"]
    for mode, kernel in ((0, "k_walk<lane>"), (2, "k_walk_seg")):
        pr = api.PrecisionRecall(A.default_config(band_mode=mode, flags=A.CFG_KEEP_PATHS))
        res = pr.run(batch)
        walks = {s.kernel.decode(): int(s.n_units) for s in pr.launch_stats() if s.kind == 3}
        assert kernel in walks, (mode, walks)
        # one round: every alignment finishes at the level the mode starts with, so every path can be downloaded
        assert set(reached(pr)) == {WE.DENSE if mode == 0 else 64}, (mode, reached(pr))
        assert walks[kernel] == 4 * batch.n_sc, walks
        if mode == 0:
            assert "k_walk<wave>" not in walks, walks
        n_compared = 0
        assert not (res.aln_status & ~np.uint32(A.ST_SWAP_TIE | A.ST_WARN_MASK)).any()
        for k, c in enumerate(cases):
            for aln in range(4):
                for sc in (k, (repeat - 1) * len(cases) + k):         # the first copy and the last
                    try:
                        got = pr.path(sc, aln)
                    except api.VprError as e:
                        raise AssertionError(f"{c.name}, band_mode {mode}, supercluster {sc}, alignment {aln}: no path ({e})")
                    diff = first_difference(got, feats[c.name][0].path)
                    assert diff is None, f"{c.name}, band_mode {mode}, supercluster {sc}, alignment {aln}, {kernel}: {diff}"
                    n_compared += 1
        assert n_compared == 8 * len(cases)
        pr.close()
    RECORD["seconds"]["lanes"] = round(time.time() - t0, 2)


def _equal_results(got, want, tag):
    for f in ("aln_dist", "aln_end_plane", "aln_beg_plane", "aln_status", "sc_phase", "orig_phase_dist", "swap_phase_dist"):
        a, b = getattr(got, f), getattr(want, f)
        assert np.array_equal(a, b), (tag, f, np.flatnonzero(a != b)[:8])
    for h in range(4):
        for w in range(2):
            for name, dt in A.Results.PER_VAR:
                x, y = getattr(got, name)[h][w], getattr(want, name)[h][w]
                if dt == np.float32:
                    x, y = x.view(np.uint32), y.view(np.uint32)
                assert np.array_equal(x, y), (tag, name, h, w, np.flatnonzero(x != y)[:8])


@pytest.mark.parametrize("family", FAMILIES)
def test_family_results_equal_the_oracle_through_both_uploads(family):
    """every result array against the oracle bit for bit (the comparisons of compare(), test_gpu_parity.py, against ONE oracle run
    per family): the path entries' reference coordinates reach the tests only through the credits"""
    t0 = time.time()
    v, batch = WK.batch_of([c for c in WK.TABLE if c.family == family])
    want = O.run(batch)
    assert not (want.aln_status & ~np.uint32(A.ST_SWAP_TIE | A.ST_WARN_MASK)).any()
    n_tie = int(((want.aln_status & A.ST_SWAP_TIE) != 0).sum())
    for mode in (1, 3, 2, 0):
        for variants in (False, True):
            pr = api.PrecisionRecall(A.default_config(band_mode=mode))
            if variants:
                pr.upload_variants(v.as_struct(), batch)
                pr.execute()
                got = pr.download()
            else:
                got = pr.run(batch)
            _equal_results(got, want, (family, mode, "vpr_upload_variants" if variants else "vpr_upload"))
            assert pr.timing().n_tie_replays >= n_tie
            pr.close()
    RECORD["seconds"][f"results-{family}"] = round(time.time() - t0, 2)
