"""The table of tests/walk_edge_cases.py is what it claims, with the oracle alone (no GPU): every feature the walks' borders ask for is
in some homozygous case, every case has the features it is named for, every border has every row-entering move on either side, the
oracle reports no error -- and the features themselves are checked against small paths written out by hand.  These are the
conditions that keep tests/test_gpu_walk_edges.py from passing vacuously."""
import time

import numpy as np
import pytest

import walk_edge_cases as WK
import window_edge_cases as WE
from vcfdist_amd import _abi as A

N_CASES = 154


@pytest.fixture(scope="module")
def feats():
    t0 = time.time()
    out = WK.feats(WK.TABLE)
    print(f"features of {len(WK.TABLE)} cases: {time.time() - t0:.1f} s")
    return out


def test_no_case_is_dropped(feats):
    assert len(WK.TABLE) == N_CASES == len({c.name for c in WK.TABLE}) == len(feats)
    fam = {}
    for c in WK.TABLE:
        fam[c.family] = fam.get(c.family, 0) + 1
    assert fam == {"rows": 38, "long": 3, "border": 24, "runs": 52, "el": 7, "other": 3, "planes": 20, "het": 4, "variation": 3}, fam
    assert len(WK.HET) == 4 and all(len(feats[c.name]) == 4 for c in WK.HET) and all(len(feats[c.name]) == 1 for c in WK.HOM)


def test_constants_come_from_the_sources():
    """the borders are what the kernels' constants make them; the two pitch rules leave ONE residue class modulo four (rows start
    on 16- and 32-byte multiples), which is what lets k_walk<wave> load its dense tile in aligned words: a rule that allowed
    another residue would need cases of its own, and this test says so"""
    assert WK.BORDERS == (WK.FS_K, WK.WALK_TR, WK.FS_W, WK.WSEG_S * WK.FS_K, WK.FS_W * WK.FS_K)
    assert len(set(WK.BORDERS)) == 5 and all(b % WK.FS_K == 0 for b in WK.BORDERS)
    assert WK.K["PITCH_WINDOW"] % 4 == 0 and WK.K["PITCH_DENSE"] % 4 == 0
    assert WK.K["LONG_LT"] < WK.K["WSEG_MIN_ROWS"]
    assert WE.STRIPE_ROWS[64] == WK.FS_K and WK.WSEG_COLS == WK.WALK_TW


def test_moves_and_features_of_paths_written_by_hand():
    """moves_of and the run / border features on two paths small enough to read"""
    #            0  1  2  3  4  5  6  7  8  9
    pl = np.array([0, 0, 0, 1, 1, 0, 0, 0, 0, 0], np.uint8)
    q = np.array([0, 1, 2, 3, 4, 5, 6, 7, 7, 8], np.int32)
    t = np.array([0, 1, 1, 2, 3, 4, 5, 5, 6, 7], np.int32)
    ed = np.array([0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 0], np.uint8)
    assert WK.moves_of(pl, q, t, ed) == [None, "MAT", "INS", "Q2R", "MAT", "R2Q", "SUB", "INS", "DEL", "MAT"]
    with pytest.raises(AssertionError):
        WK.moves_of(pl[:2], np.array([0, 2], np.int32), t[:2], ed)
    assert WK._groups([None, "a", "a", None, "b"]) == [("a", 1, 2), ("b", 4, 1)]
    # k_walk<wave>, restated: 70 MAT steps are a run of 64 that the lanes cut and one of 6; a lone INS step is single
    n = 80
    mv = [None] + ["MAT"] * 70 + ["INS"] + ["MAT"] * 8
    pl = np.zeros(n, np.uint8)
    q = np.arange(n, dtype=np.int32)
    t = np.concatenate([np.arange(71), np.arange(70, 79)]).astype(np.int32)
    F = WK.wave_trace(mv, pl, q, t, 80, 80, 79)
    assert {("wave_run", "MS", 64), ("wave_run", "MS", 6), ("wave_run_cut", "MS"), ("direct",), ("row_get", "next")} <= F, F
    assert not any(f[0] == "wave_run" and f[1] == "INS" for f in F)


def test_every_required_feature_is_in_a_homozygous_case(feats):
    have = set()
    for c in WK.HOM:
        have |= feats[c.name][0].features
    missing = [r for r in WK.REQUIRED if r not in have]
    assert not missing, missing
    # the rules leave one pitch residue, and the table says so (see test_constants_come_from_the_sources)
    assert {f for f in have if f[0] == "pitch_mod4"} == {("pitch_mod4", "dense", 0), ("pitch_mod4", "window", 0)}
    # the plane lengths cover every residue modulo four at the dense tile's right end, in both planes
    assert {f[2] for f in have if f[0] == "last4" and f[1] == 0} == {0, 1, 2, 3} and {f[2] for f in have if f[0] == "last4" and f[1] == 1} == {0, 1, 2, 3}


def test_every_case_has_the_features_its_name_claims(feats):
    for c in WK.TABLE:
        F = feats[c.name][0].features
        missing = [a for a in c.aims if a not in F]
        assert not missing, (c.name, missing)
    by = {c.name: feats[c.name][0] for c in WK.TABLE}
    lt = lambda name: by[name].lens[2]
    assert 8193 <= lt("long_65_segments") <= 8320 and 2048 <= lt("long_seg_walk") <= 2176 and 1024 <= lt("long_row_walk") <= 1100
    assert WK.K["WSEG_MIN_ROWS"] <= lt("long_seg_walk") and WK.K["LONG_LT"] <= lt("long_row_walk") < WK.K["WSEG_MIN_ROWS"]
    for n in WK.LTS:        # the end cell is the first row behind a border where the length says so
        f = by[f"lt{n}_fp"]
        assert f.lens == (n,) * 5 and ("end_row_mod", tuple(int((n - 1) % b == 0) for b in WK.BORDERS)) in f.features
    for n in WK.RUNS:       # a run case holds ONE run of its kind
        for kind in ("INS", "DEL", "SUB"):
            runs = [x for x in by[f"run_{kind.lower()}{n}"].features if x[0] == "run" and x[1] == kind]
            assert runs == [("run", kind, n)], (kind, n, runs)
            assert by[f"run_{kind.lower()}{n}"].dist == n
    for c in WK.HET:        # the four alignments of a heterozygous case differ
        assert len({(f.dist, len(f.path[0]), f.path[0].tobytes(), f.path[1].tobytes()) for f in feats[c.name]}) >= 2, c.name


def test_every_border_has_every_move_on_both_sides(feats):
    cover = {}
    for c in WK.HOM:
        for f in feats[c.name][0].features:
            if f[0] in ("enter", "ins_row"):
                cover.setdefault(f, []).append(c.name)
    print("border: move: cases whose path enters the first row behind it / the last row in front of it")
    for b in WK.BORDERS:
        for m in WK.ROW_MOVES:
            at, before = cover.get(("enter", b, m, "at"), []), cover.get(("enter", b, m, "before"), [])
            print(f"  {b:4d} {m}: {len(at)} / {len(before)}  e.g. {at[:1]} / {before[:1]}")
            assert at and before, (b, m)
        assert cover.get(("ins_row", b, "before")) and cover.get(("ins_row", b, "after")), b
    # rows 128 and 512 themselves, by the cases named for them
    for b in (WK.WSEG_ROWS, WK.CHUNK_STRIPES):
        for m in WK.ROW_MOVES:
            assert any(n.startswith(f"b{b}_") for n in cover[("enter", b, m, "at")]), (b, m)


def test_the_oracle_reports_no_error_and_paths_cost_their_distance(feats):
    for c in WK.TABLE:
        for k, f in enumerate(feats[c.name]):
            assert not (f.status & ~(A.ST_SWAP_TIE | A.ST_WARN_MASK)), (c.name, k, f.status)
            pl, q, t, sy, ed = f.path
            mv = WK.moves_of(pl, q, t, ed)
            assert sum(m in ("SUB", "INS", "DEL") for m in mv[1:]) == f.dist == int(ed[:len(pl)].sum()), (c.name, k)
            assert (int(pl[0]), int(q[0]), int(t[0])) in ((0, 0, 0), (1, 0, 0)) and int(t[-1]) == f.lens[2 + (k & 1)] - 1
            assert int(q[-1]) == (f.lens[4] if pl[-1] == A.PLANE_REF else f.lens[k >> 1]) - 1, (c.name, k)


def test_the_window_edge_and_fallback_cases_fit_the_level_they_aim_at(feats):
    """what a level must hold of them lies inside its restated windows and not in the level's below (needed_level of
    window_edge_cases.py), so the walks behind that level can meet them: the 64-cell level for the row and segment walks"""
    for c in WK.TABLE:
        if c.family in ("el", "other"):
            _, batch = WK.batch_of([c])
            need = WE.needed_level(batch, 0, 0).level
            assert need == c.we.W if c.we is not None else need <= 64, (c.name, need)
    # a diagonal path that enters a stripe's first row in window column 57 or beyond leaves the window before the stripe ends, so
    # at a segment border the high edge is met in the segment's LAST row and the low edge in its first
    el = {f for c in WK.HOM if c.family == "el" for f in feats[c.name][0].features if f[0] == "el"}
    assert {("el", "first", 0), ("el", "first", 1), ("el", "last", WK.FS_W - 1), ("el", "last", WK.FS_W - 2)} <= el, sorted(el)
