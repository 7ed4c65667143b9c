"""Minimal alignments aimed at the places where the walks of the window and dense levels change state, for pinning their PATHS on
the oracle's, entry for entry (k_walk_rows / walk_rows_range, the segment walk k_wseg_plan / map / compose / emit, k_walk<wave>,
k_walk<lane>; pr_band.hip, pr_walkseg.hip, pr_kernels.hip).

A one-off error at a chunk border of one of these kernels gives a path that is still a valid alignment of the same cost and, on
random input, usually the same credits: only the path shows it.  So every case here is one supercluster built from a variant list
on a random contig, as short as its feature allows, and what a case HAS is computed from the oracle's path, never declared:

  moves_of()      every step's move (MAT, SUB, INS, DEL, R2Q: swap REF -> QUERY, Q2R: swap QUERY -> REF) from the five path arrays
  features_of()   the feature set of one alignment, from its moves: the move that enters the rows at and in front of every border
                  (8: stripe, 32: the LDS tile of k_walk<wave>, 64: the row-constant chunk, 128: a segment, 512: 64 stripes), INS
                  runs in the rows beside a border, maximal run lengths, what ended a REF-plane run, where the sync points lie in a
                  run, the window column at the 128-row borders and the REF column's offset at a swap REF -> QUERY (with the
                  restated stripe_origin of window_edge_cases.py), the plane sizes and pitch residues -- and wave_trace(): the control
                  flow of k_walk<wave> on dense rows restated over the moves (which runs it takes, of which length, when row_get
                  skips a chunk, when col_get re-centres, when the tile is staged at a plane's right end and with which `keep` mask).

The constants 8, 16, 32, 64, 128, 256 are read out of the sources (FS_K, WSEG_S, WALK_TR, FS_W, WSEG_ROWS, WALK_TW / WSEG_COLS) and
so are the two pitch rules: a changed constant moves the borders the table is checked against.

It imports no product code beyond _abi (and oracle_lib, and the restated origins of window_edge_cases.py);
tests/test_walk_edge_cases.py shows on the CPU that the table is what it claims, tests/test_gpu_walk_edges.py runs it through the
kernels."""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

import oracle_lib as O
import window_edge_cases as WE
from vcfdist_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vcfdist_amd", "csrc")
_BASES = np.frombuffer(b"ACGT", np.uint8)
PAD = 30                # contig bases outside the region, on either side (0 on a side the case cuts at the contig's end)


# ----------------------------------------------------------------------------------------------------------------------
# constants and rules, read out of the sources
# ----------------------------------------------------------------------------------------------------------------------
def _constants():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("pr_band.hip", "pr_walkseg.hip", "pr_kernels.hip", "pr_device.h", "pr_api.hip", "pr_host.h")}

    def define(f, name):
        return int(re.search(r"#define %s (\d+)\b" % name, src[f]).group(1))

    c = dict(FS_K=define("pr_band.hip", "FS_K"), FS_W=define("pr_band.hip", "FS_W"), WSEG_S=define("pr_walkseg.hip", "WSEG_S"),
             WSEG_COLS=define("pr_walkseg.hip", "WSEG_COLS"), WALK_TR=define("pr_kernels.hip", "WALK_TR"), WALK_TW=define("pr_kernels.hip", "WALK_TW"))
    assert re.search(r"#define WSEG_ROWS \(WSEG_S \* FS_K\)", src["pr_walkseg.hip"])
    c["WSEG_ROWS"] = c["WSEG_S"] * c["FS_K"]
    # the pitch rules: window rows (window_layout, pr_device.h) and dense rows (the dense plan, pr_api.hip)
    m = [re.search(r"d\.pitch\[%d\] = int32_t\(round_up64\(W < d\.L%s \? W : d\.L%s, (\d+)\)\);" % (p, x, x), src["pr_device.h"]) for p, x in ((0, "q"), (1, "r"))]
    assert m[0] and m[1] and m[0].group(1) == m[1].group(1)
    c["PITCH_WINDOW"] = int(m[0].group(1))
    m = re.search(r"d\.pitch\[0\] = int32_t\(round_up\(d\.Lq, (\d+)\)\); d\.pitch\[1\] = int32_t\(round_up\(d\.Lr, (\d+)\)\);", src["pr_api.hip"])
    assert m and m.group(1) == m.group(2)
    c["PITCH_DENSE"] = int(m.group(1))
    c["LONG_LT"] = int(re.search(r"const int LONG_LT = (\d+);", src["pr_host.h"]).group(1))
    c["WSEG_MIN_ROWS"] = int(re.search(r'exp_getenv\("VPR_WSEG_MIN_ROWS"\); return e \? atoi\(e\) : (\d+); \}', src["pr_api.hip"]).group(1))
    # the launch size from which the wider levels walk a lane per alignment (enqueue_part, walk_launch's callers)
    m = re.search(r"const bool wave_walk = !q16 && \(long_part \|\| cnt < (\d+)\);", src["pr_api.hip"])
    c["LANE_WALK_MIN"] = int(m.group(1))
    return c


K = _constants()
FS_K, FS_W, WSEG_S, WSEG_ROWS, WSEG_COLS, WALK_TR, WALK_TW = (K[n] for n in ("FS_K", "FS_W", "WSEG_S", "WSEG_ROWS", "WSEG_COLS", "WALK_TR", "WALK_TW"))
CHUNK_STRIPES = FS_W * FS_K          # 64 stripes: the origin chunk of walk_rows_range
BORDERS = (FS_K, WALK_TR, FS_W, WSEG_ROWS, CHUNK_STRIPES)      # 8, 32, 64, 128, 512
ROW_MOVES = ("MAT", "SUB", "DEL", "R2Q", "Q2R")               # the moves that enter a row (an INS step stays in its row)


def pitches(Lq, Lr, W=None):
    """-> (pitch of the QUERY plane's rows, of the REF plane's): dense rows (W None) or the rows of a window of W cells"""
    up = lambda x, m: -(-x // m) * m
    if W is None:
        return up(Lq, K["PITCH_DENSE"]), up(Lr, K["PITCH_DENSE"])
    return up(min(W, Lq), K["PITCH_WINDOW"]), up(min(W, Lr), K["PITCH_WINDOW"])


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
# A variant is ("S", pos[, k]) | ("I", pos, n | -n | bases) | ("D", pos, n); pos counts from the region's first base.  A SNP's alternate
# base is the reference base rotated by k (1..3) in ACGT (1 when left out: the same k on two haplotypes is a shared SNP).  An
# insertion of -n is n times a base that is neither neighbour's, so that no other placement of it costs the same.
# q / t: the variants of the query's / the truth's first haplotype; q2 / t2: of the second (None: homozygous, four identical
# alignments); edit: [(pos, bytes)] written into the contig before the variants are read off it (N, lower case);
# ends: "" | "begin" | "end": the region begins / ends with the contig; we: a case of window_edge_cases.py, built by that module;
# aims: the features (features_of) the case is there for -- the CPU test asserts that it has them
Case = namedtuple("Case", "name family L q t q2 t2 edit ends we aims")
Built = namedtuple("Built", "case contig sc")


def _case(name, family, L, q=(), t=(), q2=None, t2=None, edit=(), ends="", we=None, aims=()):
    return Case(name, family, L, tuple(q), tuple(t), None if q2 is None else tuple(q2), None if t2 is None else tuple(t2), tuple(edit), ends, we,
                tuple(aims))


def is_het(case):
    return case.q2 is not None or case.t2 is not None or (case.we is not None and case.we.het)


def _variants(rng, contig, beg, specs):
    out = []
    for s in sorted(specs, key=lambda s: s[1]):
        p = beg + s[1]
        if s[0] == "S":
            k = s[2] if len(s) > 2 else 1
            up = contig[p] & 0xdf
            alt = "ACGT"[(b"ACGT".index(up) + k) % 4] if up in b"ACGT" else "ACGT"[k]
            out.append((p, A.TYPE_SUB, chr(contig[p]), alt, 30.0))
        elif s[0] == "I":
            if isinstance(s[2], str):
                alt = s[2]
            elif s[2] > 0:
                alt = bytes(rng.choice(_BASES, s[2])).decode()
            else:
                alt = chr([c for c in b"ACGT" if c not in (contig[p - 1] & 0xdf, contig[p] & 0xdf)][0]) * -s[2]
            out.append((p, A.TYPE_INS, "", alt, 30.0))
        else:
            out.append((p, A.TYPE_DEL, bytes(contig[p:p + s[2]]).decode(), "", 30.0))
    return out


def build(case, ctg=0):
    """-> Built: contig and supercluster of one case, reproducible from its name; the region holds case.L reference bases"""
    if case.we is not None:
        b = WE.build(case.we, ctg=ctg)
        return Built(case, b.contig, b.sc)
    rng = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7fffffff)
    front, back = (0 if case.ends == "begin" else PAD), (0 if case.ends == "end" else PAD)
    contig = bytearray(rng.choice(_BASES, front + case.L + back).tobytes())
    for pos, b in case.edit:
        contig[front + pos:front + pos + len(b)] = b
    vs = [_variants(rng, contig, front, v) for v in (case.q, case.q if case.q2 is None else case.q2, case.t, case.t if case.t2 is None else case.t2)]
    return Built(case, contig.decode(), dict(ctg=ctg, beg=front, end=front + case.L - 1, vars=vs))        # (end: inclusive)


def batch_of(cases, repeat=1):
    """one batch, a contig and a supercluster per case (the whole list `repeat` times over) -> (Variants, Batch)"""
    built = [build(c, ctg=i) for i, c in enumerate(cases)]
    contigs, scs = [b.contig for b in built], []
    for _ in range(repeat):
        scs += [b.sc for b in built]
    v = A.Variants.from_sites(contigs, scs)
    return v, O.generate(v)


# ----------------------------------------------------------------------------------------------------------------------
# moves and features
# ----------------------------------------------------------------------------------------------------------------------
def moves_of(pl, qri, ti, edit):
    """-> [None, move entering entry 1, ...]: "MAT" | "SUB" | "INS" | "DEL" | "R2Q" | "Q2R" """
    out = [None]
    for i in range(1, len(pl)):
        dq, dt = int(qri[i]) - int(qri[i - 1]), int(ti[i]) - int(ti[i - 1])
        if pl[i] != pl[i - 1]:
            assert dt == 1, i
            out.append("R2Q" if pl[i - 1] == A.PLANE_REF else "Q2R")
        elif (dq, dt) == (1, 1):
            out.append("SUB" if edit[i] else "MAT")
        elif (dq, dt) == (1, 0):
            out.append("INS")
        elif (dq, dt) == (0, 1):
            out.append("DEL")
        else:
            raise AssertionError(f"entry {i}: no move goes from ({pl[i - 1]}, {qri[i - 1]}, {ti[i - 1]}) to ({pl[i]}, {qri[i]}, {ti[i]})")
    return out


def _groups(keys):
    """maximal stretches of equal non-None keys -> [(key, first index, length)]"""
    out, i = [], 0
    while i < len(keys):
        j = i
        while j < len(keys) and keys[j] == keys[i]:
            j += 1
        if keys[i] is not None:
            out.append((keys[i], i, j - i))
        i = j
    return out


def wave_trace(mv, pl, qri, ti, Lq, Lr, Lt):
    """k_walk<wave> on DENSE rows (band_mode 0), its control flow restated over the oracle's moves -> set of features:
      ("wave_run", kind, n)       a run of n steps taken at once (kind "MS": MAT / SUB down a diagonal, "INS", "DEL"; n in 2 .. 64)
      ("wave_run_cut", kind)      a run of 64 steps that the 64 lanes cut: the stretch goes on
      ("wave_run_end", kind, k)   a run whose last entry is k entries in front of the path's last (k = 0: it ends on the end cell)
      ("row_get", "next"|"skip")  a single step's row lies in the next chunk of 64 rows / beyond it ("a diagonal run skipped a chunk")
      ("col_get", "recentre")     a single step's column lies outside the 64 columns held (after the first load)
      ("direct",)                 a single step read its byte from the matrix (singles < 4 and outside the tile)
      ("tile", c0 % 4 ...)        see below: a tile staged, where it lies and which `keep` masks it used
      ("tile_rows",)              a tile left through its last row (WALK_TR rows further down)
      ("last4", plane, L % 4)     a single step read its byte out of the tile from one of the plane's last four columns"""
    F = set()
    Lp = (Lq, Lr)
    n_mv = len(mv)
    i = 1                   # the next move
    skip, last, singles = 0, None, 0
    rbase, cbase = 0, [-(1 << 30), -(1 << 30)]
    tile_t0, tile_c0 = -(1 << 30), [0, 0]
    CH = FS_W

    def col_get(p, x):
        if x < cbase[p] or x >= cbase[p] + CH:
            if cbase[p] > -(1 << 30):
                F.add(("col_get", "recentre"))
            cbase[p] = max(0, x - 8)

    while i < n_mv:
        hi, x, t = int(pl[i - 1]), int(qri[i - 1]), int(ti[i - 1])
        lim_i, lim_d = min(Lp[hi] - 1 - x, CH), min(Lt - 1 - t, CH)
        lim = min(lim_i, lim_d)
        if skip > 0:
            skip -= 1
        elif last in ("INS", "DEL"):
            run = 0
            if (lim_i if last == "INS" else lim_d) >= 2:
                while run < CH and i + run < n_mv and mv[i + run] == last:
                    run += 1
            if run >= 2:
                F.add(("wave_run", last, run))
                if run == CH and i + run < n_mv and mv[i + run] == last:
                    F.add(("wave_run_cut", last))        # 64 lanes: the stretch goes on behind the run
                if n_mv - (i + run) <= 1:
                    F.add(("wave_run_end", last, n_mv - (i + run)))
                i += run
                singles = 0
                continue
            skip = 3
        elif lim >= 2:
            run = 0
            while run < CH and i + run < n_mv and mv[i + run] in ("MAT", "SUB"):
                run += 1
            if run >= 2:
                F.add(("wave_run", "MS", run))
                if run == CH and i + run < n_mv and mv[i + run] in ("MAT", "SUB"):
                    F.add(("wave_run_cut", "MS"))
                if n_mv - (i + run) <= 1:
                    F.add(("wave_run_end", "MS", n_mv - (i + run)))
                i += run
                singles = 0
                continue
            skip = 3
        # a single step from (hi, x, t): where its byte comes from
        r0 = t - tile_t0
        inside = 0 <= r0 < WALK_TR and 0 <= x - tile_c0[hi] < WALK_TW
        if not inside and singles < 4:
            F.add(("direct",))
        else:
            if not inside:
                if 0 <= x - tile_c0[hi] < WALK_TW and r0 >= WALK_TR and tile_t0 >= 0:
                    F.add(("tile_rows",))
                tile_t0 = t
                col_get(hi, x)
                for p in range(2):
                    # (the other plane's tile lies around the position the walk's maps to: not restated, no step reads it
                    # before the tile is staged again around a position of that plane)
                    if p != hi:
                        continue
                    wdt = Lp[p]
                    c0 = max(0, min(x - CH, wdt - (WALK_TW - 4))) & ~3       # (the pitch is a multiple of four: the aligned-word tile)
                    tile_c0[p] = c0
                    if c0 + WALK_TW >= wdt and wdt % 4:
                        F.add(("keep", p, wdt % 4))          # the word over the plane's last column is masked
                    F.add(("tile", p, "right" if c0 + WALK_TW >= wdt else "inner"))
            if x >= Lp[hi] - 4:
                F.add(("last4", hi, Lp[hi] % 4))
        m = mv[i]
        last = m
        singles += 1
        i += 1
        hi, x, t = int(pl[i - 1]), int(qri[i - 1]), int(ti[i - 1])
        if t >= rbase + CH:
            if t < rbase + 2 * CH:
                F.add(("row_get", "next"))
                rbase += CH
            else:
                F.add(("row_get", "skip"))
                rbase = t & ~(CH - 1)
        col_get(hi, x)
    return F


def features_of(batch, sc, aln, path):
    """-> the feature set of alignment `aln` of supercluster `sc` from the oracle's path arrays (see the module's text)"""
    pl, qri, ti, sync, edit = path
    mv = moves_of(pl, qri, ti, edit)
    q2r, t2r, tflag, r2q, Lq, Lr, Lt = WE.arrays_of(batch, sc, aln)
    loQ, loR = WE.origins(FS_W, t2r, WE.tj_of(t2r, tflag), r2q, Lq, Lr)       # stripe_origin, restated
    lo = (loQ, loR)
    F = {("Lq", Lq), ("Lr", Lr), ("Lt", Lt)}
    F |= {("pitch_mod4", "dense", p % 4) for p in pitches(Lq, Lr)} | {("pitch_mod4", "window", p % 4) for W in WE.LEVELS[1:] for p in pitches(Lq, Lr, W)}
    n_seg = -(-(-(-Lt // FS_K)) // WSEG_S)
    F |= {("segments", n_seg), ("last_seg_rows", Lt - (n_seg - 1) * WSEG_ROWS), ("end_row_mod", tuple(int((Lt - 1) % b == 0) for b in BORDERS))}
    F.add(("end_plane", int(pl[-1])))
    ins_rows = {int(ti[i]) for i in range(1, len(mv)) if mv[i] == "INS"}
    for i in range(1, len(mv)):
        m, b = mv[i], int(ti[i])
        if m == "INS":
            continue
        for kind in BORDERS:
            if b % kind == 0:
                F.add(("enter", kind, m, "at"))                 # the first row behind a border
                if b - 1 in ins_rows:
                    F.add(("ins_row", kind, "before"))
                if b in ins_rows:
                    F.add(("ins_row", kind, "after"))
            if (b + 1) % kind == 0:
                F.add(("enter", kind, m, "before"))             # the last row in front of one
        if b % WSEG_ROWS == 0:
            p0, p1 = int(pl[i - 1]), int(pl[i])
            F.add(("el", "first", int(qri[i]) - int(lo[p1][b // FS_K])))              # window column of the cell entered
            F.add(("el", "last", int(qri[i - 1]) - int(lo[p0][(b - 1) // FS_K])))     # ... of the cell left, in the segment's last row
        if m == "R2Q":          # the REF column the walk leaves, from the origin of its segment's first row (k_wseg_map's cb[1])
            t0 = (int(ti[i - 1]) // WSEG_ROWS) * WSEG_ROWS
            off = int(qri[i - 1]) - int(loR[t0 // FS_K])
            F.add(("r2q_off", off))
            if off < 0 or off >= WSEG_COLS:
                F.add(("other_fallback", "r2q"))
        if m == "Q2R":
            t0 = (int(ti[i - 1]) // WSEG_ROWS) * WSEG_ROWS
            off = int(qri[i - 1]) - int(loQ[t0 // FS_K])
            if off < 0 or off >= WSEG_COLS:
                F.add(("other_fallback", "q2r"))
    # a diagonal step out of a window's LAST column in a stripe's last row, at every window level: the cell it enters lies in the
    # next stripe's window alone (the backward sweeps take that cell's constants from the stripe above)
    tj = WE.tj_of(t2r, tflag)
    for W in WE.LEVELS:
        KW = WE.STRIPE_ROWS[W]
        loW = WE.origins(W, t2r, tj, r2q, Lq, Lr)
        for i in range(1, len(mv)):
            t = int(ti[i - 1])
            if mv[i] in ("MAT", "SUB") and (t + 1) % KW == 0 and int(qri[i - 1]) - int(loW[int(pl[i])][t // KW]) == W - 1:
                F.add(("edge_last_row", W, int(pl[i])))
    # runs: MAT / SUB mixed down one diagonal, pure SUB, INS, DEL
    ms = _groups([("MS" if m in ("MAT", "SUB") else None) for m in mv])
    for kind, groups in (("MS", ms), ("SUB", _groups([m if m == "SUB" else None for m in mv])),
                         ("INS", _groups([m if m == "INS" else None for m in mv])), ("DEL", _groups([m if m == "DEL" else None for m in mv]))):
        for _, first, n in groups:
            F.add(("run", kind, n))
            if len(mv) - (first + n) <= 1 and n >= 2:
                F.add(("run_end", kind, len(mv) - (first + n)))
    for k, (_, first, n) in enumerate(ms):
        nxt = mv[first + n] if first + n < len(mv) else None
        if pl[first] == A.PLANE_REF and nxt == "R2Q":
            F.add(("ref_run_swap", min(n, 2)))          # a run on the REF plane that a cell offering a swap ended (2: of two steps or more)
        if n >= 2 * FS_W and k + 1 < len(ms) and ms[k + 1][1] == first + n + 1 and ms[k + 1][2] >= 2:
            F.add(("long_run_single_run", nxt))
        if n >= 2:
            s = [int(x) for x in sync[first:first + n]]
            if not any(s):
                F.add(("sync", "none"))
            for where, v in (("first", s[0]), ("last", s[-1])) + tuple(("inner", x) for x in s[1:-1]):
                F.add(("sync" if v else "nosync", where))
            if "".join(map(str, s)).strip("0").count("0"):
                F.add(("sync101",))             # ones, then a stretch of zeros, then ones again: a variant's bases or an ins_loc position inside the run
    return F | wave_trace(mv, pl, qri, ti, Lq, Lr, Lt)


Feat = namedtuple("Feat", "features path dist status lens")


def feat_of(batch, sc, aln):
    ex = O.Extra(batch, want=(sc, aln))
    res = O.run(batch, extra=ex)
    path = tuple(np.array(a) for a in ex.path_arrays())
    return Feat(frozenset(features_of(batch, sc, aln, path)), path, int(res.aln_dist[4 * sc + aln]), int(res.aln_status[4 * sc + aln]), tuple(batch.lens(sc)))


def _feats_of(case):
    _, batch = batch_of([case])
    # (a homozygous case's four alignments are the same problem four times)
    return case.name, [feat_of(batch, 0, aln) for aln in ((0, 1, 2, 3) if is_het(case) else (0,))]


_FEATS = {}


def feats(cases):
    """{case name: [Feat per alignment]} (one entry for a homozygous case), computed once per process, on up to eight cores"""
    todo = [c for c in cases if c.name not in _FEATS]
    if todo:
        import multiprocessing
        import sys
        n = max(1, min(8, len(os.sched_getaffinity(0)), len(todo) // 4))
        if not os.path.exists(getattr(sys.modules.get("__main__"), "__file__", None) or ""):
            n = 1           # (a spawned worker re-imports __main__: not from a script read from standard input)
        if n > 1:
            O.lib()         # (built once, in the parent)
            # (fresh interpreters, not forks: the GPU tests call this from a process that has the device open); the costly cases first
            todo.sort(key=lambda c: -c.L)
            with multiprocessing.get_context("spawn").Pool(n) as pool:
                _FEATS.update(pool.map(_feats_of, todo, chunksize=1))
        else:
            _FEATS.update(map(_feats_of, todo))
    return {c.name: _FEATS[c.name] for c in cases}


def path_of(case, feats_of_case, aln):
    """the oracle's path of alignment aln of a case"""
    return feats_of_case[aln if is_het(case) else 0].path


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
LTS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
RUNS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 300)
PLANES = (1, 2, 3, 4, 5, 251, 252, 253, 255, 256, 257, 260)
LEAD = 20               # bases in front of a run case's variant, and behind it


def _stutter(last, n=6):
    """truth-only insertions of one base (neither neighbour's) in front of each of the n reference bases up to `last`: DEL and MAT
    steps in turn, single steps that no run takes, into the plane's last columns"""
    return [("I", last - j, -1) for j in range(n)]


def _hp(pos, n):
    """-> edit: the n bases from pos on are A, between a G and a T: a truth-only deletion of them is n INS steps in one row, n
    truth-only SNPs A -> C on them are n SUB steps, and no other alignment costs as little"""
    return (pos - 1, b"G" + b"A" * n + b"T")


def _table():
    out = []
    c = lambda *a, **k: out.append(_case(*a, **k))
    # ---- 1. truth rows: the end cell is the first row of a new stripe, tile, chunk or segment at 9, 33, 65, 129, 257, 513
    for n in LTS:
        c(f"lt{n}_fp", "rows", n, q=[("S", n // 2 if n >= 3 else n - 1)], aims=[("Lt", n)])
        if n >= 3:      # (one row: no last row but one; two rows: a variant on the region's first base is no legal input)
            c(f"lt{n}_snp", "rows", n, t=[("S", n - 2)], aims=[("Lt", n), ("run", "SUB", 1)])
    # ---- 2. long alignments: 65 segments (the second register chunk of k_wseg_compose), and one on either side of the row count
    # from which round 0's long part takes the segment walk
    spread = lambda L: ([("S", 100)], [("S", L // 8)], [("D", L // 4, 5)], [("D", 3 * L // 8, 3)], [("I", 5 * L // 8, -4)], [("I", 3 * L // 4, 2)], [("S", L - 100)])
    for name, L, aims in (("long_65_segments", 8200, [("segments", 65)]), ("long_seg_walk", 2100, [("segments", 17)]), ("long_row_walk", 1060, [("segments", 9)])):
        t_snp, sh_snp, q_del, t_del, t_ins, sh_ins, t_snp2 = spread(L)
        sh = [("I", sh_ins[0][1], "GT")]
        c(name, "long", L, q=sh_snp + q_del + sh, t=t_snp + sh_snp + t_del + t_ins + sh + t_snp2, aims=aims)
    # ---- 3. moves that enter the rows at the 128- and the 512-row border (both are stripe, tile and chunk borders too)
    for b in (WSEG_ROWS, CHUNK_STRIPES):
        L = b + LEAD
        c(f"b{b}_mat", "border", L, t=[("S", 5)], aims=[("enter", b, "MAT", "at"), ("enter", b, "MAT", "before")])
        c(f"b{b}_sub_at", "border", L, t=[("S", b)], aims=[("enter", b, "SUB", "at")])
        c(f"b{b}_sub_before", "border", L, t=[("S", b - 1)], aims=[("enter", b, "SUB", "before")])
        c(f"b{b}_del", "border", L, t=[("I", b - 2, -4)], aims=[("enter", b, "DEL", "at"), ("enter", b, "DEL", "before")])
        # a query-only SNP: the walk changes to the REF plane for its base and back behind it
        for d, aims in ((2, [("enter", b, "R2Q", "before")]), (1, [("enter", b, "R2Q", "at"), ("enter", b, "Q2R", "before")]), (0, [("enter", b, "Q2R", "at")])):
            c(f"b{b}_fp{d}_shared_behind", "border", L, q=[("S", b - d), ("S", b + 5, 2)], t=[("S", b + 5, 2)], aims=aims)
            c(f"b{b}_shared_fp{d}_behind", "border", L, q=[("S", b - 8, 2), ("S", b - d)], t=[("S", b - 8, 2)], aims=aims)
        c(f"b{b}_ins_before", "border", L + 3, t=[("D", b, 3)], edit=[_hp(b, 3)], aims=[("ins_row", b, "before")])
        c(f"b{b}_ins_after", "border", L + 3, t=[("D", b + 1, 3)], edit=[_hp(b + 1, 3)], aims=[("ins_row", b, "after")])
    # ---- 4. runs: truth-only deletions (INS), truth-only insertions (DEL), adjacent truth-only SNPs (SUB)
    # (k_walk<wave> takes four single steps before it tries an INS or DEL run: lengths 6 and 68 are its runs of 2 and of 64)
    for n in RUNS + (6, FS_W + 4):
        c(f"run_ins{n}", "runs", 2 * LEAD + n, t=[("D", LEAD, n)], edit=[_hp(LEAD, n)], aims=[("run", "INS", n)])
        c(f"run_del{n}", "runs", 2 * LEAD, t=[("I", LEAD, -n)], aims=[("run", "DEL", n)])
        c(f"run_sub{n}", "runs", 2 * LEAD + n, t=[("S", LEAD + j) for j in range(n)], edit=[_hp(LEAD, n)], aims=[("run", "SUB", n)])
    # a diagonal run of 128 rows or more, exactly one single step, another run: row_get's skipped chunk
    c("run_mat200_ins1_run", "runs", 260, t=[("D", 200, 1)], edit=[_hp(200, 1)], aims=[("long_run_single_run", "INS"), ("row_get", "skip")])
    c("run_mat200_del1_run", "runs", 260, t=[("I", 200, -1)], aims=[("long_run_single_run", "DEL"), ("row_get", "skip")])
    c("run_mat200_fp_run", "runs", 260, q=[("S", 200)], aims=[("row_get", "skip")])
    c("run_mat100_ins1_run", "runs", 160, t=[("D", 100, 1)], edit=[_hp(100, 1)], aims=[("row_get", "next")])
    # runs that end one entry in front of the end cell (a variant on the region's last base is no legal input: the end cell itself
    # ends the diagonal run of every case)
    # ... but where the contig ends with the region a deletion may take its last bases: INS steps in the LAST row, onto the end cell
    # (k_wseg_map's end test stands behind its INS loop), and a walk that ends on the REF plane
    c("run_ins3_end0", "runs", 30, t=[("D", 27, 3)], ends="end", aims=[("run_end", "INS", 0), ("end_plane", 0)])
    c("run_ref3_end0", "runs", 30, q=[("D", 27, 3)], t=[("S", 10)], ends="end", aims=[("run_end", "MS", 0), ("end_plane", 1)])
    c("run_ins5_end1", "runs", 30, t=[("D", 24, 5)], edit=[(23, b"G" + b"A" * 5)], aims=[("run_end", "INS", 1)])
    c("run_del5_end1", "runs", 30, t=[("I", 29, -5)], aims=[("run_end", "DEL", 1)])
    c("run_sub5_end1", "runs", 30, t=[("S", 24 + j) for j in range(5)], edit=[(23, b"G" + b"A" * 5)], aims=[("run_end", "SUB", 1), ("run_end", "MS", 0)])
    # a REF-plane run under a query-only deletion, ended by the first cell that offers a swap
    c("run_ref30_swap", "runs", 70, q=[("D", LEAD, 30)], aims=[("ref_run_swap", 2)])
    # ... and by a cell that offers the swap AND carries MAT (a query-only SNP right behind the deletion: staying on the REF plane is
    # optimal too, the walk's priority takes the swap): what a diagonal run of k_walk<wave> without its swap test runs through
    c("run_ref10_swap_and_mat", "runs", 60, q=[("D", LEAD, 10), ("S", LEAD + 10)], aims=[("ref_run_swap", 2)])
    c("run_ref1_swap", "runs", 40, q=[("D", LEAD, 2)], aims=[("ref_run_swap", 1)])
    # sync flags 1, 0, 1 inside a diagonal run: across a shared variant's bases, and across an ins_loc position
    c("sync_shared_ins3", "runs", 60, q=[("I", 30, "ACG")], t=[("I", 30, "ACG")], aims=[("nosync", "inner"), ("sync101",)])
    c("sync_shared_del3", "runs", 60, q=[("D", 30, 3)], t=[("D", 30, 3)], aims=[("sync", "inner")])
    c("sync_shared_ins1", "runs", 60, q=[("I", 30, "C")], t=[("I", 30, "C")], aims=[("sync101",)])
    c("sync_truth_ins_query_ref", "runs", 60, q=[("S", 10)], t=[("I", 30, -2)], aims=[("nosync", "last")])
    # ---- 5. the edge of the 64-cell window at a segment border: the tandem tract of window_edge_cases.py across row 128
    for u, sign, lead, aims in ((29, -1, 60, [("el", "first", 0)]), (28, -1, 60, [("el", "first", 1)]),
                                (27, 1, 60, [("el", "last", FS_W - 1), ("edge_last_row", 64, 0)]), (26, 1, 60, [("el", "last", FS_W - 2)])):
        c(f"el_u{u}{'+' if sign > 0 else '-'}", "el", 0, we=WE._case("shift", 64, u, sign, lead=lead, reps=4), aims=aims)
    # the same high edge at the other window levels: the path's cell in a stripe's LAST row lies in the window's last column and its
    # diagonal successor, the first base of the query's insertion, in the next stripe's window alone (unit W / 2 - 5; the tract
    # ends on a stripe border: lead + reps * u is a multiple of the level's stripe rows)
    for W, lead in ((16, 42), (256, 47), (1024, 47)):
        u = W // 2 - 5 if W > 16 else 5
        c(f"el_w{W}_u{u}+", "el", 0, we=WE._case("shift", W, u, 1, lead=lead), aims=[("edge_last_row", W, 0)])
    # ---- 6. the other() fallback of k_wseg_map: a swap REF -> QUERY from a REF column 256 or more past the segment's first-row origin
    for off in (WSEG_COLS - 1, WSEG_COLS, WSEG_COLS + 44):
        n = off - 25            # a deletion both callsets share, on a stripe border (inside a stripe no 64-cell window holds both its sides), then a query-only SNP on REF column `off`, then a shared SNP
        c(f"other_off{off}", "other", off + 40, q=[("D", FS_K, n), ("S", off), ("S", off + 10, 2)], t=[("D", FS_K, n), ("S", off + 10, 2)],
          aims=[("r2q_off", off)] + ([("other_fallback", "r2q")] if off >= WSEG_COLS else []))
    # ---- 7. plane sizes for the dense tile of k_walk<wave>: single steps into the plane's last four columns
    for n in PLANES:
        if n <= 5:
            c(f"plane{n}", "planes", n, t=[("S", n - 2)] if n >= 3 else [], aims=[("Lq", n), ("Lr", n)])
        else:
            c(f"plane{n}", "planes", n, t=_stutter(n - 1), aims=[("Lq", n), ("Lr", n), ("last4", 0, n % 4)] + ([("keep", 0, n % 4)] if n % 4 else []))
    # single steps over more rows than the tile holds: it is left through its last row
    c("plane_tile_rows", "planes", 70, t=_stutter(60, WALK_TR + 8), aims=[("tile_rows",)])
    for k in (1, 2, 3):         # Lq = Lr + k: the QUERY plane alone changes its residue
        c(f"plane256_q+{k}", "planes", 256, q=[("I", 10, k)], t=_stutter(255), aims=[("Lq", 256 + k), ("Lr", 256), ("last4", 0, k), ("keep", 0, k)])
    # the REF plane's last columns: a query-only deletion of all but the region's last base, the same single steps under it
    for n in (253, 254, 255, 256):
        c(f"plane{n}_ref", "planes", n, q=[("D", n - 16, 15)], t=_stutter(n - 2), aims=[("Lr", n), ("last4", 1, n % 4)] + ([("keep", 1, n % 4)] if n % 4 else []))
    # ---- 8. variations
    c("het_b128_sub", "het", WSEG_ROWS + LEAD, q=[("S", 60)], q2=[], t=[("S", WSEG_ROWS)], t2=[("S", WSEG_ROWS - 1)])
    c("het_ins64_del65", "het", 2 * LEAD + 64, q=[], q2=[("S", 10)], t=[("D", LEAD, 64)], t2=[("I", LEAD, -65)])
    c("het_other_off300", "het", 340, q=[("D", FS_K, 275), ("S", 300), ("S", 310, 2)], q2=[("D", FS_K, 275)], t=[("D", FS_K, 275), ("S", 310, 2)], t2=[("S", 310, 2)])
    c("het_plane253", "het", 253, q=[("I", 10, 2)], q2=[], t=_stutter(252), t2=[("S", 250)])
    c("n_and_lower_case", "variation", 150, q=[("S", 129), ("S", 135, 2)], t=[("S", 40), ("S", 135, 2), ("D", 100, 2)],
      edit=[(38, b"acgNtn"), (98, b"NNac"), (126, b"gtN")], aims=[("enter", WSEG_ROWS, "R2Q", "at")])
    c("contig_begin", "variation", 140, q=[("S", 1)], t=[("S", 2), ("D", 100, 2)], ends="begin")
    c("contig_end", "variation", 140, q=[("S", 138)], t=[("S", 137), ("D", 100, 2)], ends="end")
    return out


TABLE = _table()
HOM = [c for c in TABLE if not is_het(c)]
HET = [c for c in TABLE if is_het(c)]

# what the table must hold, in homozygous cases alone (tests/test_walk_edge_cases.py)
REQUIRED = (
    [("Lt", n) for n in LTS] + [("segments", 65), ("last_seg_rows", 1)]
    + [("enter", b, m, side) for b in BORDERS for m in ROW_MOVES for side in ("at", "before")]
    + [("ins_row", b, side) for b in BORDERS for side in ("before", "after")]
    + [("run", kind, n) for kind in ("INS", "DEL", "SUB") for n in RUNS]
    + [("wave_run", kind, n) for kind in ("MS", "INS", "DEL") for n in (2, FS_W)] + [("wave_run_cut", kind) for kind in ("MS", "INS", "DEL")]
    + [("long_run_single_run", "INS"), ("long_run_single_run", "DEL"), ("row_get", "next"), ("row_get", "skip"), ("col_get", "recentre"), ("direct",),
       ("tile", 0, "right"), ("tile", 0, "inner"), ("tile", 1, "right"), ("tile_rows",)]
    + [("run_end", "INS", 0), ("end_plane", 0), ("end_plane", 1)]
    + [("run_end", "MS", 0), ("run_end", "INS", 1), ("run_end", "DEL", 1), ("run_end", "SUB", 1), ("ref_run_swap", 1), ("ref_run_swap", 2)]
    + [("sync", w) for w in ("first", "inner", "last", "none")] + [("nosync", w) for w in ("first", "inner", "last")] + [("sync101",)]
    + [("el", "first", 0), ("el", "first", 1), ("el", "last", FS_W - 1), ("el", "last", FS_W - 2)]
    + [("r2q_off", WSEG_COLS - 1), ("r2q_off", WSEG_COLS), ("other_fallback", "r2q")]
    + [("edge_last_row", W, 0) for W in WE.LEVELS]
    + [("Lq", n) for n in PLANES] + [("Lr", n) for n in PLANES] + [("keep", 0, r) for r in (1, 2, 3)] + [("last4", 0, r) for r in (0, 1, 2, 3)]
    + [("keep", 1, r) for r in (1, 2, 3)] + [("last4", 1, r) for r in (1, 2, 3)]
)
