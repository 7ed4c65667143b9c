"""Shared by the reference pins (tests/test_ref_pins.py, tests/test_gpu_ref_pins.py, tests/golden/make_ref_goldens.py): the
case / result files of oracle/_ref/ref_harness, the fixtures under tests/golden/ref/, and "our side" of every comparison.

The harness (oracle/ref_harness.cpp) is the reference's own functions compiled by `make -C oracle ref`; it exists only where the
reference's sources do.  The fixtures hold a case's inputs and what the harness answered; the GPU tests read fixtures only.

Files of the harness: named records, `I <name> <n>` + n integers, `S <name> <n>` + n raw bytes; floats as 32-bit patterns.
Fixtures: compressed npz, `cmd` (the subcommand), `in_I_<name>` / `in_S_<name>` (the case, strings as uint8) and `out_<name>` (the
result), `timeout_s`, and for a refused case `refused` = the harness's last stderr line instead of any `out_`.

Cases
  swg / ed:  pen [x, o, e]; q, t: the pairs' strings concatenated, q_off / t_off their offsets.
             -> score, dist, cigar + cigar_off (swg) per pair.  The CIGAR is the reference's: PTR_MAT 4 / PTR_SUB 8 written TWICE
             per diagonal move (once for the query base, once for the truth base), PTR_INS 1 / PTR_DEL 2 once; in the order of the
             forward strings (the harness reverses the strings before and the CIGAR after, as edits_wrapper does).  The model's
             dm_steps list has one entry per move: steps_from_cigar() drops the second entry of every diagonal pair.
  chain / cluster / realign:  args (the option list, one per line); ctg_names, ctg_seq + ctg_off; query_ctgs / truth_ctgs (the
             contigs each callset's header lists); per hap slot s = 0..3 (query 1, query 2, truth 1, truth 2) the variant table
             v<s>_{ctg, pos, rlen, type, loc, orig_gt, phase_set, var_qual, gt_qual, refs + ref_off, alts + alt_off}, rows grouped by
             contig in ctg_names' order and sorted by position.
             -> c<s>_{off, start, left, right}: clusters per slot (off: per contig);  out_ctgs, sc_off, sc_beg, sc_end, brk<s> +
             brk_off, sc_phase, sc_orig_dist, sc_swap_dist, sc_phase_set, pb_phase, phase_blocks / switches / flips with offsets;
             p<s>_<w>_{errtype, sync_group, callq, ref_ed, query_ed, credit} per variant (rows as the input's) and phasing w;
             with -d ed_{ctg, pos, hap, type, len, sc, min_qual, max_qual}; realign: r<s>_* the realigned tables.
  chain_window_edges also stores x_case_names: the names of its cases in tests/window_edge_cases.py's table, one per line, in the
             order of its contigs (a contig and, with `-c gap 2000`, a supercluster per case).
  cluster_biwfa_edges_* store x_case_names likewise: the names of their cases in tests/wfa_cluster_cases.py's table, a contig per
             case, the case's variants in slot 0."""
import os
import re
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
GOLDEN = os.path.join(HERE, "golden", "ref")
F_INS, F_DEL, F_MAT, F_SUB = 1, 2, 4, 8
TYPE_SUB, TYPE_INS, TYPE_DEL = 1, 2, 3
BED_INSIDE = 1          # the reference's defs.h
GT_ALT1_ALT1 = 5


def have_harness():
    return os.access(HARNESS, os.X_OK)


# ---- harness files

def write_case(path, case):
    with open(path, "wb") as f:
        for name, v in case.items():
            if isinstance(v, (bytes, bytearray)):
                f.write(b"S %s %d\n" % (name.encode(), len(v)) + bytes(v) + b"\n")
            else:
                a = np.asarray(v).astype(np.int64).ravel()
                f.write(b"I %s %d\n" % (name.encode(), len(a)) + " ".join(map(str, a.tolist())).encode() + b"\n")


def read_result(path):
    out = {}
    with open(path, "rb") as f:
        while True:
            head = f.readline().split()
            if not head:
                return out
            assert head[0] == b"I", head
            out[head[1].decode()] = np.array(f.readline().split(), dtype=np.int64)
            assert len(out[head[1].decode()]) == int(head[2]), head


class Refused(Exception):
    """the harness ended with a non-zero status (the reference's ERROR() calls exit) or ran past its time limit"""


def run_harness(cmd, case, timeout=600):
    assert have_harness(), "oracle/_ref/ref_harness is not built (make -C oracle ref)"
    with tempfile.TemporaryDirectory(prefix="ref_pins_") as d:
        cp, rp = os.path.join(d, "case"), os.path.join(d, "result")
        write_case(cp, case)
        try:
            r = subprocess.run([HARNESS, cmd, cp, rp], capture_output=True, timeout=timeout, cwd=d)      # the reference writes phasing-summary.tsv where it runs
        except subprocess.TimeoutExpired:
            raise Refused(f"time limit ({timeout} s)")
        if r.returncode != 0:
            lines = [l for l in r.stderr.decode(errors="replace").strip().split("\n") if "[INFO" not in l]
            msg = lines[-1] if lines else ""
            msg = re.sub(r"^.*?\[(ERROR|WARN)[^\]]*\]\S*\s*", "", msg)        # drop the reference's time stamp
            raise Refused(f"exit {r.returncode}: {msg}")
        return read_result(rp)


# ---- fixtures

def _small(a):
    a = np.asarray(a, np.int64)
    if len(a) == 0 or (a.min() >= 0 and a.max() < 256):
        return a.astype(np.uint8)
    if a.min() >= -2**31 and a.max() < 2**31:
        return a.astype(np.int32)
    return a


def save_fixture(name, cmd, case, out, timeout_s, extra=None):
    d = {"cmd": np.frombuffer(cmd.encode(), np.uint8), "timeout_s": np.int64(timeout_s)}
    for k, v in case.items():
        if isinstance(v, (bytes, bytearray)):
            d["in_S_" + k] = np.frombuffer(bytes(v), np.uint8)
        else:
            d["in_I_" + k] = _small(v)
    if isinstance(out, str):
        d["refused"] = np.frombuffer(out.encode(), np.uint8)
    else:
        for k, v in out.items():
            d["out_" + k] = _small(v)
    for k, v in (extra or {}).items():
        d["x_" + k] = np.asarray(v)
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **d)
    return path


_SURROGATE = {}


def _surrogate(n):
    if n not in _SURROGATE:
        import demo_pipeline
        _SURROGATE[n] = bytes(demo_pipeline.surrogate_fasta(n))
    return _SURROGATE[n]


class Fixture:
    def __init__(self, name):
        self.name = name
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.cmd = bytes(z["cmd"]).decode()
        self.timeout_s = int(z["timeout_s"])
        self.case, self.out, self.extra = {}, {}, {}
        self.refused = bytes(z["refused"]).decode() if "refused" in z.files else None
        for k in z.files:
            if k.startswith("in_S_"):
                self.case[k[5:]] = bytes(z[k])
            elif k.startswith("in_I_"):
                self.case[k[5:]] = z[k].astype(np.int64)
            elif k.startswith("out_"):
                self.out[k[4:]] = z[k].astype(np.int64)
            elif k.startswith("x_"):
                self.extra[k[2:]] = z[k]
        if "surrogate_len" in self.extra:       # the demo's contig: the seeded surrogate FASTA, rebuilt instead of stored
            self.case["ctg_seq"] = _surrogate(int(self.extra["surrogate_len"]))

    def rerun(self):
        """the harness on this fixture's inputs -> result dict, or the refusal's text"""
        try:
            return run_harness(self.cmd, self.case, timeout=self.timeout_s)
        except Refused as e:
            return str(e)


def fixture_names(prefix=""):
    if not os.path.isdir(GOLDEN):
        return []
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f.startswith(prefix))


# ---- swg / ed cases

def pairs_case(pairs, pen=(3, 2, 1)):
    q = [a if isinstance(a, bytes) else a.encode() for a, _ in pairs]
    t = [b if isinstance(b, bytes) else b.encode() for _, b in pairs]
    return {"pen": list(pen), "q": b"".join(q), "q_off": np.cumsum([0] + [len(s) for s in q]), "t": b"".join(t),
            "t_off": np.cumsum([0] + [len(s) for s in t])}


def case_pairs(case):
    qo, to = case["q_off"], case["t_off"]
    return [(case["q"][qo[k]:qo[k + 1]], case["t"][to[k]:to[k + 1]]) for k in range(len(qo) - 1)]


def steps_from_cigar(cigar):
    """the reference's CIGAR (two entries per diagonal move) -> one entry per move, the model's dm_steps list"""
    out, k = [], 0
    cigar = [int(c) for c in cigar]
    while k < len(cigar):
        c = cigar[k]
        if c in (F_MAT, F_SUB):
            assert k + 1 < len(cigar) and cigar[k + 1] == c, f"diagonal move at {k} is not written twice"
            k += 2
        else:
            assert c in (F_INS, F_DEL), c
            k += 1
        out.append(c)
    return out


# ---- chain cases

def empty_slot():
    return dict(ctg=[], pos=[], rlen=[], type=[], ref=[], alt=[], var_qual=[], gt_qual=[], orig_gt=[], phase_set=[], loc=[])


def slot_from_sites(sites):
    """sites: (ctg index, pos, type, ref, alt, qual[, phase_set]) sorted by contig and position"""
    s = empty_slot()
    for site in sites:
        c, p, t, r, a, q = site[:6]
        s["ctg"].append(c); s["pos"].append(p); s["type"].append(t); s["ref"].append(r.encode() if isinstance(r, str) else bytes(r))
        s["alt"].append(a.encode() if isinstance(a, str) else bytes(a)); s["var_qual"].append(q)
        s["phase_set"].append(site[6] if len(site) > 6 else 0)
    return s


def chain_case(contigs, slots, args, query_ctgs=None, truth_ctgs=None):
    """contigs: [(name, bytes)]; slots: four dicts as empty_slot() (rlen, gt_qual, orig_gt, loc optional)"""
    case = {"args": "\n".join(args).encode(), "ctg_names": "\n".join(n for n, _ in contigs).encode(),
            "ctg_seq": b"".join(bytes(s) for _, s in contigs), "ctg_off": np.cumsum([0] + [len(s) for _, s in contigs]),
            "query_ctgs": list(range(len(contigs))) if query_ctgs is None else query_ctgs,
            "truth_ctgs": list(range(len(contigs))) if truth_ctgs is None else truth_ctgs}
    for k, s in enumerate(slots):
        n = len(s["pos"])
        p = f"v{k}_"
        case[p + "ctg"] = s["ctg"]; case[p + "pos"] = s["pos"]; case[p + "type"] = s["type"]
        case[p + "rlen"] = s["rlen"] if len(s.get("rlen", [])) == n and n else [len(r) for r in s["ref"]]
        case[p + "loc"] = s["loc"] if len(s.get("loc", [])) == n and n else [BED_INSIDE] * n
        case[p + "orig_gt"] = s["orig_gt"] if len(s.get("orig_gt", [])) == n and n else [GT_ALT1_ALT1] * n
        case[p + "phase_set"] = s["phase_set"] if len(s.get("phase_set", [])) == n and n else [0] * n
        case[p + "var_qual"] = np.asarray(s["var_qual"], np.float32).view(np.uint32)
        gq = s["gt_qual"] if len(s.get("gt_qual", [])) == n and n else [0.0] * n
        case[p + "gt_qual"] = np.asarray(gq, np.float32).view(np.uint32)
        case[p + "refs"] = b"".join(s["ref"]); case[p + "ref_off"] = np.cumsum([0] + [len(r) for r in s["ref"]])
        case[p + "alts"] = b"".join(s["alt"]); case[p + "alt_off"] = np.cumsum([0] + [len(a) for a in s["alt"]])
    return case


def case_args(case):
    """the options of a chain case as a dict: cluster (method, gap), penalties, max_qual, distance"""
    a = case["args"].decode().split("\n")
    o = dict(cluster=("biwfa", 0), sub=5, open=6, extend=2, eval_sub=3, eval_open=2, eval_extend=1, max_qual=60, distance="-d" in a,
             max_supercluster_size=10000, max_cluster_itrs=4)
    names = {"-x": "sub", "-o": "open", "-e": "extend", "-ex": "eval_sub", "-eo": "eval_open", "-ee": "eval_extend", "-mx": "max_qual",
             "-s": "max_supercluster_size", "-i": "max_cluster_itrs"}
    for k, tok in enumerate(a):
        if tok == "-c":
            o["cluster"] = (a[k + 1], int(a[k + 2]) if a[k + 1] != "biwfa" else 0)
        elif tok in names:
            o[names[tok]] = int(a[k + 1])
    return o


def case_contigs(case):
    names = case["ctg_names"].decode().split("\n") if case["ctg_names"] else []
    off = case["ctg_off"]
    return [(n, case["ctg_seq"][off[k]:off[k + 1]]) for k, n in enumerate(names)]


def case_slot(case, k, ctg):
    """slot k's variants on contig index ctg -> (dict of columns, first row, one past the last row)"""
    p = f"v{k}_"
    rows = np.nonzero(case[p + "ctg"] == ctg)[0]
    a, b = (int(rows[0]), int(rows[-1]) + 1) if len(rows) else (0, 0)
    assert len(rows) == b - a, "a contig's rows are not contiguous"
    ro, ao = case[p + "ref_off"], case[p + "alt_off"]
    return dict(pos=case[p + "pos"][a:b].astype(np.int32), type=case[p + "type"][a:b].astype(np.uint8), rlen=case[p + "rlen"][a:b].astype(np.int32),
                ref=[case[p + "refs"][ro[i]:ro[i + 1]] for i in range(a, b)], alt=[case[p + "alts"][ao[i]:ao[i + 1]] for i in range(a, b)],
                var_qual=case[p + "var_qual"][a:b].astype(np.uint32).view(np.float32), gt_qual=case[p + "gt_qual"][a:b].astype(np.uint32).view(np.float32),
                phase_set=case[p + "phase_set"][a:b].astype(np.int32), orig_gt=case[p + "orig_gt"][a:b].astype(np.uint8)), a, b


def hap_columns(s):
    """a case's slot (ref_pins.case_slot) as the reader's columns that realign_model and api.realign take"""
    pool = b"".join(r + al for r, al in zip(s["ref"], s["alt"]))
    lens = np.array([[len(r), len(al)] for r, al in zip(s["ref"], s["alt"])], np.int64).reshape(-1, 2)
    starts = np.concatenate([[0], np.cumsum(lens.ravel())])[:-1].reshape(-1, 2)
    return dict(s, ref_len=lens[:, 0].astype(np.int32), alt_len=lens[:, 1].astype(np.int32), ref_off=starts[:, 0].astype(np.int64),
                alt_off=starts[:, 1].astype(np.int64), pool=np.frombuffer(pool + b"\0", np.uint8))


def ref_clusters(out, k, ci):
    """the reference's clusters of slot k on the ci-th contig: (starts, left reaches, right reaches)"""
    p = f"c{k}_"
    a, b = int(out[p + "off"][ci]), int(out[p + "off"][ci + 1])
    return out[p + "start"][a:b], out[p + "left"][a:b], out[p + "right"][a:b]


def our_clusters(case, ctg, lib=None, prefix="vco", slots=range(4)):
    """clusters of one contig by oracle/cluster_oracle.cpp + wfa_oracle.cpp (prefix vco, lib = the oracle) or by the host
    cluster.cpp of the library (prefix vcl, simple clustering only) -> (HapSeq list, Clusters list)"""
    from vcfdist_amd import cluster as K
    o = case_args(case)
    seq = case_contigs(case)[ctg][1]
    haps, cl = [], []
    for k in slots:
        s, _, _ = case_slot(case, k, ctg)
        h = K.HapSeq(s["pos"], s["type"], s["ref"], s["alt"])
        haps.append(h)
        method, gap = o["cluster"]
        if method == "biwfa":
            cl.append(K.wfa_cluster(h, bytes(seq), sub=o["sub"], open=o["open"], extend=o["extend"], max_cluster_itrs=o["max_cluster_itrs"],
                                    reach_min_gap=10, L=lib, prefix=prefix)[0])
        else:
            cl.append(K.simple_cluster(h, 1 if method == "size" else 0, gap, 10, L=lib, prefix=prefix))
    return haps, cl


def our_variants(case, ctg, haps, sc):
    """the A.Variants of one contig's superclusters (sc: a cluster.Superclusters, ours or rebuilt from the reference's)"""
    from vcfdist_amd import _abi as A
    seq = np.frombuffer(case_contigs(case)[ctg][1], np.uint8)
    quals = [case_slot(case, k, ctg)[0]["var_qual"] for k in range(4)]
    return A.Variants(np.array([0, len(seq)], np.int64), seq, np.zeros(sc.n, np.int32), sc.beg, sc.end, [sc.var_off(i) for i in range(4)],
                      [h.pos for h in haps], [h.type for h in haps], quals, [h.ref_off for h in haps], [h.ref_len for h in haps],
                      [h.alt_off for h in haps], [h.alt_len for h in haps], [h.pool for h in haps])


PER_VAR = ("errtype", "sync_group", "callq", "ref_ed", "query_ed", "credit")


def ref_per_variant(fx, ctg, ci):
    """the reference's six per-variant columns of contig index ctg: {(name, slot, w): int64 array (floats as bit patterns)}"""
    out = {}
    for k in range(4):
        _, a, b = case_slot(fx.case, k, ctg)
        for w in range(2):
            for name in PER_VAR:
                out[name, k, w] = fx.out[f"p{k}_{w}_{name}"][a:b]
    return out


def results_per_variant(res):
    """an A.Results' six per-variant columns in the same shape"""
    out = {}
    for k in range(4):
        for w in range(2):
            for name in PER_VAR:
                a = np.asarray(getattr(res, name)[k][w])
                out[name, k, w] = (a.view(np.uint32) if a.dtype == np.float32 else a).astype(np.int64)
    return out


def ref_superclusters(fx, ci):
    """the reference's superclusters of the ci-th contig of out_ctgs: dict(beg, end (inclusive, as vpr_variants'), brk, phase, ...)"""
    o = fx.out
    a, b = int(o["sc_off"][ci]), int(o["sc_off"][ci + 1])
    ba, bb = int(o["brk_off"][ci]), int(o["brk_off"][ci + 1])
    return dict(n=b - a, beg=o["sc_beg"][a:b], end=o["sc_end"][a:b], brk=[o[f"brk{k}"][ba:bb] for k in range(4)], sc_phase=o["sc_phase"][a:b],
                orig=o["sc_orig_dist"][a:b], swap=o["sc_swap_dist"][a:b], phase_set=o["sc_phase_set"][a:b], pb_phase=o["pb_phase"][a:b],
                switches=o["switches"][int(o["sw_off"][ci]):int(o["sw_off"][ci + 1])], flips=o["flips"][int(o["fl_off"][ci]):int(o["fl_off"][ci + 1])],
                first=a)


def ref_edits(fx, ctg):
    """the reference's editData records of contig index ctg as the model's rows (sc, hap, pos, type, len, min_qual, max_qual)"""
    o = fx.out
    m = o["ed_ctg"] == ctg
    return np.stack([o["ed_sc"][m], o["ed_hap"][m], o["ed_pos"][m], o["ed_type"][m], o["ed_len"][m], o["ed_min_qual"][m], o["ed_max_qual"][m]], 1)


# ---- fixture-only inputs for the library (no oracle anywhere: the reference's own clusters and superclusters)

def ref_cluster_objects(fx, ctg):
    """the reference's clusters of every slot on contig index ctg as cluster.Clusters (empty for a slot without variants)"""
    from vcfdist_amd import cluster as K
    out = []
    for k in range(4):
        st, le, ri = ref_clusters(fx.out, k, ctg)
        n = len(st)
        le = np.concatenate([le, np.full(n - len(le), K.SENTINEL, np.int64)]) if len(le) < n else le      # wf_swg_cluster keeps no sentinel
        ri = np.concatenate([ri, np.full(n - len(ri), K.SENTINEL, np.int64)]) if len(ri) < n else ri
        out.append(K.Clusters(st, le, ri))
    return out


def ref_variants(fx, ci):
    """the A.Variants of the ci-th contig of out_ctgs built from the fixture alone: the case's tables, the reference's
    superclusters (begs, ends, cluster breaks) and clusters"""
    from vcfdist_amd import _abi as A, cluster as K
    ctg = int(fx.out["out_ctgs"][ci])
    rs = ref_superclusters(fx, ci)
    seq = np.frombuffer(case_contigs(fx.case)[ctg][1], np.uint8)
    haps, quals, var_off = [], [], []
    for k in range(4):
        s, _, _ = case_slot(fx.case, k, ctg)
        haps.append(K.HapSeq(s["pos"], s["type"], s["ref"], s["alt"]))
        quals.append(s["var_qual"])
        starts = ref_clusters(fx.out, k, ctg)[0]
        var_off.append(starts[rs["brk"][k]].astype(np.int64) if len(starts) else np.zeros(rs["n"] + 1, np.int64))
    return A.Variants(np.array([0, len(seq)], np.int64), seq, np.zeros(rs["n"], np.int32), rs["beg"], rs["end"], var_off, [h.pos for h in haps],
                      [h.type for h in haps], quals, [h.ref_off for h in haps], [h.ref_len for h in haps], [h.alt_off for h in haps],
                      [h.alt_len for h in haps], [h.pool for h in haps])


def concat_variants(vs):
    """several one-contig A.Variants as one batch, contigs and superclusters in the given order"""
    from vcfdist_amd import _abi as A
    ctg_off = np.concatenate([[0], np.cumsum([len(v.ctg_seq) for v in vs])]).astype(np.int64)
    cat = lambda arrs, dt: np.concatenate([np.asarray(a, dt) for a in arrs]) if arrs else np.zeros(0, dt)
    var_off, pos, typ, qual, roff, rlen, aoff, alen, pool = [], [], [], [], [], [], [], [], []
    for h in range(4):
        nv = np.concatenate([[0], np.cumsum([v.n_vars(h) for v in vs])])
        pl = np.concatenate([[0], np.cumsum([len(v.allele_pool[h]) for v in vs])])
        var_off.append(np.concatenate([[0]] + [v.var_off[h][1:] + nv[i] for i, v in enumerate(vs)]).astype(np.int64))
        pos.append(cat([v.var_pos[h] for v in vs], np.int32)); typ.append(cat([v.var_type[h] for v in vs], np.uint8))
        qual.append(cat([v.var_qual[h] for v in vs], np.float32))
        roff.append(cat([v.var_ref_off[h] + pl[i] for i, v in enumerate(vs)], np.int64)); rlen.append(cat([v.var_ref_len[h] for v in vs], np.int32))
        aoff.append(cat([v.var_alt_off[h] + pl[i] for i, v in enumerate(vs)], np.int64)); alen.append(cat([v.var_alt_len[h] for v in vs], np.int32))
        pool.append(cat([v.allele_pool[h] for v in vs], np.uint8))
    return A.Variants(ctg_off, cat([v.ctg_seq for v in vs], np.uint8), cat([np.full(v.n_sc, i, np.int32) for i, v in enumerate(vs)], np.int32),
                      cat([v.sc_beg for v in vs], np.int32), cat([v.sc_end for v in vs], np.int32), var_off, pos, typ, qual, roff, rlen, aoff, alen, pool)


def ref_batch(fx):
    """every contig with superclusters as one A.Variants + what the reference answered in the same order:
    -> (variants, dict(sc_phase, orig, swap, per-variant columns {(name, slot, w)}, edits [n, 7] with batch-wide supercluster numbers))"""
    vs, want = [], dict(sc_phase=[], orig=[], swap=[], cols={}, edits=[])
    n_sc = 0
    for ci, ctg in enumerate(fx.out["out_ctgs"].tolist()):
        rs = ref_superclusters(fx, ci)
        if rs["n"] == 0:
            continue
        vs.append(ref_variants(fx, ci))
        for f, key in (("sc_phase", "sc_phase"), ("orig", "orig"), ("swap", "swap")):
            want[f].append(rs[key])
        for key, a in ref_per_variant(fx, ctg, ci).items():
            want["cols"].setdefault(key, []).append(a)
        if "ed_ctg" in fx.out:
            e = ref_edits(fx, ctg)
            e[:, 0] += n_sc
            want["edits"].append(e)
        n_sc += rs["n"]
    if not vs:
        return None, None
    for f in ("sc_phase", "orig", "swap"):
        want[f] = np.concatenate(want[f])
    want["cols"] = {k: np.concatenate(a) for k, a in want["cols"].items()}
    want["edits"] = np.concatenate(want["edits"]) if want["edits"] else np.zeros((0, 7), np.int64)
    return concat_variants(vs), want
