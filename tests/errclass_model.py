"""Brute-force model of the error classes (include/vcfdist_errclass.h) for the tests: the class byte of every hap-variant from the
variant tables, the results and the phasing; the counts by direct enumeration over the thresholds (no fold of a histogram); and
the text of error-classes.tsv / error-classes-summary.tsv."""
import numpy as np

import report_oracle as RO
from vcfdist_amd import _abi as A

NAMES = ["gt", "sync", "phase", "site", "near", "alone", "lowq"]
VARTYPE_STR = ["SNP", "INDEL", "SV", "ALL"]
COLUMNS = ["QUERY_FP"] + ["FP_" + n.upper() for n in NAMES[:6]] + ["TRUTH_FN"] + ["FN_" + n.upper() for n in NAMES]


def phasing(res, pb_phase):
    """the selected phasing of every supercluster: ORIG 0, SWAP 1, NONE pb_phase != 0 (0 without pb_phase)"""
    out = []
    for k, p in enumerate(np.asarray(res.sc_phase).tolist()):
        out.append(0 if p == A.PHASE_ORIG else 1 if p == A.PHASE_SWAP else int(pb_phase is not None and pb_phase[k] != 0))
    return out


def _alt(v, s, u):
    o, n = int(v.var_alt_off[s][u]), int(v.var_alt_len[s][u])
    return bytes(v.allele_pool[s][o:o + n])


def _is_copy(v, s, i, x, u):
    return (v.var_pos[s][i] == v.var_pos[x][u] and v.var_type[s][i] == v.var_type[x][u] and v.var_ref_len[s][i] == v.var_ref_len[x][u]
            and v.var_alt_len[s][i] == v.var_alt_len[x][u] and _alt(v, s, i) == _alt(v, x, u))


def classes(v, res, pb_phase, window):
    """per hap slot the uint8 class (A.EC_*, A.EC_NONE) of every variant"""
    w_of = phasing(res, pb_phase)
    out = [np.full(v.n_vars(s), A.EC_NONE, np.uint8) for s in range(A.HAPS)]
    for s in range(A.HAPS):
        truth = s >= 2
        for sc in range(v.n_sc):
            w = w_of[sc]
            rng = lambda x: range(int(v.var_off[x][sc]), int(v.var_off[x][sc + 1]))
            compared = (s - 2) ^ w if truth else 2 + (s ^ w)
            cross = compared ^ 1
            for i in rng(s):
                e = int(res.errtype[s][w][i])
                if e >= 3:
                    continue
                if e != (A.ERRTYPE_FN if truth else A.ERRTYPE_FP):
                    if truth and e == A.ERRTYPE_TP:
                        out[s][i] = A.EC_LOWQ
                    continue
                pos = int(v.var_pos[s][i])
                others = [(x, u) for x in (compared, cross) for u in rng(x)]
                dist = [abs(int(v.var_pos[x][u]) - pos) for x, u in others]
                if any(_is_copy(v, s, i, s ^ 1, u) and res.errtype[s ^ 1][w][u] == A.ERRTYPE_TP for u in rng(s ^ 1)):
                    c = A.EC_GT
                elif any(_is_copy(v, s, i, compared, u) for u in rng(compared)):
                    c = A.EC_SYNC
                elif any(_is_copy(v, s, i, cross, u) for u in rng(cross)):
                    c = A.EC_PHASE
                elif any(d == 0 for d in dist):
                    c = A.EC_SITE
                elif any(0 < d <= window for d in dist):
                    c = A.EC_NEAR
                else:
                    c = A.EC_ALONE
                out[s][i] = c
    return out


def counts(v, res, pb_phase, cls_bytes, var_class, min_qual=0, max_qual=60):
    """counts [2][4][7][nq]: every classified variant visited at every threshold"""
    nq = max_qual - min_qual + 1
    out = np.zeros((2, 4, A.EC_CLASSES, nq), np.int64)
    w_of = phasing(res, pb_phase)
    for s in range(A.HAPS):
        sc_of = np.repeat(np.arange(v.n_sc), np.diff(v.var_off[s]))
        for i in np.nonzero(cls_bytes[s] != A.EC_NONE)[0].tolist():
            c, t = int(cls_bytes[s][i]), min(int(var_class[s][i]), 2)
            q = np.float32(res.callq[s][w_of[sc_of[i]]][i])
            last = -1 if q < np.float32(min_qual) else min(int(np.floor(q)) - min_qual, nq - 1)      # the last threshold index it passes
            for k in range(nq):
                if s < 2:
                    hit = k <= last
                elif c == A.EC_LOWQ:
                    hit = k > last
                else:
                    hit = True
                if hit:
                    out[s >> 1, t, c, k] += 1
                    out[s >> 1, 3, c, k] += 1
    return out


def tsv_text(class_counts, pr_counts, min_qual=0, max_qual=60):
    """-> (error-classes.tsv text, error-classes-summary.tsv text); BEST is the threshold of precision-recall-summary.tsv"""
    def cells(t, k):
        q, tr = class_counts[0, t, :6, k], class_counts[1, t, :, k]
        return "\t".join(str(int(x)) for x in [q.sum()] + list(q) + [tr.sum()] + list(tr))
    a = ["VAR_TYPE\tMIN_QUAL\t" + "\t".join(COLUMNS) + "\n"]
    for t in range(4):
        for q in range(min_qual, max_qual + 1):
            a.append(f"{VARTYPE_STR[t]}\t{q}\t{cells(t, q - min_qual)}\n")
    s = ["VAR_TYPE\tTHRESHOLD\tMIN_QUAL\t" + "\t".join(COLUMNS) + "\n"]
    for line in RO.precision_recall(pr_counts, min_qual, max_qual)[1].split("\n")[1:-1]:
        name, thr, q = line.split("\t")[:3]
        s.append(f"{name}\t{thr}\t{q}\t{cells(VARTYPE_STR.index(name), int(q) - min_qual)}\n")
    return "".join(a), "".join(s)
