"""Model of the label counts cut by stratum and resampled (include/vcfdist_errclass.h, "Cut by stratum and resampled") for the
tests, in terms of the models the label passes already have: a cut masks the label bytes and calls errclass_model.counts /
matchkind_model.counts; a replicate is the sum of w x counts(bytes masked to the superclusters of weight w) over w = 1..12.  No new
brute force.  `fast` holds the same sums taken from one call of the pass model per labelled variant (counts are additive over
variants), which tests/test_labelcut_model.py holds to the literal statement; the GPU tests use it where the literal one would take minutes.  The
percentile pick and the text of the six files are here too."""
import types

import numpy as np

import bootstrap_model as BM
import errclass_model as EM
import matchkind_model as MM
import report_oracle as RO
from vcfdist_amd import _abi as A

NONE = 255
VARTYPE_STR = ("SNP", "INDEL", "SV", "ALL")

# a label pass: its model's counts, the number of labels, the columns of its tables (label index lists per callset), the
# errtype column of the counters each callset's labels sum to, and the files' stem
ERRCLASS = types.SimpleNamespace(name="errclass", counts=EM.counts, labels=A.EC_CLASSES, columns=EM.COLUMNS, query=list(range(6)), truth=list(range(7)),
                                 sums=(A.ERRTYPE_FP, A.ERRTYPE_FN), stem="error-classes", tsv_text=EM.tsv_text)
MATCHKIND = types.SimpleNamespace(name="matchkind", counts=MM.counts, labels=A.MK_KINDS, columns=MM.COLUMNS, query=list(range(4)), truth=list(range(4)),
                                  sums=(A.ERRTYPE_TP, A.ERRTYPE_TP), stem="match-kinds", tsv_text=MM.tsv_text)
PASSES = {"errclass": ERRCLASS, "matchkind": MATCHKIND}


def member_of(words, k):
    """per hap slot the bool membership of stratum k in words[slot] (uint64 [n_words, n_var])"""
    return [((np.asarray(w, np.uint64)[k >> 6] >> np.uint64(k & 63)) & np.uint64(1)).astype(bool) for w in words]


def masked(bytes_, member):
    """the label bytes with "no label" wherever member[slot] is False"""
    return [np.where(np.asarray(m, bool), b, NONE).astype(np.uint8) for b, m in zip(bytes_, member)]


def strata_counts(P, v, res, pb, bytes_, cls, words, n_strata, min_qual=0, max_qual=60):
    """counts [n_strata][2][4][L][nq]: C_P(bytes masked by stratum k)"""
    return np.stack([P.counts(v, res, pb, masked(bytes_, member_of(words, k)), cls, min_qual, max_qual) for k in range(n_strata)])


def sc_member(v, on):
    """per hap slot the bool array of the variants whose supercluster is in the bool array `on`"""
    return [np.repeat(np.asarray(on, bool), np.diff(v.var_off[s])) for s in range(A.HAPS)]


def boot_counts(P, v, res, pb, bytes_, cls, keys, seed, n_rep, min_qual=0, max_qual=60, member=None):
    """counts [n_rep][2][4][L][nq], literally: sum over w = 1..12 of w x C_P(bytes masked to the superclusters of weight w)"""
    if member is not None:
        bytes_ = masked(bytes_, member)
    w = BM.weights(seed, n_rep, keys)
    out = np.zeros((n_rep, 2, 4, P.labels, max_qual - min_qual + 1), np.int64)
    for r in range(n_rep):
        for x in range(1, A.BOOT_MAX_WEIGHT + 1):
            if (w[r] == x).any():
                out[r] += x * P.counts(v, res, pb, masked(bytes_, sc_member(v, w[r] == x)), cls, min_qual, max_qual)
    return out


class fast:
    """The same sums from one table taken once per (bytes, range): counts are additive over variants, so every labelled variant is
    given to the pass model's counts() ALONE, which yields its one row (callset, type, label) and the thresholds it counts at; a
    stratum's counts are the rows of its members added up, a replicate's the rows times the weight of their superclusters."""

    def __init__(self, P, v, res, pb, bytes_, cls, min_qual=0, max_qual=60):
        self.P, self.nq = P, max_qual - min_qual + 1
        slot, idx, sc_of, cell, rows = [], [], [], [], []
        for s in range(A.HAPS):
            scs = np.repeat(np.arange(v.n_sc), np.diff(v.var_off[s]))
            for i in np.nonzero(np.asarray(bytes_[s]) != NONE)[0].tolist():
                sc = int(scs[i])
                sub = types.SimpleNamespace(n_sc=1, var_off=[np.array([0, int(x == s)], np.int64) for x in range(A.HAPS)])
                r1 = types.SimpleNamespace(sc_phase=np.asarray(res.sc_phase)[sc:sc + 1],
                                           callq=[[res.callq[x][w][i:i + 1] if x == s else np.zeros(0, np.float32) for w in range(2)] for x in range(A.HAPS)])
                one = [np.asarray(bytes_[x])[i:i + 1] if x == s else np.zeros(0, np.uint8) for x in range(A.HAPS)]
                c1 = [np.asarray(cls[x])[i:i + 1] if x == s else np.zeros(0, np.uint8) for x in range(A.HAPS)]
                c = P.counts(sub, r1, None if pb is None else np.asarray(pb)[sc:sc + 1], one, c1, min_qual, max_qual)
                hit = np.argwhere(c[:, :3].any(-1))
                assert len(hit) <= 1
                if len(hit):                                      # (none: it counts at no threshold)
                    cs, t, lab = (int(x) for x in hit[0])
                    assert cs == s >> 1 and lab == int(bytes_[s][i]) and np.array_equal(c[cs, 3, lab], c[cs, t, lab]) and c.sum() == 2 * c[cs, t, lab].sum()
                    cell.append((cs * 3 + t) * P.labels + lab)
                    rows.append(c[cs, t, lab])
                    slot.append(s); idx.append(i); sc_of.append(sc)
        self.slot, self.idx, self.sc = (np.array(x, np.int64) for x in (slot, idx, sc_of))
        self.rows = np.array(rows, np.int64).reshape(len(rows), self.nq)
        self.onehot = np.zeros((len(rows), 6 * P.labels), np.int64)
        self.onehot[np.arange(len(rows)), np.array(cell, np.int64)] = 1

    def weighted(self, weight):
        """counts [2][4][L][nq] with variant j of the table counted weight[j] times"""
        c = ((self.onehot * np.asarray(weight, np.int64)[:, None]).T @ self.rows).reshape(2, 3, self.P.labels, self.nq)
        return np.concatenate([c, c.sum(1, keepdims=True)], axis=1)

    def members(self, member):
        return np.array([bool(member[s][i]) for s, i in zip(self.slot.tolist(), self.idx.tolist())], bool).reshape(len(self.slot))

    def total(self):
        return self.weighted(np.ones(len(self.slot), np.int64))

    def strata_counts(self, words, n_strata):
        return np.stack([self.weighted(self.members(member_of(words, k))) for k in range(n_strata)])

    def boot_counts(self, keys, seed, n_rep, member=None):
        w = BM.weights(seed, n_rep, keys)[:, self.sc] if len(self.sc) else np.zeros((n_rep, 0), np.int64)
        if member is not None:
            w = w * self.members(member)[None, :]
        c = np.zeros((n_rep, 6 * self.P.labels, self.nq), np.int64)      # weighted() for every replicate at once, cell by cell
        for g in np.nonzero(self.onehot.any(0))[0].tolist():
            of_g = self.onehot[:, g] == 1
            c[:, g] = w[:, of_g] @ self.rows[of_g]
        c = c.reshape(n_rep, 2, 3, self.P.labels, self.nq)
        return np.concatenate([c, c.sum(2, keepdims=True)], axis=2)


def pick(n_rep):
    """indices of LO and HI in the ascending replicate counts: floor(0.025 n), ceil(0.975 n) - 1"""
    return n_rep // 40, -(-39 * n_rep // 40) - 1


# ---- the text of the files

def _cells(P, c, t, k):
    q, tr = c[0, t, P.query, k], c[1, t, P.truth, k]
    return [int(q.sum())] + [int(x) for x in q] + [int(tr.sum())] + [int(x) for x in tr]


def _summary_rows(pr_counts, min_qual, max_qual):
    """(VAR_TYPE, THRESHOLD, quality) of the rows of precision-recall-summary.tsv of these counters"""
    return [tuple(line.split("\t")[:3]) for line in RO.precision_recall(pr_counts, min_qual, max_qual)[1].split("\n")[1:-1]]


def stratified_text(P, names, label_counts, pr_counts_strata, min_qual=0, max_qual=60):
    """-> (stratified-<stem>.tsv, stratified-<stem>-summary.tsv): the pass's two tables once per stratum behind STRATUM"""
    a, s = [], []
    for k, name in enumerate(names):
        one, summ = P.tsv_text(label_counts[k], pr_counts_strata[k], min_qual, max_qual)
        for out, text in ((a, one), (s, summ)):
            lines = text.split("\n")[:-1]
            if k == 0:
                out.append("STRATUM\t" + lines[0] + "\n")
            out += [f"{name}\t{l}\n" for l in lines[1:]]
    return "".join(a), "".join(s)


def bootstrap_text(P, label_counts, pr_counts, label_boot, min_qual=0, max_qual=60):
    """-> bootstrap-<stem>-summary.tsv: the summary table's rows, every count column followed by its _LO and _HI"""
    n_rep = len(label_boot)
    lo, hi = pick(n_rep)
    out = ["VAR_TYPE\tTHRESHOLD\tMIN_QUAL\t" + "\t".join(f"{c}\t{c}_LO\t{c}_HI" for c in P.columns) + "\n"]
    for name, thr, q in _summary_rows(pr_counts, min_qual, max_qual):
        t, k = VARTYPE_STR.index(name), int(q) - min_qual
        point = _cells(P, label_counts, t, k)
        x = np.sort(np.array([_cells(P, c, t, k) for c in label_boot], np.int64), axis=0)
        out.append(f"{name}\t{thr}\t{q}\t" + "\t".join(f"{p}\t{int(x[lo, j])}\t{int(x[hi, j])}" for j, p in enumerate(point)) + "\n")
    return "".join(out)
