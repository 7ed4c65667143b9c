"""Model of the bootstrap replicates of the precision/recall counters (include/vcfdist_bootstrap.h) for the tests: the
definition in numpy.  The hash in uint64, the weight table, a weighted histogram from downloaded results, the fold of a
histogram into counters, the float32 metrics, the percentile pick and both writers."""
import decimal

import numpy as np

from vcfdist_amd import _abi as A

M64 = (1 << 64) - 1
T = np.array(A.BOOT_T, np.uint64)
VARTYPE_STR = ("SNP", "INDEL", "SV", "ALL")
SUM_HEADER = "VAR_TYPE\tTHRESHOLD\tMIN_QUAL\tREPLICATES\tSEED\tPREC\tPREC_LO\tPREC_HI\tRECALL\tRECALL_LO\tRECALL_HI\tF1_SCORE\tF1_LO\tF1_HI\n"
REP_HEADER = "REPLICATE\tVAR_TYPE\tTHRESHOLD\tMIN_QUAL\tTRUTH_TP\tQUERY_TP\tTRUTH_FN\tQUERY_FP\tPREC\tRECALL\tF1_SCORE\n"


def table_from_cdf():
    """T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!) in 60-digit decimal arithmetic"""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        e1, acc, fact, out = decimal.Decimal(-1).exp(), decimal.Decimal(0), decimal.Decimal(1), []
        for k in range(A.BOOT_MAX_WEIGHT):
            if k:
                fact *= k
            acc += e1 / fact
            out.append(int((acc * (1 << 32)).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    return out


def draw(seed, r, key):
    """u(seed, r, key), 32 bits; r and key broadcast against each other"""
    r, key = np.asarray(r, np.uint64), np.asarray(key, np.uint64)
    salt = np.uint64((int(seed) * 0xD1B54A32D192ED03) & M64)
    with np.errstate(over="ignore"):
        z = key + np.uint64(0x9E3779B97F4A7C15) * (r + np.uint64(1)) + salt
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def weight_of_draw(u):
    """w = number of k with u >= T[k]"""
    return (np.asarray(u, np.uint64)[..., None] >= T).sum(axis=-1).astype(np.int64)


def weights(seed, n_rep, keys):
    """int64 [n_rep, len(keys)]"""
    return weight_of_draw(draw(seed, np.arange(n_rep, dtype=np.uint64)[:, None], np.asarray(keys, np.uint64)[None, :]))


def variant_bins(var_off, res, cls, pb, min_qual=0, max_qual=60, member=None):
    """per hap slot (supercluster of every counted variant, its bin of the histogram [3 classes][3][nq + 1]): the variants
    k_pr_hist counts, in the columns (ORIG / SWAP) it reads; member[slot]: bool per variant (a stratum), or None"""
    nq = max_qual - min_qual + 1
    out = []
    for s in range(A.HAPS):
        off = np.asarray(var_off[s], np.int64)
        sc = np.repeat(np.arange(len(off) - 1), np.diff(off))
        ph = np.asarray(res.sc_phase)[sc]
        swap = np.where(ph == A.PHASE_ORIG, 0, np.where(ph == A.PHASE_SWAP, 1, (np.asarray(pb)[sc] != 0).astype(np.int64)))
        e = np.where(swap == 1, res.errtype[s][1], res.errtype[s][0]).astype(np.int64)
        q = np.where(swap == 1, res.callq[s][1], res.callq[s][0]).astype(np.float32)
        b = np.where(q < np.float32(min_qual), nq, np.minimum(np.floor(q).astype(np.int64) - min_qual, nq - 1))
        t = np.minimum(np.asarray(cls[s], np.int64), 2)
        keep = e < 3
        if member is not None:
            keep &= np.asarray(member[s], bool)
        out.append((sc[keep], ((t * 3 + e) * (nq + 1) + b)[keep]))
    return out


def fold(hist, nq):
    """pr_fold_counts: histogram [2][3][3][nq + 1] -> counts [2][4][3][nq]"""
    hist = np.asarray(hist, np.int64).reshape(2, 3, 3, nq + 1)
    counts = np.zeros((2, 4, 3, nq), np.int64)
    at_or_above = np.cumsum(hist[..., :nq][..., ::-1], axis=-1)[..., ::-1]       # variants whose last threshold index is >= k
    counts[:, :3] += at_or_above
    own = hist.sum(axis=2)                                                        # [2][3][nq + 1]: any errtype
    below = own[1, :, nq:nq + 1] + np.concatenate([np.zeros((3, 1), np.int64), np.cumsum(own[1, :, :nq - 1], axis=-1)], axis=-1)
    counts[1, :3, A.ERRTYPE_FN] += below                                          # truth variants below threshold k: FN there
    counts[:, 3] = counts[:, :3].sum(axis=1)
    return counts


def expected_counts(var_off, res, cls, pb, keys, seed, n_rep, min_qual=0, max_qual=60, member=None):
    """counts [n_rep][2][4][3][nq] of the definition"""
    nq = max_qual - min_qual + 1
    nb = 9 * (nq + 1)
    w = weights(seed, n_rep, keys)
    bins = variant_bins(var_off, res, cls, pb, min_qual, max_qual, member)
    out = np.zeros((n_rep, 2, 4, 3, nq), np.int64)
    for r in range(n_rep):
        hist = np.zeros((2, nb), np.int64)
        for s, (sc, b) in enumerate(bins):
            hist[s >> 1] += np.bincount(b, weights=w[r][sc], minlength=nb).astype(np.int64)
        out[r] = fold(hist, nq)
    return out


def metrics(counts, t, k):
    """(truth_tp, query_tp, truth_fn, query_fp, precision, recall, f1) of report.cpp's metrics(): float32 arithmetic"""
    f = np.float32
    qtp, qfp, ttp, tfn = (int(counts[0, t, 0, k]), int(counts[0, t, 1, k]), int(counts[1, t, 0, k]), int(counts[1, t, 2, k]))
    p = f(1) if qtp + qfp == 0 else f(qtp) / f(qtp + qfp)
    r = f(1) if ttp + tfn == 0 else f(ttp) / f(ttp + tfn)
    f1 = f(2) * p * r / (p + r) if p + r > 0 else f(0)
    return ttp, qtp, tfn, qfp, f(p), f(r), f(f1)


def best_qual(counts, t, min_qual, max_qual):
    best, bq = np.float32(0), 0
    for q in range(min_qual, max_qual + 1):
        f1 = metrics(counts, t, q - min_qual)[6]
        if f1 > best:
            best, bq = f1, q
    return bq if min_qual <= bq <= max_qual else min_qual


def pick(n_rep):
    """indices of LO and HI in the ascending replicates: floor(0.025 n), ceil(0.975 n) - 1"""
    return n_rep // 40, (39 * n_rep + 39) // 40 - 1


def summary_rows(counts, counts_boot, seed, min_qual, max_qual, lead=""):
    n_rep = len(counts_boot)
    lo, hi = pick(n_rep)
    rows, quals = [], []
    for t in range(4):
        quals.append((min_qual, best_qual(counts, t, min_qual, max_qual)))
        for name, q in zip(("NONE", "BEST"), quals[t]):
            m = metrics(counts, t, q - min_qual)
            reps = np.array([metrics(c, t, q - min_qual)[4:] for c in counts_boot], np.float32)
            x = np.sort(reps, axis=0)
            cols = [v for j in range(3) for v in (m[4 + j], x[lo, j], x[hi, j])]
            rows.append(f"{lead}{VARTYPE_STR[t]}\t{name}\t{q}\t{n_rep}\t{int(seed)}\t" + "\t".join("%f" % float(v) for v in cols) + "\n")
    return rows, quals


def bootstrap_files(counts, counts_boot, seed, min_qual, max_qual):
    """(bootstrap-precision-recall-summary.tsv, bootstrap-replicates.tsv) as text"""
    rows, quals = summary_rows(counts, counts_boot, seed, min_qual, max_qual)
    rep = [REP_HEADER]
    for r, c in enumerate(counts_boot):
        for t in range(4):
            for name, q in zip(("NONE", "BEST"), quals[t]):
                m = metrics(c, t, q - min_qual)
                rep.append(f"{r}\t{VARTYPE_STR[t]}\t{name}\t{q}\t{m[0]}\t{m[1]}\t{m[2]}\t{m[3]}\t" + "\t".join("%f" % float(v) for v in m[4:]) + "\n")
    return SUM_HEADER + "".join(rows), "".join(rep)


def stratified_file(names, counts, counts_boot, seed, min_qual, max_qual):
    """stratified-bootstrap-precision-recall-summary.tsv as text"""
    out = ["STRATUM\t" + SUM_HEADER]
    for k, name in enumerate(names):
        out += summary_rows(counts[k], counts_boot[k], seed, min_qual, max_qual, lead=name + "\t")[0]
    return "".join(out)
