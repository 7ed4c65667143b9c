"""Numpy statement of the repeat strata (include/vcfdist_repeats.h) for the tests: valid starts, canonical codes, repeated starts,
tracts, padding and merge, step by step as the header defines them.  The implementation is compared against this model, never
the other way round.  Vectorised: k rounds of shift-or over uint64 arrays, then one np.unique over the genome's valid starts."""
import numpy as np

import context_model as CM

as_bytes = CM.as_bytes


def codes(s):
    """A 0, C 1, G 2, T 3 (anything else 0: such a base makes its starts invalid)"""
    c = np.zeros(len(s), np.uint64)
    for b, v in ((67, 1), (71, 2), (84, 3)):
        c[s == b] = v
    return c


def starts(s, k):
    """steps 1 and 2 for one contig: (valid[L] bool, canon[L] uint64; canon is meaningless where valid is False)"""
    L = len(s)
    valid, canon = np.zeros(L, bool), np.zeros(L, np.uint64)
    n = L - k + 1                                      # starts with i + k <= L
    if n <= 0:
        return valid, canon
    bad = np.concatenate(([0], np.cumsum(~CM.called(s)))).astype(np.int64)
    valid[:n] = bad[k:k + n] - bad[:n] == 0
    c = codes(s)
    fwd, rc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + n]                            # the first base ends up most significant
        rc |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    canon[:n] = np.minimum(fwd, rc)
    return valid, canon


def repeated(contigs, k):
    """step 3 for the genome: per contig the bool array rep[L], and (valid starts, repeated starts) of the genome"""
    contigs = [as_bytes(c) if not isinstance(c, np.ndarray) else c for c in contigs]
    vc = [starts(c, k) for c in contigs]
    keys = np.concatenate([c[v] for v, c in vc]) if vc else np.zeros(0, np.uint64)
    _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    rep_valid = counts[inverse] > 1 if len(keys) else np.zeros(0, bool)
    out, at = [], 0
    for v, _ in vc:
        rep = np.zeros(len(v), bool)
        n = int(v.sum())
        rep[v] = rep_valid[at:at + n]
        at += n
        out.append(rep)
    return out, len(keys), int(rep_valid.sum())


def intervals_of(rep, k, slop):
    """steps 4 and 5 for one contig"""
    a, b = CM.runs(rep)
    return CM.pad_merge(a, b - 1 + k, slop, len(rep))


def all_intervals(contigs, specs):
    """rows[spec][contig] = (starts, stops), the layout of api.PrecisionRecall.download_repeat_intervals, and the stats
    (n_valid[spec], n_repeated[spec]) of api.PrecisionRecall.repeat_stats"""
    rows, n_valid, n_rep = [], [], []
    memo = {}
    for sp in specs:
        if sp.k not in memo:
            memo[sp.k] = repeated(contigs, sp.k)
        reps, nv, nr = memo[sp.k]
        rows.append([intervals_of(r, sp.k, sp.slop) for r in reps])
        n_valid.append(nv); n_rep.append(nr)
    return rows, np.array(n_valid, np.int64), np.array(n_rep, np.int64)


repeat_bed_text = CM.context_bed_text            # repeat-strata.bed has the format and order of context-strata.bed
bed_rows = CM.bed_rows
write_model_strata = CM.write_model_strata
same = CM.same
