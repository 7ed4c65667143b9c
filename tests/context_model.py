"""Numpy statement of the sequence-context strata (include/vcfdist_context.h) for the tests: per stratum the flags, the runs,
the filter, the padding and the merge, step by step as the header defines them.  The implementation is compared against this
model, never the other way round."""
import numpy as np

import strata_model as M
from vcfdist_amd import _abi as A


def as_bytes(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8)


def called(s):
    return (s == 65) | (s == 67) | (s == 71) | (s == 84)


def runs(flag):
    """maximal runs [a, b) of a bool array"""
    d = np.diff(np.concatenate(([0], flag.astype(np.int8), [0])))
    return np.nonzero(d == 1)[0].astype(np.int64), np.nonzero(d == -1)[0].astype(np.int64)


def period_flags(s, p):
    m = np.zeros(len(s), bool)
    if len(s) > p:
        m[p:] = (s[p:] == s[:-p]) & called(s[p:])
    return m


def period_tracts(s, p, min_len, max_len):
    """the kept tracts [start, stop) of period p: steps 1 - 3"""
    a, b = runs(period_flags(s, p))
    start, stop = a - p, b
    length = stop - start
    keep = length >= min_len
    if max_len:
        keep &= length <= max_len
    for q in range(1, p):                 # primitive: the first p bases are no repetition of a word of length q | p
        if p % q == 0:
            rep = np.ones(len(start), bool)
            for k in range(q, p):
                rep &= s[start + k] == s[start + k - q]
            keep &= ~rep
    return start[keep], stop[keep]


def gc_flags(s, lo, hi, W):
    L = len(s)
    flag = np.zeros(L, bool)
    if L < W:
        return flag
    g = np.concatenate(([0], np.cumsum((s == 71) | (s == 67)))).astype(np.int64)
    n = np.concatenate(([0], np.cumsum(called(s)))).astype(np.int64)
    a = np.arange(0, L - W + 1)           # window starts that lie wholly inside the contig; the window of base a + W // 2
    gw = g[a + W] - g[a]
    flag[a + W // 2] = (n[a + W] - n[a] == W) & (lo * W <= 100 * gw) & (100 * gw < hi * W)
    return flag


def pad_merge(start, stop, slop, L):
    """steps 4 and 5: pad, clip, and merge what overlaps or abuts"""
    if len(start) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    ps, pe = np.maximum(0, start - slop), np.minimum(L, stop + slop)
    top = np.maximum.accumulate(pe)
    first = np.ones(len(ps), bool)
    first[1:] = ps[1:] > top[:-1]
    last = np.concatenate((first[1:], [True]))
    return ps[first].astype(np.int32), top[last].astype(np.int32)


def intervals(s, spec):
    """the sorted, merged intervals of one stratum on one contig"""
    s = as_bytes(s) if not isinstance(s, np.ndarray) else s
    if spec.kind == A.CTX_PERIOD:
        start, stop = period_tracts(s, spec.period, spec.min_len, spec.max_len)
    else:
        start, stop = runs(gc_flags(s, spec.gc_lo, spec.gc_hi, spec.window))
    return pad_merge(start, stop, spec.slop, len(s))


def all_intervals(contigs, specs):
    """rows[spec][contig] = (starts, stops), the layout of api.PrecisionRecall.download_context_intervals"""
    contigs = [as_bytes(c) if not isinstance(c, np.ndarray) else c for c in contigs]
    return [[intervals(c, sp) for c in contigs] for sp in specs]


def contigs_of(v):
    """the contig sequences of an A.Variants"""
    return [np.asarray(v.ctg_seq[int(v.ctg_off[c]):int(v.ctg_off[c + 1])], np.uint8) for c in range(len(v.ctg_off) - 1)]


def bed_rows(rows_of_spec, ctg_names):
    """one stratum's model intervals as BED rows (contig, start, stop)"""
    return [(ctg_names[c], int(a), int(b)) for c, (st, sp) in enumerate(rows_of_spec) for a, b in zip(st, sp)]


def write_model_strata(tmp, names, ctg_names, rows, list_name="context.tsv"):
    """the model's intervals as BEDs plus a strata list (strata_model.write_strata), so that strata_model.locations / words_of /
    expected_counts are reused as they are -> (path of the list, [(name, bed rows)])"""
    strata = [(n, bed_rows(r, ctg_names)) for n, r in zip(names, rows)]
    return M.write_strata(tmp, strata, list_name), strata


def context_bed_text(names, ctg_names, rows):
    """context-strata.bed: by contig, then by stratum in table order, then by start"""
    out = []
    for c, cn in enumerate(ctg_names):
        for n, r in zip(names, rows):
            out += [f"{cn}\t{int(a)}\t{int(b)}\t{n}\n" for a, b in zip(*r[c])]
    return "".join(out)


def same(got, want):
    """the list of (spec, contig) rows in which two results of the layout above differ"""
    return [(k, c) for k in range(len(want)) for c in range(len(want[k]))
            if not (np.array_equal(got[k][c][0], want[k][c][0]) and np.array_equal(got[k][c][1], want[k][c][1]))]
