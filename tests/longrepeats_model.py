"""The definition of the long repeat strata (include/vcfdist_longrepeats.h) stated over Python bytes, for the tests: for every valid
start min(k-mer, reverse complement) -- bytes compare as strings over A < C < G < T -- into a dictionary of counts, then the tracts,
padding and merge of tests/repeats_model.py.  Any k >= 4 is accepted, so that the model can be held against repeats_model at
k <= 32.  The implementation is compared against this model, never the other way round."""
import numpy as np

import context_model as CM
import repeats_model as RM

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def canon_of_starts(s, k):
    """steps 1 and 2 for one contig: {start: canon} of the valid starts"""
    s = bytes(s)
    out = {}
    bad = np.concatenate(([0], np.cumsum(~CM.called(np.frombuffer(s, np.uint8))))).astype(np.int64)
    for i in range(len(s) - k + 1):
        if bad[i + k] == bad[i]:
            w = s[i:i + k]
            out[i] = min(w, revcomp(w))
    return out


def repeated(contigs, k):
    """step 3 for the genome: per contig the bool array rep[L], and (valid starts, repeated starts) of the genome"""
    assert k >= 4
    canon = [canon_of_starts(bytes(CM.as_bytes(c)) if not isinstance(c, np.ndarray) else c.tobytes(), k) for c in contigs]
    count = {}
    for d in canon:
        for w in d.values():
            count[w] = count.get(w, 0) + 1
    out, n_valid, n_rep = [], 0, 0
    for c, d in zip(contigs, canon):
        rep = np.zeros(len(c), bool)
        for i, w in d.items():
            rep[i] = count[w] > 1
        out.append(rep)
        n_valid += len(d); n_rep += int(rep.sum())
    return out, n_valid, n_rep


def all_intervals(contigs, specs):
    """rows[spec][contig] = (starts, stops), the layout of api.PrecisionRecall.download_longrepeat_intervals, and the stats
    (n_valid[spec], n_repeated[spec]) of api.PrecisionRecall.longrepeat_stats"""
    rows, n_valid, n_rep, memo = [], [], [], {}
    for sp in specs:
        if sp.k not in memo:
            memo[sp.k] = repeated(contigs, sp.k)
        reps, nv, nr = memo[sp.k]
        rows.append([RM.intervals_of(r, sp.k, sp.slop) for r in reps])
        n_valid.append(nv); n_rep.append(nr)
    return rows, np.array(n_valid, np.int64), np.array(n_rep, np.int64)


long_repeat_bed_text = CM.context_bed_text       # long-repeat-strata.bed has the format and order of context-strata.bed
bed_rows = CM.bed_rows
write_model_strata = CM.write_model_strata
same = CM.same
