"""Numpy statement of the near-repeat strata (include/vcfdist_nearrepeats.h) for the tests.  The implementation is compared against
this model, never the other way round.

The definition.  Genome, called bases, codes and valid starts are those of repeats_model (vcfdist_repeats.h, steps 1 and 2).
F(c, i) is the forward 2-bit code of the k-mer at a valid start, RC(c, i) the code of its reverse complement, ham(a, b) the number
of the k base positions at which two codes differ.  A near-repeat stratum is (k, m, slop) with 0 <= m <= 3, 8 (m + 1) <= k <= 32
and slop >= 0.
  1. near(c, i) holds iff the start is valid and some OTHER valid start (c', i') != (c, i), on any contig, has
     min(ham(F(c, i), F(c', i')), ham(F(c, i), RC(c', i'))) <= m.  A start is never its own partner (a k-mer within m of its own
     reverse complement that occurs once is not near-repeated); overlapping occurrences count.
  2. Tracts, pad and merge: steps 4 and 5 of repeats_model, unchanged.
At m = 0 this is the stratum (k, slop) of repeats_model; the stratum at m contains the one at m - 1.
What this is not: a reproduction of GIAB's LowMappability BEDs; it counts substitutions only (no indels), covers k <= 32 only, and
looks at both strands.  Limits of the implementation: at most 2^31 - 1 bases in total.

Two statements: `brute`, the definition (each valid start against all others, both strands, self excluded; O(n^2), the yardstick),
and `fast`, the pigeonhole over the m + 1 fixed blocks with a table popcount, for genomes `brute` cannot do.
tests/test_nearrepeats_model.py holds `fast` to `brute`."""
import numpy as np

import context_model as CM
import repeats_model as RM

as_bytes = CM.as_bytes
MAX_M, MAX_K, MAX_SPEC = 3, 32, 4
_POP16 = np.array([bin(v).count("1") for v in range(1 << 16)], np.uint8)
_ODD = np.uint64(0x5555555555555555)


def ham(a, b):
    """differing base positions of 2-bit codes (uint64 arrays, broadcast)"""
    x = a ^ b
    y = (x | (x >> np.uint64(1))) & _ODD
    n = _POP16[(y & np.uint64(0xFFFF)).astype(np.int64)].astype(np.int32)
    for sh in (16, 32, 48):
        n = n + _POP16[((y >> np.uint64(sh)) & np.uint64(0xFFFF)).astype(np.int64)]
    return n


def blocks(k, m):
    """the fixed blocks: block j covers bases [floor(j k / (m + 1)), floor((j + 1) k / (m + 1)))"""
    return [(j * k // (m + 1), (j + 1) * k // (m + 1)) for j in range(m + 1)]


def name(k, m):
    return f"near_k{k}_m{m}"


def strands(s, k):
    """per contig: (valid[L] bool, fwd[L], rc[L] uint64; meaningless where valid is False)"""
    L = len(s)
    valid, F, R = np.zeros(L, bool), np.zeros(L, np.uint64), np.zeros(L, np.uint64)
    n = L - k + 1
    if n <= 0:
        return valid, F, R
    bad = np.concatenate(([0], np.cumsum(~CM.called(s)))).astype(np.int64)
    valid[:n] = bad[k:k + n] - bad[:n] == 0
    c = RM.codes(s)
    fwd, rc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + n]
        rc |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    F[:n], R[:n] = fwd, rc
    return valid, F, R


def _genome(contigs, k):
    contigs = [as_bytes(c) if not isinstance(c, np.ndarray) else c for c in contigs]
    per = [strands(c, k) for c in contigs]
    F = np.concatenate([f[v] for v, f, _ in per]) if per else np.zeros(0, np.uint64)
    R = np.concatenate([r[v] for v, _, r in per]) if per else np.zeros(0, np.uint64)
    return per, F, R


def _back(per, near_valid):
    out, at = [], 0
    for v, _, _ in per:
        near = np.zeros(len(v), bool)
        n = int(v.sum())
        near[v] = near_valid[at:at + n]
        at += n
        out.append(near)
    return out, len(near_valid), int(near_valid.sum())


def brute(contigs, k, m):
    """step 1 by the definition: per contig the bool array near[L], and (valid starts, near-repeated starts) of the genome"""
    per, F, R = _genome(contigs, k)
    n = len(F)
    near = np.zeros(n, bool)
    for g in range(n):
        d = np.minimum(ham(F[g], F), ham(F[g], R))
        d[g] = k + 1                                   # never its own partner
        near[g] = bool((d <= m).any())
    return _back(per, near)


def fast(contigs, k, m, small=48, chunk=512):
    """step 1 by the pigeonhole: records (code, start) of both strands, per block sorted by the block's bases; inside a run of equal
    block bases every pair of records of different starts within m flags both starts (RC is an isometry and an involution, so what
    holds for a record holds for its start)"""
    per, F, R = _genome(contigs, k)
    n = len(F)
    near = np.zeros(n, bool)
    if n == 0:
        return _back(per, near)
    code = np.concatenate([F, R])
    gid = np.concatenate([np.arange(n), np.arange(n)])
    for b0, b1 in blocks(k, m):
        w = b1 - b0
        mask = np.uint64((1 << (2 * w)) - 1) if w < 32 else np.uint64(0xFFFFFFFFFFFFFFFF)
        key = (code >> np.uint64(2 * (k - b1))) & mask
        order = np.argsort(key, kind="stable")
        sk, sc, sg = key[order], code[order], gid[order]
        head = np.concatenate(([True], sk[1:] != sk[:-1]))
        first = np.flatnonzero(head)
        length = np.diff(np.concatenate((first, [2 * n])))
        run_len = np.repeat(length, length)
        # short runs: record i against record i + d of its run, for every d
        for d in range(1, min(int(length.max()), small)):
            i = np.flatnonzero((sk[:-d] == sk[d:]) & (run_len[:-d] <= small))
            if len(i) == 0:
                continue
            hit = (ham(sc[i], sc[i + d]) <= m) & (sg[i] != sg[i + d])
            near[sg[i[hit]]] = True
            near[sg[i[hit] + d]] = True
        # long runs: the records whose start is not flagged yet against the run, a chunk of partners at a time
        for a, ln in zip(first[length > small], length[length > small]):
            idx = np.arange(a, a + ln)
            todo = idx[~near[sg[idx]]]
            for c0 in range(0, ln, chunk):
                if len(todo) == 0:
                    break
                part = idx[c0:c0 + chunk]
                close = (ham(sc[todo][:, None], sc[part][None, :]) <= m) & (sg[todo][:, None] != sg[part][None, :])
                near[sg[todo[close.any(axis=1)]]] = True
                near[sg[part[close.any(axis=0)]]] = True
                todo = todo[~near[sg[todo]]]
    return _back(per, near)


intervals_of = RM.intervals_of                   # steps 4 and 5 are those of the repeat strata


def all_intervals(contigs, specs, how=fast):
    """rows[spec][contig] = (starts, stops), the layout of api.PrecisionRecall.download_nearrepeat_intervals, and the stats
    (n_valid[spec], n_near[spec]) of api.PrecisionRecall.nearrepeat_stats; specs have k, m and slop"""
    rows, n_valid, n_near = [], [], []
    memo = {}
    for sp in specs:
        if (sp.k, sp.m) not in memo:
            memo[(sp.k, sp.m)] = how(contigs, sp.k, sp.m)
        nears, nv, nn = memo[(sp.k, sp.m)]
        rows.append([intervals_of(r, sp.k, sp.slop) for r in nears])
        n_valid.append(nv); n_near.append(nn)
    return rows, np.array(n_valid, np.int64), np.array(n_near, np.int64)


near_repeat_bed_text = CM.context_bed_text       # near-repeat-strata.bed has the format and order of repeat-strata.bed
bed_rows = CM.bed_rows
write_model_strata = CM.write_model_strata
same = CM.same
