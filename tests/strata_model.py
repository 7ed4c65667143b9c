"""Model of the region-stratified counters (include/vcfdist_strata.h) for the tests.

Membership is the host's vio_bed_contains, called through ctypes on BEDs written to a temporary directory: the existing host
function is the specification.  Expected counts come from the existing counting oracle: the downloaded results are copied, the
errtype of every non-member is set to ERRTYPE_UN in both swaps, and oracle_lib.oracle_pr_counts counts what is left -- the
oracle skips such variants exactly as the kernel does, so no new counting model is needed."""
import ctypes as C
import os
import types

import numpy as np

import oracle_lib as O
from vcfdist_amd import _abi as A
from vcfdist_amd import api, io as IO

OUTSIDE, INSIDE, BORDER, OFFCTG = 0, 1, 2, 3


def write_bed(path, rows):
    """rows: (contig, start, stop) in file order"""
    with open(path, "w") as fh:
        for c, a, b in rows:
            fh.write(f"{c}\t{int(a)}\t{int(b)}\n")
    return str(path)


def write_strata(tmp, strata, list_name="strata.tsv"):
    """strata: [(name, rows)] -> the path of a strata list in `tmp` whose BEDs lie beside it (relative paths)"""
    with open(os.path.join(str(tmp), list_name), "w") as fh:
        fh.write("# name\tpath\n\n")
        for name, rows in strata:
            write_bed(os.path.join(str(tmp), name + ".bed"), rows)
            fh.write(f"{name}\t{name}.bed\n")
    return os.path.join(str(tmp), list_name)


def var_contig(v, slot):
    """contig index of every variant of one hap slot"""
    return np.repeat(np.asarray(v.sc_ctg, np.int64), np.diff(v.var_off[slot]))


def locations(beds, ctg_names, v):
    """vio_bed_contains of every variant against every BED: per hap slot a uint8 array [n_strata, n_var] of VIO_BED_*"""
    L = api.lib()
    f = L.vio_bed_contains
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32]
    names = [c.encode() for c in ctg_names]
    out = []
    for s in range(A.HAPS):
        ctg = var_contig(v, s)
        pos, rl, ty = v.var_pos[s].tolist(), v.var_ref_len[s].tolist(), v.var_type[s].tolist()
        cn = [names[c] for c in ctg.tolist()]
        loc = np.zeros((len(beds), len(pos)), np.uint8)
        for k, b in enumerate(beds):
            h = b._h
            loc[k] = [f(h, cn[i], pos[i], pos[i] + rl[i], ty[i]) for i in range(len(pos))]
        out.append(loc)
    return out


def words_of(loc):
    """the membership words [n_words, n_var] of one hap slot's locations: bit k & 63 of word k >> 6 is stratum k"""
    k, n = loc.shape
    w = np.zeros(((k + 63) // 64, n), np.uint64)
    for i in range(k):
        w[i >> 6] |= (loc[i] == INSIDE).astype(np.uint64) << np.uint64(i & 63)
    return w


def strata_of(beds, ctg_names):
    return IO.contig_strata(beds, ctg_names)


def expected_counts(var_off, res, cls, pb, member, min_qual=0, max_qual=60):
    """counts [2][4][3][nq] of one stratum: member[slot] is a bool array over the slot's variants"""
    cut = types.SimpleNamespace(sc_phase=res.sc_phase, callq=res.callq,
                                errtype=[[np.where(member[s], res.errtype[s][w], A.ERRTYPE_UN).astype(np.uint8) for w in range(2)]
                                         for s in range(A.HAPS)])
    return O.oracle_pr_counts(O.lib(), var_off, cut, cls, pb, min_qual, max_qual)
