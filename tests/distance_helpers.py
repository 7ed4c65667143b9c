"""Shared by the distance tests: the CPU model (tests/distance_model.cpp, compiled with g++ into a temporary directory) behind
ctypes, and the calls that feed it a vpr_variants batch."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_MODEL = None


def model():
    global _MODEL
    if _MODEL is None:
        d = tempfile.mkdtemp(prefix="distance_model_")
        so = os.path.join(d, "distance_model.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "distance_model.cpp")])
        L = C.CDLL(so)
        P = C.POINTER
        L.dm_job.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 8 + [P(C.c_int), P(C.c_int), C.c_int]
        L.dm_steps.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, P(C.c_int), C.c_int]
        L.dm_run.restype = C.c_long
        L.dm_run.argtypes = [P(C.c_uint8), P(C.c_int64), P(C.c_int32), C.c_int, P(C.c_int32), P(C.c_int32), P(C.c_void_p), P(C.c_int32), P(C.c_uint8),
                             C.c_int, C.c_int, C.c_int, C.c_int]
        L.dm_jobs.argtypes = [P(C.c_int)]
        L.dm_n_records.restype = C.c_long
        L.dm_records.argtypes = [P(C.c_int)]
        L.dm_write.argtypes = [C.c_char_p, P(C.c_char_p), P(C.c_int), C.c_long] + [C.c_int] * 7 + [C.c_char_p, C.c_long]
        _MODEL = L
    return _MODEL


def job(q, t, x=3, o=2, e=1, beg=0, sc=0, hap=0, minq=0, maxq=62):
    """one alignment on explicit (forward) strings -> (distance, [(sc, hap, pos, type, len, minq, maxq), ...])"""
    L = model()
    d = C.c_int()
    rec = (C.c_int * (7 * 4096))()
    n = L.dm_job(q.encode(), t.encode(), x, o, e, beg, sc, hap, minq, maxq, C.byref(d), rec, 4096)
    assert n >= 0
    return d.value, [tuple(rec[7 * k:7 * k + 7]) for k in range(n)]


def steps(q, t, x=3, o=2, e=1):
    buf = (C.c_int * (len(q) + len(t) + 8))()
    n = model().dm_steps(q.encode(), t.encode(), x, o, e, buf, len(buf))
    assert n >= 0
    return list(buf[:n])


def run(v, sc_phase, skip, x=3, o=2, e=1, max_qual=60):
    """the model over an A.Variants -> (jobs int[n, 5]: sc, hap, minq, maxq, dist; records int[n, 7])"""
    L = model()
    cols = (C.c_void_p * 32)()
    keep = []
    for s in range(4):
        arrs = [np.ascontiguousarray(a) for a in (v.var_off[s], v.var_pos[s], v.var_type[s], v.var_qual[s], v.var_ref_len[s],
                                                   v.var_alt_len[s], v.var_alt_off[s], v.allele_pool[s])]
        keep += arrs
        for k, a in enumerate(arrs):
            cols[8 * s + k] = a.ctypes.data
    seq = np.ascontiguousarray(v.ctg_seq, np.uint8)
    beg, end = np.ascontiguousarray(v.sc_beg, np.int32), np.ascontiguousarray(v.sc_end, np.int32)
    ph = np.ascontiguousarray(sc_phase, np.int32)
    sk = np.ascontiguousarray(skip, np.uint8)
    co, sct = np.ascontiguousarray(v.ctg_off, np.int64), np.ascontiguousarray(v.sc_ctg, np.int32)
    n = L.dm_run(seq.ctypes.data_as(C.POINTER(C.c_uint8)), co.ctypes.data_as(C.POINTER(C.c_int64)), sct.ctypes.data_as(C.POINTER(C.c_int32)), v.n_sc, beg.ctypes.data_as(C.POINTER(C.c_int32)),
                 end.ctypes.data_as(C.POINTER(C.c_int32)), cols, ph.ctypes.data_as(C.POINTER(C.c_int32)),
                 sk.ctypes.data_as(C.POINTER(C.c_uint8)), x, o, e, max_qual)
    assert n >= 0, "the model failed on a job"
    jobs = np.zeros((n, 5), np.int32)
    L.dm_jobs(jobs.ctypes.data_as(C.POINTER(C.c_int)))
    m = L.dm_n_records()
    recs = np.zeros((m, 7), np.int32)
    L.dm_records(recs.ctypes.data_as(C.POINTER(C.c_int)))
    return jobs, recs


def write(prefix, ctg_of, recs, min_qual, max_qual, x=3, o=2, e=1, verbosity=1, write_files=True):
    """the model's writers: files under prefix, -> summary text"""
    recs = np.ascontiguousarray(recs, np.int32).reshape(-1, 7)
    names = (C.c_char_p * max(len(ctg_of), 1))(*[c.encode() for c in ctg_of])
    buf = C.create_string_buffer(1 << 16)
    n = model().dm_write((prefix or "").encode(), names, recs.ctypes.data_as(C.POINTER(C.c_int)), len(recs), min_qual, max_qual, x, o, e,
                         verbosity, 1 if write_files else 0, buf, len(buf))
    assert n >= 0
    return buf.value.decode()


def sets_from_records(name, recs):
    """one vrp_edits set (vcfdist_amd.report.write_distance / write_edits) from model records"""
    r = np.asarray(recs, np.int32).reshape(-1, 7)
    return (name, dict(edit_sc=r[:, 0], edit_hap=r[:, 1].astype(np.uint8), edit_pos=r[:, 2], edit_type=r[:, 3].astype(np.uint8),
                       edit_len=r[:, 4], edit_min_qual=r[:, 5], edit_max_qual=r[:, 6]))
