"""Python binding of the C ABI (include/vcfdist_pr.h) -- ctypes over
vcfdist_amd/lib/libvcfdist_pr.so.  Plumbing only: every result comes from the
HIP kernels behind the ABI; there is no Python or CPU fallback, and a missing
library or GPU raises."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libvcfdist_pr.so")
CSRC = os.path.join(HERE, "csrc")
_LIB = None


class VprError(RuntimeError):
    pass


def build(force=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h"))]
    inc = os.path.join(os.path.dirname(HERE), "include")
    srcs += [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")]
    cli = os.path.join(os.path.dirname(LIB_PATH), "vcfdist_gpu")       # (the C++ command line, csrc/main.cpp: built beside the library)
    newest = min(os.path.getmtime(p) for p in (LIB_PATH, cli)) if os.path.exists(LIB_PATH) and os.path.exists(cli) else None
    stale = newest is None or any(os.path.getmtime(s) > newest and not (s.endswith("main.cpp") and os.path.getmtime(s) <= os.path.getmtime(cli))
                                  for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s"] + (["-B"] if force else []))
    return LIB_PATH


# The path keeps up to eight HIP streams busy at once (two parts of round 0, two retry ladders, two tie ladders and
# their side streams); the runtime's default of four hardware queues would serialise them pairwise.  Read by the HIP
# runtime when it initialises, so it has to be in the environment before the first HIP call of the process.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise VprError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no fallback path)")
    L = C.CDLL(LIB_PATH)
    H = C.c_void_p
    L.vpr_version.restype = C.c_char_p
    L.vpr_last_error.restype = C.c_char_p
    L.vpr_last_error.argtypes = [H]
    L.vpr_create.argtypes = [C.POINTER(A.VprConfig), C.POINTER(H)]
    L.vpr_destroy.argtypes = [H]
    L.vpr_run.argtypes = [H, C.POINTER(A.VprBatch), C.POINTER(A.VprResults)]
    L.vpr_upload.argtypes = [H, C.POINTER(A.VprBatch)]
    L.vpr_upload_variants.argtypes = [H, C.POINTER(A.VprVariants)]
    L.vpr_execute.argtypes = [H]
    L.vpr_download.argtypes = [H, C.POINTER(A.VprResults)]
    L.vpr_host_alloc.restype = C.c_void_p
    L.vpr_host_alloc.argtypes = [C.c_size_t]
    L.vpr_host_free.argtypes = [C.c_void_p]
    L.vpr_results_alloc.argtypes = [H, C.POINTER(A.VprResults), C.POINTER(C.c_void_p)]
    L.vpr_get_timing.argtypes = [H, C.POINTER(A.VprTiming)]
    L.vpr_get_launch_stats.argtypes = [H, C.POINTER(A.VprLaunchStat), C.c_int32]
    L.vpr_get_tally.argtypes = [H, C.POINTER(C.c_int64)]
    L.vpr_strip_plan_count.argtypes = [H]
    L.vpr_strip_plan_record.argtypes = [H, C.c_int32, C.POINTER(A.VprStripPlanRec), A.P_i32, C.c_int32]
    L.vpr_download_path.restype = C.c_int64
    L.vpr_download_path.argtypes = [H, C.c_int32, C.c_int32, C.c_int64, A.P_u8, A.P_i32, A.P_i32, A.P_u8, A.P_u8]
    L.vpr_store_phase.restype = C.c_int32
    L.vpr_store_phase.argtypes = [C.POINTER(C.c_int32), C.c_double, A.P_i32, A.P_i32]
    L.vpr_batch_from_variants.argtypes = [C.POINTER(A.VprVariants), C.POINTER(H)]
    L.vpr_owned_batch_view.restype = C.POINTER(A.VprBatch)
    L.vpr_owned_batch_view.argtypes = [H]
    L.vpr_owned_batch_free.argtypes = [H]
    L.vpr_synth_default_params.argtypes = [C.POINTER(A.VprSynthParams)]
    L.vpr_synth_create.argtypes = [C.POINTER(A.VprSynthParams), C.POINTER(H)]
    L.vpr_synth_variants.restype = C.POINTER(A.VprVariants)
    L.vpr_synth_variants.argtypes = [H]
    L.vpr_synth_destroy.argtypes = [H]
    L.vpr_distance.argtypes = [H, C.POINTER(A.VprVariants), C.POINTER(A.VprDistConfig)]
    L.vpr_distance_info.argtypes = [H, C.POINTER(A.VprDistInfo)]
    L.vpr_distance_download.argtypes = [H, C.POINTER(A.VprDistResults)]
    P_u64 = C.POINTER(C.c_uint64)
    L.vpr_strata_masks.argtypes = [H, C.POINTER(A.VprVariants), C.POINTER(A.VprStrata)]
    L.vpr_strata_download_masks.argtypes = [H, P_u64 * A.HAPS]
    L.vpr_strata_upload_masks.argtypes = [H, C.c_int32, A.P_i64, P_u64 * A.HAPS]
    L.vpr_pr_counts_strata.argtypes = [H, C.c_void_p, A.P_i32, C.c_int32, C.c_int32, A.P_i64]
    L.vpr_allreduce_counts_strata.argtypes = [H, C.c_void_p, C.c_void_p, A.P_i32, C.c_int32, C.c_int32, A.P_i64]
    L.vpr_strata_timing.argtypes = [H, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.vpr_context_default.argtypes = [C.POINTER(C.POINTER(A.VprContextStratum)), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.c_int32)]
    L.vpr_context_masks.argtypes = [H, C.POINTER(A.VprVariants), C.POINTER(A.VprStrata), C.POINTER(A.VprContextStratum), C.c_int32]
    L.vpr_context_interval_counts.argtypes = [H, A.P_i64]
    L.vpr_context_download_intervals.argtypes = [H, A.P_i32, A.P_i32]
    L.vpr_context_info.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.vpr_context_timing.argtypes = [H, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.vpr_repeats_default.argtypes = [C.POINTER(C.POINTER(A.VprRepeatStratum)), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.c_int32)]
    L.vpr_repeat_intervals.argtypes = [H, C.c_int32, A.P_i64, A.P_u8, C.POINTER(A.VprRepeatStratum), C.c_int32]
    L.vpr_repeat_interval_counts.argtypes = [H, A.P_i64]
    L.vpr_repeat_download_intervals.argtypes = [H, A.P_i32, A.P_i32]
    L.vpr_repeat_stats.argtypes = [H, A.P_i64, A.P_i64]
    L.vpr_repeat_timing.argtypes = [H] + [C.POINTER(C.c_double)] * 4
    L.vpr_repeat_sort_floor.argtypes = [H, C.c_int64, C.c_int32, C.c_uint64, C.POINTER(C.c_double)]
    L.vpr_longrepeats_default.argtypes = L.vpr_repeats_default.argtypes
    L.vpr_longrepeat_intervals.argtypes = L.vpr_repeat_intervals.argtypes
    L.vpr_longrepeat_interval_counts.argtypes = [H, A.P_i64]
    L.vpr_longrepeat_download_intervals.argtypes = [H, A.P_i32, A.P_i32]
    L.vpr_longrepeat_stats.argtypes = [H, A.P_i64, A.P_i64, A.P_i64, A.P_i64]
    L.vpr_longrepeat_timing.argtypes = [H] + [C.POINTER(C.c_double)] * 4
    L.vpr_nearrepeat_intervals.argtypes = [H, C.c_int32, A.P_i64, A.P_u8, C.POINTER(A.VprNearStratum), C.c_int32]
    L.vpr_nearrepeat_interval_counts.argtypes = [H, A.P_i64]
    L.vpr_nearrepeat_download_intervals.argtypes = [H, A.P_i32, A.P_i32]
    L.vpr_nearrepeat_stats.argtypes = [H, A.P_i64, A.P_i64, A.P_i64, A.P_i64]
    L.vpr_nearrepeat_timing.argtypes = [H] + [C.POINTER(C.c_double)] * 4
    L.vpr_nearrepeat_name.argtypes = [C.POINTER(A.VprNearStratum), C.c_char_p, C.c_size_t]
    L.vpr_varstrata_default.argtypes = [C.POINTER(C.POINTER(A.VprVariantStratum)), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.c_int32)]
    L.vpr_varstrata_masks.argtypes = [H, C.POINTER(A.VprVariants), C.POINTER(A.VprVariantStratum), C.c_int32, C.c_int32]
    L.vpr_varstrata_timing.argtypes = [H, C.POINTER(C.c_double)]
    L.vpr_derive_masks.argtypes = [H, A.P_i32, A.P_i32, C.c_int32]
    L.vpr_derive_timing.argtypes = [H, C.POINTER(C.c_double)]
    L.vpr_derive_compile.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.c_char_p, C.c_size_t, A.P_i32, C.c_int32, C.POINTER(C.c_int32)]
    L.vpr_derive_cross.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, A.P_i32, C.c_int32, C.POINTER(C.c_int32)]
    L.vpr_derive_last_error.restype = C.c_char_p
    L.vpr_derive_last_error.argtypes = []
    for name, own in (("errclass", [C.c_int32]), ("matchkind", [])):      # the label passes; own: errclass' window
        args = [C.POINTER(A.VprVariants), C.c_void_p, A.P_i32] + own + [C.c_int32, C.c_int32, A.P_i64]
        getattr(L, f"vpr_{name}").argtypes = [H] + args
        getattr(L, f"vpr_allreduce_{name}").argtypes = [H, C.c_void_p] + args
        getattr(L, f"vpr_{name}_download").argtypes = [H, A.P_u8 * A.HAPS]
        getattr(L, f"vpr_{name}_timing").argtypes = [H, C.POINTER(C.c_double)]
        getattr(L, f"vpr_{name}_names").restype = C.POINTER(C.c_char_p)
        getattr(L, f"vpr_{name}_names").argtypes = []
        # the pass's counts cut by stratum and resampled (pr_cut.hip)
        getattr(L, f"vpr_{name}_strata").argtypes = [H, C.c_int32, C.c_int32, A.P_i64]
        getattr(L, f"vpr_allreduce_{name}_strata").argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, A.P_i64]
        cut_boot = [C.c_int32, C.c_int32, P_u64, C.c_uint64, C.c_int32, C.c_int32, A.P_i64]
        getattr(L, f"vpr_{name}_boot").argtypes = [H] + cut_boot
        getattr(L, f"vpr_allreduce_{name}_boot").argtypes = [H, C.c_void_p] + cut_boot
        getattr(L, f"vpr_{name}_cut_timing").argtypes = [H, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        getattr(L, f"vpr_{name}_cut_info").argtypes = [H, C.POINTER(C.c_int32 * 6)]
    boot = [C.c_void_p, A.P_i32, C.c_int32, C.c_int32, P_u64, C.c_uint64, C.c_int32, C.c_int32, A.P_i64]
    L.vpr_pr_counts_boot.argtypes = [H] + boot
    L.vpr_allreduce_counts_boot.argtypes = [H, C.c_void_p] + boot
    L.vpr_boot_info.argtypes = [H, C.POINTER(C.c_int32 * 3), C.POINTER(C.c_double)]
    from .cluster import VclHapSeq, VclClusters
    L.vrl_realign.argtypes = [C.POINTER(VclHapSeq), A.P_f32, A.P_f32, A.P_i32, A.P_u8, C.POINTER(VclClusters), A.P_u8, C.c_int32,
                              C.POINTER(A.VrlConfig), C.c_int32, C.POINTER(C.POINTER(A.VrlResult))]
    L.vrl_result_free.argtypes = [C.POINTER(A.VrlResult)]
    _LIB = L
    return L


def call_or_allreduce(h, plain, reduced, comm, *args):
    """the entry `plain` on handle h, or with a communicator its all-reduce form `reduced` -> the return code"""
    if comm is None:
        return getattr(lib(), plain)(h, *args)
    return getattr(lib(), reduced)(h, comm if isinstance(comm, C.c_void_p) else C.c_void_p(comm), *args)


EXPORTED = [
    "vpr_create", "vpr_destroy", "vpr_last_error", "vpr_version", "vpr_run", "vpr_upload",
    "vpr_upload_variants", "vpr_download_level_a", "vpr_select_device", "vpr_execute", "vpr_download", "vpr_host_alloc", "vpr_host_free", "vpr_get_timing", "vpr_get_launch_stats",
    "vpr_get_tally", "vpr_strip_plan_count", "vpr_strip_plan_record",
    "vpr_download_path", "vpr_phase", "vpr_var_class", "vpr_upload_var_class", "vpr_results_alloc", "vpr_pr_counts", "vpr_pr_summary",
    "vpr_store_phase", "vpr_batch_from_variants", "vpr_owned_batch_view", "vpr_owned_batch_free",
    "vpr_synth_default_params", "vpr_synth_create", "vpr_synth_variants", "vpr_synth_destroy",
]
# include/vcfdist_distance.h
DIST_EXPORTED = ["vpr_distance", "vpr_distance_info", "vpr_distance_download"]
# include/vcfdist_strata.h
STRATA_EXPORTED = ["vpr_strata_masks", "vpr_strata_download_masks", "vpr_strata_upload_masks", "vpr_pr_counts_strata",
                   "vpr_allreduce_counts_strata", "vpr_strata_timing"]
# include/vcfdist_context.h
CONTEXT_EXPORTED = ["vpr_context_default", "vpr_context_masks", "vpr_context_interval_counts", "vpr_context_download_intervals",
                    "vpr_context_info", "vpr_context_timing"]
# include/vcfdist_repeats.h
REPEATS_EXPORTED = ["vpr_repeats_default", "vpr_repeat_intervals", "vpr_repeat_interval_counts", "vpr_repeat_download_intervals",
                    "vpr_repeat_stats", "vpr_repeat_timing", "vpr_repeat_sort_floor", "vrp_write_repeat_bed"]
# include/vcfdist_longrepeats.h
LONGREPEATS_EXPORTED = ["vpr_longrepeats_default", "vpr_longrepeat_intervals", "vpr_longrepeat_interval_counts",
                        "vpr_longrepeat_download_intervals", "vpr_longrepeat_stats", "vpr_longrepeat_timing", "vrp_write_long_repeat_bed"]
# include/vcfdist_nearrepeats.h
NEARREPEATS_EXPORTED = ["vpr_nearrepeat_intervals", "vpr_nearrepeat_interval_counts", "vpr_nearrepeat_download_intervals",
                        "vpr_nearrepeat_stats", "vpr_nearrepeat_timing", "vpr_nearrepeat_name", "vrp_write_near_repeat_bed"]
# include/vcfdist_varstrata.h
VARSTRATA_EXPORTED = ["vpr_varstrata_default", "vpr_varstrata_masks", "vpr_varstrata_timing", "vrp_write_variant_strata"]
# include/vcfdist_derive.h
DERIVE_EXPORTED = ["vpr_derive_masks", "vpr_derive_timing", "vpr_derive_compile", "vpr_derive_cross", "vpr_derive_last_error",
                   "vrp_write_derived_strata"]
# include/vcfdist_errclass.h
ERRCLASS_EXPORTED = ["vpr_errclass", "vpr_allreduce_errclass", "vpr_errclass_download", "vpr_errclass_timing", "vpr_errclass_names",
                     "vrp_write_error_classes"]
# include/vcfdist_matchkind.h
MATCHKIND_EXPORTED = ["vpr_matchkind", "vpr_allreduce_matchkind", "vpr_matchkind_download", "vpr_matchkind_timing", "vpr_matchkind_names",
                      "vrp_write_match_kinds"]
# include/vcfdist_errclass.h and include/vcfdist_matchkind.h: the label counts cut by stratum and resampled
LABELCUT_EXPORTED = [f"vpr_{a}{p}_{c}" for p in ("errclass", "matchkind") for a in ("", "allreduce_") for c in ("strata", "boot")] + \
                    [f"vpr_{p}_cut_{c}" for p in ("errclass", "matchkind") for c in ("timing", "info")] + \
                    [f"vrp_write_{n}_{c}" for n in ("error_classes", "match_kinds") for c in ("stratified", "bootstrap")]
# include/vcfdist_bootstrap.h
BOOT_EXPORTED = ["vpr_pr_counts_boot", "vpr_allreduce_counts_boot", "vpr_boot_info", "vrp_write_bootstrap", "vrp_write_bootstrap_stratified"]
# include/vcfdist_realign.h
RL_EXPORTED = ["vrl_realign", "vrl_result_free"]

RL_COLS = (("pos", np.int32), ("rlen", np.int32), ("type", np.uint8), ("ref_len", np.int32), ("alt_len", np.int32), ("ref_off", np.int64),
           ("alt_off", np.int64), ("var_qual", np.float32), ("gt_qual", np.float32), ("phase_set", np.int32), ("orig_gt", np.uint8))


def realign(hap, clusters, seq, sub=5, open=6, extend=2, max_qual=60, round_bytes=0, job_bytes_limit=0, device=0):
    """vrl_realign (include/vcfdist_realign.h) of one (contig, hap).  hap: a dict of the reader's columns (vcfdist_amd.io: pos, rlen,
    type, ref_len, alt_len, ref_off, alt_off, pool, var_qual, phase_set and optionally gt_qual, orig_gt); clusters: a
    cluster.Clusters of it; seq: the contig's sequence.  -> (dict of the realigned, left-shifted columns in the same layout,
    cluster_status uint8[n_clusters], VrlInfo).  A refusal raises VprError with the return code."""
    from . import cluster as K
    L = lib()
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dt)
        if a.size == 0:
            a = np.zeros(1, dt)
        keep.append(a)
        return A._ptr(a, np.ctypeslib.as_ctypes_type(dt))
    n = len(hap["pos"])
    hs = K.VclHapSeq()
    hs.cols.n_var = n
    for f in ("pos", "rlen", "ref_len", "alt_len"):
        setattr(hs.cols, f, arr(hap[f], np.int32))
    hs.cols.type = arr(hap["type"], np.uint8)
    hs.ref_off, hs.alt_off = arr(hap["ref_off"], np.int64), arr(hap["alt_off"], np.int64)
    hs.pool = arr(hap["pool"], np.uint8)
    cs = clusters.as_struct()
    seq = np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, np.uint8)
    cfg = A.VrlConfig(sub=sub, open=open, extend=extend, max_qual=max_qual, round_bytes=round_bytes, job_bytes_limit=job_bytes_limit)
    out = C.POINTER(A.VrlResult)()
    gq = arr(hap["gt_qual"], np.float32) if "gt_qual" in hap else None
    og = arr(hap["orig_gt"], np.uint8) if "orig_gt" in hap else None
    rc = L.vrl_realign(C.byref(hs), arr(hap["var_qual"], np.float32), gq, arr(hap["phase_set"], np.int32), og, C.byref(cs),
                       arr(seq, np.uint8), len(seq), C.byref(cfg), device, C.byref(out))
    if rc:
        raise VprError(f"vrl_realign failed ({rc})")
    try:
        r = out.contents
        cols = {f: A._from_ptr(getattr(r, f), r.n, dt).copy() if r.n else np.zeros(0, dt) for f, dt in RL_COLS}
        cols["pool"] = A._from_ptr(r.pool, int(r.pool_len), np.uint8).copy() if r.pool_len else np.zeros(1, np.uint8)
        status = A._from_ptr(r.cluster_status, r.n_clusters, np.uint8).copy() if r.n_clusters else np.zeros(0, np.uint8)
        info = A.VrlInfo.from_buffer_copy(r.info)
    finally:
        L.vrl_result_free(out)
    return cols, status, info


def context_default():
    """the command lines' default context strata (vpr_context_default): (names, [A.VprContextStratum])"""
    spec, names, n = C.POINTER(A.VprContextStratum)(), C.POINTER(C.c_char_p)(), C.c_int32()
    rc = lib().vpr_context_default(C.byref(spec), C.byref(names), C.byref(n))
    if rc:
        raise VprError(f"vpr_context_default failed ({rc})")
    return [names[k].decode() for k in range(n.value)], [A.VprContextStratum.from_buffer_copy(spec[k]) for k in range(n.value)]


def repeats_default():
    """the command lines' default repeat strata (vpr_repeats_default): (names, [A.VprRepeatStratum])"""
    spec, names, n = C.POINTER(A.VprRepeatStratum)(), C.POINTER(C.c_char_p)(), C.c_int32()
    rc = lib().vpr_repeats_default(C.byref(spec), C.byref(names), C.byref(n))
    if rc:
        raise VprError(f"vpr_repeats_default failed ({rc})")
    return [names[k].decode() for k in range(n.value)], [A.VprRepeatStratum.from_buffer_copy(spec[k]) for k in range(n.value)]


def nearrepeat_name(spec):
    """the name of a near-repeat stratum in the tables (vpr_nearrepeat_name): near_k<K>_m<M>"""
    buf = C.create_string_buffer(64)
    rc = lib().vpr_nearrepeat_name(C.byref(spec), buf, len(buf))
    if rc != 0:
        raise VprError(f"vpr_nearrepeat_name failed ({rc})")
    return buf.value.decode()


def longrepeats_default():
    """the command lines' default long repeat strata (vpr_longrepeats_default): (names, [A.VprRepeatStratum])"""
    spec, names, n = C.POINTER(A.VprRepeatStratum)(), C.POINTER(C.c_char_p)(), C.c_int32()
    rc = lib().vpr_longrepeats_default(C.byref(spec), C.byref(names), C.byref(n))
    if rc:
        raise VprError(f"vpr_longrepeats_default failed ({rc})")
    return [names[k].decode() for k in range(n.value)], [A.VprRepeatStratum.from_buffer_copy(spec[k]) for k in range(n.value)]


def varstrata_default():
    """the command lines' default variant strata (vpr_varstrata_default): (names, [A.VprVariantStratum])"""
    spec, names, n = C.POINTER(A.VprVariantStratum)(), C.POINTER(C.c_char_p)(), C.c_int32()
    rc = lib().vpr_varstrata_default(C.byref(spec), C.byref(names), C.byref(n))
    if rc:
        raise VprError(f"vpr_varstrata_default failed ({rc})")
    return [names[k].decode() for k in range(n.value)], [A.VprVariantStratum.from_buffer_copy(spec[k]) for k in range(n.value)]


def _c_names(names):
    return (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])


def derive_compile(entry, names, code_cap=A.DV_MAX_CODE):
    """one NAME=EXPR of --stratify-derive against `names`, the strata in front of it in table order (vpr_derive_compile,
    include/vcfdist_derive.h) -> (NAME, the postfix program as int32).  A malformed entry raises VprError with the library's text."""
    name, code, n = C.create_string_buffer(len(entry.encode()) + 1), np.zeros(max(code_cap, 1), np.int32), C.c_int32()
    if lib().vpr_derive_compile(entry.encode(), _c_names(names), len(names), name, len(name), A._ptr(code, C.c_int32), code_cap, C.byref(n)):
        raise VprError(lib().vpr_derive_last_error().decode())
    return name.value.decode(), code[:n.value].copy()


def derive_cross(entry, names, pairs_cap=A.DV_MAX_CLI):
    """one LIST:LIST of --stratify-cross against `names` (vpr_derive_cross) -> [(a, b)], indices into names, left-major; the crossed
    stratum is a & b, named names[a] + "&" + names[b].  A malformed entry raises VprError with the library's text."""
    pairs, n = np.zeros(2 * max(pairs_cap, 1), np.int32), C.c_int32()
    if lib().vpr_derive_cross(entry.encode(), _c_names(names), len(names), A._ptr(pairs, C.c_int32), pairs_cap, C.byref(n)):
        raise VprError(lib().vpr_derive_last_error().decode())
    return [(int(pairs[2 * i]), int(pairs[2 * i + 1])) for i in range(n.value)]


def _label_names(entry, n):
    names = getattr(lib(), entry)()
    return [names[k].decode() for k in range(n)]


def errclass_names():
    """the names of the seven error classes (vpr_errclass_names), in the order of their codes A.EC_*"""
    return _label_names("vpr_errclass_names", A.EC_CLASSES)


def matchkind_names():
    """the names of the four match kinds (vpr_matchkind_names), in the order of their codes A.MK_*"""
    return _label_names("vpr_matchkind_names", A.MK_KINDS)


def context_info():
    """(bases per workgroup, bases per lane) of the interval kernels (vpr_context_info; a property of the build)"""
    a, b = C.c_int32(), C.c_int32()
    rc = lib().vpr_context_info(None, C.byref(a), C.byref(b))
    if rc:
        raise VprError(f"vpr_context_info failed ({rc})")
    return a.value, b.value


def store_phase(s, thr=0.6):
    arr = (C.c_int32 * 4)(*[int(x) for x in s])
    o, w = C.c_int32(), C.c_int32()
    ph = lib().vpr_store_phase(arr, thr, C.byref(o), C.byref(w))
    return ph, o.value, w.value


def batch_from_variants(variants: A.Variants) -> A.Batch:
    """Host marshalling (generate_ptrs_strs x4 per supercluster) -> Level A Batch."""
    L = lib()
    vs = variants.as_struct()
    ob = C.c_void_p()
    rc = L.vpr_batch_from_variants(C.byref(vs), C.byref(ob))
    if rc:
        raise VprError(f"vpr_batch_from_variants failed: {rc}" + (
            " (input generate_ptrs_strs cannot process: unsorted / overlapping variants on a haplotype, a variant type other than "
            "SUB/INS/DEL, or a supercluster region that leaves its contig -- a variant ending on the last base of a contig; see "
            "include/vcfdist_pr.h)" if rc == -1 else ""))
    try:
        return A.Batch.from_struct(L.vpr_owned_batch_view(ob).contents)
    finally:
        L.vpr_owned_batch_free(ob)


def synth_params(**kw) -> A.VprSynthParams:
    p = A.VprSynthParams()
    lib().vpr_synth_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class _Owned:
    """Keeps a vpr_owned_batch alive for numpy views into it."""

    def __init__(self, h):
        self._h = h

    def __del__(self):
        try:
            if self._h:
                lib().vpr_owned_batch_free(self._h)
                self._h = None
        except Exception:
            pass


class Synth:
    """Owns a generated synthetic workload (variants + reference) inside the library."""

    def __init__(self, **kw):
        self.params = synth_params(**kw)
        self._h = C.c_void_p()
        rc = lib().vpr_synth_create(C.byref(self.params), C.byref(self._h))
        if rc:
            raise VprError(f"vpr_synth_create failed: {rc}")

    @property
    def struct(self):
        return lib().vpr_synth_variants(self._h).contents

    def variants(self) -> A.Variants:
        return A.Variants.from_struct(self.struct)

    def var_class(self, sv_threshold=50):
        """SNP / INDEL / SV class of every variant of the four hap slots (print.cpp:362-372), from views into the
        generator's tables (variants() copies the allele pools and the contigs as well)"""
        s = self.struct
        L = lib()
        L.vpr_var_class.restype = None
        L.vpr_var_class.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        out = []
        for h in range(A.HAPS):
            nv = int(s.var_off[h][s.n_sc])
            o = np.zeros(nv, np.uint8)
            if nv:
                L.vpr_var_class(C.cast(s.var_type[h], C.c_void_p), C.cast(s.var_ref_len[h], C.c_void_p),
                                C.cast(s.var_alt_len[h], C.c_void_p), nv, sv_threshold, o.ctypes.data)
            out.append(o)
        return out

    def batch(self, copy=True) -> A.Batch:
        """Level A batch of the workload.  copy=False returns numpy views into the library-owned
        buffers (no second copy of a multi-GB batch); the Batch keeps them alive."""
        L = lib()
        ob = C.c_void_p()
        rc = L.vpr_batch_from_variants(L.vpr_synth_variants(self._h), C.byref(ob))
        if rc:
            raise VprError(f"vpr_batch_from_variants failed: {rc}" + (
            " (input generate_ptrs_strs cannot process: unsorted / overlapping variants on a haplotype, a variant type other than "
            "SUB/INS/DEL, or a supercluster region that leaves its contig -- a variant ending on the last base of a contig; see "
            "include/vcfdist_pr.h)" if rc == -1 else ""))
        if not copy:
            return A.Batch.from_struct(L.vpr_owned_batch_view(ob).contents, copy=False, owner=_Owned(ob))
        try:
            return A.Batch.from_struct(L.vpr_owned_batch_view(ob).contents)
        finally:
            L.vpr_owned_batch_free(ob)

    def close(self):
        if self._h:
            lib().vpr_synth_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PrecisionRecall:
    """Mirror of the reference's precision_recall_wrapper for a batch of superclusters."""

    def __init__(self, cfg: A.VprConfig = None, device=0, **kw):
        self.cfg = cfg or A.default_config(device=device, **kw)
        self._h = C.c_void_p()
        L = lib()
        rc = L.vpr_create(C.byref(self.cfg), C.byref(self._h))
        if rc:
            raise VprError(f"vpr_create failed ({rc}): {L.vpr_last_error(None).decode()}")
        self._batch = None

    def _chk(self, rc, what):
        if rc:
            raise VprError(f"{what} failed ({rc}): {lib().vpr_last_error(self._h).decode()}")

    def upload(self, batch: A.Batch):
        self._batch = batch
        self._strata = None       # (the library releases the membership words with the batch)
        s = batch.as_struct()
        self._chk(lib().vpr_upload(self._h, C.byref(s)), "vpr_upload")

    def execute(self):
        self._chk(lib().vpr_execute(self._h), "vpr_execute")

    def download(self, res: A.Results = None) -> A.Results:
        """Copy the results of the last execute to host memory.  Pass a previous Results to reuse its
        buffers (every field is overwritten), which avoids re-allocating hundreds of MB per call."""
        if res is None:       # page-locked buffers: the copies then run at the link rate
            L = lib()
            s = A.VprResults()
            blk = C.c_void_p()
            # one block laid out like the device's result columns: a single copy per download
            if L.vpr_results_alloc(self._h, C.byref(s), C.byref(blk)) == 0 and blk.value:
                res = A.Results.mirror(s, self._batch.n_sc, [self._batch.n_vars(h) for h in range(A.HAPS)], blk.value, L.vpr_host_free)
            else:
                res = A.Results.for_batch(self._batch, L.vpr_host_alloc, L.vpr_host_free)
        s = res.as_struct()
        self._chk(lib().vpr_download(self._h, C.byref(s)), "vpr_download")
        return res

    def run(self, batch: A.Batch) -> A.Results:
        self.upload(batch)
        self.execute()
        return self.download()

    def distance(self, variants, eval_sub=3, eval_open=2, eval_extend=1, min_qual=0, max_qual=60, round_bytes=0):
        """The distance metrics (include/vcfdist_distance.h) of the batch the last execute evaluated.  variants: the
        A.Variants (or a VprVariants struct) the batch was made from.  -> dict of numpy arrays: job_* per (supercluster, hap,
        threshold) job, qual_dists [max_qual + 2], edit_* per record; plus 'info' (VprDistInfo)."""
        vs = variants.as_struct() if isinstance(variants, A.Variants) else variants
        cfg = A.VprDistConfig(eval_sub=eval_sub, eval_open=eval_open, eval_extend=eval_extend, min_qual=min_qual, max_qual=max_qual,
                              flags=0, round_bytes=round_bytes)
        L = lib()
        self._chk(L.vpr_distance(self._h, C.byref(vs), C.byref(cfg)), "vpr_distance")
        info = A.VprDistInfo()
        self._chk(L.vpr_distance_info(self._h, C.byref(info)), "vpr_distance_info")
        nj, ne = int(info.n_jobs), int(info.n_edits)
        out = dict(info=info, qual_dists=np.zeros(max_qual + 2, np.int64))
        cols = dict(job_sc=(nj, np.int32), job_hap=(nj, np.uint8), job_min_qual=(nj, np.int32), job_max_qual=(nj, np.int32),
                    job_dist=(nj, np.int32), job_status=(nj, np.uint8), edit_sc=(ne, np.int32), edit_hap=(ne, np.uint8),
                    edit_pos=(ne, np.int32), edit_type=(ne, np.uint8), edit_len=(ne, np.int32), edit_min_qual=(ne, np.int32),
                    edit_max_qual=(ne, np.int32))
        r = A.VprDistResults()
        for name, (n, dt) in cols.items():
            out[name] = np.zeros(max(n, 1), dt)
            setattr(r, name, A._ptr(out[name], C.c_int32 if dt == np.int32 else C.c_uint8))
        r.qual_dists = A._ptr(out["qual_dists"], C.c_int64)
        self._chk(L.vpr_distance_download(self._h, C.byref(r)), "vpr_distance_download")
        for name, (n, _) in cols.items():
            out[name] = out[name][:n]
        return out

    def strata_masks(self, variants, strata: A.Strata):
        """Membership words of the variants' four hap slots for every stratum (include/vcfdist_strata.h), computed and kept on the
        device until the next upload.  variants: an A.Variants (or a VprVariants struct); it need not be the executed batch."""
        vs = variants.as_struct() if isinstance(variants, A.Variants) else variants
        n_sc = int(vs.n_sc)
        ss = strata.as_struct()
        self._chk(lib().vpr_strata_masks(self._h, C.byref(vs), C.byref(ss)), "vpr_strata_masks")
        self._strata = (strata.n_strata, [int(vs.var_off[h][n_sc]) for h in range(A.HAPS)])

    def download_strata_masks(self):
        """the resident words: per hap slot a uint64 array [n_words, n_var]; bit k & 63 of word k >> 6 is stratum k"""
        n_strata, nv = getattr(self, "_strata", None) or (1, [0] * A.HAPS)     # (without words the call refuses: VPR_ERR_STATE)
        nw = (n_strata + 63) // 64
        out = [np.zeros((nw, n), np.uint64) for n in nv]
        keep = [o if o.size else np.zeros(1, np.uint64) for o in out]
        arr = (C.POINTER(C.c_uint64) * A.HAPS)(*[A._ptr(k, C.c_uint64) for k in keep])
        self._chk(lib().vpr_strata_download_masks(self._h, arr), "vpr_strata_download_masks")
        return out

    def upload_strata_masks(self, n_strata, masks):
        """make caller-supplied words resident (a rank's share of download_strata_masks(), or words made elsewhere):
        masks[slot] is uint64 [n_words, n_var]"""
        nw = (int(n_strata) + 63) // 64
        ms = [np.ascontiguousarray(m, np.uint64).reshape(nw, -1) for m in masks]
        nv = np.asarray([m.shape[1] for m in ms], np.int64)
        keep = [m if m.size else np.zeros(1, np.uint64) for m in ms]
        arr = (C.POINTER(C.c_uint64) * A.HAPS)(*[A._ptr(k, C.c_uint64) for k in keep])
        self._chk(lib().vpr_strata_upload_masks(self._h, int(n_strata), A._ptr(nv, C.c_int64), arr), "vpr_strata_upload_masks")
        self._strata = (int(n_strata), [int(n) for n in nv])

    def strata_timing(self):
        """(ms of the last strata_masks' kernels, ms of the last stratified histogram's) from HIP events on the handle's stream"""
        a, b = C.c_double(), C.c_double()
        self._chk(lib().vpr_strata_timing(self._h, C.byref(a), C.byref(b)), "vpr_strata_timing")
        return a.value, b.value

    def context_masks(self, variants, spec, bed: A.Strata = None):
        """The sequence-context strata (include/vcfdist_context.h): the intervals of every entry of `spec` (A.ctx_period /
        A.ctx_gc) are built on the device from the variants' contig sequences, and the membership words of the variants become
        resident as after strata_masks: the strata of `bed` first (if given), the context strata behind them in spec order."""
        vs = variants.as_struct() if isinstance(variants, A.Variants) else variants
        n_sc = int(vs.n_sc)
        arr = (A.VprContextStratum * max(len(spec), 1))(*spec)
        ss = bed.as_struct() if bed is not None else None
        self._context = None
        self._chk(lib().vpr_context_masks(self._h, C.byref(vs), C.byref(ss) if ss is not None else None, arr, len(spec)), "vpr_context_masks")
        self._context = (len(spec), int(vs.n_ctg))
        self._strata = ((bed.n_strata if bed is not None else 0) + len(spec), [int(vs.var_off[h][n_sc]) for h in range(A.HAPS)])

    def download_context_intervals(self):
        """the intervals of the last context_masks: rows[spec][contig] = (starts, stops), int32 arrays, 0-based half-open"""
        n_spec, n_ctg = getattr(self, "_context", None) or (0, 1)      # (before a call the library refuses: VPR_ERR_STATE)
        off = np.zeros(n_spec * n_ctg + 1, np.int64)
        self._chk(lib().vpr_context_interval_counts(self._h, A._ptr(off, C.c_int64)), "vpr_context_interval_counts")
        st, sp = np.zeros(max(int(off[-1]), 1), np.int32), np.zeros(max(int(off[-1]), 1), np.int32)
        self._chk(lib().vpr_context_download_intervals(self._h, A._ptr(st, C.c_int32), A._ptr(sp, C.c_int32)), "vpr_context_download_intervals")
        return [[(st[off[k * n_ctg + c]:off[k * n_ctg + c + 1]], sp[off[k * n_ctg + c]:off[k * n_ctg + c + 1]]) for c in range(n_ctg)]
                for k in range(n_spec)]

    def context_info(self):
        """(bases per workgroup, bases per lane) of the interval kernels"""
        return context_info()

    def context_timing(self):
        """(ms of the last context_masks' interval kernels, ms of its membership kernel) from HIP events on the handle's stream"""
        a, b = C.c_double(), C.c_double()
        self._chk(lib().vpr_context_timing(self._h, C.byref(a), C.byref(b)), "vpr_context_timing")
        return a.value, b.value

    @staticmethod
    def _genome(contigs):
        """(ctg_off int64, ctg_seq uint8 or None) of the contigs' sequences, or of (ctg_off, ctg_seq) as the library takes them"""
        if isinstance(contigs, tuple):
            off, seq = np.ascontiguousarray(contigs[0], np.int64), contigs[1]
        else:
            parts = [np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, np.uint8) for s in contigs]
            off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
            seq = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        if seq is not None:
            seq = np.ascontiguousarray(seq, np.uint8)
            if seq.size == 0:
                seq = np.zeros(1, np.uint8)
        return off, seq

    def _repeat_call(self, entry, attr, contigs, spec, stratum=A.VprRepeatStratum):
        off, seq = self._genome(contigs)
        arr = (stratum * max(len(spec), 1))(*spec) if spec is not None else None
        setattr(self, attr, None)
        self._chk(getattr(lib(), entry)(self._h, len(off) - 1, A._ptr(off, C.c_int64), A._ptr(seq, C.c_uint8) if seq is not None else None,
                                        arr, len(spec) if spec is not None else 1), entry)
        setattr(self, attr, (len(spec), len(off) - 1))

    def _repeat_rows(self, stem, attr):
        n_spec, n_ctg = getattr(self, attr, None) or (0, 1)      # (before a call the library refuses: VPR_ERR_STATE)
        off = np.zeros(n_spec * n_ctg + 1, np.int64)
        self._chk(getattr(lib(), f"{stem}_interval_counts")(self._h, A._ptr(off, C.c_int64)), f"{stem}_interval_counts")
        st, sp = np.zeros(max(int(off[-1]), 1), np.int32), np.zeros(max(int(off[-1]), 1), np.int32)
        self._chk(getattr(lib(), f"{stem}_download_intervals")(self._h, A._ptr(st, C.c_int32), A._ptr(sp, C.c_int32)), f"{stem}_download_intervals")
        return [[(st[off[k * n_ctg + c]:off[k * n_ctg + c + 1]], sp[off[k * n_ctg + c]:off[k * n_ctg + c + 1]]) for c in range(n_ctg)]
                for k in range(n_spec)]

    def longrepeat_intervals(self, contigs, spec):
        """The long repeat strata (include/vcfdist_longrepeats.h): the intervals of every entry of `spec` (A.rep_kmer with 33 <= k <=
        256) for the whole genome, built on the device in one call.  contigs: as for repeat_intervals.  The handle needs no batch."""
        self._repeat_call("vpr_longrepeat_intervals", "_longrepeats", contigs, spec)

    def download_longrepeat_intervals(self):
        """the intervals of the last longrepeat_intervals: rows[spec][contig] = (starts, stops), int32 arrays, 0-based half-open"""
        return self._repeat_rows("vpr_longrepeat", "_longrepeats")

    def longrepeat_stats(self, levels=False):
        """(valid starts, repeated starts) per entry of the last longrepeat_intervals: two int64 arrays; with `levels` also the
        candidates of every entry's last level and (pairs of the base level, candidates of the levels 64 and 128)"""
        n_spec = (getattr(self, "_longrepeats", None) or (1, 1))[0]
        a, b, c, lv = np.zeros(n_spec, np.int64), np.zeros(n_spec, np.int64), np.zeros(n_spec, np.int64), np.zeros(3, np.int64)
        self._chk(lib().vpr_longrepeat_stats(self._h, A._ptr(a, C.c_int64), A._ptr(b, C.c_int64), A._ptr(c, C.c_int64), A._ptr(lv, C.c_int64)),
                  "vpr_longrepeat_stats")
        return (a, b, c, lv) if levels else (a, b)

    def longrepeat_timing(self):
        """(ms_base, ms_levels, ms_last, ms_intervals) of the last longrepeat_intervals, from HIP events on the handle's stream"""
        t = [C.c_double() for _ in range(4)]
        self._chk(lib().vpr_longrepeat_timing(self._h, *[C.byref(x) for x in t]), "vpr_longrepeat_timing")
        return tuple(x.value for x in t)

    def nearrepeat_intervals(self, contigs, spec):
        """The near-repeat strata (include/vcfdist_nearrepeats.h): the intervals of every entry of `spec` (A.near_kmer) for the whole
        genome, built on the device in one call.  contigs: as for repeat_intervals.  The handle needs no batch."""
        self._repeat_call("vpr_nearrepeat_intervals", "_nearrepeats", contigs, spec, A.VprNearStratum)

    def download_nearrepeat_intervals(self):
        """the intervals of the last nearrepeat_intervals: rows[spec][contig] = (starts, stops), int32 arrays, 0-based half-open"""
        return self._repeat_rows("vpr_nearrepeat", "_nearrepeats")

    def nearrepeat_stats(self, cost=False):
        """(valid starts, near-repeated starts) per entry of the last nearrepeat_intervals: two int64 arrays; with `cost` also the
        compares made and the longest run of equal block keys"""
        n_spec = (getattr(self, "_nearrepeats", None) or (1, 1))[0]
        a, b, c, d = (np.zeros(n_spec, np.int64) for _ in range(4))
        self._chk(lib().vpr_nearrepeat_stats(self._h, *[A._ptr(x, C.c_int64) for x in (a, b, c, d)]), "vpr_nearrepeat_stats")
        return (a, b, c, d) if cost else (a, b)

    def nearrepeat_timing(self):
        """(ms_pack, ms_sort, ms_probe, ms_intervals) of the last nearrepeat_intervals, from HIP events on the handle's stream"""
        t = [C.c_double() for _ in range(4)]
        self._chk(lib().vpr_nearrepeat_timing(self._h, *[C.byref(x) for x in t]), "vpr_nearrepeat_timing")
        return tuple(x.value for x in t)

    def repeat_intervals(self, contigs, spec):
        """The repeat strata (include/vcfdist_repeats.h): the intervals of every entry of `spec` (A.rep_kmer) for the whole genome,
        built on the device in one call.  contigs: the sequences (bytes or uint8 arrays) in order, or (ctg_off, ctg_seq) as the
        library takes them.  The handle needs no batch."""
        self._repeat_call("vpr_repeat_intervals", "_repeats", contigs, spec)

    def download_repeat_intervals(self):
        """the intervals of the last repeat_intervals: rows[spec][contig] = (starts, stops), int32 arrays, 0-based half-open"""
        return self._repeat_rows("vpr_repeat", "_repeats")

    def repeat_stats(self):
        """(valid starts, repeated starts) per entry of the last repeat_intervals: two int64 arrays"""
        n_spec = (getattr(self, "_repeats", None) or (1, 1))[0]
        a, b = np.zeros(n_spec, np.int64), np.zeros(n_spec, np.int64)
        self._chk(lib().vpr_repeat_stats(self._h, A._ptr(a, C.c_int64), A._ptr(b, C.c_int64)), "vpr_repeat_stats")
        return a, b

    def repeat_timing(self):
        """(ms_pack, ms_sort, ms_mark, ms_intervals) of the last repeat_intervals, from HIP events on the handle's stream"""
        t = [C.c_double() for _ in range(4)]
        self._chk(lib().vpr_repeat_timing(self._h, *[C.byref(x) for x in t]), "vpr_repeat_timing")
        return tuple(x.value for x in t)

    def repeat_sort_floor(self, n, k, seed=1):
        """ms of the bare sort of repeat_intervals (key bits [0, 2k)) over n random keys: the floor under an entry with n valid starts"""
        ms = C.c_double()
        self._chk(lib().vpr_repeat_sort_floor(self._h, int(n), int(k), int(seed), C.byref(ms)), "vpr_repeat_sort_floor")
        return ms.value

    def varstrata_masks(self, variants, spec, append=False):
        """The variant strata (include/vcfdist_varstrata.h): the bits of every entry of `spec` (A.vs_size / A.vs_kind / A.vs_near)
        are made on the device from the variant tables and become the resident membership words (append False), or follow the
        resident ones of strata_masks / context_masks / upload_strata_masks for the same variant counts (append True)."""
        vs = variants.as_struct() if isinstance(variants, A.Variants) else variants
        n_sc = int(vs.n_sc)
        arr = (A.VprVariantStratum * max(len(spec), 1))(*spec)
        self._chk(lib().vpr_varstrata_masks(self._h, C.byref(vs), arr, len(spec), 1 if append else 0), "vpr_varstrata_masks")
        n_old = self._strata[0] if append else 0
        self._strata = (n_old + len(spec), [int(vs.var_off[h][n_sc]) for h in range(A.HAPS)])

    def derive_masks(self, code_off, code):
        """The derived strata (include/vcfdist_derive.h): entry j's postfix program code[code_off[j]:code_off[j + 1]] (operands >= 0,
        A.DV_AND / A.DV_OR / A.DV_NOT) runs on the device over every hap-variant's resident membership bits and becomes stratum
        n_prev + j behind the resident ones.  Reads no variant tables."""
        off, code = np.ascontiguousarray(code_off, np.int32), np.ascontiguousarray(code, np.int32)
        n = len(off) - 1
        if code.size == 0:
            code = np.zeros(1, np.int32)
        self._chk(lib().vpr_derive_masks(self._h, A._ptr(off, C.c_int32), A._ptr(code, C.c_int32), n), "vpr_derive_masks")
        self._strata = (self._strata[0] + n, self._strata[1])

    def derive_timing(self):
        """ms of the last derive_masks' kernel launches, from HIP events on the handle's stream"""
        return self._timing("vpr_derive_timing")

    def _timing(self, entry):
        """the one device time (ms) that `entry` returns"""
        a = C.c_double()
        self._chk(getattr(lib(), entry)(self._h, C.byref(a)), entry)
        return a.value

    def varstrata_timing(self):
        """ms of the last varstrata_masks' kernel launches, from HIP events on the handle's stream"""
        return self._timing("vpr_varstrata_timing")

    def _label_pass(self, name, n_labels, variants, var_class_per_slot, pb_phase, own, min_qual, max_qual, comm):
        """a label pass (vpr_<name>, or vpr_allreduce_<name> with comm) -> int64 [2][4][n_labels][nq]; own: the pass's own arguments"""
        vs = variants.as_struct() if isinstance(variants, A.Variants) else variants
        nq = max_qual - min_qual + 1
        out = np.zeros((2, 4, n_labels, max(nq, 1)), np.int64)      # (min_qual > max_qual: the call refuses)
        pb = None if pb_phase is None else np.ascontiguousarray(pb_phase, dtype=np.int32)
        arr = None
        if var_class_per_slot is not None:
            cls = [np.ascontiguousarray(c, dtype=np.uint8) for c in var_class_per_slot]
            arr = (A.P_u8 * 4)(*[A._ptr(c, C.c_uint8) for c in cls])
        args = (C.byref(vs), arr, None if pb is None else A._ptr(pb, C.c_int32), *own, min_qual, max_qual, A._ptr(out, C.c_int64))
        rc = call_or_allreduce(self._h, f"vpr_{name}", f"vpr_allreduce_{name}", comm, *args)
        self._chk(rc, f"vpr_{name}")
        return out

    def _label_download(self, entry):
        """the label bytes of the last call of a label pass: one uint8 array per hap slot"""
        out = [np.zeros(self._batch.n_vars(h) if self._batch is not None else 0, np.uint8) for h in range(A.HAPS)]
        keep = [o if o.size else np.zeros(1, np.uint8) for o in out]
        arr = (A.P_u8 * A.HAPS)(*[A._ptr(k, C.c_uint8) for k in keep])
        self._chk(getattr(lib(), entry)(self._h, arr), entry)
        return out

    def errclass(self, variants, var_class_per_slot, pb_phase=None, window=A.EC_DEFAULT_WINDOW, min_qual=0, max_qual=60, comm=None):
        """The error classes of the last execute (include/vcfdist_errclass.h): every query FP and truth FN gets the first class
        that applies (A.EC_*), joined across the callsets inside its supercluster on the device -> int64 [2][4][7][nq].
        variants: the A.Variants (or a VprVariants struct) the batch was made from; var_class_per_slot None: the classes are
        resident; comm: an ncclComm_t (as an integer) for vpr_allreduce_errclass."""
        return self._label_pass("errclass", A.EC_CLASSES, variants, var_class_per_slot, pb_phase, (int(window),), min_qual, max_qual, comm)

    def errclass_download(self):
        """the class bytes (A.EC_*, A.EC_NONE) of the last errclass: one uint8 array per hap slot"""
        return self._label_download("vpr_errclass_download")

    def errclass_timing(self):
        """ms of the last errclass' kernel launches, from HIP events on the handle's stream"""
        return self._timing("vpr_errclass_timing")

    def matchkind(self, variants, var_class_per_slot, pb_phase=None, min_qual=0, max_qual=60, comm=None):
        """The match kinds of the last execute (include/vcfdist_matchkind.h): every TP of either callset gets the first kind that
        applies (A.MK_*), joined across the callsets inside its supercluster on the device -> int64 [2][4][4][nq].
        variants: the A.Variants (or a VprVariants struct) the batch was made from; var_class_per_slot None: the classes are
        resident; comm: an ncclComm_t (as an integer) for vpr_allreduce_matchkind."""
        return self._label_pass("matchkind", A.MK_KINDS, variants, var_class_per_slot, pb_phase, (), min_qual, max_qual, comm)

    def matchkind_download(self):
        """the kind bytes (A.MK_*, A.MK_NONE) of the last matchkind: one uint8 array per hap slot"""
        return self._label_download("vpr_matchkind_download")

    def matchkind_timing(self):
        """ms of the last matchkind's kernel launches, from HIP events on the handle's stream"""
        return self._timing("vpr_matchkind_timing")

    def _label_strata(self, name, n_labels, min_qual, max_qual, comm):
        """vpr_<name>_strata (or its all-reduce with comm) -> int64 [n_strata][2][4][n_labels][nq]"""
        n_strata = (getattr(self, "_strata", None) or (1, None))[0]      # (without words the call refuses: VPR_ERR_STATE)
        out = np.zeros((n_strata, 2, 4, n_labels, max(max_qual - min_qual + 1, 1)), np.int64)
        args = (min_qual, max_qual, A._ptr(out, C.c_int64))
        rc = call_or_allreduce(self._h, f"vpr_{name}_strata", f"vpr_allreduce_{name}_strata", comm, *args)
        self._chk(rc, f"vpr_{name}_strata")
        return out

    def _label_boot(self, name, n_labels, sc_key, n_rep, seed, min_qual, max_qual, stratum, comm):
        """vpr_<name>_boot (or its all-reduce with comm) -> int64 [n_rep][2][4][n_labels][nq]"""
        kp = None                                                        # (a null sc_key: the call refuses)
        if sc_key is not None:
            keys = np.ascontiguousarray(sc_key, np.uint64)
            n_sc = self._batch.n_sc if self._batch is not None else 0
            if keys.shape != (n_sc,):
                raise VprError(f"vpr_{name}_boot: {keys.shape} keys for {n_sc} superclusters")
            keys = keys if keys.size else np.zeros(1, np.uint64)
            kp = A._ptr(keys, C.c_uint64)
        n_rep = int(n_rep)
        out = np.zeros((n_rep if 1 <= n_rep <= A.BOOT_MAX_REPLICATES else 1, 2, 4, n_labels, max(max_qual - min_qual + 1, 1)), np.int64)
        args = (min_qual, max_qual, kp, int(seed) & (2 ** 64 - 1), n_rep, int(stratum), A._ptr(out, C.c_int64))
        rc = call_or_allreduce(self._h, f"vpr_{name}_boot", f"vpr_allreduce_{name}_boot", comm, *args)
        self._chk(rc, f"vpr_{name}_boot")
        return out

    def _label_cut_timing(self, name):
        a, b = C.c_double(), C.c_double()
        self._chk(getattr(lib(), f"vpr_{name}_cut_timing")(self._h, C.byref(a), C.byref(b)), f"vpr_{name}_cut_timing")
        return a.value, b.value

    def _label_cut_info(self, name):
        g = (C.c_int32 * 6)()
        self._chk(getattr(lib(), f"vpr_{name}_cut_info")(self._h, C.byref(g)), f"vpr_{name}_cut_info")
        return dict(zip(("chunk", "chunks", "lds", "spans", "groups", "slices"), (int(x) for x in g)))

    def errclass_strata(self, min_qual=0, max_qual=60, comm=None):
        """The error-class counts of the last errclass cut by the resident membership words (include/vcfdist_errclass.h): stratum
        k counts the class bytes of the variants whose bit k is set -> int64 [n_strata][2][4][7][nq].  The phasing and the
        variant classes are the errclass call's; comm: an ncclComm_t (as an integer) for vpr_allreduce_errclass_strata."""
        return self._label_strata("errclass", A.EC_CLASSES, min_qual, max_qual, comm)

    def errclass_boot(self, sc_key, n_rep, seed=1, min_qual=0, max_qual=60, stratum=-1, comm=None):
        """The bootstrap replicates of the error-class counts of the last errclass: replicate r counts every classified variant
        w(seed, r, sc_key[its supercluster]) times (include/vcfdist_bootstrap.h's weight) -> int64 [n_rep][2][4][7][nq].
        stratum >= 0: only the variants of that stratum of the resident membership words."""
        return self._label_boot("errclass", A.EC_CLASSES, sc_key, n_rep, seed, min_qual, max_qual, stratum, comm)

    def errclass_cut_timing(self):
        """(ms of the last errclass_strata's kernels, ms of the last errclass_boot's) from HIP events on the handle's stream"""
        return self._label_cut_timing("errclass")

    def errclass_cut_info(self):
        """the launch shapes of the last errclass_strata (chunk: strata of a workgroup, chunks, lds bytes) and errclass_boot
        (spans, groups of 64 replicates, quality slices)"""
        return self._label_cut_info("errclass")

    def matchkind_strata(self, min_qual=0, max_qual=60, comm=None):
        """errclass_strata for the match kinds of the last matchkind -> int64 [n_strata][2][4][4][nq]"""
        return self._label_strata("matchkind", A.MK_KINDS, min_qual, max_qual, comm)

    def matchkind_boot(self, sc_key, n_rep, seed=1, min_qual=0, max_qual=60, stratum=-1, comm=None):
        """errclass_boot for the match kinds of the last matchkind -> int64 [n_rep][2][4][4][nq]"""
        return self._label_boot("matchkind", A.MK_KINDS, sc_key, n_rep, seed, min_qual, max_qual, stratum, comm)

    def matchkind_cut_timing(self):
        """(ms of the last matchkind_strata's kernels, ms of the last matchkind_boot's)"""
        return self._label_cut_timing("matchkind")

    def matchkind_cut_info(self):
        """errclass_cut_info for the match kinds"""
        return self._label_cut_info("matchkind")

    def pr_counts_boot(self, var_class_per_slot, pb_phase, sc_key, n_rep, seed=1, min_qual=0, max_qual=60, stratum=-1, comm=None):
        """The bootstrap replicates of the counters of the last execute (include/vcfdist_bootstrap.h): replicate r counts every
        variant w(seed, r, sc_key[its supercluster]) times -> int64 [n_rep][2][4][3][nq].  stratum >= 0: only the variants of
        that stratum of the resident membership words; comm: an ncclComm_t (as an integer) for vpr_allreduce_counts_boot."""
        from . import summary
        return summary.pr_counts_boot(self, var_class_per_slot, pb_phase, sc_key, n_rep, seed, min_qual, max_qual, stratum, comm)

    def boot_info(self):
        """((spans, replicate groups, quality slices), device ms) of the last pr_counts_boot"""
        g, ms = (C.c_int32 * 3)(), C.c_double()
        self._chk(lib().vpr_boot_info(self._h, C.byref(g), C.byref(ms)), "vpr_boot_info")
        return tuple(int(x) for x in g), ms.value

    def timing(self) -> A.VprTiming:
        t = A.VprTiming()
        self._chk(lib().vpr_get_timing(self._h, C.byref(t)), "vpr_get_timing")
        return t

    def tally(self):
        """int64[2 callsets][TP,FP,FN] accumulated on the device by the last execute."""
        out = (C.c_int64 * 6)()
        self._chk(lib().vpr_get_tally(self._h, out), "vpr_get_tally")
        return np.array(list(out), dtype=np.int64).reshape(2, 3)

    def launch_stats(self):
        L = lib()
        n = L.vpr_get_launch_stats(self._h, None, 0)
        arr = (A.VprLaunchStat * max(n, 1))()
        L.vpr_get_launch_stats(self._h, arr, n)
        return [arr[i] for i in range(n)]

    def strip_plan(self):
        """test aid (A.CFG_KEEP_STRIP_PLAN): what the strip planner (k_strip_plan) decided in the last execute -> one dict per
        planner call and alignment, in call order: sc, aln, from_window, tie_round, call, ok (1 strips, 0 one-workgroup kernels,
        2 neither) and strips, the list of (lo_q, lo_r, hi_q, hi_r).  Empty without the flag."""
        L = lib()
        n = L.vpr_strip_plan_count(self._h)
        self._chk(min(n, 0), "vpr_strip_plan_count")
        out = []
        for k in range(n):
            rec = A.VprStripPlanRec()
            self._chk(L.vpr_strip_plan_record(self._h, k, C.byref(rec), None, 0), "vpr_strip_plan_record")
            lohi = np.zeros((max(rec.n_strips, 1), 4), np.int32)
            self._chk(L.vpr_strip_plan_record(self._h, k, C.byref(rec), lohi.ctypes.data_as(A.P_i32), rec.n_strips), "vpr_strip_plan_record")
            d = {f: int(getattr(rec, f)) for f, _ in A.VprStripPlanRec._fields_ if f != "n_strips"}
            d["strips"] = [tuple(int(x) for x in row) for row in lohi[:rec.n_strips]]
            out.append(d)
        return out

    def upload_variants(self, variants_struct, batch_for_results):
        """Upload a vpr_variants struct (e.g. Synth.struct): the host sizes and checks the regions, the device writes the
        haplotype strings and pointer arrays (generate_ptrs_strs, pr_gen.hip).  `batch_for_results` only sizes the result
        buffers: anything with n_sc and n_vars(h) (a Batch, a Variants)."""
        self._batch = batch_for_results
        self._strata = None
        self._chk(lib().vpr_upload_variants(self._h, C.byref(variants_struct)), "vpr_upload_variants")

    def download_level_a(self, like: A.Batch) -> A.Batch:
        """test aid: the resident Level A arrays (written by the host marshalling or by the device generator) as a Batch
        shaped like `like` (same offsets)"""
        z = lambda a: np.zeros_like(a)
        out = A.Batch(like.n_sc, [z(a) for a in like.hap_off], [z(a) for a in like.hap_seq], [z(a) for a in like.hap_ptr],
                      [z(a) for a in like.hap_flag], z(like.ref_off), z(like.ref_seq), [z(a) for a in like.ref_ptr],
                      [z(a) for a in like.ref_flag], like.var_off, like.var_pos, like.var_qual)
        s = out.as_struct()
        L = lib()
        L.vpr_download_level_a.argtypes = [C.c_void_p, C.POINTER(A.VprBatch)]
        self._chk(L.vpr_download_level_a(self._h, C.byref(s)), "vpr_download_level_a")
        return out

    def path(self, sc, aln):
        """(plane, qri, ti, sync, edit) arrays of one alignment's walk (last workspace chunk only)."""
        lq1, lq2, lt1, lt2, lr = self._batch.lens(sc)
        cap = lq1 + lq2 + lr + lt1 + lt2 + 8
        pl = np.zeros(cap, np.uint8); q = np.zeros(cap, np.int32); t = np.zeros(cap, np.int32)
        sy = np.zeros(cap, np.uint8); ed = np.zeros(cap, np.uint8)
        n = lib().vpr_download_path(self._h, sc, aln, cap, pl.ctypes.data_as(A.P_u8), q.ctypes.data_as(A.P_i32),
                                    t.ctypes.data_as(A.P_i32), sy.ctypes.data_as(A.P_u8), ed.ctypes.data_as(A.P_u8))
        if n < 0:
            raise VprError(f"vpr_download_path failed: {n}")
        return pl[:n], q[:n], t[:n], sy[:n], ed[:n]

    def close(self):
        if self._h:
            lib().vpr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
