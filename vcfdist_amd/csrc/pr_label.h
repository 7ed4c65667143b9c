// pr_label.h -- the host side of a label pass: an entry that gives every hap-variant of the executed batch one label byte, by a
// kernel of its own that joins the two callsets inside the supercluster, and counts the labels by callset, type and threshold
// (vpr_errclass, pr_errclass.hip: the error classes; vpr_matchkind, pr_matchkind.hip: the match kinds).  A pass brings its kernel,
// its launch loop, its names and a LabelDesc; everything around the launches is here (pr_label.hip), and so are the pass's counts
// cut by stratum and resampled (pr_cut.hip), which need the LabelDesc alone.
#pragma once

#include "pr_host.h"
#include "pr_cut.h"
#include "pr_vartab.h"

// What a pass keeps in the handle (vpr_handle::label[LabelDesc::pass]), created by its first call, released with the batch
struct LabelState {
    DevBuf<uint8_t> bytes[VPR_HAPS];                             // the label bytes of the last call
    DevBuf<unsigned long long> hist;                             // [2][3 types][labels][nq + 1]
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms = 0;
    bool valid = false;
    // for the cuts (pr_cut.hip): a cut must use the phasing the bytes were made under, so the call's phase-block words stay
    DevBuf<int32_t> pb;                                          // the last call's pb_phase [n_sc]
    bool has_pb = false;                                         // (false: the call had none)
    CutState cut;                                                // labelcut_strata, labelcut_boot; labelcut_timing, labelcut_info
};

// The thresholds a variant of bin b (pr_count_row, pr_counts.h: bin nq is callq < min_qual) counts at
enum LabelFold {
    LABEL_FOLD_UPTO,       // the threshold indices <= b, at none for bin nq: pr_fold_counts' rule for a query variant and for a TP
    LABEL_FOLD_EVERY,      // every threshold: a truth FN is one whatever the threshold
    LABEL_FOLD_ABOVE,      // the thresholds above b, at every one for bin nq: where a truth TP has turned into an FN
};

struct LabelDesc {
    int pass;                                  // LABEL_ERRCLASS / LABEL_MATCHKIND (pr_host.h)
    const char *entry, *noun;                  // for the messages: "vpr_errclass", "class"
    int labels;                                // label codes 0 .. labels - 1 are counted (the code of "no label" is not)
    LabelFold (*fold)(int callset, int label);
};

// thresholds of one call: the block histogram, 3 * labels * (nq + 1) words of dynamic LDS, stays within 64 KiB
inline int label_max_nq(const LabelDesc &D) { return 64 * 1024 / 4 / (3 * D.labels) - 1; }

// One call between label_begin and label_finish: what the pass's launch loop needs
struct LabelCall {
    LabelState *S = nullptr;
    VarTables T;                               // the columns and the pools: one block that lives as long as the call
    int32_t *d_pb = nullptr;                   // the caller's phase-block phasing on the device (null without pb_phase)
    int nq = 0;
    size_t nb = 0;                             // words of the block histogram, 3 * labels * (nq + 1)
};

// The front of a call, after the pass's own argument checks: the shared argument checks (VPR_ERR_ARG, before any allocation),
// pr_counts_begin, vartab_check, the state (invalid from here on), its buffers, the variant tables and the callers' inputs on the
// device, the zeroed histogram and the first event.  The launches follow on h->stream, each with c->nb * 4 bytes of LDS.
int label_begin(vpr_handle *h, const LabelDesc &D, void *comm, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS],
                const int32_t *pb_phase, int32_t min_qual, int32_t max_qual, const int64_t *counts, LabelCall *c);
// The back: the second event, pr_counts_finish (the all-reduce with comm, the histogram to the host, the wait), the device time,
// the bytes become valid, the fold into counts [2][VPR_VARTYPES][labels][nq]
int label_finish(vpr_handle *h, const LabelDesc &D, void *comm, LabelCall *c, int64_t *counts);
// histogram [2][3 types][labels][nq + 1] -> counts [2][VPR_VARTYPES][labels][nq] by D.fold, the types summed into VPR_VARTYPE_ALL
void fold_labels(const LabelDesc &D, const unsigned long long *hist, int nq, int64_t *counts);
int label_download(vpr_handle *h, const LabelDesc &D, uint8_t *const bytes[VPR_HAPS]);
int label_timing(const vpr_handle *h, const LabelDesc &D, double *ms);

// ---- pr_cut.hip: the counts of the resident label bytes cut by the resident membership words and resampled; the entries of
// a pass are <D.entry>_strata, <D.entry>_boot, <D.entry>_cut_timing and <D.entry>_cut_info (their names are in the messages)
// counts[n_strata][2][VPR_VARTYPES][labels][nq]: the bytes masked by stratum k (comm non-null: one all-reduce of the histogram)
int labelcut_strata(vpr_handle *h, const LabelDesc &D, void *comm, int32_t min_qual, int32_t max_qual, int64_t *counts);
// counts[n_rep][2][VPR_VARTYPES][labels][nq]: every labelled variant counted w(seed, r, sc_key[sc]) times; stratum -1: no mask
int labelcut_boot(vpr_handle *h, const LabelDesc &D, void *comm, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed,
                  int32_t n_rep, int32_t stratum, int64_t *counts);
int labelcut_timing(const vpr_handle *h, const LabelDesc &D, double *ms_strata, double *ms_boot);
// the last launches' shape: strata of a workgroup, chunks, LDS bytes | variant spans, replicate groups, quality slices
int labelcut_info(const vpr_handle *h, const LabelDesc &D, int32_t shape[6]);
