/* vcfdist_labelcut.h -- the declarations behind the last sections of vcfdist_errclass.h and vcfdist_matchkind.h, which include
 * this file: the label counts of a label pass (the error classes, the match kinds) cut by stratum and resampled.  The definitions
 * are in vcfdist_errclass.h ("Cut by stratum and resampled"); tests/labelcut_model.py states them in terms of the passes' models.
 *
 * Device code: pr_cut.hip (k_label_hist_strata, k_label_boot; both generic over the pass).  No CPU fallback.
 */
#ifndef VCFDIST_LABELCUT_H_
#define VCFDIST_LABELCUT_H_

#include "vcfdist_pr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The class counts of the last vpr_errclass cut by the resident membership words (include/vcfdist_strata.h):
   counts[n_strata][2][VPR_VARTYPES][VPR_EC_CLASSES][nq], stratum k laid out as vpr_errclass lays out its result.  The entry takes
   no var_class and no pb_phase: the classes are the resident ones, the phasing is the one the vpr_errclass call was made under
   (its phase-block words stay on the device).  VPR_ERR_STATE without valid class bytes (before vpr_errclass, or after the next
   upload) and without resident words whose per-slot variant counts equal the batch's; VPR_ERR_ARG for a null counts,
   max_qual < min_qual or more thresholds than vpr_errclass takes (before any allocation); VPR_ERR_NOMEM when the histogram
   cannot be allocated.  Every message names the entry. */
int vpr_errclass_strata(vpr_handle *h, int32_t min_qual, int32_t max_qual, int64_t *counts);
/* The same with ONE all-reduce of the device histogram over the ranks of nccl_comm, between the kernel and the copy. */
int vpr_allreduce_errclass_strata(vpr_handle *h, void *nccl_comm, int32_t min_qual, int32_t max_qual, int64_t *counts);
/* The replicates of the class counts of the last vpr_errclass: counts[n_rep][2][VPR_VARTYPES][VPR_EC_CLASSES][nq].
   sc_key[n_sc of the executed batch], seed, n_rep (1 .. VPR_BOOT_MAX_REPLICATES) and stratum (-1: every variant; k >= 0: the
   variants of stratum k of the resident words, VPR_ERR_ARG when k >= n_strata) are vpr_pr_counts_boot's
   (include/vcfdist_bootstrap.h); the states and the other refusals are vpr_errclass_strata's. */
int vpr_errclass_boot(vpr_handle *h, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep,
                      int32_t stratum, int64_t *counts);
int vpr_allreduce_errclass_boot(vpr_handle *h, void *nccl_comm, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key,
                                uint64_t seed, int32_t n_rep, int32_t stratum, int64_t *counts);
/* Device time (HIP events on the handle's stream, ms) of the last vpr_errclass_strata's and the last vpr_errclass_boot's kernel
   launches (0 before a call). */
int vpr_errclass_cut_timing(const vpr_handle *h, double *ms_strata, double *ms_boot);
/* The last launches' shape: shape[0] the strata of a workgroup of the stratum cut (a power of two up to 64, chosen from a 40 KiB
   LDS budget; 1 when one stratum's bins exceed it), shape[1] its chunks, shape[2] its LDS bytes; shape[3] the largest number of
   variant spans of a hap slot of the replicate cut, shape[4] its groups of 64 replicates, shape[5] its slices of the quality bins. */
int vpr_errclass_cut_info(const vpr_handle *h, int32_t shape[6]);

/* The same six for the kinds of the last vpr_matchkind: counts[...][2][VPR_VARTYPES][VPR_MK_KINDS][nq]. */
int vpr_matchkind_strata(vpr_handle *h, int32_t min_qual, int32_t max_qual, int64_t *counts);
int vpr_allreduce_matchkind_strata(vpr_handle *h, void *nccl_comm, int32_t min_qual, int32_t max_qual, int64_t *counts);
int vpr_matchkind_boot(vpr_handle *h, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep,
                       int32_t stratum, int64_t *counts);
int vpr_allreduce_matchkind_boot(vpr_handle *h, void *nccl_comm, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key,
                                 uint64_t seed, int32_t n_rep, int32_t stratum, int64_t *counts);
int vpr_matchkind_cut_timing(const vpr_handle *h, double *ms_strata, double *ms_boot);
int vpr_matchkind_cut_info(const vpr_handle *h, int32_t shape[6]);

/* <prefix>stratified-error-classes.tsv and <prefix>stratified-error-classes-summary.tsv: the two tables of
   vrp_write_error_classes once per stratum behind a leading STRATUM column, strata in table order.  class_counts[n_strata][...]:
   vpr_errclass_strata's; pr_counts[n_strata][...]: vpr_pr_counts_strata's of the same evaluation, from which BEST is taken per
   stratum by the rule of stratified-precision-recall-summary.tsv.  Host code; errors as include/vcfdist_report.h. */
int vrp_write_error_classes_stratified(const char *prefix, const char *const *names, int32_t n_strata, const int64_t *class_counts,
                                       const int64_t *pr_counts, int32_t min_qual, int32_t max_qual);
/* <prefix>bootstrap-error-classes-summary.tsv: the rows and columns of error-classes-summary.tsv with every count column followed
   by its _LO and _HI, all integers.  class_counts: vpr_errclass'; pr_counts: vpr_pr_counts' (BEST's quality is the point
   estimate's); class_boot[n_rep][...]: vpr_errclass_boot's.  Per column the replicate counts are sorted as integers,
   LO = x[floor(0.025 n)], HI = x[ceil(0.975 n) - 1].  There is no replicate file. */
int vrp_write_error_classes_bootstrap(const char *prefix, const int64_t *class_counts, const int64_t *pr_counts, const int64_t *class_boot,
                                      int32_t n_rep, int32_t min_qual, int32_t max_qual);
/* stratified-match-kinds.tsv, stratified-match-kinds-summary.tsv and bootstrap-match-kinds-summary.tsv, in the same way. */
int vrp_write_match_kinds_stratified(const char *prefix, const char *const *names, int32_t n_strata, const int64_t *kind_counts,
                                     const int64_t *pr_counts, int32_t min_qual, int32_t max_qual);
int vrp_write_match_kinds_bootstrap(const char *prefix, const int64_t *kind_counts, const int64_t *pr_counts, const int64_t *kind_boot,
                                    int32_t n_rep, int32_t min_qual, int32_t max_qual);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_LABELCUT_H_ */
