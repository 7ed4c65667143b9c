/* vcfdist_strata.h -- C ABI of the region-stratified precision/recall counters on the MI355X.
 *
 * One evaluation, cut by region afterwards: the per-variant results of vpr_execute stay on the device, every variant gets
 * a bit per stratum (a stratum is a BED: the GIAB stratifications), and the histogram behind vpr_pr_counts is repeated into
 * every stratum whose bit is set.  The reference (vcfdist v2.6.4) has no such output; the only way to get one there is to
 * rerun the whole evaluation once per BED, which changes the clusters and is therefore not a cut of one evaluation.
 *
 * Membership (the definition everything is tested against): variant v of a hap slot belongs to stratum k iff
 *     vio_bed_contains(bed_k, contig(v), pos, pos + ref_len, type) == VIO_BED_INSIDE          (include/vcfdist_io.h)
 * on the variant's parsed columns (var_pos, var_ref_len, var_type of vpr_variants; an insertion has ref_len 0, hence
 * start == stop).  BORDER, OUTSIDE and OFFCTG are all "not a member".  Query and truth variants are each assigned by their
 * own position.
 *
 * Device code: pr_strata.hip (k_strata_mask), pr_cut.hip (k_pr_hist_strata).  No CPU fallback.
 */
#ifndef VCFDIST_STRATA_H_
#define VCFDIST_STRATA_H_

#include "vcfdist_pr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Intervals are 0-based half-open; per (stratum, contig) sorted, non-overlapping and non-empty (abutting ones are allowed,
   as in the reference's BED check).  Anything else is VPR_ERR_ARG with a message. */
typedef struct vpr_strata {
    int32_t n_strata, n_ctg;          /* contig numbering = the vpr_variants passed with it */
    const int64_t *iv_off;            /* [n_strata * n_ctg + 1], row = stratum * n_ctg + ctg */
    const int32_t *iv_start, *iv_stop;
} vpr_strata;

/* Membership words of the variants of `v`, computed on the device on the handle's stream and kept resident there: bit
   k & 63 of word k >> 6 of a variant is its membership of stratum k.  `v` need not be the executed batch (a sharded caller
   computes a whole contig's words and keeps its share); only var_off, sc_ctg, var_pos, var_ref_len and var_type are read
   and uploaded.  Any n_strata >= 1; n_strata = 0 is VPR_ERR_ARG.  The words are released when the next batch is uploaded
   (not by a further vpr_execute of the same batch). */
int vpr_strata_masks(vpr_handle *h, const vpr_variants *v, const vpr_strata *s);
/* The resident words of each hap slot, word-major: mask[slot][w * n_var[slot] + variant], w < (n_strata + 63) / 64.
   VPR_ERR_STATE without resident words. */
int vpr_strata_download_masks(vpr_handle *h, uint64_t *const mask[VPR_HAPS]);
/* Makes caller-supplied words resident (a rank's share, or words made elsewhere), same layout. */
int vpr_strata_upload_masks(vpr_handle *h, int32_t n_strata, const int64_t n_var[VPR_HAPS], const uint64_t *const mask[VPR_HAPS]);
/* vpr_pr_counts, repeated into every stratum whose bit is set: counts[n_strata][2][VPR_VARTYPES][3][max_qual-min_qual+1].
   VPR_ERR_STATE unless words are resident whose per-slot variant counts equal the executed batch's. */
int vpr_pr_counts_strata(vpr_handle *h, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                         int32_t min_qual, int32_t max_qual, int64_t *counts);
/* The same with one ncclAllReduce of the whole stratified histogram, in place on the device, between the kernel and the
   copy (see vpr_allreduce_counts). */
int vpr_allreduce_counts_strata(vpr_handle *h, void *nccl_comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                                int32_t min_qual, int32_t max_qual, int64_t *counts);
/* Device time (HIP events on the handle's stream, ms) of the last vpr_strata_masks' kernel launches and of the last
   stratified histogram's; 0 where none has run since the words were made resident. */
int vpr_strata_timing(const vpr_handle *h, double *ms_mask, double *ms_hist);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_STRATA_H_ */
