/* vcfdist_errclass.h -- C ABI of the error classes on the MI355X: why each false positive and false negative is wrong.
 *
 * The strata headers cut the one evaluation by region, sequence context and what the variants are.  This header says WHY a call
 * is wrong: for every query FP and truth FN, whether the allele is present elsewhere in the other callset (wrong genotype, same
 * haplotype, other haplotype), whether the other callset has anything at the site or near it, or nothing at all.
 * **These are this project's own definitions, in the spirit of hap.py's FP.gt / FP.al columns; they are NOT a reproduction of
 * hap.py**, and the reference (vcfdist v2.6.4) prints SNP / INDEL / SV / ALL only.
 *
 * Definitions (everything is tested against these; tests/errclass_model.py is their brute-force statement).
 *   Everything is local to the supercluster, the unit the evaluation aligns and credits on its own: every search below runs over
 *   the variants of v's own supercluster sc only, [var_off[slot][sc], var_off[slot][sc + 1]).  (Under a sharding by
 *   superclusters a rank therefore classifies its own share and never sees a shard's edge.)
 *   Slots 0, 1 are the query haplotypes, slots 2, 3 the truth haplotypes.  For a hap-variant v of slot s in supercluster sc:
 *   - the selected phasing w is the choice the counters make: sc_phase ORIG gives 0, SWAP gives 1, NONE gives pb_phase[sc] != 0,
 *     or 0 when pb_phase is null;  e(v), callq(v) are the errtype and callq of v in that phasing;
 *   - the partner slot is s ^ 1 (the other haplotype of v's callset);
 *   - the compared slot is the haplotype of the other callset that v's haplotype was aligned to under w (ORIG pairs q1-t1,
 *     q2-t2; SWAP pairs q1-t2, q2-t1): 2 + (s ^ w) for a query slot s, (s - 2) ^ w for a truth slot s;
 *   - the cross slot is the other haplotype of the other callset;
 *   - a copy of v is a hap-variant of v's supercluster that agrees with v on pos, type, ref_len, alt_len and all ALT bytes
 *     (vcfdist_varstrata.h's copy, restricted to the supercluster).
 *   A hap-variant is an error iff it is a query variant with e == FP or a truth variant with e == FN.  Its class is the FIRST of
 *     VPR_EC_GT     a copy of v in the partner slot has errtype TP in the selected phasing (a zygosity error);
 *     VPR_EC_SYNC   a copy of v lies in the compared slot (the allele is where it was aligned to and fails with its sync group);
 *     VPR_EC_PHASE  a copy of v lies in the cross slot (the allele is there, on the other haplotype);
 *     VPR_EC_SITE   some hap-variant of the other callset (either slot) starts at exactly pos_v;
 *     VPR_EC_NEAR   some hap-variant of the other callset starts within W bases, 0 < |pos_u - pos_v| <= W (start positions only,
 *                   as for VPR_VS_NEAR);
 *     VPR_EC_ALONE  none of the above.
 *   VPR_EC_LOWQ exists for truth only: a truth variant with e == TP.  It appears as FN above its own quality threshold only.
 *   A variant with e >= 3 (not counted), a query variant that is not FP and a truth-side FP have class VPR_EC_NONE (255) and are
 *   not counted.  (The evaluation gives a truth variant TP or FN only.)
 *   W is the argument `window` >= 0; VPR_EC_DEFAULT_WINDOW = 50 is this project's choice (it matches the stratum iso_50).
 *
 * Counting: counts[2 callsets][VPR_VARTYPES][VPR_EC_CLASSES][nq], nq = max_qual - min_qual + 1, the bin of a variant by the
 * quality rule of vpr_pr_counts.  A query FP counts in its class at every threshold index <= its bin (at none when
 * callq < min_qual); a truth FN counts in its class at every threshold; a LOWQ truth variant at every threshold above its own bin
 * (at every threshold when callq < min_qual); ALL is the sum of the three types.  This is the counters' rule cut by class: for every
 * type and threshold the query's classes sum to vpr_pr_counts' query FP and the truth's classes to its truth FN.
 *
 * Cut by stratum and resampled (the declarations are in vcfdist_labelcut.h, included below; tests/labelcut_model.py states this in
 * terms of tests/errclass_model.py).  A label pass P is the error classes or the match kinds (vcfdist_matchkind.h); its bytes are b,
 * its counts C_P(b), [2][VPR_VARTYPES][L][nq], by the counting rule above.
 *   Stratum cut.  counts[k] = C_P(b masked by stratum k): the mask replaces the byte of every hap-variant whose bit k of the resident
 *     membership words (vcfdist_strata.h) is clear by "no label".  Query and truth variants are each assigned by their own
 *     membership, as everywhere else.  So for every stratum, type and threshold the query's classes sum to QUERY_FP of
 *     vpr_pr_counts_strata and the truth's to its TRUTH_FN (the kinds: to QUERY_TP and TRUTH_TP), and a stratum that holds every
 *     variant reproduces the unstratified counts exactly.
 *   Replicates.  Replicate r's counts are C_P with every labelled variant counted w(seed, r, key[sc]) times, w exactly
 *     vcfdist_bootstrap.h's weight; conditional on the phasing, as there.  An optional stratum k restricts them as above (-1: none).
 *     For every replicate the labels sum to the matching column of vpr_pr_counts_boot.
 *   Intervals.  For each label-count column at the NONE and BEST rows the replicate counts are sorted as integers;
 *     LO = x[floor(0.025 n)], HI = x[ceil(0.975 n) - 1].  BEST's quality is the point estimate's, not re-optimised per replicate.
 *   A cut uses the phasing the bytes were made under: the label call's phase-block words stay on the device, and the cut entries
 *   take no pb_phase and no var_class.
 *
 * Device code: pr_errclass.hip (k_errclass); pr_cut.hip for the cuts.  No CPU fallback.
 */
#ifndef VCFDIST_ERRCLASS_H_
#define VCFDIST_ERRCLASS_H_

#include "vcfdist_pr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_EC_GT 0
#define VPR_EC_SYNC 1
#define VPR_EC_PHASE 2
#define VPR_EC_SITE 3
#define VPR_EC_NEAR 4
#define VPR_EC_ALONE 5
#define VPR_EC_LOWQ 6
#define VPR_EC_CLASSES 7
#define VPR_EC_NONE 255
#define VPR_EC_DEFAULT_WINDOW 50

/* Classifies the errors of the batch the last vpr_execute evaluated, on the device (on the handle's stream), and counts them:
   counts[2][VPR_VARTYPES][VPR_EC_CLASSES][nq].  `v` holds the variant tables the batch was made from: its n_sc and per-slot
   variant counts must equal the resident batch's (VPR_ERR_STATE otherwise).  Read and uploaded for the call: var_off, var_pos,
   var_type, var_ref_len, var_alt_len, var_alt_off and allele_pool.  var_class / pb_phase as for vpr_pr_counts (var_class may be
   NULL when the classes are resident).  Checked on the host before anything is launched (VPR_ERR_ARG with a message that names
   the place): var_off starts at 0 and is monotone; var_pos is non-decreasing within each supercluster's range (no order between
   superclusters is required); allele offsets and lengths are non-negative; window >= 0; min_qual <= max_qual; a quality range of
   at most 779 thresholds (the block histogram is in LDS).  An exhausted device is VPR_ERR_NOMEM.  The per-variant class bytes stay resident until the next upload or vpr_destroy. */
int vpr_errclass(vpr_handle *h, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                 int32_t window, int32_t min_qual, int32_t max_qual, int64_t *counts);
/* The same with ONE all-reduce of the device histogram over the ranks of nccl_comm (an ncclComm_t), as vpr_allreduce_counts. */
int vpr_allreduce_errclass(vpr_handle *h, void *nccl_comm, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS],
                           const int32_t *pb_phase, int32_t window, int32_t min_qual, int32_t max_qual, int64_t *counts);
/* The class bytes (VPR_EC_*) of the last vpr_errclass, cls[slot][n_var of the slot].  VPR_ERR_STATE before a call and after the
   next upload. */
int vpr_errclass_download(vpr_handle *h, uint8_t *const cls[VPR_HAPS]);
/* Device time (HIP events on the handle's stream, ms) of the last vpr_errclass' kernel launches (uploads excluded). */
int vpr_errclass_timing(const vpr_handle *h, double *ms);
/* The static table of the VPR_EC_CLASSES names: gt, sync, phase, site, near, alone, lowq. */
const char *const *vpr_errclass_names(void);

/* <prefix>error-classes.tsv: the rows and the leading VAR_TYPE, MIN_QUAL columns of precision-recall.tsv, then QUERY_FP and its
   six classes, TRUTH_FN and its seven.  <prefix>error-classes-summary.tsv: the NONE and BEST rows and the leading columns of
   precision-recall-summary.tsv, then the same fifteen columns.  class_counts: vpr_errclass' counts; pr_counts: vpr_pr_counts'
   of the same evaluation, from which BEST is taken by vpr_pr_summary's rule.  Host code; an error's text is vrp_last_error()'s
   (include/vcfdist_report.h). */
int vrp_write_error_classes(const char *prefix, const int64_t *class_counts, const int64_t *pr_counts, int32_t min_qual,
                            int32_t max_qual);

#ifdef __cplusplus
}
#endif

/* the class counts cut by stratum and resampled: the entries and the writers of stratified-error-classes*.tsv and
   bootstrap-error-classes-summary.tsv */
#include "vcfdist_labelcut.h"

#endif /* VCFDIST_ERRCLASS_H_ */
