/* vcfdist_matchkind.h -- C ABI of the match kinds on the MI355X: how each true positive was matched.
 *
 * vcfdist_errclass.h says why a call is wrong.  This header says HOW a call is right: the evaluation credits a call that spells the
 * truth differently -- a shifted indel, one record against two, a near miss above the credit threshold -- and precision-recall.tsv
 * prints one TP figure for all of them.  Here every TP gets one of four kinds, the first of which is what an allele-for-allele
 * comparison would have found.
 * **These are this project's own definitions; they are NOT a reproduction of any other tool's match categories**, and the
 * reference (vcfdist v2.6.4) prints TP only.
 *
 * Definitions (everything is tested against these; tests/matchkind_model.py is their brute-force statement).
 *   Everything is local to the supercluster, as in vcfdist_errclass.h: slots 0, 1 are the query haplotypes, slots 2, 3 the truth
 *   haplotypes; the selected phasing w, the compared slot c of a slot s and a copy of a hap-variant are exactly that header's.
 *   For a hap-variant v of slot s in supercluster sc, with g = sync_group[s][w][v]:
 *   - the members M(x, g) of a slot x are the hap-variants u of slot x in v's supercluster with errtype[x][w][u] < 3 and
 *     sync_group[x][w][u] == g;  nO = |M(s, g)| (it counts v itself), nC = |M(c, g)|;
 *   - the members of a group are NOT contiguous in a slot: a query variant passed on the REF plane gets a group id of its own
 *     and can sit between two members of one group; variants that no alignment wrote keep ERRTYPE_UN and group 0, which is why
 *     the errtype < 3 condition is there;
 *   - v is matched iff errtype[s][w][v] is TP, for query and for truth alike.
 *   The kind of a matched variant is the FIRST of
 *     VPR_MK_EXACT      some u in M(c, g) is a copy of v (even where the rest of the group is matched otherwise);
 *     VPR_MK_SHIFTED    query_ed[s][w][v] == 0, nO == 1 and nC == 1: one record against one record, the same haplotype, another
 *                       placement or other bytes;
 *     VPR_MK_REGROUPED  query_ed == 0 otherwise: split, merged or complex (this includes nC == 0);
 *     VPR_MK_PARTIAL    query_ed > 0: credited at or above the credit threshold without reproducing the truth haplotype.
 *   Every other variant has VPR_MK_NONE (255) and is not counted.
 *
 * Counting: counts[2 callsets][VPR_VARTYPES][VPR_MK_KINDS][nq], nq = max_qual - min_qual + 1, the bin of a variant by the quality
 * rule of vpr_pr_counts.  A matched variant of either callset counts in its kind at every threshold index <= its bin (at none when
 * callq < min_qual); ALL is the sum of the three types.  This is the counters' rule cut by kind: for every type and threshold the
 * query's four kinds sum to vpr_pr_counts' query TP and the truth's four to its truth TP.
 *
 * Device code: pr_matchkind.hip (k_matchkind).  No CPU fallback.
 */
#ifndef VCFDIST_MATCHKIND_H_
#define VCFDIST_MATCHKIND_H_

#include "vcfdist_pr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_MK_EXACT 0
#define VPR_MK_SHIFTED 1
#define VPR_MK_REGROUPED 2
#define VPR_MK_PARTIAL 3
#define VPR_MK_KINDS 4
#define VPR_MK_NONE 255

/* Gives every TP of the batch the last vpr_execute evaluated its kind, on the device (on the handle's stream), and counts them:
   counts[2][VPR_VARTYPES][VPR_MK_KINDS][nq].  `v`, var_class, pb_phase, the host checks, the state rules and the return codes are
   those of vpr_errclass (vcfdist_errclass.h); there is no window, and a quality range of more than 1364 thresholds is VPR_ERR_ARG
   (the block histogram lives in LDS).  The per-variant kind bytes stay resident until the next upload
   or vpr_destroy. */
int vpr_matchkind(vpr_handle *h, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                  int32_t min_qual, int32_t max_qual, int64_t *counts);
/* The same with ONE all-reduce of the device histogram over the ranks of nccl_comm (an ncclComm_t), as vpr_allreduce_counts. */
int vpr_allreduce_matchkind(vpr_handle *h, void *nccl_comm, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS],
                            const int32_t *pb_phase, int32_t min_qual, int32_t max_qual, int64_t *counts);
/* The kind bytes (VPR_MK_*) of the last vpr_matchkind, kind[slot][n_var of the slot].  VPR_ERR_STATE before a call and after the
   next upload. */
int vpr_matchkind_download(vpr_handle *h, uint8_t *const kind[VPR_HAPS]);
/* Device time (HIP events on the handle's stream, ms) of the last vpr_matchkind's kernel launches (uploads excluded). */
int vpr_matchkind_timing(const vpr_handle *h, double *ms);
/* The static table of the VPR_MK_KINDS names: exact, shifted, regrouped, partial. */
const char *const *vpr_matchkind_names(void);

/* <prefix>match-kinds.tsv: the rows and the leading VAR_TYPE, MIN_QUAL columns of precision-recall.tsv, then QUERY_TP and its
   four kinds, TRUTH_TP and its four.  <prefix>match-kinds-summary.tsv: the NONE and BEST rows and the leading columns of
   precision-recall-summary.tsv, then the same ten columns.  kind_counts: vpr_matchkind's counts; pr_counts: vpr_pr_counts' of
   the same evaluation, from which BEST is taken by vpr_pr_summary's rule.  Host code; an error's text is vrp_last_error()'s
   (include/vcfdist_report.h). */
int vrp_write_match_kinds(const char *prefix, const int64_t *kind_counts, const int64_t *pr_counts, int32_t min_qual,
                          int32_t max_qual);

#ifdef __cplusplus
}
#endif

/* The kind counts cut by stratum and resampled, by the definitions of vcfdist_errclass.h ("Cut by stratum and resampled") with
   the kinds as labels: for every stratum (replicate), type and threshold the query's kinds sum to QUERY_TP of vpr_pr_counts_strata
   (vpr_pr_counts_boot) and the truth's to its TRUTH_TP.  The entries and the writers of stratified-match-kinds*.tsv and
   bootstrap-match-kinds-summary.tsv: */
#include "vcfdist_labelcut.h"

#endif /* VCFDIST_MATCHKIND_H_ */
