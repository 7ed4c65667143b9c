/* vcfdist_bootstrap.h -- C ABI of the bootstrap confidence intervals for precision, recall and F1 on the MI355X.
 *
 * One evaluation, resampled afterwards: the per-variant results of vpr_execute stay on the device, and the histogram behind
 * vpr_pr_counts is repeated n_rep times with every supercluster's variants counted w times.  The reference (vcfdist v2.6.4)
 * prints its figures without an interval; rerunning it on resampled inputs changes clusters and phasing and is therefore
 * not a resampling of one evaluation.
 *
 * The definition (everything is tested against it):
 *
 * Poisson bootstrap over superclusters.  The supercluster is the evaluation's independent unit (every one is aligned and
 * credited on its own).  Replicate r (0 <= r < n_rep) gives supercluster s the integer weight w(seed, r, key[s]), where
 * key[s] is a 64-bit identity the caller supplies.  Both command lines use
 *     key = (ordinal of the contig in the run's contig list << 32) | index of the supercluster within its contig
 * so that a rank's share, a split batch and a permuted batch all draw the same weights.  All arithmetic is mod 2^64:
 *
 *     z = key + 0x9E3779B97F4A7C15 * (r + 1) + seed * 0xD1B54A32D192ED03
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z =  z ^ (z >> 31)
 *     u = z >> 32                                                 (32 bits)
 *     w = number of k in 0..11 with u >= T[k]                     (0 <= w <= 12)
 *     T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!)                 (the Poisson(1) distribution function, VPR_BOOT_T below)
 *
 * Replicate counts.  Replicate r's counters are vpr_pr_counts' counters with every variant counted w times, w being the
 * weight of the variant's supercluster.  Everything else is vpr_pr_counts': the sc_phase / pb_phase choice of the ORIG or
 * SWAP columns, the class, the quality bin, the skip of errtype >= 3.  The phasing is the point estimate's: this is a
 * bootstrap CONDITIONAL ON THE PHASING (a replicate does not re-run the phasing of its resampled superclusters).
 *
 * Intervals (vrp_write_bootstrap).  Per VAR_TYPE and per threshold row of precision-recall-summary.tsv (NONE and BEST; BEST's
 * quality is the point estimate's and is NOT re-optimised per replicate), precision, recall and F1 of every replicate at that
 * quality are each sorted ascending as floats; LO = x[floor(0.025 * n_rep)], HI = x[ceil(0.975 * n_rep) - 1]: the 95 %
 * percentile interval (x[25] and x[974] of 1 000; both x[0] of 1).
 *
 * Device code: pr_cut.hip (k_pr_boot).  No CPU fallback.
 */
#ifndef VCFDIST_BOOTSTRAP_H_
#define VCFDIST_BOOTSTRAP_H_

#include "vcfdist_pr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_BOOT_MAX_WEIGHT 12
#define VPR_BOOT_MAX_REPLICATES 100000
#define VPR_BOOT_T { 1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, \
                     4294609777u, 4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u }

/* The replicate counters of the batch the last vpr_execute evaluated: counts[n_rep][2][VPR_VARTYPES][3][max_qual-min_qual+1],
   replicate r laid out as vpr_pr_counts lays out its result.  var_class, pb_phase, min_qual, max_qual: as vpr_pr_counts.
   sc_key[n_sc of the executed batch]; 1 <= n_rep <= VPR_BOOT_MAX_REPLICATES.  stratum = -1 counts every variant; stratum = k
   >= 0 only the variants whose bit k is set in the resident membership words (include/vcfdist_strata.h): VPR_ERR_STATE without
   words or with words of another batch, VPR_ERR_ARG when k >= n_strata.  VPR_ERR_STATE before vpr_execute; VPR_ERR_ARG for a
   null sc_key or counts or an n_rep out of range; VPR_ERR_NOMEM when the replicate histogram cannot be allocated. */
int vpr_pr_counts_boot(vpr_handle *h, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase, int32_t min_qual,
                       int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep, int32_t stratum, int64_t *counts);
/* The same with one ncclAllReduce of the whole replicate histogram, in place on the device, between the kernel and the copy
   (see vpr_allreduce_counts): every rank passes its share's keys and gets the sum. */
int vpr_allreduce_counts_boot(vpr_handle *h, void *nccl_comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                              int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep,
                              int32_t stratum, int64_t *counts);
/* The last replicate call's launch shape -- grid[0] the largest number of variant spans of a hap slot, grid[1] the groups
   of 64 replicates, grid[2] the slices of the quality bins -- and the device time of its launches (HIP events on the
   handle's stream, ms).  VPR_ERR_ARG before the first call. */
int vpr_boot_info(const vpr_handle *h, int32_t grid[3], double *ms);

/* <prefix>bootstrap-precision-recall-summary.tsv (the rows and point columns of precision-recall-summary.tsv with the
   interval bounds) and <prefix>bootstrap-replicates.tsv (every replicate's row per type and threshold) from the point
   counters (vpr_pr_counts) and the replicate counters (vpr_pr_counts_boot), both summed over contigs by the caller.
   Return codes and vrp_last_error: include/vcfdist_report.h. */
int vrp_write_bootstrap(const char *prefix, const int64_t *counts, const int64_t *counts_boot, int32_t n_rep, uint64_t seed,
                        int32_t min_qual, int32_t max_qual);
/* <prefix>stratified-bootstrap-precision-recall-summary.tsv: the first table once per stratum behind a leading STRATUM
   column; counts[n_strata][...] (vpr_pr_counts_strata), counts_boot[n_strata][n_rep][...] (one vpr_pr_counts_boot per
   stratum).  No replicate file. */
int vrp_write_bootstrap_stratified(const char *prefix, const char *const *names, int32_t n_strata, const int64_t *counts,
                                   const int64_t *counts_boot, int32_t n_rep, uint64_t seed, int32_t min_qual, int32_t max_qual);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_BOOTSTRAP_H_ */
