/* vcfdist_nearrepeats.h -- C ABI of the near-repeat strata on the MI355X: where a k-mer of the reference occurs again within a few
 * mismatches.
 *
 * vcfdist_repeats.h answers "does this k-mer occur again, exactly?".  A read with a sequencing error or a SNP in it runs into
 * something else: a k-mer that occurs again with up to m substitutions.  Equality classes are gone then, so neither canonical
 * codes nor ranks apply; vpr_nearrepeat_intervals finds the partners exactly by the pigeonhole over m + 1 blocks (two k-mers with
 * at most m mismatches agree on all bases of at least one block): per block one narrow radix sort and a wave-cooperative
 * all-pairs compare inside the runs of equal block bases.  The intervals then enter vpr_strata_masks as ordinary BED rows.
 *
 * Definitions (everything is tested against these; tests/nearrepeats_model.py is their numpy statement).  Genome, called bases,
 * codes and valid starts are those of vcfdist_repeats.h, steps 1 and 2.  F(c, i) is the forward 2-bit code of the k-mer at a
 * valid start (the first base most significant), RC(c, i) the code of its reverse complement, ham(a, b) the number of the k base
 * positions at which two codes differ.  A near-repeat stratum is (k, m, slop) with 0 <= m <= 3, 8 (m + 1) <= k <= 32, slop >= 0.
 *   1. Near-repeated start.  near(c, i) holds iff the start is valid and some OTHER valid start (c', i') != (c, i), on any contig,
 *      has min(ham(F(c, i), F(c', i')), ham(F(c, i), RC(c', i'))) <= m.  The relation is symmetric, because RC is an isometry and
 *      an involution.  A start is never its own partner: a k-mer within m of its own reverse complement that occurs once is not
 *      near-repeated (the palindrome rule of the exact family).  Overlapping occurrences count: with m >= 1 the two starts of a
 *      homopolymer of k bases and its one-base shift are partners at distance 1.  This is intended (within m mismatches the two
 *      placements cannot be told apart).
 *   2. Tracts, pad and merge.  Steps 4 and 5 of vcfdist_repeats.h, unchanged, over the near-repeated starts.
 * At m = 0 the stratum is exactly (k, slop) of vpr_repeat_intervals; the stratum at m contains the stratum at m - 1.
 *
 * The blocks are fixed: block j of m + 1 covers bases [floor(j k / (m + 1)), floor((j + 1) k / (m + 1))) of the compared strings,
 * at most 16 bases for m >= 1.
 *
 * What this is NOT: it is not a reproduction of GIAB's LowMappability BEDs; it counts substitutions only (Hamming distance, no
 * indels); it covers k <= 32 only; and it looks at both strands.
 *
 * Cost.  There is no cap on a run's length and the answer is exact: a record that finds no partner is compared with every
 * record of its run of equal block bases, so the cost is quadratic in the run for such records.  vpr_nearrepeat_stats reports
 * the compares made and the longest run.
 *
 * Limits: at most 2^31 - 1 bases in total (a forward and a reverse-complement record per valid start share one sorted array, the
 * strand in the lowest bit of the 32-bit value); a contig of at most INT32_MAX bases.  Device memory (the formula is repeated in
 * csrc/pr_kmer.h): 1 byte per base (the sequence) + 1/8 byte per base (the flag bits) + per valid start 60 bytes (12 for the
 * packed forward pairs, 2 x 2 x 12 for both strands' key and value, double-buffered for the sort) + rocPRIM's temporary.
 *
 * Device code: pr_nearrepeats.hip (keys, probe), pr_repeats.hip (the pack, with the forward code), pr_plan.hip (the sort),
 * pr_context.hip (the run passes).  No CPU fallback.
 */
#ifndef VCFDIST_NEARREPEATS_H_
#define VCFDIST_NEARREPEATS_H_

#include <stddef.h>
#include "vcfdist_pr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_NREP_MAX_M 3
#define VPR_NREP_MAX_K 32
#define VPR_NREP_MAX_SPEC 4

typedef struct vpr_near_stratum { int32_t k, m, slop; } vpr_near_stratum;

/* There is no default set: the pass is expensive and the user chooses (k, m). */

/* Builds the intervals of every spec entry for the whole genome in one call, on the handle's stream; ctg_off and ctg_seq as for
   vpr_repeat_intervals.  The handle needs no batch.  The intervals stay resident until the next vpr_nearrepeat_intervals or
   vpr_destroy; a refused call leaves none.  VPR_ERR_ARG, with a message that names the entry, for a spec outside the limits, two
   equal entries, n_spec outside 1..VPR_NREP_MAX_SPEC, ctg_off[0] != 0, a contig above INT32_MAX bases and a total above
   2^31 - 1 bases -- all checked before a byte of ctg_seq is read; an exhausted device is VPR_ERR_NOMEM with the bytes needed in
   the message.  Two calls on the same input give identical arrays. */
int vpr_nearrepeat_intervals(vpr_handle *h, int32_t n_ctg, const int64_t *ctg_off, const uint8_t *ctg_seq, const vpr_near_stratum *spec,
                             int32_t n_spec);
/* The intervals of the last vpr_nearrepeat_intervals (VPR_ERR_STATE before a successful one), laid out as those of
   vpr_repeat_interval_counts / vpr_repeat_download_intervals. */
int vpr_nearrepeat_interval_counts(vpr_handle *h, int64_t *iv_off);
int vpr_nearrepeat_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop);
/* int64_t[n_spec] each: the valid starts, the near-repeated starts, the Hamming compares made and the longest run of equal block
   keys (over the entry's blocks; a run holds the records of both strands) of every entry of the last call.  The compares depend
   on the order of the entries' blocks (a start flagged by an earlier block does not probe again), never on the run of the call. */
int vpr_nearrepeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_near, int64_t *n_compares, int64_t *max_run);
/* Device time (HIP events on the handle's stream, ms, summed over the entries) of the last call's passes: pack (count, scan,
   write), sort (the blocks' keys and sorts), probe, and the run passes that make the intervals.  The upload is excluded. */
int vpr_nearrepeat_timing(const vpr_handle *h, double *ms_pack, double *ms_sort, double *ms_probe, double *ms_intervals);
/* The stratum's name in the tables, near_k<K>_m<M>, into buf (the one copy both command lines use); VPR_ERR_ARG if it does not fit. */
int vpr_nearrepeat_name(const vpr_near_stratum *spec, char *buf, size_t size);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_NEARREPEATS_H_ */
