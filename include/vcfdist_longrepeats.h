/* vcfdist_longrepeats.h -- C ABI of the long repeat strata on the MI355X: where the reference sequence is not unique for k-mers
 * of 33 to 256 bases, the lengths of reads.
 *
 * vcfdist_repeats.h stops at k = 32, where a canonical k-mer fills one 64-bit sort key.  The tracks that answer "could a 150- or
 * 250-base read be placed here?" are built from 100-mers and 250-mers.  vpr_longrepeat_intervals finds the repeated k-mers of all
 * contigs for such k with the 64-bit sort the project has, by rank doubling over the repeated k-mers only (below), and turns them
 * into the sorted interval lists of a vpr_strata, which enter vpr_strata_masks / vpr_context_masks as ordinary BED rows.
 *
 * Definitions (everything is tested against these; tests/longrepeats_model.py is their statement over Python bytes).  The genome is
 * the contigs s_c[0..L_c), upper-case bytes.  A long repeat stratum is (k, slop) with 33 <= k <= 256 and slop >= 0, a
 * vpr_repeat_stratum.  Steps 1, 3, 4 and 5 are those of vcfdist_repeats.h, word for word:
 *   1. Valid start.  Start (c, i) is valid iff i + k <= L_c and all k bases s_c[i..i+k) are called.
 *   2. Canonical k-mer.  canon is the lexicographically smaller of the k-mer and its reverse complement, as strings over
 *      A < C < G < T.  For k <= 32 this is min(fwd, rc) of vcfdist_repeats.h: the two definitions are one family.
 *   3. Repeated start.  rep(c, i) holds iff the start is valid and some OTHER valid start (c', i') != (c, i), on any contig, has
 *      the same canon.  A k-mer equal to its own reverse complement that occurs at one start is not repeated.  Overlapping
 *      occurrences count: inside a homopolymer of k + 1 bases both starts are repeated.  Occurrences on different contigs count.
 *      Only exact matches count.
 *   4. Tracts.  Every maximal run [a, b) of repeated starts within a contig gives the tract [a, b - 1 + k): the bases covered by
 *      at least one repeated k-mer.  A tract never leaves its contig, because a valid start has i + k <= L_c.
 *   5. Pad and merge.  Tracts are padded to [max(0, start - slop), min(L_c, stop + slop)); padded tracts that overlap or abut
 *      are merged into their union.
 * The result per (stratum, contig) is sorted, non-overlapping and non-empty: the contract of vpr_strata.
 *
 * This is in the spirit of exact-match mappability tracks (GIAB's LowMappability set has an exact-match 250-mer member) and NOT a
 * reproduction of GIAB's BEDs: it matches exactly (no mismatches), it compares both strands, and a base is in the stratum when
 * some repeated k-mer covers it.
 *
 * Method (pr_longrepeats.hip).  Only equality classes matter.  For a length a every global start g has two 32-bit ids, F_a[g] of
 * the a-mer at g and R_a[g] of its reverse complement, built as (class rank << 1) | orientation, so that two oriented a-mers are
 * equal exactly when their ids are.  The base level a = 32 comes from the pack, sort and neighbour compare of vcfdist_repeats.h.
 * A level a -> b (a < b <= 2a, d = b - a) sorts the keys min((F_a[g] << 32) | F_a[g + d], (R_a[g + d] << 32) | R_a[g]) of the
 * starts whose two halves are kept, 32 -> 64 -> 128 -> k without the levels above k; the last level marks.  A level keeps an
 * a-mer iff its canonical class has at least two starts OR it is its own reverse complement: a reverse palindrome of b + d bases
 * placed once has two repeated b-mers whose shared a-mer occurs nowhere else.
 *
 * Limits: 33 <= k <= 256; at most 2^32 - 1 bases in total (the sort's values are 32-bit global starts); a contig of at most
 * INT32_MAX bases; fewer than 2^31 - 1 kept classes at a level (checked when it runs; real genomes are nowhere near).  Device memory
 * (pr_longrepeats.hip has it as csrc/pr_kmer.h's plus the ids), with N the bases padded to whole tiles of 4096 plus one tile: N bytes (the
 * sequence) + N / 8 (the flag bits) + 16 N (four id arrays: F and R of the level read and of the level written) + per valid
 * 32-mer start 2 x 12 bytes (the base level's key and value, double-buffered for the sort) and 8 bytes (class heads and their
 * scan); the upper levels use the same buffers for their candidates only, which are fewer; + rocPRIM's temporary + what the run
 * passes take (pr_context.hip).
 *
 * Device code: pr_longrepeats.hip (ids, pairs, ranks), pr_repeats.hip (pack, mark), pr_plan.hip (sort, scan), pr_context.hip (the
 * run passes).  No CPU fallback.
 */
#ifndef VCFDIST_LONGREPEATS_H_
#define VCFDIST_LONGREPEATS_H_

#include "vcfdist_repeats.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_LREP_MIN_K 33
#define VPR_LREP_MAX_K 256
#define VPR_LREP_MAX_SPEC 8

/* The default set of the command lines (the one copy both use): rep_k64, rep_k100, rep_k250, all with slop 0.  The tables are
   static. */
int vpr_longrepeats_default(const vpr_repeat_stratum **spec, const char *const **names, int32_t *n);

/* Builds the intervals of every spec entry for the whole genome in one call, on the handle's stream: ctg_off[n_ctg + 1] are the
   contigs' offsets into the concatenated ctg_seq (ctg_off[0] == 0).  The handle needs no batch.  Within the call the base level
   and the levels 64 and 128 are computed once and shared by the entries that need them.  The intervals stay with the handle until
   the next vpr_longrepeat_intervals or vpr_destroy and are independent of those of vpr_repeat_intervals on the same handle; a
   refused call leaves none.  VPR_ERR_ARG, with a message that names the entry, for a spec outside the limits, n_spec outside
   1..VPR_LREP_MAX_SPEC, ctg_off[0] != 0, a contig above INT32_MAX bases and a total above UINT32_MAX bases -- all checked before a
   byte of ctg_seq is read; an exhausted device is VPR_ERR_NOMEM with the bytes needed in the message; 2^31 - 1 or more kept
   classes at a level is VPR_ERR_ARG with the level and the count.  Two calls on the same input give identical arrays. */
int vpr_longrepeat_intervals(vpr_handle *h, int32_t n_ctg, const int64_t *ctg_off, const uint8_t *ctg_seq, const vpr_repeat_stratum *spec,
                             int32_t n_spec);
/* The intervals of the last vpr_longrepeat_intervals (VPR_ERR_STATE before a successful one): iv_off[n_spec * n_ctg + 1], row =
   spec * n_ctg + ctg, and the intervals themselves (0-based half-open, contig coordinates), iv_off[n_spec * n_ctg] of each. */
int vpr_longrepeat_interval_counts(vpr_handle *h, int64_t *iv_off);
int vpr_longrepeat_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop);
/* int64_t[n_spec] each: the valid starts, the repeated starts and the candidates of the last level (the pairs it sorted) of every
   entry of the last call; n_level[3] (may be null): the pairs sorted by the base level (the valid 32-mer starts) and the
   candidates of the levels 64 and 128 (0 for a level the call did not need). */
int vpr_longrepeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_repeated, int64_t *n_last, int64_t *n_level);
/* Device time (HIP events on the handle's stream, ms) of the last call's passes: the base level (pack, sort, ranks, ids), the
   doubling levels 64 and 128 (pairs, sort, ranks, ids), the entries' last levels (valid starts, pairs, sort, mark) and the run
   passes that make the intervals.  The sequence upload is excluded. */
int vpr_longrepeat_timing(const vpr_handle *h, double *ms_base, double *ms_levels, double *ms_last, double *ms_intervals);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_LONGREPEATS_H_ */
