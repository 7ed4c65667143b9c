/* vcfdist_repeats.h -- C ABI of the repeat strata on the MI355X: where the reference sequence is not unique.
 *
 * vcfdist_context.h builds strata whose predicates are local (a base's flag depends on a few neighbours).  Non-uniqueness is a
 * property of the whole genome: every k-mer against every other, on both strands, across contigs.  vpr_repeat_intervals finds
 * the repeated k-mers of all contigs with one 64-bit radix sort per stratum and turns them into the sorted interval lists of a
 * vpr_strata, which then enter vpr_strata_masks / vpr_context_masks as ordinary BED rows.  The reference (vcfdist v2.6.4) has no
 * strata at all.
 *
 * Definitions (everything is tested against these; tests/repeats_model.py is their numpy statement).  The genome is the
 * contigs s_c[0..L_c), upper-case bytes; called bases are coded A=0, C=1, G=2, T=3.  A repeat stratum is (k, slop) with
 * 4 <= k <= 32 and slop >= 0.
 *   1. Valid start.  Start (c, i) is valid iff i + k <= L_c and all k bases s_c[i..i+k) are called.
 *   2. Canonical code.  fwd = sum_j code(s[i+j]) << 2(k-1-j) (the first base is most significant), rc = sum_j (3 - code(s[i+j]))
 *      << 2j (the code of the reverse complement), canon = min(fwd, rc) as unsigned 64-bit.  At k = 32 all 64 bits are used.
 *   3. Repeated start.  rep(c, i) holds iff the start is valid and some OTHER valid start (c', i') != (c, i), on any contig, has
 *      the same canon.  A palindromic k-mer (fwd == rc) that occurs once is not repeated.  Overlapping occurrences count: inside
 *      a homopolymer of k + 1 bases both starts are repeated.  This is intended (the two k-mers cannot be told apart).
 *   4. Tracts.  Every maximal run [a, b) of repeated starts within a contig gives the tract [a, b - 1 + k): the bases covered by
 *      at least one repeated k-mer.  A tract never leaves its contig, because a valid start has i + k <= L_c.
 *   5. Pad and merge.  Tracts are padded to [max(0, start - slop), min(L_c, stop + slop)); padded tracts that overlap or abut
 *      are merged into their union (needed at slop 0 too: two runs one start apart give overlapping tracts).
 * The result per (stratum, contig) is sorted, non-overlapping and non-empty: the contract of vpr_strata.  Membership of a
 * variant is vio_bed_contains(...) == VIO_BED_INSIDE on these intervals, exactly as if they had been written to a BED and
 * passed to --stratify.
 *
 * This is in the spirit of k-mer uniqueness / mappability tracks and NOT a reproduction of GIAB's LowMappability or SegDup
 * BEDs: it matches exactly (no mismatches), k <= 32 (longer k-mers: vcfdist_longrepeats.h), and it compares both strands.
 *
 * Limits: 4 <= k <= 32; at most 2^32 - 1 bases in total (the sort's values are 32-bit global starts); a contig of at most
 * INT32_MAX bases.  Device memory (the formula is repeated in csrc/pr_kmer.h): 1 byte per base (the sequence) + 1/8 byte per
 * base (the flag bits) + per valid start 2 x 12 bytes (key and value, double-buffered for the sort) + rocPRIM's temporary.
 *
 * Device code: pr_repeats.hip (pack, mark), pr_plan.hip (the sort), pr_context.hip (the run passes).  No CPU fallback.
 */
#ifndef VCFDIST_REPEATS_H_
#define VCFDIST_REPEATS_H_

#include "vcfdist_pr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_REP_MIN_K 4
#define VPR_REP_MAX_K 32
#define VPR_REP_MAX_SPEC 8

typedef struct vpr_repeat_stratum { int32_t k, slop; } vpr_repeat_stratum;

/* The default set of the command lines (the one copy both use): rep_k16, rep_k24, rep_k32, all with slop 0.  The tables are
   static. */
int vpr_repeats_default(const vpr_repeat_stratum **spec, const char *const **names, int32_t *n);

/* Builds the intervals of every spec entry for the whole genome in one call, on the handle's stream: ctg_off[n_ctg + 1] are the
   contigs' offsets into the concatenated ctg_seq (ctg_off[0] == 0).  The handle needs no batch.  The intervals stay resident
   until the next vpr_repeat_intervals or vpr_destroy; a refused call leaves none.  VPR_ERR_ARG, with a message that names the
   entry, for a spec outside the limits, n_spec outside 1..VPR_REP_MAX_SPEC, ctg_off[0] != 0, a contig above INT32_MAX bases
   and a total above UINT32_MAX bases -- all checked before a byte of ctg_seq is read; an exhausted device is VPR_ERR_NOMEM
   with the bytes needed in the message.  Two calls on the same input give identical arrays. */
int vpr_repeat_intervals(vpr_handle *h, int32_t n_ctg, const int64_t *ctg_off, const uint8_t *ctg_seq, const vpr_repeat_stratum *spec,
                         int32_t n_spec);
/* The intervals of the last vpr_repeat_intervals (VPR_ERR_STATE before a successful one): iv_off[n_spec * n_ctg + 1], row =
   spec * n_ctg + ctg, and the intervals themselves (0-based half-open, contig coordinates), iv_off[n_spec * n_ctg] of each. */
int vpr_repeat_interval_counts(vpr_handle *h, int64_t *iv_off);
int vpr_repeat_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop);
/* int64_t[n_spec] each: the valid starts and the repeated starts of every entry of the last call. */
int vpr_repeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_repeated);
/* Device time (HIP events on the handle's stream, ms, summed over the entries) of the last call's passes: pack (count, scan,
   write), sort, mark (clear, mark and scatter) and the run passes that make the intervals.  The sequence upload is excluded. */
int vpr_repeat_timing(const vpr_handle *h, double *ms_pack, double *ms_sort, double *ms_mark, double *ms_intervals);

/* A measurement aid (tools/repeats_bench.py): the device time (ms) of the bare sort of vpr_repeat_intervals -- key bits [0, 2k) --
   over n random 64-bit keys with 32-bit values, the floor under an entry with n valid starts.  Touches no state of the handle. */
int vpr_repeat_sort_floor(vpr_handle *h, int64_t n, int32_t k, uint64_t seed, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_REPEATS_H_ */
