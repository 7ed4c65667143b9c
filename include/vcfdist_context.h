/* vcfdist_context.h -- C ABI of the sequence-context strata on the MI355X: strata that are a function of the FASTA alone.
 *
 * vcfdist_strata.h cuts the one evaluation by region, given BEDs.  The two cuts looked at first -- low-complexity sequence
 * (homopolymers, short tandem repeats) and GC extremes -- hold no outside knowledge: they follow from the contig sequences the
 * run has read anyway.  vpr_context_masks builds their interval lists on the device from ctg_off / ctg_seq of a vpr_variants
 * and hands them to the membership kernel of vcfdist_strata.h without a host round trip; everything behind the membership
 * words (vpr_pr_counts_strata, the all-reduce, vpr_pr_counts_boot with a stratum) works on them unchanged.  The reference
 * (vcfdist v2.6.4) has no strata at all.
 *
 * Definitions (everything is tested against these; tests/context_model.py is their numpy statement).  A contig is s[0..L),
 * upper-case bytes; a called base is A, C, G or T; all arithmetic is integer.
 *
 * Period stratum (period p, min_len, max_len, slop), 1 <= p <= 6, min_len > p, max_len == 0 (unbounded) or >= min_len, slop >= 0:
 *   1. m[i] = i >= p && s[i] == s[i-p] && called(s[i]).
 *   2. every maximal run [a, b) of m gives a tract [a - p, b) of length b - a + p.
 *   3. a tract is kept iff min_len <= length (and length <= max_len when set) and it is primitive: its first p bases are not
 *      a repetition of a shorter word whose length divides p (AAAA... is no dinucleotide tract, ACAC... no period-4 tract).
 *   4. kept tracts are padded to [max(0, start - slop), min(L, stop + slop)).
 *   5. padded intervals that overlap or abut are merged into their union (needed at slop 0 too: two period-p tracts can share
 *      up to p - 1 bases, two homopolymers of different bases abut).
 * GC stratum (lo, hi, window W, slop), 0 <= lo < hi <= 101, W >= 1, slop >= 0:
 *   1. the window of base i is [i - W/2, i - W/2 + W) (integer division).
 *   2. the base is flagged iff the window lies wholly inside the contig, all W of its bases are called, and
 *      lo * W <= 100 * g < hi * W with g the window's count of G and C.
 *   3. maximal runs of flagged bases are padded by slop and merged as above.
 * Runs never cross a contig boundary of the concatenated ctg_seq.  The result per (stratum, contig) is sorted, non-overlapping
 * and non-empty: the contract of vpr_strata.  Membership of a variant is vio_bed_contains(...) == VIO_BED_INSIDE on these
 * intervals, exactly as if they had been written to a BED and passed as one.
 *
 * Device code: pr_context.hip (the interval kernels), pr_strata.hip (k_strata_mask).  No CPU fallback.
 */
#ifndef VCFDIST_CONTEXT_H_
#define VCFDIST_CONTEXT_H_

#include "vcfdist_strata.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_CTX_PERIOD 0
#define VPR_CTX_GC 1
#define VPR_CTX_MAX_SPEC 64

typedef struct vpr_context_stratum {
    int32_t kind;                     /* VPR_CTX_PERIOD or VPR_CTX_GC */
    int32_t period, min_len, max_len; /* VPR_CTX_PERIOD (max_len 0: unbounded); ignored for VPR_CTX_GC */
    int32_t gc_lo, gc_hi, window;     /* VPR_CTX_GC: lo <= 100 * g / W < hi in integers; ignored for VPR_CTX_PERIOD */
    int32_t slop;
} vpr_context_stratum;

/* The default set of the command lines (the one copy both use): hp_4to6, hp_7to11, hp_ge12, tr_di_ge10, tr_tri_ge14,
   tr_quad_ge19 (slop 5) and gc_lt25, gc_25to30, gc_30to55, gc_55to65, gc_ge65 (W 100, slop 0).  In the spirit of GIAB's
   LowComplexity and GC stratifications, not a reproduction of them.  The tables are static. */
int vpr_context_default(const vpr_context_stratum **spec, const char *const **names, int32_t *n);

/* Builds the intervals of every spec entry for every contig of `v` on the device (from ctg_off / ctg_seq, on the handle's
   stream) and then makes the membership words of `v`'s variants resident, as vpr_strata_masks does: strata 0..n_bed-1 are
   those of `bed_or_null` (exactly the words vpr_strata_masks would make), the context strata follow in spec order, so
   n_strata = n_bed + n_spec for every later call of vcfdist_strata.h / vcfdist_bootstrap.h.  The words keep the lifetime rule
   of vpr_strata_masks; the intervals stay resident until the next vpr_context_masks or vpr_destroy.
   1 <= n_spec <= VPR_CTX_MAX_SPEC; a spec outside the limits above is VPR_ERR_ARG with a message that names the entry; an
   exhausted device is VPR_ERR_NOMEM. */
int vpr_context_masks(vpr_handle *h, const vpr_variants *v, const vpr_strata *bed_or_null, const vpr_context_stratum *spec, int32_t n_spec);
/* The context intervals of the last vpr_context_masks (VPR_ERR_STATE before one has run): iv_off[n_spec * n_ctg + 1], row =
   spec * n_ctg + ctg, and the intervals themselves (0-based half-open, contig coordinates), iv_off[n_spec * n_ctg] of each. */
int vpr_context_interval_counts(vpr_handle *h, int64_t *iv_off);
int vpr_context_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop);
/* The tiling of the per-base kernels: bases of a workgroup and of a lane (the run passes behind them take four lanes' worth
   per lane and four workgroups' worth per workgroup, so their seams are a subset).  A property of the build: h may be null. */
int vpr_context_info(const vpr_handle *h, int32_t *bases_per_workgroup, int32_t *bases_per_lane);
/* Device time (HIP events on the handle's stream, ms) of the last vpr_context_masks: the interval kernels of all spec
   entries (sequence upload excluded) and the membership kernel. */
int vpr_context_timing(const vpr_handle *h, double *ms_intervals, double *ms_mask);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_CONTEXT_H_ */
