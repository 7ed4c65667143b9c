/* vcfdist_varstrata.h -- C ABI of the variant strata on the MI355X: strata that are a function of the variant tables alone.
 *
 * vcfdist_strata.h cuts the one evaluation by region, vcfdist_context.h by sequence context.  The cut looked at first is by
 * what the variants themselves are: transitions and transversions, insertions and deletions in size bins, genotype, and how
 * closely variants crowd together.  vpr_varstrata_masks makes those bits on the device from a vpr_variants and puts them into
 * the membership words of vcfdist_strata.h, alone or behind the resident ones; everything behind the words
 * (vpr_pr_counts_strata, the all-reduce, vpr_pr_counts_boot with a stratum) works on them unchanged.  The reference
 * (vcfdist v2.6.4) prints SNP / INDEL / SV / ALL only.
 *
 * Definitions (everything is tested against these; tests/varstrata_model.py is their brute-force statement).
 *   A hap-variant v of slot s has pos, type (VPR_TYPE_*), ref_len, alt_len, its REF and ALT bytes in allele_pool[s], and the
 *   contig sc_ctg[supercluster of v].  The partner slot is s ^ 1: the other haplotype of the same callset.  A copy of v is
 *   another hap-variant u != v of slot s or s ^ 1 that agrees with v on contig, pos, type, ref_len, alt_len and all alt_len ALT
 *   bytes.  Query and truth variants are each assigned from their own callset, as in vcfdist_strata.h.
 *
 * VPR_VS_SIZE (type = VPR_TYPE_INS or VPR_TYPE_DEL, min_len >= 1, max_len == 0 (unbounded) or >= min_len):
 *   v is a member iff v.type == type and min_len <= len (and len <= max_len when set); len is alt_len for INS, ref_len for DEL.
 * VPR_VS_TI / VPR_VS_TV:
 *   v is a member of one of them iff type == VPR_TYPE_SUB, ref_len == alt_len == 1, both bytes are one of ACGT and they differ;
 *   of TI when the pair is a transition (A<->G, C<->T), of TV otherwise.  The REF byte is the one in allele_pool, not the
 *   contig's.  Longer substitutions and uncalled bases belong to neither.
 * VPR_VS_HOM / VPR_VS_HET:
 *   HOM iff a copy of v exists in slot s ^ 1; HET iff not HOM.  There is deliberately no "hetalt": HET includes a site whose
 *   other haplotype carries a different allele.
 * VPR_VS_NEAR (window W >= 0, min_n >= 0, max_n == -1 (unbounded) or >= min_n):
 *   N(v) = the number of hap-variants u of slot s or s ^ 1 on v's contig that are not v, not a copy of v, and have
 *   |pos_u - pos_v| <= W.  Only start positions count; two copies of one other allele count twice.
 *   v is a member iff min_n <= N(v) (and N(v) <= max_n when set).
 *
 * Preconditions, checked on the host before anything is launched (VPR_ERR_ARG with a message that names the place): sc_ctg is
 * non-decreasing over the superclusters; within a slot var_pos is non-decreasing within a contig; the spec limits above;
 * 1 <= n_spec <= VPR_VS_MAX_SPEC.
 *
 * Device code: pr_varstrata.hip (k_varstrata_mask).  No CPU fallback.
 */
#ifndef VCFDIST_VARSTRATA_H_
#define VCFDIST_VARSTRATA_H_

#include "vcfdist_strata.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_VS_SIZE 0
#define VPR_VS_TI 1
#define VPR_VS_TV 2
#define VPR_VS_HOM 3
#define VPR_VS_HET 4
#define VPR_VS_NEAR 5
#define VPR_VS_MAX_SPEC 64

typedef struct vpr_variant_stratum {
    int32_t kind;                     /* VPR_VS_* */
    int32_t type, min_len, max_len;   /* VPR_VS_SIZE (max_len 0: unbounded); ignored otherwise */
    int32_t window, min_n, max_n;     /* VPR_VS_NEAR (max_n -1: unbounded); ignored otherwise */
} vpr_variant_stratum;

/* The default set of the command lines (the one copy both use), 14 strata: snp_ti, snp_tv, ins_1to5, ins_6to15, ins_16to49,
   ins_ge50, del_1to5, del_6to15, del_16to49, del_ge50, hom, het, iso_50 (W 50, N == 0), near_10 (W 10, N >= 1).  The size bins
   are fixed (they do not follow -sv); the thresholds are this project's choice, in the spirit of hap.py's subtypes, not a
   reproduction of them.  The tables are static. */
int vpr_varstrata_default(const vpr_variant_stratum **spec, const char *const **names, int32_t *n);

/* Makes the bits of every spec entry for the variants of `v` on the device (on the handle's stream) and puts them into the
   membership words of vcfdist_strata.h.  Read and uploaded: var_off, sc_ctg, var_pos, var_type, var_ref_off, var_ref_len,
   var_alt_off, var_alt_len and allele_pool.
   append == 0: the words of `v` hold these strata alone, n_strata = n_spec; they replace whatever was resident.
   append == 1: membership words must be resident (vpr_strata_masks, vpr_context_masks or vpr_strata_upload_masks) with per-slot
   variant counts equal to `v`'s, else VPR_ERR_STATE; the new strata follow the resident ones, n_strata = n_old + n_spec, the
   old bits are unchanged and the word array grows when a 64-bit boundary is crossed.
   The words keep the lifetime rule of vpr_strata_masks.  An exhausted device is VPR_ERR_NOMEM. */
int vpr_varstrata_masks(vpr_handle *h, const vpr_variants *v, const vpr_variant_stratum *spec, int32_t n_spec, int32_t append);
/* Device time (HIP events on the handle's stream, ms) of the last vpr_varstrata_masks' kernel launches (uploads excluded). */
int vpr_varstrata_timing(const vpr_handle *h, double *ms_mask);

/* <prefix>variant-strata.tsv: one row per variant stratum -- name, kind, its parameters ('.' where the kind has none or the bound
   is open) and the number of query and of truth hap-variants that are members (n_query[k], n_truth[k]).  Host code; an error's
   text is vrp_last_error()'s (include/vcfdist_report.h). */
int vrp_write_variant_strata(const char *prefix, const char *const *names, const vpr_variant_stratum *spec, int32_t n_spec,
                             const int64_t *n_query, const int64_t *n_truth);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_VARSTRATA_H_ */
