/* vcfdist_derive.h -- C ABI of the derived strata on the MI355X: boolean combinations of the strata that are there.
 *
 * Every family of strata (vcfdist_strata.h, vcfdist_context.h, the k-mer families, vcfdist_varstrata.h) ends in one structure: the
 * membership words resident on the device, bit k & 63 of word k >> 6 per hap-variant.  vpr_derive_masks makes new strata from those
 * bits on the device -- "deletions of 1 to 5 bases inside long homopolymers", an indel size bin crossed with a homopolymer bin,
 * "in no difficult stratum" -- and appends them to the same words; everything behind the words (vpr_pr_counts_strata, the
 * all-reduce, vpr_pr_counts_boot with a stratum, the label cuts) works on them unchanged.
 *
 * Definition (everything is tested against it; tests/derive_model.py states it on the text and on the program).
 *   A derived stratum is a boolean function of one hap-variant's membership bits of the strata in front of it in the table:
 *     x & y   the variant is a member of both;
 *     x | y   the variant is a member of at least one;
 *     !x      a hap-variant of the slot that is not a member of x.
 *   It is defined on the BITS, not on intervals.  A variant on a region's border is a member of no BED stratum (vcfdist_strata.h:
 *   only INSIDE counts), so it is a member of !x: x and !x partition the hap-variants of every slot exactly, whatever x is.
 *   !x is therefore not "the variants inside the complement of x's regions".  Query and truth variants are each assigned from their
 *   own bits, as everywhere else.
 *
 * Program.  An entry's program is postfix int32_t code over a stack of booleans:
 *     c >= 0        pushes the membership of stratum c;
 *     VPR_DV_AND    pops two values and pushes their conjunction;   VPR_DV_OR   the same with their disjunction;
 *     VPR_DV_NOT    replaces the top value by its negation.
 *   Entry j of a call becomes stratum n_prev + j (n_prev: the resident strata).  It may name any stratum c < n_prev + j, earlier
 *   entries of the same call included.  A program is valid iff the stack never underflows, ends at depth 1, never exceeds
 *   VPR_DV_MAX_DEPTH and every operand is in range.
 * Limits: 1 <= n_entries <= VPR_DV_MAX_SPEC, at most VPR_DV_MAX_CODE ints of code per call.  Anything else is VPR_ERR_ARG with a
 * message that names the entry, checked on the host before anything is launched; the resident words stay as they were.
 *
 * The text (one compiler for both command lines, host code).
 *   A derived entry is NAME=EXPR.  NAME is [A-Za-z0-9_.+-]+ and must not be a name that is there.  EXPR is made of operands, the
 *   operators | (lowest precedence), & and unary ! (highest), and parentheses; blanks and tabs may stand between tokens.  An operand
 *   is a maximal run of characters outside " \t()&|!=,:" and names a stratum in front of the entry.  A stratum whose name holds one
 *   of those characters (a crossed stratum's does) cannot be named; a name that holds '*' can only be matched by a glob.  There
 *   is no quoting.  An operand that holds '*' is a glob: '*' matches any run of characters, the empty one included, and the glob
 *   stands for the union of every stratum in front of the entry that matches, in table order; the unions are emitted
 *   left-associated, so a glob over hundreds of strata needs a stack of 2.  A glob that matches nothing is an error.
 *   A crossed entry is LIST:LIST, LIST being glob[,glob...]: each side is the set of matching strata in table order, each once, and
 *   the entry stands for every pair (a, b), a from the left, b from the right, a != b, left-major: the stratum a & b, named "a&b".
 *
 * Not here: set algebra on intervals and a BED of a derived stratum (the strata are bits), XOR or difference operators (write
 * them with & | !), quoting of names, a per-variant file.
 *
 * Device code: pr_derive.hip (k_derive_mask).  No CPU fallback.
 */
#ifndef VCFDIST_DERIVE_H_
#define VCFDIST_DERIVE_H_

#include <stddef.h>

#include "vcfdist_strata.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_DV_AND (-1)
#define VPR_DV_OR (-2)
#define VPR_DV_NOT (-3)
#define VPR_DV_MAX_DEPTH 32
#define VPR_DV_MAX_SPEC 1024
#define VPR_DV_MAX_CODE 65536
/* the command lines' limit on the derived plus the crossed strata of one run */
#define VPR_DV_MAX_CLI 512
/* the KIND column of derived-strata.tsv */
#define VPR_DV_KIND_DERIVE 0
#define VPR_DV_KIND_CROSS 1

/* Runs the n_entries programs code[code_off[j] .. code_off[j + 1]) on the resident membership words (on the handle's stream) and
   appends their strata behind the resident ones: n_strata = n_prev + n_entries, the old bits are unchanged, the bits at and above
   n_strata in the last word are 0, and the word array grows when a 64-bit boundary is crossed.  Reads no variant tables: the
   per-slot variant counts are the resident words'.  Without resident words (vpr_strata_masks, vpr_context_masks,
   vpr_varstrata_masks or vpr_strata_upload_masks) VPR_ERR_STATE.  The words keep the lifetime rule of vpr_strata_masks.  An
   exhausted device is VPR_ERR_NOMEM. */
int vpr_derive_masks(vpr_handle *h, const int32_t *code_off /* [n_entries + 1] */, const int32_t *code, int32_t n_entries);
/* Device time (HIP events on the handle's stream, ms) of the last vpr_derive_masks' kernel launches (the code's upload excluded). */
int vpr_derive_timing(const vpr_handle *h, double *ms_mask);

/* Compiles one NAME=EXPR against names[0 .. n_names), the strata in front of the entry in table order: NAME (NUL-terminated)
   into name_out[name_cap], the program into code[code_cap], its length into *n_code.  0, or -1 with the reason in
   vpr_derive_last_error(): every message names the entry, and the offending token or glob where there is one -- a missing '=', an
   empty, a bad or a duplicate name, an empty expression, an unknown stratum (a later entry is one: only the names in front are
   known), a reference to the entry itself, a glob that matches nothing, an unbalanced parenthesis, a dangling operator, nesting
   deeper than VPR_DV_MAX_DEPTH (parentheses, or the program's stack), code longer than code_cap. */
int vpr_derive_compile(const char *entry, const char *const *names, int32_t n_names, char *name_out, size_t name_cap, int32_t *code,
                       int32_t code_cap, int32_t *n_code);
/* Compiles one LIST:LIST against the same names: the pairs (a, b) as indices into names, pairs[2 i], pairs[2 i + 1], *n_pairs of
   them (at most pairs_cap).  0, or -1 with the reason in vpr_derive_last_error(): a missing or a second ':', an empty side or
   glob, an unknown stratum, a glob that matches nothing, a cross that yields no pair, more pairs than pairs_cap, a pair whose
   name "a&b" is there already. */
int vpr_derive_cross(const char *entry, const char *const *names, int32_t n_names, int32_t *pairs, int32_t pairs_cap, int32_t *n_pairs);
/* the text of the calling thread's last failed vpr_derive_compile / vpr_derive_cross */
const char *vpr_derive_last_error(void);

/* <prefix>derived-strata.tsv: one row per derived or crossed stratum -- NAME, KIND (derive / cross, kind[k] = VPR_DV_KIND_*),
   EXPRESSION (the text as given; a&b for a cross), QUERY_MEMBERS, TRUTH_MEMBERS (the hap-variants that are members).  Host code; an
   error's text is vrp_last_error()'s (include/vcfdist_report.h). */
int vrp_write_derived_strata(const char *prefix, const char *const *names, const int32_t *kind, const char *const *expression, int32_t n,
                             const int64_t *n_query, const int64_t *n_truth);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_DERIVE_H_ */
