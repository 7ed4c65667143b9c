/* vcfdist_realign.h -- C ABI of the realignment of a callset's variants (the reference's `-rq / --realign-query`,
 * `-rt / --realign-truth`, `-ro / --realign-only`) on the MI355X.
 *
 * Replaces, for one (contig, hap) per call:
 *     wf_swg_realign                                        src/dist.cpp:2496-2594
 *   with its per-cluster kernels
 *     generate_str                                          src/dist.cpp:81-138
 *     wf_swg_align / wf_swg_backtrack                       src/dist.cpp:1510-1652, 2625-2757
 *     variantData::add_variants                             src/variant.cpp:332-391
 *   and then
 *     variantData::left_shift                               src/variant.cpp:57-127
 * A job is one cluster: its region [poss[first] - 1, poss[last] + rlens[last] + 1), the cluster's haplotype over it and the
 * reference over it, both reversed, aligned with full history and backtracked into SUB / DEL / INS records on the device
 * (pr_realign.hip, the recurrence and walk of pr_swg.h that the distance metrics use too).  No CPU fallback.  left_shift is host
 * code, sequential and O(#records), like the reference's.
 *
 * Every new record carries the cluster's minimum var_qual (starting from max_qual) truncated to an integer (add_variants takes
 * `int qual`), gt_qual = max_qual, orig_gt = GT_REF_REF (2) and the cluster's first non-zero phase set.
 *
 * Limits (documented, counted, never silent): a cluster that is not realigned keeps its original variants (with their own
 * columns) and gets a status bit:
 *   - VRL_ST_EDGE  its region starts before position 0 (a variant at position 0; the reference throws out_of_range there);
 *   - VRL_ST_LIMIT its alignment history (or pass-1 scratch) exceeds the per-job memory limit (half the device's free memory,
 *                  or vrl_config.job_bytes_limit); checkpointed recomputation is not built;
 *   - VRL_ST_ERROR its strings are inconsistent (overlapping variants: generate_str's "ref_end < ref_pos" ERROR, a variant past
 *                  the contig's end) or the backtrack met a pointer the reference would ERROR on.
 * A region past the contig's end is clamped, as the reference's substr clamps it.  left_shift runs over every record of the
 * (contig, hap), kept clusters' included, as the reference's runs over the whole callset.
 * sub and extend must be at least 1 (the recurrence reads the wavefront row it is writing at 0): VRL_ERR_ARG.
 */
#ifndef VCFDIST_REALIGN_H_
#define VCFDIST_REALIGN_H_

#include "vcfdist_cluster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VRL_OK          0
#define VRL_ERR_ARG    -1     /* = VPR_ERR_ARG: null pointer, penalty out of range, unsorted positions, inconsistent cluster table */
#define VRL_ERR_DEVICE -2     /* no HIP device / HIP runtime error (no CPU fallback) */
#define VRL_ERR_NOMEM  -3     /* the device cannot hold the job tables or one job */

/* per-cluster status bits */
#define VRL_ST_EDGE   1u
#define VRL_ST_LIMIT  2u
#define VRL_ST_ERROR  4u

#define VRL_GT_REF_REF 2      /* orig_gt of the new records (src/defs.h:57) */

typedef struct vrl_config {
    int32_t sub;              /* g.sub    (5) */
    int32_t open;             /* g.open   (6) */
    int32_t extend;           /* g.extend (2) */
    int32_t max_qual;         /* g.max_qual (60): the start of the cluster quality's minimum, and the new records' gt_qual */
    int64_t round_bytes;      /* >0: device bytes one round of jobs may occupy (a test aid that makes small inputs run in many
                                 rounds); 0: 4 GiB for pass 1, the memory plan for pass 2 */
    int64_t job_bytes_limit;  /* >0: the per-job limit behind VRL_ST_LIMIT (a test aid); 0: the memory plan (half the free memory) */
} vrl_config;

typedef struct vrl_info {
    int64_t n_clusters;       /* clusters of the call = jobs */
    int64_t n_realigned;      /* clusters whose records replace their variants */
    int64_t n_records;        /* records of the realigned clusters (before left_shift, which keeps their number) */
    int64_t n_kept;           /* clusters that kept their original variants (any status bit) */
    int64_t n_edge, n_limit, n_error;   /* clusters with each status bit */
    int64_t n_rounds;         /* pass-1 rounds; pass-2 sub-rounds are counted in n_hist_rounds */
    int64_t n_hist_rounds;
    int64_t arena_bytes;      /* peak bytes one round occupied */
    int64_t plan_bytes;       /* the per-job limit in force */
    double  ms_upload;        /* host wall time of the uploads */
    double  ms_jobs;          /* kernel time: job list, string lengths, region checks */
    double  ms_score;         /* kernel time: pass 1 */
    double  ms_hist;          /* kernel time: pass 2 */
    double  ms_back;          /* kernel time: backtracks (count + write) and their scans */
    double  ms_host;          /* host wall time: merging the records with the kept clusters, left_shift */
    double  ms_wall;          /* host wall time of the whole call */
} vrl_info;

/* the realigned and left-shifted (contig, hap) in the reader's layout (include/vcfdist_io.h, vio_hap_vars).  Records carry no
   BED location: every new record is INSIDE (add_variants sets BED_INSIDE), which is what the writers assume without one. */
typedef struct vrl_result {
    int32_t n;                /* records */
    int32_t *pos, *rlen;
    uint8_t *type;            /* VPR_TYPE_SUB / INS / DEL */
    int32_t *ref_len, *alt_len;
    int64_t *ref_off, *alt_off;   /* into pool */
    uint8_t *pool;
    int64_t pool_len;
    float   *var_qual, *gt_qual;
    int32_t *phase_set;
    uint8_t *orig_gt;
    int32_t n_clusters;
    uint8_t *cluster_status;  /* [n_clusters] VRL_ST_* */
    vrl_info info;
} vrl_result;

/* One (contig, hap): hap's variants (sorted by position) with their var_qual and phase_set (required) and gt_qual / orig_gt
   (NULL: a kept cluster's records get max_qual / VRL_GT_REF_REF), its clusters (vcl_simple_cluster / vcl_wfa_cluster), and the
   contig's sequence.  device: HIP device ordinal.  *out is released with vrl_result_free. */
int vrl_realign(const vcl_hap_seq *hap, const float *var_qual, const float *gt_qual, const int32_t *phase_set, const uint8_t *orig_gt,
                const vcl_clusters *clusters, const uint8_t *ctg_seq, int32_t ctg_len, const vrl_config *cfg, int32_t device,
                vrl_result **out);
void vrl_result_free(vrl_result *r);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_REALIGN_H_ */
