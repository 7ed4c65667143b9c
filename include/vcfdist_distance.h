/* vcfdist_distance.h -- C ABI of the alignment-distance metrics (the reference's `-d / --distance` mode) on the MI355X.
 *
 * Replaces the body of the reference's
 *     editData edits_wrapper(superclusterData*)              src/dist.cpp:1908-2077
 * with its per-alignment kernels
 *     wf_swg_align                                          src/dist.cpp:1510-1652
 *     wf_swg_backtrack                                      src/dist.cpp:2625-2757
 *     count_dist                                            src/dist.cpp:2596-2620
 *     editData::add_edits                                   src/edit.cpp:4-78
 * for one executed batch.  It runs behind vpr_execute and only reads what that left on the device (sc_phase and the
 * alignments' status bits); the variant sets are not touched.  A job is (supercluster, query hap, quality threshold); the
 * jobs are listed, their strings built, aligned with full history and backtracked on the device (pr_dist.hip).  No CPU
 * fallback.
 *
 * Limits (documented, reported, never silent):
 *   - eval_sub and eval_extend must be at least 1 (the reference accepts 0, where its recurrence reads the wavefront row
 *     it is writing; VPR_ERR_ARG here);
 *   - a job whose alignment history alone does not fit the device's memory plan gets VPR_DIST_ST_LIMIT in job_status and
 *     contributes neither a distance nor edits (checkpointed recomputation is not built);
 *   - a job whose strings are inconsistent (the supercluster's variants overlap) or whose backtrack meets a pointer the
 *     reference would ERROR on gets VPR_DIST_ST_ERROR.
 */
#ifndef VCFDIST_DISTANCE_H_
#define VCFDIST_DISTANCE_H_

#include "vcfdist_pr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* edit types of the records (src/defs.h:33-35, VPR_TYPE_*) */
#define VPR_DIST_SUB VPR_TYPE_SUB
#define VPR_DIST_INS VPR_TYPE_INS
#define VPR_DIST_DEL VPR_TYPE_DEL

/* per-job status bits */
#define VPR_DIST_ST_LIMIT 1u    /* history beyond the memory plan: not aligned */
#define VPR_DIST_ST_ERROR 2u    /* inconsistent strings or an unexpected pointer in the backtrack */

typedef struct vpr_dist_config {
    int32_t eval_sub;        /* g.eval_sub    src/globals.h:53 (3) */
    int32_t eval_open;       /* g.eval_open   (2) */
    int32_t eval_extend;     /* g.eval_extend (1) */
    int32_t min_qual;        /* g.min_qual (0): the writers' range; the jobs do not depend on it */
    int32_t max_qual;        /* g.max_qual (60): thresholds end at max_qual + 2 */
    int32_t flags;           /* 0 */
    int64_t round_bytes;     /* >0: the device bytes one round of jobs may occupy (pass-1 scratch and pass-2 history; a test aid
                                that makes small inputs run in many rounds); 0 = 4 GiB for pass 1, the memory plan for pass 2.  A job larger than this runs alone,
                                one larger than half the device's free memory gets VPR_DIST_ST_LIMIT */
} vpr_dist_config;

typedef struct vpr_dist_info {
    int64_t n_jobs;          /* (supercluster, hap, threshold) alignments of the last vpr_distance */
    int64_t n_edits;         /* edit records */
    int64_t n_limit;         /* jobs with VPR_DIST_ST_LIMIT */
    int64_t n_error;         /* jobs with VPR_DIST_ST_ERROR */
    int64_t n_rounds;        /* pass-1 rounds; pass-2 sub-rounds are counted in n_hist_rounds */
    int64_t n_hist_rounds;
    int64_t arena_bytes;     /* peak bytes one round occupied in the arena (pass-1 scratch / pass-2 history) */
    int64_t plan_bytes;      /* the memory plan's limit for one job */
    int64_t input_bytes;     /* variant tables and contig sequence uploaded by the call */
    int64_t history_cells;   /* wavefront cells kept for the backtracks (band-compacted, all three matrices) */
    double  ms_upload;       /* host wall time of the table upload */
    double  ms_jobs;         /* kernel time: listing the jobs */
    double  ms_score;        /* kernel time: pass 1 (score and history size) */
    double  ms_hist;         /* kernel time: pass 2 (wavefronts with history) */
    double  ms_back;         /* kernel time: backtracks (count + write), scans of the record counts */
    double  ms_wall;         /* host wall time of the whole call */
} vpr_dist_info;

/* Every pointer may be NULL (that column is not copied).  Sizes: vpr_dist_info.n_jobs / n_edits, qual_dists
   max_qual + 2.  Jobs are in (supercluster, hap, threshold) order, records in job order and, inside a job, in the order
   add_edits appends them; edit_pos is the absolute 0-based contig position (begs[sc] + the offset along the alignment). */
typedef struct vpr_dist_results {
    int32_t *job_sc;
    uint8_t *job_hap;
    int32_t *job_min_qual, *job_max_qual;   /* [prev_qual, qual) of the threshold */
    int32_t *job_dist;                      /* count_dist of the job's CIGAR */
    uint8_t *job_status;                    /* VPR_DIST_ST_* */
    int64_t *qual_dists;                    /* all_qual_dists: sum of job_dist over the jobs whose range holds the quality */
    int32_t *edit_sc;
    uint8_t *edit_hap;
    int32_t *edit_pos;
    uint8_t *edit_type;                     /* VPR_DIST_SUB / INS / DEL */
    int32_t *edit_len;
    int32_t *edit_min_qual, *edit_max_qual;
} vpr_dist_results;

/* Distance metrics of the batch the last vpr_execute evaluated.  `variants` is the vpr_variants that batch was made from
   (vpr_upload_variants, or vpr_batch_from_variants + vpr_upload); the call uploads the columns it needs.  Superclusters
   with an alignment that carries a VPR_ST_ERR_* bit produce no jobs.  Runs on the library's stream and returns when the
   results are on the device; the call's work buffers are released when it returns, the results when the next batch is
   uploaded or executed (vpr_distance_info / _download then return VPR_ERR_ARG until the next vpr_distance).  VPR_ERR_ARG: no execute yet, variants->n_sc differs from the executed batch, or a penalty
   out of range.  VPR_ERR_NOMEM: the device cannot hold the job tables or one round. */
int vpr_distance(vpr_handle *h, const vpr_variants *variants, const vpr_dist_config *cfg);
int vpr_distance_info(const vpr_handle *h, vpr_dist_info *out);
int vpr_distance_download(vpr_handle *h, vpr_dist_results *out);

#ifdef __cplusplus
}
#endif
#endif /* VCFDIST_DISTANCE_H_ */
