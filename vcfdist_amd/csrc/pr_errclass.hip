// pr_errclass.hip -- the error classes (include/vcfdist_errclass.h): why each query FP and truth FN is wrong.  k_errclass joins the
// two callsets inside each supercluster -- one lane per hap-variant, bisections over the supercluster's sorted positions, as
// k_varstrata_mask (pr_varstrata.hip) does inside a contig -- writes a class byte per hap-variant and counts the classes in a
// block histogram, as k_pr_hist (pr_collect.hip) counts the errtypes.  The bin rule is pr_counts.h's; the host side around the
// launches is the label passes' (pr_label.h).
#include "pr_host.h"
#include "pr_counts.h"
#include "pr_varscan.h"
#include "pr_label.h"
#include "../../include/vcfdist_errclass.h"

namespace {

const char *const EC_NAMES[VPR_EC_CLASSES] = {"gt", "sync", "phase", "site", "near", "alone", "lowq"};

// the run of variants of slot x's range [lo, hi) that start at pos: *site = it is not empty; true iff it holds a copy
__device__ __forceinline__ bool ec_copy_at(const VsCols &x, int64_t lo, int64_t hi, int32_t pos, uint8_t type, int32_t ref_len, int32_t alt_len,
                                           const uint8_t *__restrict__ alt, bool *site) {
    int64_t u = vs_lower(x.pos, lo, hi, pos);
    *site = u < hi && x.pos[u] == pos;
    for (; u < hi && x.pos[u] == pos; u++)
        if (vs_is_copy(x, u, type, ref_len, alt_len, alt)) return true;
    return false;
}

// some variant of slot x's range [lo, hi) starts within W bases of pos and not at pos: the window's first or last one
__device__ __forceinline__ bool ec_near(const VsCols &x, int64_t lo, int64_t hi, int32_t pos, int32_t W) {
    const int64_t a = vs_lower(x.pos, lo, hi, int64_t(pos) - W), b = vs_upper(x.pos, lo, hi, int64_t(pos) + W);
    return a < b && (x.pos[a] != pos || x.pos[b - 1] != pos);
}

}  // namespace

extern "C" {

// One lane per hap-variant of slot `own`.  par: the partner slot; oa / ob: the slots of the other callset with the same / the
// other haplotype index, so that the compared slot is oa under ORIG and ob under SWAP.  e0 / e1 / q0 / q1: the lane's errtype and
// callq columns of the two phasings (four pointers, as pr_count_row takes them); pe0 / pe1: the partner slot's errtype columns.
// A variant that is no error leaves after the loads k_pr_hist makes; an error walks the class list -- the searches are divergent,
// few lanes of a wave run them.  Classes are counted in LDS ([3 types][VPR_EC_CLASSES][nq + 1] words) and flushed once.
__global__ void __launch_bounds__(256) k_errclass(VsCols own, VsCols par, VsCols oa, VsCols ob, int64_t n_var, int n_sc,
                                                  const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                                                  const int32_t *__restrict__ pb_phase, const uint8_t *e0, const uint8_t *e1, const float *q0,
                                                  const float *q1, const uint8_t *pe0, const uint8_t *pe1, int callset, int window, int min_qual,
                                                  int max_qual, uint8_t *__restrict__ out,
                                                  unsigned long long *__restrict__ hist /* [2][3][VPR_EC_CLASSES][nq + 1] */) {
    extern __shared__ unsigned int blk[];      // [3][VPR_EC_CLASSES][nq + 1]
    const int nq = max_qual - min_qual + 1, nb = 3 * VPR_EC_CLASSES * (nq + 1);
    for (int k = threadIdx.x; k < nb; k += blockDim.x) blk[k] = 0;
    __syncthreads();
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n_var) {
        const int sc = sc_of_var(own.var_off, n_sc, v);
        int bin = 0, c = VPR_EC_NONE, t = 0;
        const int row = pr_count_row(sc, v, sc_phase, pb_phase, e0, e1, q0, q1, cls, min_qual, nq, &bin);
        if (row >= 0) {
            t = row / 3;
            const int e = row - 3 * t;
            if (e == (callset ? VPR_ERRTYPE_FN : VPR_ERRTYPE_FP)) {
                const int w = pr_phase_swap(sc, sc_phase, pb_phase);
                const int32_t pos = own.pos[v], ref_len = own.ref_len[v], alt_len = own.alt_len[v];
                const uint8_t type = own.type[v];
                const uint8_t *__restrict__ alt = own.pool + own.alt_off[v];
                const uint8_t *pe = w ? pe1 : pe0;
                bool gt = false;
                const int64_t p1 = par.var_off[sc + 1];
                for (int64_t u = vs_lower(par.pos, par.var_off[sc], p1, pos); !gt && u < p1 && par.pos[u] == pos; u++)
                    gt = pe[u] == VPR_ERRTYPE_TP && vs_is_copy(par, u, type, ref_len, alt_len, alt);
                if (gt) {
                    c = VPR_EC_GT;
                } else {
                    const int64_t a0 = oa.var_off[sc], a1 = oa.var_off[sc + 1], b0 = ob.var_off[sc], b1 = ob.var_off[sc + 1];
                    bool site_a, site_b;
                    const bool copy_a = ec_copy_at(oa, a0, a1, pos, type, ref_len, alt_len, alt, &site_a);
                    const bool copy_b = ec_copy_at(ob, b0, b1, pos, type, ref_len, alt_len, alt, &site_b);
                    if (w ? copy_b : copy_a) c = VPR_EC_SYNC;
                    else if (w ? copy_a : copy_b) c = VPR_EC_PHASE;
                    else if (site_a || site_b) c = VPR_EC_SITE;
                    else c = ec_near(oa, a0, a1, pos, window) || ec_near(ob, b0, b1, pos, window) ? VPR_EC_NEAR : VPR_EC_ALONE;
                }
            } else if (callset && e == VPR_ERRTYPE_TP) {
                c = VPR_EC_LOWQ;
            }
        }
        out[v] = uint8_t(c);
        if (c != VPR_EC_NONE) atomicAdd(&blk[(t * VPR_EC_CLASSES + c) * (nq + 1) + bin], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += blockDim.x)
        if (blk[k]) atomicAdd(&hist[size_t(callset) * nb + k], (unsigned long long)blk[k]);
}

}  // extern "C"

namespace {

// pr_fold_counts' rule cut by class.  A query FP counts at the threshold indices <= its bin; a truth FN at every threshold; a LOWQ
// truth variant at the thresholds above its bin (bin nq, callq < min_qual: at every one)
LabelFold ec_fold(int callset, int c) { return !callset ? LABEL_FOLD_UPTO : c != VPR_EC_LOWQ ? LABEL_FOLD_EVERY : LABEL_FOLD_ABOVE; }
const LabelDesc EC = {LABEL_ERRCLASS, "vpr_errclass", "class", VPR_EC_CLASSES, ec_fold};

int errclass_impl(vpr_handle *h, void *comm, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                  int32_t window, int32_t min_qual, int32_t max_qual, int64_t *counts) {
    if (!h) return VPR_ERR_ARG;
    // (the window is looked at behind the null arguments, which label_begin refuses)
    if (v && counts && window < 0) return fail(h, VPR_ERR_ARG, "vpr_errclass: window %d is negative", window);
    LabelCall c;
    if (int rc = label_begin(h, EC, comm, v, var_class, pb_phase, min_qual, max_qual, counts, &c)) return rc;
    const VsCols *cols = c.T.cols;
    for (int s = 0; s < VPR_HAPS; s++) {
        const int64_t nv = h->n_var[s];
        if (!nv) continue;
        const int oa = (s ^ 2), ob = (s ^ 3);      // the other callset's slot of the same / of the other haplotype index
        hipLaunchKernelGGL(k_errclass, dim3(unsigned((nv + 255) / 256)), dim3(256), c.nb * 4, h->stream, cols[s], cols[s ^ 1], cols[oa], cols[ob], nv,
                           int(v->n_sc), h->d_cls[s], h->dR.sc_phase, c.d_pb, h->dR.v[s][0].errtype, h->dR.v[s][1].errtype, h->dR.v[s][0].callq,
                           h->dR.v[s][1].callq, h->dR.v[s ^ 1][0].errtype, h->dR.v[s ^ 1][1].errtype, s >> 1, int(window), int(min_qual), int(max_qual),
                           c.S->bytes[s].p, c.S->hist.p);
        HIPCHK(h, hipGetLastError());
    }
    return label_finish(h, EC, comm, &c, counts);
}

}  // namespace

extern "C" {

int vpr_errclass(vpr_handle *h, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase, int32_t window,
                 int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return errclass_impl(h, nullptr, v, var_class, pb_phase, window, min_qual, max_qual, counts);
}

int vpr_allreduce_errclass(vpr_handle *h, void *nccl_comm, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS],
                           const int32_t *pb_phase, int32_t window, int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return nccl_comm ? errclass_impl(h, nccl_comm, v, var_class, pb_phase, window, min_qual, max_qual, counts) : VPR_ERR_ARG;
}

int vpr_errclass_download(vpr_handle *h, uint8_t *const cls[VPR_HAPS]) { return label_download(h, EC, cls); }

int vpr_errclass_timing(const vpr_handle *h, double *ms) { return label_timing(h, EC, ms); }

const char *const *vpr_errclass_names(void) { return EC_NAMES; }

// the counts cut by stratum and resampled (pr_cut.hip)
int vpr_errclass_strata(vpr_handle *h, int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return labelcut_strata(h, EC, nullptr, min_qual, max_qual, counts);
}

int vpr_allreduce_errclass_strata(vpr_handle *h, void *nccl_comm, int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return nccl_comm ? labelcut_strata(h, EC, nccl_comm, min_qual, max_qual, counts) : VPR_ERR_ARG;
}

int vpr_errclass_boot(vpr_handle *h, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep, int32_t stratum,
                   int64_t *counts) {
    return labelcut_boot(h, EC, nullptr, min_qual, max_qual, sc_key, seed, n_rep, stratum, counts);
}

int vpr_allreduce_errclass_boot(vpr_handle *h, void *nccl_comm, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed,
                             int32_t n_rep, int32_t stratum, int64_t *counts) {
    return nccl_comm ? labelcut_boot(h, EC, nccl_comm, min_qual, max_qual, sc_key, seed, n_rep, stratum, counts) : VPR_ERR_ARG;
}

int vpr_errclass_cut_timing(const vpr_handle *h, double *ms_strata, double *ms_boot) { return labelcut_timing(h, EC, ms_strata, ms_boot); }

int vpr_errclass_cut_info(const vpr_handle *h, int32_t shape[6]) { return labelcut_info(h, EC, shape); }

}  // extern "C"
