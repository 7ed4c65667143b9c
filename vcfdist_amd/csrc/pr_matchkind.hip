// pr_matchkind.hip -- the match kinds (include/vcfdist_matchkind.h): how each true positive was matched.  k_matchkind is the
// counterpart of k_errclass (pr_errclass.hip) on the TP side: one lane per hap-variant, the same join of the two callsets inside
// the supercluster (pr_varscan.h), here on the resident sync groups and query_ed; a kind byte per hap-variant and a block
// histogram flushed as k_pr_hist's (pr_collect.hip).  The bin rule is pr_counts.h's; the host side around the launches is the label
// passes' (pr_label.h).
#include "pr_host.h"
#include "pr_counts.h"
#include "pr_varscan.h"
#include "pr_label.h"
#include "../../include/vcfdist_matchkind.h"

namespace {

const char *const MK_NAMES[VPR_MK_KINDS] = {"exact", "shifted", "regrouped", "partial"};

// members of sync group g among the variants [lo, hi) of a slot, up to 2 ("0, 1, more than 1" decides every kind): e / grp are
// the slot's errtype and sync_group columns of the selected phasing.  The members are not contiguous (a REF-plane FP with a group
// of its own can sit between two of them), so this is a scan of the range that stops at the second one
__device__ __forceinline__ int mk_members(const uint8_t *__restrict__ e, const int32_t *__restrict__ grp, int64_t lo, int64_t hi, int32_t g) {
    int n = 0;
    for (int64_t u = lo; u < hi && n < 2; u++) n += e[u] < 3 && grp[u] == g;
    return n;
}

}  // namespace

extern "C" {

// One lane per hap-variant of slot `own`.  oa / ob: the slots of the other callset with the same / the other haplotype index, so
// that the compared slot is oa under ORIG and ob under SWAP.  e0 / e1 / q0 / q1: the lane's errtype and callq columns of the two
// phasings (four pointers, as pr_count_row takes them); g0 / g1 / d0 / d1: its sync_group and query_ed columns; ae0 / ag0: oa's
// errtype and sync_group in the original phasing, be1 / bg1: ob's in the swapped one (the only phasing each is compared in).
// A variant that is no TP leaves after the loads k_pr_hist makes; a TP bisects the compared slot's range for its position and
// tests the run for a copy of its group, and only where there is none and query_ed is 0 counts the members of both ranges.
// Kinds are counted in LDS ([3 types][VPR_MK_KINDS][nq + 1] words) and flushed once.
__global__ void __launch_bounds__(256) k_matchkind(VsCols own, VsCols oa, VsCols ob, int64_t n_var, int n_sc, const uint8_t *__restrict__ cls,
                                                   const int32_t *__restrict__ sc_phase, const int32_t *__restrict__ pb_phase, const uint8_t *e0,
                                                   const uint8_t *e1, const float *q0, const float *q1, const int32_t *g0, const int32_t *g1,
                                                   const int32_t *d0, const int32_t *d1, const uint8_t *ae0, const int32_t *ag0, const uint8_t *be1,
                                                   const int32_t *bg1, int callset, int min_qual, int max_qual, uint8_t *__restrict__ out,
                                                   unsigned long long *__restrict__ hist /* [2][3][VPR_MK_KINDS][nq + 1] */) {
    extern __shared__ unsigned int blk[];      // [3][VPR_MK_KINDS][nq + 1]
    const int nq = max_qual - min_qual + 1, nb = 3 * VPR_MK_KINDS * (nq + 1);
    for (int k = threadIdx.x; k < nb; k += blockDim.x) blk[k] = 0;
    __syncthreads();
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n_var) {
        const int sc = sc_of_var(own.var_off, n_sc, v);
        int bin = 0, c = VPR_MK_NONE, t = 0;
        const int row = pr_count_row(sc, v, sc_phase, pb_phase, e0, e1, q0, q1, cls, min_qual, nq, &bin);
        if (row >= 0 && row % 3 == VPR_ERRTYPE_TP) {
            t = row / 3;
            const int w = pr_phase_swap(sc, sc_phase, pb_phase);
            const int32_t g = (w ? g1 : g0)[v];
            const int32_t pos = own.pos[v], ref_len = own.ref_len[v], alt_len = own.alt_len[v];
            const uint8_t type = own.type[v];
            const uint8_t *__restrict__ alt = own.pool + own.alt_off[v];
            // the compared slot: its columns and its errtype / sync_group in the selected phasing
            VsCols cmp;
            cmp.var_off = w ? ob.var_off : oa.var_off; cmp.ref_off = nullptr; cmp.alt_off = w ? ob.alt_off : oa.alt_off;
            cmp.pos = w ? ob.pos : oa.pos; cmp.ref_len = w ? ob.ref_len : oa.ref_len; cmp.alt_len = w ? ob.alt_len : oa.alt_len;
            cmp.type = w ? ob.type : oa.type; cmp.pool = w ? ob.pool : oa.pool;
            const uint8_t *ce = w ? be1 : ae0;
            const int32_t *cg = w ? bg1 : ag0;
            const int64_t c0 = cmp.var_off[sc], c1 = cmp.var_off[sc + 1];
            bool exact = false;
            for (int64_t u = vs_lower(cmp.pos, c0, c1, pos); !exact && u < c1 && cmp.pos[u] == pos; u++)
                exact = ce[u] < 3 && cg[u] == g && vs_is_copy(cmp, u, type, ref_len, alt_len, alt);
            if (exact) {
                c = VPR_MK_EXACT;
            } else if ((w ? d1 : d0)[v] > 0) {
                c = VPR_MK_PARTIAL;
            } else {
                c = VPR_MK_REGROUPED;
                if (mk_members(w ? e1 : e0, w ? g1 : g0, own.var_off[sc], own.var_off[sc + 1], g) == 1 && mk_members(ce, cg, c0, c1, g) == 1)
                    c = VPR_MK_SHIFTED;
            }
        }
        out[v] = uint8_t(c);
        if (c != VPR_MK_NONE) atomicAdd(&blk[(t * VPR_MK_KINDS + c) * (nq + 1) + bin], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += blockDim.x)
        if (blk[k]) atomicAdd(&hist[size_t(callset) * nb + k], (unsigned long long)blk[k]);
}

}  // extern "C"

namespace {

// pr_fold_counts' TP rule cut by kind: a matched variant of either callset counts at the threshold indices <= its bin (bin nq,
// callq < min_qual: at none)
LabelFold mk_fold(int, int) { return LABEL_FOLD_UPTO; }
const LabelDesc MK = {LABEL_MATCHKIND, "vpr_matchkind", "kind", VPR_MK_KINDS, mk_fold};

int matchkind_impl(vpr_handle *h, void *comm, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                   int32_t min_qual, int32_t max_qual, int64_t *counts) {
    if (!h) return VPR_ERR_ARG;
    LabelCall c;
    if (int rc = label_begin(h, MK, comm, v, var_class, pb_phase, min_qual, max_qual, counts, &c)) return rc;
    const VsCols *cols = c.T.cols;
    for (int s = 0; s < VPR_HAPS; s++) {
        const int64_t nv = h->n_var[s];
        if (!nv) continue;
        const int oa = (s ^ 2), ob = (s ^ 3);      // the other callset's slot of the same / of the other haplotype index
        hipLaunchKernelGGL(k_matchkind, dim3(unsigned((nv + 255) / 256)), dim3(256), c.nb * 4, h->stream, cols[s], cols[oa], cols[ob], nv,
                           int(v->n_sc), h->d_cls[s], h->dR.sc_phase, c.d_pb, h->dR.v[s][0].errtype, h->dR.v[s][1].errtype, h->dR.v[s][0].callq,
                           h->dR.v[s][1].callq, h->dR.v[s][0].sync_group, h->dR.v[s][1].sync_group, h->dR.v[s][0].query_ed, h->dR.v[s][1].query_ed,
                           h->dR.v[oa][0].errtype, h->dR.v[oa][0].sync_group, h->dR.v[ob][1].errtype, h->dR.v[ob][1].sync_group, s >> 1,
                           int(min_qual), int(max_qual), c.S->bytes[s].p, c.S->hist.p);
        HIPCHK(h, hipGetLastError());
    }
    return label_finish(h, MK, comm, &c, counts);
}

}  // namespace

extern "C" {

int vpr_matchkind(vpr_handle *h, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase, int32_t min_qual,
                  int32_t max_qual, int64_t *counts) {
    return matchkind_impl(h, nullptr, v, var_class, pb_phase, min_qual, max_qual, counts);
}

int vpr_allreduce_matchkind(vpr_handle *h, void *nccl_comm, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS],
                            const int32_t *pb_phase, int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return nccl_comm ? matchkind_impl(h, nccl_comm, v, var_class, pb_phase, min_qual, max_qual, counts) : VPR_ERR_ARG;
}

int vpr_matchkind_download(vpr_handle *h, uint8_t *const kind[VPR_HAPS]) { return label_download(h, MK, kind); }

int vpr_matchkind_timing(const vpr_handle *h, double *ms) { return label_timing(h, MK, ms); }

const char *const *vpr_matchkind_names(void) { return MK_NAMES; }

// the counts cut by stratum and resampled (pr_cut.hip)
int vpr_matchkind_strata(vpr_handle *h, int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return labelcut_strata(h, MK, nullptr, min_qual, max_qual, counts);
}

int vpr_allreduce_matchkind_strata(vpr_handle *h, void *nccl_comm, int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return nccl_comm ? labelcut_strata(h, MK, nccl_comm, min_qual, max_qual, counts) : VPR_ERR_ARG;
}

int vpr_matchkind_boot(vpr_handle *h, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep, int32_t stratum,
                   int64_t *counts) {
    return labelcut_boot(h, MK, nullptr, min_qual, max_qual, sc_key, seed, n_rep, stratum, counts);
}

int vpr_allreduce_matchkind_boot(vpr_handle *h, void *nccl_comm, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed,
                             int32_t n_rep, int32_t stratum, int64_t *counts) {
    return nccl_comm ? labelcut_boot(h, MK, nccl_comm, min_qual, max_qual, sc_key, seed, n_rep, stratum, counts) : VPR_ERR_ARG;
}

int vpr_matchkind_cut_timing(const vpr_handle *h, double *ms_strata, double *ms_boot) { return labelcut_timing(h, MK, ms_strata, ms_boot); }

int vpr_matchkind_cut_info(const vpr_handle *h, int32_t shape[6]) { return labelcut_info(h, MK, shape); }

}  // extern "C"
