// pr_results.hip -- what a caller reads back: vpr_download (one copy of the result columns into a page-locked mirror block),
// vpr_results_alloc / vpr_host_alloc / vpr_host_free, the TP / FP / FN tally, the timing record and the launch statistics of the
// last vpr_execute.  The fields are the ones the reference writes in place (variant.h:49-60, cluster.h:39-42).
#include "pr_host.h"

namespace {
// page-locked result blocks handed out by vpr_results_alloc (base -> bytes), until vpr_host_free: vpr_download takes its
// single-copy path only into one of these
std::mutex g_result_blocks_m;
std::unordered_map<void *, size_t> g_result_blocks;
}  // namespace

extern "C" {

int vpr_get_launch_stats(const vpr_handle *h, vpr_launch_stat *out, int32_t cap) {
    if (!h) return VPR_ERR_ARG;
    const int32_t n = int32_t(h->events.size());
    for (int32_t k = 0; k < n && k < cap && out; k++) out[k] = h->events[k].st;
    return n;
}

int vpr_strip_plan_count(const vpr_handle *h) {
    if (!h) return VPR_ERR_ARG;
    return int(h->strip_recs.size());
}

int vpr_strip_plan_record(const vpr_handle *h, int32_t k, vpr_strip_plan_rec *rec, int32_t *lohi, int32_t cap) {
    if (!h || !rec || k < 0 || size_t(k) >= h->strip_recs.size()) return VPR_ERR_ARG;
    const vpr_handle::StripPlanRec &R = h->strip_recs[size_t(k)];
    rec->sc = R.sc; rec->aln = R.aln; rec->from_window = R.from_window; rec->tie_round = R.tie_round; rec->call = R.call;
    rec->ok = R.ok; rec->n_strips = R.n_strips;
    for (int32_t j = 0; lohi && j < R.n_strips && j < cap; j++)
        for (int w = 0; w < 4; w++) lohi[4 * j + w] = h->strip_lohi[size_t(R.strip_off + j) * 4 + size_t(w)];
    return VPR_OK;
}

int vpr_get_timing(const vpr_handle *h, vpr_timing *t) {
    if (!h || !t) return VPR_ERR_ARG;
    *t = h->timing;
    return VPR_OK;
}

int vpr_download(vpr_handle *h, vpr_results *res) {
    if (!h || !res) return VPR_ERR_ARG;
    if (!h->executed) return fail(h, VPR_ERR_STATE, "vpr_download before vpr_execute");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const DevResults &R = h->dR;
    const size_t na = h->descs.size(), n = size_t(h->n_sc);
    hipStream_t st = h->stream;
    // results were finalised on the device (k_finalize / k_phase_tally): plain copies into the caller's buffers, all
    // enqueued before the one wait (page-locked destinations, vpr_host_alloc, are written by DMA at the link rate)
    auto get = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    // A block of vpr_results_alloc -- of this upload, or of an earlier upload of a batch of the same shape (a caller that streams
    // batches of one size keeps its block: the columns lie at the same offsets) -- takes ONE copy: every pointer of *res has to
    // sit where the device's column sits in the result region.
    uint8_t *mirror = h->res_mirror;
    if (!mirror && h->res_bytes && na && res->aln_dist) {
        // (an inferred base counts only if it IS a block vpr_results_alloc handed out, alive and at least as large as the result
        // region: a caller's own contiguous layout without the trailing padding, or a smaller block of an earlier upload, must
        // not be overrun by the single copy)
        uint8_t *cand = reinterpret_cast<uint8_t *>(res->aln_dist) - (reinterpret_cast<const uint8_t *>(R.aln_dist) - h->res_dev);
        std::lock_guard<std::mutex> g(g_result_blocks_m);
        const auto it = g_result_blocks.find(cand);
        if (it != g_result_blocks.end() && it->second >= h->res_bytes) mirror = cand;
    }
    if (mirror && h->res_bytes) {
        auto at = [&](const void *dst, const void *src) {
            return static_cast<const uint8_t *>(dst) - mirror == static_cast<const uint8_t *>(src) - h->res_dev;
        };
        bool all = at(res->aln_dist, R.aln_dist) && at(res->aln_end_plane, R.aln_end_plane) && at(res->aln_beg_plane, R.aln_beg_plane) &&
                   at(res->aln_status, R.aln_status) && at(res->sc_phase, R.sc_phase) && at(res->orig_phase_dist, R.orig_phase_dist) &&
                   at(res->swap_phase_dist, R.swap_phase_dist);
        for (int s = 0; s < 4 && all; s++)
            for (int w = 0; w < 2; w++)
                // (a hap slot without variants has columns of length 0: whatever address the caller's views carry matches)
                all = all && (h->n_var[s] == 0 ||
                      (at(res->errtype[s][w], R.v[s][w].errtype) && at(res->sync_group[s][w], R.v[s][w].sync_group) &&
                      at(res->credit[s][w], R.v[s][w].credit) && at(res->ref_ed[s][w], R.v[s][w].ref_ed) &&
                      at(res->query_ed[s][w], R.v[s][w].query_ed) && at(res->callq[s][w], R.v[s][w].callq)));
        if (all) {
            HIPCHK(h, get(mirror, h->res_dev, h->res_bytes));
            HIPCHK(h, x_sync(h, st, SITE));
            return VPR_OK;
        }
    }
    if (na) {
        HIPCHK(h, get(res->aln_dist, R.aln_dist, na * 4));
        HIPCHK(h, get(res->aln_end_plane, R.aln_end_plane, na));
        HIPCHK(h, get(res->aln_beg_plane, R.aln_beg_plane, na));
        HIPCHK(h, get(res->aln_status, R.aln_status, na * 4));
        HIPCHK(h, get(res->sc_phase, R.sc_phase, n * 4));
        HIPCHK(h, get(res->orig_phase_dist, R.orig_phase_dist, n * 4));
        HIPCHK(h, get(res->swap_phase_dist, R.swap_phase_dist, n * 4));
    }
    for (int s = 0; s < 4; s++) {
        const size_t nv = size_t(h->n_var[s]);
        for (int w = 0; w < 2; w++) {
            HIPCHK(h, get(res->errtype[s][w], R.v[s][w].errtype, nv));
            HIPCHK(h, get(res->sync_group[s][w], R.v[s][w].sync_group, nv * 4));
            HIPCHK(h, get(res->credit[s][w], R.v[s][w].credit, nv * 4));
            HIPCHK(h, get(res->ref_ed[s][w], R.v[s][w].ref_ed, nv * 4));
            HIPCHK(h, get(res->query_ed[s][w], R.v[s][w].query_ed, nv * 4));
            HIPCHK(h, get(res->callq[s][w], R.v[s][w].callq, nv * 4));
        }
    }
    HIPCHK(h, x_sync(h, st, SITE));
    return VPR_OK;
}

int vpr_results_alloc(vpr_handle *h, vpr_results *res, void **block) {
    if (!h || !res || !block) return VPR_ERR_ARG;
    if (!h->uploaded || !h->res_dev) return fail(h, VPR_ERR_STATE, "vpr_results_alloc before vpr_upload");
    void *p = nullptr;
    if (hipHostMalloc(&p, h->res_bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, VPR_ERR_NOMEM, "vpr_results_alloc: %zu page-locked bytes", h->res_bytes);
    }
    uint8_t *m = static_cast<uint8_t *>(p);
    const DevResults &R = h->dR;
    auto mir = [&](const void *dev) { return m + (static_cast<const uint8_t *>(dev) - h->res_dev); };
    res->aln_dist = reinterpret_cast<int32_t *>(mir(R.aln_dist));
    res->aln_end_plane = reinterpret_cast<uint8_t *>(mir(R.aln_end_plane));
    res->aln_beg_plane = reinterpret_cast<uint8_t *>(mir(R.aln_beg_plane));
    res->aln_status = reinterpret_cast<uint32_t *>(mir(R.aln_status));
    res->sc_phase = reinterpret_cast<int32_t *>(mir(R.sc_phase));
    res->orig_phase_dist = reinterpret_cast<int32_t *>(mir(R.orig_phase_dist));
    res->swap_phase_dist = reinterpret_cast<int32_t *>(mir(R.swap_phase_dist));
    for (int s = 0; s < 4; s++)
        for (int w = 0; w < 2; w++) {
            res->errtype[s][w] = reinterpret_cast<uint8_t *>(mir(R.v[s][w].errtype));
            res->sync_group[s][w] = reinterpret_cast<int32_t *>(mir(R.v[s][w].sync_group));
            res->credit[s][w] = reinterpret_cast<float *>(mir(R.v[s][w].credit));
            res->ref_ed[s][w] = reinterpret_cast<int32_t *>(mir(R.v[s][w].ref_ed));
            res->query_ed[s][w] = reinterpret_cast<int32_t *>(mir(R.v[s][w].query_ed));
            res->callq[s][w] = reinterpret_cast<float *>(mir(R.v[s][w].callq));
        }
    h->res_mirror = m;
    { std::lock_guard<std::mutex> g(g_result_blocks_m); g_result_blocks[p] = h->res_bytes; }
    *block = p;
    return VPR_OK;
}

int vpr_select_device(int32_t device) {
    return hipSetDevice(device) == hipSuccess ? VPR_OK : VPR_ERR_DEVICE;
}

void *vpr_host_alloc(size_t bytes) {
    void *p = nullptr;
    // (portable: usable by every device of the process; the allocation still initialises the calling thread's current
    // device, which a multi-GPU process selects first with vpr_select_device)
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void vpr_host_free(void *p) {
    if (p) {
        { std::lock_guard<std::mutex> g(g_result_blocks_m); g_result_blocks.erase(p); }
        (void)hipHostFree(p);
    }
}

int vpr_get_tally(const vpr_handle *h, int64_t out[6]) {
    if (!h || !out || !h->executed) return VPR_ERR_ARG;
    unsigned long long t[6];
    if (hipMemcpy(t, h->dR.tally, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) return VPR_ERR_DEVICE;
    for (int k = 0; k < 6; k++) out[k] = int64_t(t[k]);
    return VPR_OK;
}

}  // extern "C"
