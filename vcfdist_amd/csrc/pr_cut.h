// pr_cut.h -- what a count cut keeps between calls (pr_cut.hip: the counters and the label counts, cut by stratum and resampled).
// One CutState per owner: the membership words' (StrataState, pr_strata.hip: the counters cut by stratum), the handle's
// (vpr_handle::boot: the counters resampled) and a label pass's (LabelState, pr_label.h: both cuts of its counts).  Created by the
// owner's first call, released with the batch.
#pragma once

#include "pr_host.h"

struct CutState {
    DevBuf<unsigned long long> hist;     // [n_strata][2][rows][nq + 1], or replicate-minor [2][rows][nq + 1][groups * 64]
    DevBuf<uint64_t> keys;               // the caller's sc_key
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms_strata = 0, ms_boot = 0;   // device time of the last stratified / replicate launches (0: none that succeeded)
    // the last successful launches' shape: strata of a workgroup, chunks, LDS bytes | variant spans, replicate groups, quality slices
    int32_t shape[6] = {0, 0, 0, 0, 0, 0};
};

// the event pair around the timed launches on h->stream: cut_mark(.., 0) in front of them (it creates the events on first use),
// cut_mark(.., 1) behind them, cut_elapsed once the caller has synchronised the stream
int cut_mark(vpr_handle *h, CutState &C, int k);
double cut_elapsed(const CutState &C);
void cut_release(vpr_handle *h, CutState &C);      // the buffers and the events

// pr_strata.hip: the cut state that lives with the resident membership words (valid after a strata_view that succeeded)
CutState &strata_cut(vpr_handle *h);
