// pr_kmer.h -- the host scaffold of a genome-wide k-mer call, shared by pr_repeats.hip (which defines it, beside k_rep_pack, k_rep_mark
// and k_rep_piece_words) and pr_longrepeats.hip: the argument checks, the upload, the compaction "count per tile, scan, read the
// total, make room, write behind the scanned counts", the sort, the mark, the rows of an entry, and the state the rows end in.
//
// Device memory of a call, with N the bases padded to whole tiles of 4096 plus one tile: N bytes (the sequence, resident for the
// call) + N / 8 (the flag bits) + 1/8 byte per base of the largest piece (its masked copy) + per pair sorted 2 x 12 bytes (key and
// value, double-buffered for the sort) + the tiles' counts + rocPRIM's temporary + what the run passes take (pr_context.hip).  All
// of it goes with the call: the rows are downloaded at its end and live in host memory until the next call or vpr_destroy.  At
// most 2^32 - 1 bases: values are 32-bit.  The near-repeat strata (pr_nearrepeats.hip) keep a forward and a reverse-complement
// record per valid start, the strand in the value's lowest bit: per valid start 12 bytes (the packed forward pairs, kept over the
// entry's blocks) + 2 x 2 x 12 bytes (both records, double-buffered for the sort), 60 in all, and at most 2^31 - 1 bases.
#ifndef PR_KMER_H_
#define PR_KMER_H_
#include "pr_host.h"
#include "../../include/vcfdist_repeats.h"

// The rows of the last call of a family, in the caller's order, and its counts and device times.
struct KmerState {
    int32_t n_spec = 0, n_ctg = 0;
    std::vector<int64_t> off;                          // [n_spec * n_ctg + 1]
    std::vector<int32_t> start, stop;                  // [off.back()]
    std::vector<int64_t> n_valid, n_repeated;          // [n_spec]
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms[4] = {0, 0, 0, 0};                       // the family's four buckets, in the order of its timing entry
    bool valid = false;
    int init(vpr_handle *h, int32_t n_spec_, int32_t n_ctg_);          // the events, the sizes, zero counts
};

// the state of a family goes: repeats_free and longrepeats_free
template <typename S>
void kmer_free(vpr_handle *h, S *vpr_handle::*member) {
    S *s = h->*member;
    if (!s) return;
    (void)hipStreamSynchronize(h->stream);
    for (int k = 0; k < 2; k++) if (s->ev[k]) (void)hipEventDestroy(s->ev[k]);
    delete s;
    h->*member = nullptr;
}

// The bodies of a family's accessors; `self` and `entry` name the accessor and the family's entry in the messages.  h is not null.
int kmer_interval_counts(vpr_handle *h, const KmerState *S, const char *self, const char *entry, int64_t *iv_off);
int kmer_download_intervals(vpr_handle *h, const KmerState *S, const char *self, const char *entry, int32_t *start, int32_t *stop);
// (bufs: all of the accessor's buffers are there, those it copies itself included)
int kmer_stats(vpr_handle *h, const KmerState *S, const char *self, const char *entry, bool bufs, int64_t *n_valid, int64_t *n_repeated);
int kmer_timing(const KmerState *S, double *ms0, double *ms1, double *ms2, double *ms3);

// The genome-wide arrays of one call (released when it goes) and the passes over them.  The timed segments are W's: set W.ms to
// the bucket, and where a method says so a segment is open on entry and on return.
struct KmerWork {
    vpr_handle *h;
    CtxWork W;
    const char *room_entry;              // the name under which a refused allocation of the genome-wide arrays is reported
    DevBuf<uint8_t> flags, cnt, keys, vals, sort_tmp;
    DevBuf<int64_t> d_off;               // [rows + 1] in the order the entries are computed; the intervals behind them
    DevBuf<int32_t> d_start, d_stop;
    const uint8_t *d_seq = nullptr;
    const int64_t *d_ctg = nullptr;
    const int64_t *ctg_off = nullptr;    // the caller's
    int n_ctg = 0;
    size_t n_rows = 0;                   // rows of d_off: entries x contigs
    int64_t N = 0, n_pad = 0, n_tiles = 0, nw = 0;     // bases, with the padding, tiles of the pack, 64-bit flag words
    unsigned long long *d_count = nullptr;             // two counter words
    uint64_t *keys_out = nullptr;        // the sorted pairs of the last sort
    uint32_t *vals_out = nullptr;
    std::vector<CtxPiece> pieces;
    KmerWork(vpr_handle *h_, const char *entry, const char *room_entry_ = nullptr) : h(h_), W(h_, entry), room_entry(room_entry_ ? room_entry_ : entry) {}
    ~KmerWork() {
        (void)hipStreamSynchronize(h->stream);
        dev_release(h, flags, cnt, keys, vals, sort_tmp, d_off, d_start, d_stop);
    }
    // the checks of an entry, every one before a byte of ctg_seq is read
    static int check_args(vpr_handle *h, const char *entry, int min_k, int max_k, int max_spec, int32_t n_ctg, const int64_t *ctg_off,
                          const uint8_t *ctg_seq, const vpr_repeat_stratum *spec, int32_t n_spec);
    // room for exactly `bytes` (the arrays that scale with the genome are not given the quarter more of ctx_need)
    int need(DevBuf<uint8_t> &b, size_t bytes, const char *what);
    // the padded sequence, the contig offsets, the flag words, the tiles' counts (also for a compaction over tiles of other_tile
    // starts, where that is not 0), the row offsets of n_rows rows, the pieces
    int upload(int32_t n_ctg, const int64_t *ctg_off, const uint8_t *ctg_seq, size_t n_rows, int other_tile = 0);
    // behind the upload and the caller's own allocations, in front of the first segment: S's events time the segments, the stream is drained
    int begin_timing(KmerState *S);
    int scan(const uint32_t *in, uint32_t *out, size_t n);
    int pair_room(size_t n);
    // the n pairs at the front of keys / vals, sorted over key bits [0, bits) into keys_out / vals_out; sort_room alone makes the
    // room (for a caller that does not want it made under its clock)
    int sort_room(size_t n, unsigned bits, size_t *bytes = nullptr);
    int sort(size_t n, unsigned bits);
    // launch(false, counts, null, null) counts the pairs of each of n_tiles tiles, launch(true, offsets, keys, vals) writes them behind
    // the exclusive scan of the counts; *n_out pairs, at the front of keys / vals.  A timed segment is open on entry and on return.
    template <typename F>
    int compact(int64_t n_tiles_, F launch, uint32_t *n_out) {
        uint32_t *c = as<uint32_t>(cnt), *off = c + (n_tiles_ + 1);
        uint32_t n = 0;
        *n_out = 0;
        if (n_tiles_) {
            HIPCHK(h, hipMemsetAsync(c + n_tiles_, 0, 4, h->stream));
            launch(false, c, (uint64_t *)nullptr, (uint32_t *)nullptr);
            HIPCHK(h, hipGetLastError());
            if (int rc = scan(c, off, size_t(n_tiles_ + 1))) return rc;
            HIPCHK(h, hipMemcpyAsync(&n, off + n_tiles_, 4, hipMemcpyDeviceToHost, h->stream));
        }
        if (int rc = W.seg_end()) return rc;
        if (n) if (int rc = pair_room(n)) return rc;
        if (int rc = W.seg_begin()) return rc;
        if (n) {
            launch(true, off, as<uint64_t>(keys), as<uint32_t>(vals));
            HIPCHK(h, hipGetLastError());
        }
        *n_out = n;
        return VPR_OK;
    }
    // (canon, start) of the valid starts of length k <= 32 (k_rep_pack), by compact; forward: (fwd, start), the strands kept apart
    int pack(int k, uint32_t *n, bool forward = false);
    // the flags cleared; with n > 0 the repeated ones of the n sorted pairs flagged at their last base and counted (k_rep_mark)
    int mark(uint32_t n, int k, unsigned long long *n_rep);
    // the rows of an entry from the flags, piece by piece (k_rep_piece_words, ctx_intervals_from_flags), into row `slot` of d_off
    // behind the *n_iv intervals there; no segment is open on return
    int rows_of_entry(int k, int slop, int spec_entry, int slot, int64_t *n_iv);
    // row offsets and intervals to the host, as computed
    int download_rows(int64_t n_iv, std::vector<int64_t> &off, std::vector<int32_t> &start, std::vector<int32_t> &stop);
};
#endif
