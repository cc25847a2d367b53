// pd_ctx.h — what the library's own translation units (pd_capi.hip, pd_decode.hip, pd_windows.hip, pd_rows.hip, pd_gcbias.hip) share: the guarded device allocator, the context
// (struct pd_ctx, struct pd_runs, the window result buffer's owner WinKeep) and the few helpers that cross the file boundary (namespace pdi).  Not
// installed; include/*.h is the interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "pd_kernels.h"
#include "pd_win_rule.h"
#include "../../include/pandepth_amd_dev.h"
#include "pd_bamwalk.h"

using namespace pdk;

// ---- guarded device allocations (PANDEPTH_GUARD=1; pd_guard_check in include/pandepth_amd_dev.h) ---------------------------
// Every device buffer this file allocates goes through the two functions below.  Normally they ARE hipMalloc / hipFree.  With
// PANDEPTH_GUARD set, a buffer of n bytes is allocated as [256 B canary | n bytes | 256 B canary] (the second canary starting at
// byte n exactly, not at a rounded size), the canaries are filled with a pattern, and they are compared — after a device
// synchronize — whenever the buffer is freed and whenever pd_guard_check runs (pd_reset, pd_destroy, pd_comm_destroy call it):
// a kernel that writes in front of or behind its buffer is named by the line that allocated the buffer, instead of landing in
// the allocator's padding unseen.
namespace pdguard {
bool on();
hipError_t gmalloc(void **out, size_t bytes, const char *file, int line);
hipError_t gfree(void *user);
void adopt(void *user, size_t bytes, const char *file, int line);
void drop(void *user);
uint64_t check_all();
} // namespace pdguard

template <class T> static inline hipError_t pd_dmalloc(T **out, size_t bytes, const char *file, int line) { return pdguard::gmalloc((void **)out, bytes, file, line); }
#define hipMalloc(p, n) pd_dmalloc((p), (n), __FILE_NAME__, __LINE__)
#define hipFree(p) pdguard::gfree((void *)(p))

struct pd_runs;

namespace pdi {

constexpr int N_STAGE = 1024;                       // upper bound; slots are created on demand
constexpr size_t STAGE_CAP = (size_t)1 << 18;        // runs per staging slot (3 MiB pinned + 3 MiB HBM)
constexpr size_t DEV_BATCH_MAX = 0xFFFFFF00ull;       // runs per sorted batch (32-bit run indices)
constexpr uint64_t OVF_MAX = (uint64_t)64 << 20;     // overflow-list entries (ends of runs longer than lmax) per tile pass
constexpr uint32_t LMAX_DEFAULT = 512;               // look-back bound for owner tiles (cells)
constexpr uint32_t SAMPLE_DEFAULT = 64;              // sparse index stride (runs)

struct Stage {
    pd_iv *host = nullptr, *dev = nullptr;
    hipEvent_t copied = nullptr, done = nullptr;
    int state = 0;                                   // 0 free, 1 held by caller, 2 in flight
    uint64_t seq = 0;
};

struct ProfRec { std::string name; hipEvent_t a, b; };

struct Pending { const pd_iv *iv; uint32_t n; uint32_t disorder; int slot; pd_runs *cr = nullptr; };   // slot: staging slot or -1; cr: a compact sample (iv NULL until expanded)

} // namespace pdi

using namespace pdi;

// a whole sample in the compact form (include/pandepth_amd.h: pd_runs_create; layout: C8Sample in pd_kernels.h)
struct pd_runs {
    pd_ctx *ctx = nullptr;
    uint32_t *lo = nullptr, *hi = nullptr;                       // the runs' two planes (C8Sample), one allocation with lo first; each [sorted stream: n_s runs, file order | ... | other runs by bucket at o_base]
    uint32_t n_s = 0, n_o = 0, o_base = 0, n = 0;                // n = n_s + n_o
    uint16_t *nar = nullptr;                                     // the sorted stream's narrow plane, n_s half-words behind lo | hi in the same allocation (C8Sample::nar)
    uint32_t n_wide_sorted = 0;                                  // sorted runs longer than 255 cells, which a half-word cannot hold: with any, k_direct_c8's narrow form is not launched
    uint32_t *b1 = nullptr, *o1 = nullptr;                       // (n_tiles << bshift) + 1 bucket starts per stream (one allocation: b1 | o1 | td, c8_index_bytes)
    TileDesc *td = nullptr;                                      // per tile: what k_direct_c8 reads before the tile's runs (made by runs_finish)
    uint32_t bshift = 4;                                         // 16 buckets of 512 cells per tile
    uint32_t n_long = 0;                                         // runs longer than a bucket: the direct kernels cannot use the sample
    uint32_t n_heavy = 0;                                        // pile-up tiles (more than PD_C8_HEAVY_CAND candidates): k_direct_c8 leaves them to the int-window pass
    uint32_t *heavy_tiles = nullptr;                             // ... and their numbers, n_heavy of them in no particular order (behind td in the index allocation; k_c8_tile_desc)
    pd_iv *iv12 = nullptr;                                       // the expanded copy, made on first need
    bool own_lo = true;                                          // the planes are this object's allocation (false: they live in the decode session's arena)
    C8Sample view() const { return C8Sample{lo, hi, b1, o1, o_base, bshift, nar}; }
};

// The window calls' result buffer and everything that goes with it: ONE owner (the methods that queue work are pd_windows.hip's).  The statistics of the
// last window call stay on the device (pd_text_append_window_rows formats the table's rows from them): commit() says which call's they are, pd_reset
// clears `valid` only.
struct WinKeep {
    static constexpr size_t PIN_BYTES = pdwin::PIN_BYTES;
    unsigned char *buf = nullptr; size_t bytes = 0;              // [sums | covers | status words] of pdwin::WinLayout
    uint32_t w = 0; pdwin::WinLayout lay; bool valid = false; std::vector<uint64_t> woff;      // what the last committed call left: its width, layout and window offsets
    // the window offsets of width woff_w on the device: an allocation of their own (c->scratch is every other call's too), uploaded only when a call
    // asks for another width, from woff_host — page-locked and the context's, so that no sync has to guard the upload's source (offsets)
    uint64_t *d_woff = nullptr, *woff_host = nullptr; uint32_t woff_w = 0;
    pdwin::WordsState words;                                     // the direct call's two sets of status words behind its results (pdwin::words_turn)
    // the direct path's results (sums | covers | status words, contiguous in buf) come back in ONE copy into this page-locked buffer of PIN_BYTES,
    // made by the first call that needs it (pin_fit); larger results go straight to the caller's arrays
    unsigned char *pin = nullptr, *pin_dev = nullptr;            // (pin_dev: its device address, what k_window_gather stores through)

    int fit(pd_ctx *c, size_t need);                             // room for `need` bytes; whoever calls writes the buffer: nothing kept is valid, the status words are unknown
    int offsets(pd_ctx *c, uint32_t width, const std::vector<uint64_t> &wo, const uint64_t **d_wo);
    int pin_fit(pd_ctx *c);
    void commit(uint32_t width, const pdwin::WinLayout &l, const std::vector<uint64_t> &wo) { w = width; lay = l; woff = wo; valid = true; }
    void release();                                              // pd_destroy: the buffer, the offsets and the page-locked memory
    // of a call with layout l (before its commit) ...
    unsigned long long *sums() const { return (unsigned long long *)buf; }
    uint32_t *covers(const pdwin::WinLayout &l) const { return (uint32_t *)(buf + l.b_sum); }
    uint32_t *status(const pdwin::WinLayout &l, unsigned turn) const { return (uint32_t *)(buf + l.b_res + turn * pdwin::STATUS_BYTES); }
    // ... and of the committed call: contig tid's rows from row_first on
    uint64_t n_rows(int32_t tid) const { return woff[(size_t)tid + 1] - woff[(size_t)tid]; }
    void rows(int32_t tid, uint64_t row_first, const unsigned long long **sum, const uint32_t **cover) const
    {
        const uint64_t g0 = woff[(size_t)tid] + row_first;
        *sum = sums() + g0; *cover = covers(lay) + g0;
    }
};

static inline size_t slice_flag_bytes(uint64_t n_tiles) { return (size_t)((n_tiles + 16 + 15) / 16 * 16); }

struct pd_ctx {
    int device = 0;
    hipStream_t stream = nullptr, copy_stream = nullptr;
    // the direct window call's pile-up pass runs on a stream of its own beside k_direct_c8 (not copy_stream, whose users must not be reordered): it waits
    // for ev_fork, recorded on `stream` in front of that kernel, and `stream` waits for ev_join, recorded behind the pass, before the gather.  Both are made
    // with the context.  Whoever frees or reuses what the pass reads (the sample, c->scratch) syncs `stream`, which is behind the join on every path.
    hipStream_t side_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int32_t n_contigs = 0;
    std::vector<uint32_t> len;
    std::vector<uint64_t> off;                       // first cell of each slot
    uint64_t n_cells = 0, n_tiles = 0, n_words = 0;
    int *buf = nullptr;                              // [n_cells diff | n_tiles sums | pad]
    uint8_t *slab = nullptr;                         // ONE allocation behind the seventeen small buffers below (carry .. chk)
    int *sums = nullptr, *carry = nullptr, *bsum = nullptr;
    uint64_t *d_off = nullptr; uint32_t *d_len = nullptr; uint32_t *d_tile_contig = nullptr;
    uint32_t *ub_a[PD_MAXPEND] = {}, *cand_lo[PD_MAXPEND] = {};   // per pending batch, indexed by 4096-cell tile
    BatchDesc *desc = nullptr; CheckWords *chk = nullptr;         // desc: PD_MAXPEND entries
    uint8_t *hstate = nullptr; uint32_t n_half = 0;               // "written since reset" per 4096 cells
    uint8_t *slice_flags = nullptr;                               // pd_slice_sweep_i4: tiles that own exceptions
    bool accumulate_packed = true;                                // pd_accumulate_from: 4-bit transport
    bool direct_windows = false;                                  // pd_keep_deferred: a whole deferred sample stays deferred, the direct kernels may read it
    bool pristine = true;                                         // nothing materialised in the arrays since the last reset
    bool sums_stale = false;                                      // the tile sums hold what a direct export wrote while the sample is still deferred
    uint32_t *direct_words = nullptr;                             // [n_long, fail, heavy_count, diagnostics ..., [12] tiles settled by the cover pass | heavy tile list at +16]
                                                                  // (the status words of a direct WINDOW call lie behind its results in WinKeep::buf, so that one copy brings both back; the export's are here)
    bool dec_crc = true;                                          // the decoder checks every member's CRC-32 ("decode_crc")
    unsigned lz_group = 16;                                       // chunks per workgroup of the LDS parse ("lz_group", up to 16; 0: every chunk parses with its text in memory).  Round 5's default: sixteen
                                                                  // chunks of 8 + 2 KiB share a CU's LDS (158 KB: 32 KiB of history + their text), 16 waves per CU — 8.6 ms against 11.8 for the 60 MB call of
                                                                  // profiles/r04_lz_parse_ab.txt, and the text is fetched once instead of ~1 000 times; chunks of 16 KiB fit seven to a CU and lose
    unsigned dec_waves = 20;                                      // one-wave inflate workgroups per CU and launch ("inflate_waves")
    std::atomic<uint32_t> dec_oth_div{41};                        // inflated bytes per slot for a later run in a batch's arrays: 41 (a kept record's minimum size) until a batch
                                                                  // does not fit (long reads: a later run per 8 bytes of CIGAR), then 8 for the batches that follow
    int dec_sync_event = 1;                                       // "decode_sync_event": pd_decode_collect waits for the batch's last event (0: for its stream, as until round 6)
    int dec_h2d_fifo = 1;                                         // "decode_h2d_fifo": the batches' compressed bytes go up ONE after the other on a copy stream of their own (see pd_decode_queue)
    std::mutex dec_copy_mu; int dec_h2d_lanes = 1; uint64_t dec_copy_seq = 0; hipStream_t dec_copy_st2 = nullptr;   // "decode_h2d_lanes": 2 = the batches' copies alternate between the main stream and a second one (two on the link at a time)
    int dec_h2d_kernel = 0;                                       // "decode_h2d_kernel": a batch's compressed bytes fetched from the pinned buffer by a copy KERNEL on the batch's stream instead of the copy engine
    bool dec_fast = true;                                         // the record chain of a batch is confirmed on the device where the session allows it ("decode_fast")
    uint32_t dec_spoil = 0;                                       // test hook: every k-th segment's guess is spoilt after pass 1 ("decode_spoil")
    uint32_t dec_max_redo = 256;                                  // ... with at most this many segments walking again per batch ("decode_max_redo")
    uint64_t dec_c8_reserve = 0;                                  // test hook ("decode_c8_reserve" = n > 0): a compact session's first estimate is at most n first runs and its sample grows
                                                                  // without the 2^16 runs of slack, so that files of a few thousand records make the sample grow and move (0: off)
    // which way the last session went (read through pd_profile_get, names "decode_*"; cleared by pd_decode_begin)
    enum { DN_GROW, DN_END_COMPACT, DN_END_C8_FALLBACK, DN_END_RUNS_MAKE, DN_END_SCATTER, DN_END_UNSORTED, DN_END_PEND, DN_GUESS, DN_COUNT };
    std::atomic<uint64_t> dec_n[DN_COUNT] = {};
    std::atomic<uint64_t> dec_n_fast{0}, dec_n_slow{0}, dec_n_redo{0};   // batches finished without / with the host's chain check; segments the device walked again
    uint32_t direct_sample = 256;                                 // index stride of the direct path (runs)
    uint32_t q_wave_max = 512, q_split = 262144;                  // "quantile_wave_max" / "quantile_split_cells": the cell counts up to which a quantile row takes the narrow / the workgroup kernel
    uint32_t t_wave_max = 65536;                                  // "threshold_wave_max": the cell count up to which a threshold row is counted by a group of lanes, not in pieces
    uint64_t gc_piece_cells = (uint64_t)1 << 25;                  // "gcbias_piece_cells": the cells (= base bytes) of one piece of pd_depth_gc_bias, rounded down to whole windows (at least one)
    uint32_t gc_wave_max = 4096;                                  // "gcbias_wave_max": the window width up to which a window is read by a group of lanes, not by a workgroup
    int hist_variant = 1;                                        // "hist_variant": the histogram kernels' LDS form (launch_sweep_hist): 1 = one copy per workgroup, folded (measured best)
    int direct_un = 0;                                           // 0 = the default form of the direct kernels (launch_direct_tiles, launch_direct_c8)
    bool direct_cover = true;                                    // k_direct_c8's default form settles covered tiles from the runs (false: the window path for every tile)
    uint32_t direct_cover_min = 2048;                            // ... of tiles with at least this many candidates (launch_direct_c8)
    bool cover_narrow = true;                                    // ... from the sorted stream's narrow plane where the sample allows it ("cover_narrow"; pd_runs::n_wide_sorted == 0)
    bool cover_fast = true;                                      // ... whose full chunks are first tried as fast chunks ("cover_fast"; pd_cover_rule.h)
    uint64_t direct_fast = 0;                                    // chunks the narrow sweep accepted as fast chunks in the last direct_windows call ("direct_cover_fast")
    uint64_t direct_narrow = 0;                                  // 1: the last direct_windows call launched the narrow form ("direct_cover_narrow")
    uint64_t direct_settled = 0;                                 // tiles the cover pass settled in the last direct_windows call
    uint64_t direct_pileup = 0;                                  // pile-up tiles k_direct_c8 listed in the last direct_windows call (the int-window pass did them)
    bool all_valid_host = false;
    std::vector<Pending> pend;
    // ---- device decode (pd_decode_*): a few batch slots, each with its own stream and buffers ----
    struct DecSlot {
        bool busy = false;
        bool warming = false;                                     // the session's warm-up thread is still making this slot's buffer and stream (dec_mu)
        hipStream_t st = nullptr;
        hipEvent_t ev[6] = {};
        hipEvent_t ev_rs[2] = {};                                 // around k_record_stats (PD_DECODE_RECORD_STATS sessions that are timed; made on first need)
        hipEvent_t ev_rc[2] = {};                                 // around k_row_counts (PD_DECODE_ROW_COUNTS sessions, likewise)
        hipEvent_t ev_as[2] = {};                                 // around k_aln_stats (PD_DECODE_ALN_STATS sessions, likewise)
        hipEvent_t ev_done = nullptr;                             // recorded behind everything pd_decode_queue puts on the stream: what pd_decode_collect waits for
        uint8_t *h_blob = nullptr; size_t h_cap = 0;              // page-locked (pin_alloc)
        bool h_mapped = false;                                    // ... as huge pages of its own registered with the runtime (freed by pin_free)
        uint8_t *h_small = nullptr; size_t h_small_cap = 0;       // pinned: the batch's small tables on their way to and from the device
        void *d[9] = {}; size_t cap[9] = {};                      // (DS_* of pd_decode.hip) blob, inflated, tables (members | segments | member counter), status, lanes, redo list,
                                                                  // ChainOut + per-segment keys (compact emission), and the runs of a batch whose chain the device
                                                                  // confirms itself: first runs (8 B; a compact session's as two planes), later runs (12 B) — copied to exact arrays when the batch is collected
        void *d_tok = nullptr; unsigned tok_wg = 0;               // wave scratch (match tokens) and the number of workgroups it was sized for
        // a batch between pd_decode_queue and pd_decode_collect (pd_decode_submit: the two back to back)
        struct Job {
            bool open = false, queued = false, c8 = false, fast = false, owes_count = false, timed = false;
            bool rc_timed = false;                                 // ev_rc were recorded for this batch
            bool as_timed = false;                                 // ev_as were recorded for this batch
            bool segs_sent = false, rs_timed = false;              // the host's segments (bases, RS_SKIP marks) are on the device; ev_rs were recorded for this batch
            bool collecting = false;                               // some thread is inside dec_collect on this slot (set and tested under dec_mu): one ticket, one collect
            uint64_t order = 0; size_t n_bytes = 0; uint64_t inflated = 0; uint32_t n_seg = 0;
            std::vector<pd_bgzf_block> blocks; std::vector<pd_decode_unit> units; std::vector<pdb2::Seg> segs; std::vector<uint32_t> seg0;
            // where the batch's small tables lie in the staging area (and, up to `up`, in the device's copy of it): members, segments, member counter |
            // member statuses, ChainOut, the segments' keys, the order words
            struct Tabs { size_t blk = 0, seg = 0, next = 0, up = 0, bst = 0, co = 0, so = 0, ord = 0; } o;
            pdb2::Cfg cfg{};
            uint8_t *d_tab = nullptr;                              // the batch's tables on the device: the slot's table buffer, or behind the members in the blob buffer (one copy)
            uint64_t cap_first = 0, cap_other = 0, t_mark = 0, t_q0 = 0, t_q1 = 0;      // (t_q0 / t_q1: PANDEPTH_DEVTRACE)
        } job;
        uint32_t gen = 0;
    };
    struct RunSeg { uint64_t order; pd_iv *first; uint64_t n_first; pd_iv *other; uint64_t n_other; pd_iv *far; uint64_t n_far; uint32_t max_span; uint32_t unsorted; uint64_t first_key, last_key; uint64_t n_long = 0;
                    void release(pd_ctx *c); };                      // gives back the arrays that are allocations of their own (not the arena's)
    static constexpr int N_DEC = 12;
    uint8_t *arena = nullptr; size_t arena_cap = 0; std::atomic<size_t> arena_used{0};   // the batches' run arrays (bump allocated)
    DecSlot dec[N_DEC];
    std::mutex dec_mu; std::condition_variable dec_cv;
    bool dec_open = false;
    bool dec_warm_on = false;                                     // "decode_warm"
    std::thread dec_warm;                                         // pd_decode_begin's helper: the first slots' page-locked buffers, streams and hardware queues, one after the other, beside the caller
    void *dec_warm_word = nullptr;
    uint32_t dec_near_span = 0xFFFFFFFFu;                         // "decode_near_span": split the later runs into two streams (off)
    bool dec_deletions = false;                                   // "decode_deletions": pd_push_bgzf_units opens its session with PD_DECODE_DELETIONS
    bool dec_fragments = false;                                   // "decode_fragments": ... with PD_DECODE_FRAGMENTS
    uint32_t dec_frag_max = 0;                                    // "decode_frag_max": a PD_DECODE_FRAGMENTS session's bound on |tlen| (0: none), read by pd_decode_begin ...
    uint32_t dec_frag_bound = 0x7FFFFFFFu;                        // ... into this, the open session's bound
    // PD_DECODE_RECORD_STATS: the open (or last ended) session's sums — PD_RECSTAT_FIXED + rs_bins + 1 words, then 3 per contig (pd_recstats.h) —, zeroed by
    // pd_decode_begin, added to by every batch's k_record_stats, read by pd_decode_record_stats between pd_decode_end and the next pd_decode_begin
    uint32_t dec_isize_bins = 0;                                  // "decode_isize_bins": the insert bins of the next such session (1 .. 65536), read by pd_decode_begin ...
    uint32_t rs_bins = 0;                                         // ... into this
    unsigned long long *d_recstat = nullptr; size_t recstat_words = 0; bool rs_ready = false;
    std::atomic<uint64_t> rs_launches{0}, rs_ns{0};               // "decode_record_stats": launches of the session, and their summed time where the batches are timed
    // PD_DECODE_ROW_COUNTS (pd_rowcounts.h): rb_* is the table pd_decode_row_bins left for the sessions begun after it (host copies); pd_decode_begin takes
    // it to the device as the open session's (rc_*: offsets, edges, rc_nbins bins of PD_ROWCOUNT_WORDS words, zeroed), every batch's k_row_counts adds to
    // d_rowcnt, pd_decode_row_counts reads it between pd_decode_end and the next pd_decode_begin
    bool rb_set = false; uint32_t rb_w = 0; std::vector<uint64_t> rb_off; std::vector<uint32_t> rb_edges; uint64_t rb_nbins = 0;
    uint32_t rc_w = 0; uint64_t rc_nbins = 0; uint64_t *d_rc_off = nullptr; uint32_t *d_rc_edges = nullptr; size_t rc_edges_cap = 0;
    unsigned long long *d_rowcnt = nullptr; size_t rowcnt_words = 0; bool rc_ready = false;
    std::atomic<uint64_t> rc_launches{0}, rc_ns{0};               // "decode_row_counts": launches of the session, and their summed time where the batches are timed
    // PD_DECODE_ALN_STATS (pd_alnstats.h): the open (or last ended) session's PD_ALNSTAT_WORDS sums, zeroed by pd_decode_begin, added to by every batch's
    // k_aln_stats, read by pd_decode_aln_stats between pd_decode_end and the next pd_decode_begin
    uint32_t dec_len_bin_width = 0;                               // "decode_len_bin_width": the width of a length bin of the next such session (1 .. 65536), read by pd_decode_begin ...
    uint32_t as_width = 0;                                        // ... into this
    unsigned long long *d_alnstat = nullptr; bool as_ready = false;
    std::atomic<uint64_t> as_launches{0}, as_ns{0};               // "decode_aln_stats": launches of the session, and their summed time where the batches are timed
    pd_decode_cfg dec_cfg{}; uint8_t *d_contig_on = nullptr; uint32_t *d_span_off = nullptr; int32_t *d_spans = nullptr;
    std::vector<RunSeg> run_segs;
    pd_iv *run_first = nullptr, *run_other = nullptr, *run_far = nullptr;   // the concatenated sample (owned until the next reset)
    pd_runs *dec_runs = nullptr;                                  // ... or the whole of it as a compact sample (PD_DECODE_COMPACT)
    // A decode session that emits the compact form directly (PD_DECODE_COMPACT + pd_decode_cfg::n_batches): every batch's pass 2 writes its
    // first runs as 8-byte compact runs (and marks the buckets' first runs, keyed by (batch, index in the batch)); as soon as every
    // earlier batch has been counted, a batch's runs are copied — on a stream of their own, behind the decode — to their FINAL places in
    // the sample's sorted stream, and its later runs behind those of the batches before it.  No feeder ever waits for another one, and at
    // the end nothing is concatenated or converted: only the marks become indices and the later runs are sorted by bucket.
    struct C8Dec {
        bool on = false;
        uint8_t *base = nullptr; size_t bytes = 0;               // ONE allocation: [lo plane x (cap_s + cap_o) | hi plane x (cap_s + cap_o) | pd_iv x cap_o | 64 bytes, to a 16-byte boundary | narrow plane: half-word x cap_s | slack]
        size_t cap_s = 0, cap_o = 0;
        uint32_t *b1 = nullptr; size_t nbw = 0;                  // bucket starts: b1 | o1, nbw words each, then the sample's tile descriptors (c8_index_bytes)
        unsigned long long *marks = nullptr;                     // per bucket: min (batch << 32 | index in the batch) of a run that begins there; behind the nbw marks one more
                                                                 // 8 bytes: a word that counts the first runs longer than 255 cells as they are placed (wide())
        uint32_t bshift = 4;
        uint64_t n_s = 0, n_o = 0, turn = 0, n_batches = 0;
        struct Batch { bool counted = false; uint64_t nf = 0, no = 0; uint32_t *seg_s = nullptr; pd_iv *seg_o = nullptr; hipEvent_t ev = nullptr; };   // seg_s: the nf first runs' lo plane, their hi plane c8_plane_words(nf) behind it
        std::vector<Batch> batch;                                // by order
        std::vector<uint32_t> base_s;                            // first place of every batch's first runs in the sorted stream
        hipStream_t compose = nullptr;
        std::string err;                                         // what went wrong while runs were being placed (reported by pd_decode_end)
        std::mutex mu;
        uint32_t *lo() const { return (uint32_t *)base; }
        uint32_t *hi() const { return (uint32_t *)base + cap_s + cap_o; }
        pd_iv *oth() const { return (pd_iv *)(base + (cap_s + cap_o) * sizeof(Run8)); }
        static size_t nar_off(size_t cs, size_t co) { return ((cs + co) * sizeof(Run8) + co * sizeof(pd_iv) + 64 + 15) & ~(size_t)15; }
        static size_t total_bytes(size_t cs, size_t co) { return nar_off(cs, co) + cs * 2 + 64 + 256; }
        uint16_t *nar() const { return (uint16_t *)(base + nar_off(cap_s, cap_o)); }
        uint32_t *wide() const { return (uint32_t *)(marks + nbw); }
    } c8;
    uint64_t *ovf = nullptr; uint32_t ovf_cap = 0;    // ends of runs longer than lmax (grown on demand)
    std::vector<Stage> stage;                        // grows on demand, up to N_STAGE
    uint64_t seq = 0;
    void *scratch = nullptr; size_t scratch_bytes = 0;
    int state = 0;                                   // 0 accumulating (diff), 1 depth
    uint32_t lmax = LMAX_DEFAULT, sample = SAMPLE_DEFAULT;
    unsigned grid_tiles = 0;                         // 0 = sized per pass from the number of runs
    int stile = 8192; int n_cu = 256;
    // pd_deflate_parse's work buffers (device memory, grown on demand, kept until pd_destroy): two slots, each with its stream, so that
    // two calls overlap (one's copies under the other's kernels)
    struct LzWork {
        static constexpr int N = 16;
        void *p[N] = {}; size_t cap[N] = {};
        bool fit(int k, size_t bytes)
        {
            if (bytes <= cap[k]) return true;
            if (p[k]) { (void)hipFree(p[k]); p[k] = nullptr; cap[k] = 0; }
            const size_t want = bytes + bytes / 8 + 4096;
            if (hipMalloc(&p[k], want) != hipSuccess) return false;
            cap[k] = want;
            return true;
        }
        void release() { for (int k = 0; k < N; ++k) { if (p[k]) (void)hipFree(p[k]); p[k] = nullptr; cap[k] = 0; } if (st) { (void)hipStreamDestroy(st); st = nullptr; }
                         if (h_stage) { (void)hipHostFree(h_stage); h_stage = nullptr; } for (auto &e : ev_stage) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
        hipStream_t st = nullptr;
        void *h_stage = nullptr; hipEvent_t ev_stage[2] = {nullptr, nullptr};     // page-locked staging of the symbols' way back
        std::mutex mu;
    } lz[4];                                                      // (a round's provider calls in flight at once: two until round 6, up to four)
    std::atomic<unsigned> lz_turn{0}; unsigned lz_slots = 2;         // "lz_slots": 2 or 4 of lz[] in use
    bool lz_mix = false;                                          // "lz_mix": see lz_run
    WinKeep win;                                                  // the window calls' result buffer and what the last call left in it
    bool prof = false;
    std::vector<ProfRec> prof_pending;
    std::vector<hipEvent_t> ev_pool;
    std::map<std::string, std::pair<double, uint64_t>> prof_acc;
    std::mutex mu;
    std::string err;
};

namespace pdi {

int fail(pd_ctx *c, int code, const std::string &msg);
int need_state(pd_ctx *c, int want, const char *fn);      // every entry point that needs the arrays in a given state (0 accumulating, 1 depth)

#define HIPOK(ctx, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(ctx, PD_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));        \
    } while (0)

ContigTab tab_of(pd_ctx *c);
hipEvent_t get_event(pd_ctx *c);

struct ProfScope {
    pd_ctx *c; ProfRec r; bool on;
    ProfScope(pd_ctx *ctx, const char *name) : c(ctx), on(ctx->prof)
    {
        if (on) { r.name = name; r.a = get_event(c); r.b = get_event(c); (void)hipEventRecord(r.a, c->stream); }
    }
    ~ProfScope()
    {
        if (on) { (void)hipEventRecord(r.b, c->stream); c->prof_pending.push_back(r); }
    }
};

int flush_pending(pd_ctx *c);
int ensure_scratch(pd_ctx *c, size_t bytes);
int check_words(pd_ctx *c);
// the pending sample made ready for a tile pass: compact batches expanded, ps filled, every batch's sparse index (stride runs) launched; *all = its runs.
// skip: the caller's kernel reads the lone compact sample as it is — only the count
int pend_prepare(pd_ctx *c, uint32_t stride, uint32_t n_stiles, int stile, bool skip, PendSet *ps, uint64_t *all);
// the windows of width w: the contigs' first windows into wo (pd_window_layout), the result layout returned
pdwin::WinLayout win_table(const pd_ctx *c, uint32_t w, std::vector<uint64_t> *wo);
int scatter_device(pd_ctx *c, const pd_iv *d, size_t n, unsigned flags, int slot, bool *deferred);
uint8_t *pin_alloc(size_t bytes, bool *mapped);
void pin_free(uint8_t *p, size_t bytes, bool mapped);
void runs_free(pd_runs *r);
uint32_t runs_bshift(const pd_ctx *c);
void runs_finish(pd_ctx *c, pd_runs *r, const pd_iv *const *others, const size_t *n_others, int n_arr, uint32_t *tmp, uint32_t *words);
int runs_make(pd_ctx *c, const pd_iv *sorted, size_t n_sorted, const pd_iv *const *others, const size_t *n_others, int n_arr, pd_runs **out);
inline uint64_t dec_now_us() { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

} // namespace pdi
