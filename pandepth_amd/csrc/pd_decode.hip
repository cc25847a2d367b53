// pd_decode.hip — the batched BAM decode session of include/pandepth_amd.h (pd_decode_*, pd_push_bgzf_units) on the context of pd_ctx.h.
//
// A session is pd_decode_begin, then per batch pd_decode_acquire + pd_decode_submit (or pd_decode_queue + pd_decode_collect), then
// pd_decode_end.  A batch is dec_queue (everything it needs goes onto its slot's stream) and dec_collect (wait, finish, report); each is a
// short list of steps, and every step is a function of this file.
#include "pd_ctx.h"
#include "pd_recstats.h"
#include "pd_rowcounts.h"
#include "pd_alnstats.h"

// ---------------------------------------------------------------------------------------------------------------
// GPU-side BAM decode in asynchronous batches (include/pandepth_amd.h: pd_decode_*)
// ---------------------------------------------------------------------------------------------------------------
namespace {

using DecSlot = pd_ctx::DecSlot;
using Job = pd_ctx::DecSlot::Job;
using RunSeg = pd_ctx::RunSeg;

// a slot's device buffers, DecSlot::d.  (The segments once had a buffer of their own, DS_SEG; they travel in DS_BLK's tables and the place is dropped.)
enum { DS_BLOB, DS_INF, DS_BLK, DS_ST, DS_LANE, DS_ONLY, DS_SEGOUT, DS_R8, DS_OTH, DS_COUNT };
static_assert(DS_COUNT == sizeof(DecSlot::d) / sizeof(void *) && DS_COUNT == sizeof(DecSlot::cap) / sizeof(size_t), "DecSlot::d and cap: one place per DS_*");

// PANDEPTH_TIMING=1: where the host side of the decode path spends its time (thread-microseconds, summed)
std::atomic<uint64_t> g_dec_us[8];
struct DecTimer { int k; uint64_t t0; explicit DecTimer(int k_) : k(k_), t0(dec_now_us()) {} ~DecTimer() { g_dec_us[k] += dec_now_us() - t0; } };
// the time since the job's last mark goes to timer k
void dec_lap(Job &J, int k) { const uint64_t n = dec_now_us(); g_dec_us[k] += n - J.t_mark; J.t_mark = n; }

const bool g_dec_devtrace = getenv("PANDEPTH_DEVTRACE") != nullptr;  // (development: host-clock times at which a batch's stages were seen to end, a line per batch)
const bool g_dec_timing = getenv("PANDEPTH_TIMING") != nullptr || g_dec_devtrace;     // the per-batch device events are recorded only when somebody reads them

int dec_fail(pd_ctx *c, int code, const std::string &msg) { std::lock_guard<std::mutex> lk(c->mu); return fail(c, code, msg); }

#define HIPDEC(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return dec_fail(c, PD_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

std::mutex g_alloc_mu;                   // pinned / device allocations of the decode slots, one at a time

int dec_ensure(pd_ctx *c, DecSlot &sl, int k, size_t bytes)
{
    if (bytes <= sl.cap[k]) return PD_OK;
    std::lock_guard<std::mutex> al(g_alloc_mu);
    if (sl.d[k]) { HIPDEC(hipStreamSynchronize(sl.st)); HIPDEC(hipFree(sl.d[k])); sl.d[k] = nullptr; sl.cap[k] = 0; }
    const size_t want = bytes + bytes / 8 + 4096;
    if (hipMalloc(&sl.d[k], want) != hipSuccess) return dec_fail(c, PD_ENOMEM, "device-decode buffer allocation failed");
    sl.cap[k] = want;
    return PD_OK;
}

// the host side of a batch after pass 1: pdb2::check_chain (pd_bamwalk.h)
uint32_t dec_finish(std::vector<pdb2::Seg> &segs, std::vector<uint32_t> *redo) { return pdb2::check_chain(segs, redo); }

static_assert(sizeof(pdb2::R8) == sizeof(Run8), "the decoder's 8-byte run is the kernels' Run8");
size_t c8_seg_bytes(uint64_t nf) { return 2 * c8_plane_words((size_t)nf) * 4; }      // a batch's first runs as two planes

// ---- who owns a batch's run arrays: the session's arena (bump allocated, given back as a whole) or an allocation of their own ----
bool arena_owns(const pd_ctx *c, const void *p) { return c->arena && (const uint8_t *)p >= c->arena && (const uint8_t *)p < c->arena + c->arena_cap; }
void arena_free(pd_ctx *c, void *p) { if (p && !arena_owns(c, p)) (void)hipFree(p); }

// room for a batch's runs: the arena first, an allocation of its own when that is full
bool dec_grab(pd_ctx *c, size_t bytes, void **out)
{
    bytes = (bytes + 255) & ~(size_t)255;
    const size_t at = c->arena_used.fetch_add(bytes);
    if (at + bytes <= c->arena_cap) { *out = c->arena + at; return true; }
    if (hipMalloc(out, bytes) == hipSuccess) return true;
    (void)hipGetLastError(); *out = nullptr;
    return false;
}

// The arrays (and, for a compact batch, the event) a call has taken for its batch and not yet handed on — to the session's list of
// batches or to c8_counted: every early return gives them back.
struct Owned {
    pd_ctx *c; void *p[3] = {nullptr, nullptr, nullptr}; hipEvent_t ev = nullptr; bool kept = false;
    bool grab(int k, size_t bytes) { return dec_grab(c, bytes, &p[k]); }
    ~Owned()
    {
        if (kept) return;
        for (void *q : p) arena_free(c, q);
        if (ev) (void)hipEventDestroy(ev);
    }
};

} // namespace

void pd_ctx::RunSeg::release(pd_ctx *c) { for (pd_iv *q : {first, other, far}) arena_free(c, q); }

namespace {

// ---- compact decode sessions (pd_ctx::C8Dec) ----
void c8_drop(pd_ctx *c)
{
    pd_ctx::C8Dec &x = c->c8;
    if (x.compose) (void)hipStreamSynchronize(x.compose);
    if (x.base) { (void)hipFree(x.base); x.base = nullptr; }
    if (x.b1) { (void)hipFree(x.b1); x.b1 = nullptr; }
    if (x.marks) { (void)hipFree(x.marks); x.marks = nullptr; }
    for (auto &b : x.batch) {
        arena_free(c, b.seg_s);
        arena_free(c, b.seg_o);
        if (b.ev) (void)hipEventDestroy(b.ev);
    }
    x.batch.clear(); x.base_s.clear();
    x.on = false; x.bytes = 0; x.cap_s = x.cap_o = 0; x.n_s = x.n_o = x.turn = x.n_batches = 0;
}

// room for n_s first runs and n_o later runs in the sample's final arrays (the caller holds c8.mu; copies placed earlier may still be
// running — the device is waited for before anything moves).  Returns PD_OK / PD_ENOMEM / PD_EHIP, no message.
int c8_reserve(pd_ctx *c, uint64_t n_s, uint64_t n_o, bool exact = false)
{
    pd_ctx::C8Dec &x = c->c8;
    if (n_s <= x.cap_s && n_o <= x.cap_o && x.base) return PD_OK;
    const size_t slack = c->dec_c8_reserve ? 0 : (size_t)1 << 16;
    const size_t ns = std::max<size_t>((size_t)n_s + (exact ? 0 : (size_t)n_s / 2) + slack, x.cap_s), no = std::max<size_t>((size_t)n_o + (exact ? 0 : (size_t)n_o / 2) + slack, x.cap_o);
    const size_t bytes = pd_ctx::C8Dec::total_bytes(ns, no);
    uint8_t *nb = nullptr;
    if (x.base) (void)hipDeviceSynchronize();
    if (hipMalloc(&nb, bytes) != hipSuccess) { (void)hipGetLastError(); return PD_ENOMEM; }
    if (x.base) {
        ++c->dec_n[pd_ctx::DN_GROW];
        hipError_t e = hipSuccess;
        if (x.n_s) e = hipMemcpy(nb, x.lo(), (size_t)x.n_s * 4, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && x.n_s) e = hipMemcpy(nb + (ns + no) * 4, x.hi(), (size_t)x.n_s * 4, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && x.n_o) e = hipMemcpy(nb + (ns + no) * sizeof(Run8), x.oth(), (size_t)x.n_o * sizeof(pd_iv), hipMemcpyDeviceToDevice);
        if (e == hipSuccess && x.n_s) e = hipMemcpy(nb + pd_ctx::C8Dec::nar_off(ns, no), x.nar(), (size_t)x.n_s * 2, hipMemcpyDeviceToDevice);
        (void)hipFree(x.base);
        if (e != hipSuccess) { (void)hipFree(nb); x.base = nullptr; return PD_EHIP; }
    }
    x.base = nb; x.bytes = bytes; x.cap_s = ns; x.cap_o = no;
    return PD_OK;
}

// A batch has been counted (its runs are being written to its own segment, `ev` follows that kernel): it and every batch behind it whose
// predecessors are all counted now get their final places, and the copies there are queued on the compose stream.  Nobody waits.
void c8_counted(pd_ctx *c, uint64_t order, uint64_t nf, uint64_t no, uint32_t *seg_s, pd_iv *seg_o, hipEvent_t ev)
{
    pd_ctx::C8Dec &x = c->c8;
    std::lock_guard<std::mutex> lk(x.mu);
    if (order >= x.batch.size() || x.batch[(size_t)order].counted) { if (x.err.empty()) x.err = "a batch number was submitted twice or lies outside the session"; return; }
    pd_ctx::C8Dec::Batch &me = x.batch[(size_t)order];
    me.counted = true; me.nf = nf; me.no = no; me.seg_s = seg_s; me.seg_o = seg_o; me.ev = ev;
    while (x.turn < x.n_batches && x.batch[(size_t)x.turn].counted) {
        pd_ctx::C8Dec::Batch &b = x.batch[(size_t)x.turn];
        x.base_s[(size_t)x.turn] = (uint32_t)x.n_s;
        if (b.nf + b.no) {
            hipError_t e = hipSuccess;
            // (when the sample outgrows its arrays — every growth waits for the device and moves what is there — they are made large enough for
            // the REST of the file at the rate seen so far, not half again: a long-read file has 1 600 later runs per first run where the first
            // estimate assumed one in four, and eight growths of gigabytes stalled every feeder — 8 thread-seconds on 128 batches)
            uint64_t want_s = x.n_s + b.nf, want_o = x.n_o + b.no;
            if ((want_s > x.cap_s || want_o > x.cap_o) && x.n_batches > x.turn + 1) {
                const double f = 1.05 * (double)x.n_batches / (double)(x.turn + 1);
                want_s = std::max<uint64_t>(want_s, (uint64_t)((double)want_s * f)); want_o = std::max<uint64_t>(want_o, (uint64_t)((double)want_o * f));
                if (c8_reserve(c, want_s, want_o, /*exact=*/true) != PD_OK) { want_s = x.n_s + b.nf; want_o = x.n_o + b.no; }      // (no room for the projection: what is needed now)
            }
            if (c8_reserve(c, x.n_s + b.nf, x.n_o + b.no) != PD_OK) e = hipErrorOutOfMemory;
            if (e == hipSuccess && b.ev) e = hipStreamWaitEvent(x.compose, b.ev, 0);
            // (EVERY first run of the session reaches the sample through this copy and no other way: it is where the narrow plane is written, from the
            // lo words on their way, and where the runs that plane cannot hold are counted)
            if (e == hipSuccess && b.nf) launch_copy_planes(x.compose, x.lo() + x.n_s, x.hi() + x.n_s, b.seg_s, b.seg_s + c8_plane_words((size_t)b.nf), b.nf, x.nar() + x.n_s, x.wide());
            if (e == hipSuccess && b.no) launch_copy_words(x.compose, x.oth() + x.n_o, b.seg_o, b.no * (sizeof(pd_iv) / 4));
            if (e == hipSuccess) e = hipGetLastError();
            if (e != hipSuccess && x.err.empty()) x.err = std::string("placing a batch's runs: ") + hipGetErrorString(e);
            x.n_s += b.nf; x.n_o += b.no;
        }
        ++x.turn;
    }
}

// every batch with an order below n_batches is counted exactly once, whatever way its calls end; a batch that had something queued
// and is counted empty through an error path leaves the session in error (its totals would silently disagree with the file)
struct C8Owes {
    pd_ctx *c; Job *j; bool armed = true;
    ~C8Owes()
    {
        if (!armed || !j->owes_count) return;
        j->owes_count = false;
        if (j->queued) { std::lock_guard<std::mutex> lk(c->c8.mu); if (c->c8.err.empty()) c->c8.err = "a batch of the session failed on the device"; }
        c8_counted(c, j->order, 0, 0, nullptr, nullptr, nullptr);
    }
};

// A compact batch's runs are handed to the session: segments of their own for the nf first runs (8 bytes each, as two planes) and the no later runs
// (12 bytes), an event; `fill(seg_s, seg_o)` puts on the slot's stream what writes them (a copy of what the device emitted, or the
// emission itself) and the event follows it; c8_counted then queues the copies to the runs' final places for every batch whose
// predecessors are all counted.  The segments and the event are this call's until c8_counted has taken them.
template <class Fill>
int c8_hand_over(pd_ctx *c, DecSlot &sl, uint64_t nf, uint64_t no, Fill fill)
{
    Owned g{c};
    if (nf + no) {
        if ((nf && !g.grab(0, c8_seg_bytes(nf))) || (no && !g.grab(1, (size_t)no * sizeof(pd_iv))) ||
            hipEventCreateWithFlags(&g.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return dec_fail(c, PD_ENOMEM, "run segment allocation failed"); }
        if (const int rc = fill((uint32_t *)g.p[0], (pd_iv *)g.p[1])) return rc;
        HIPDEC(hipEventRecord(g.ev, sl.st));
    }
    sl.job.owes_count = false; g.kept = true;
    c8_counted(c, sl.job.order, nf, no, (uint32_t *)g.p[0], (pd_iv *)g.p[1], g.ev);
    return PD_OK;
}

// ---- a slot's resources ----
// The slot's stream, its six timing events and ev_done (the slot has none of them); what was made is undone when one cannot be made.
hipError_t slot_streams(DecSlot &sl)
{
    hipError_t e = hipStreamCreateWithFlags(&sl.st, hipStreamNonBlocking);
    for (auto &ev : sl.ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming);
    if (e == hipSuccess) return e;
    (void)hipGetLastError();
    for (auto &ev : sl.ev) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    if (sl.ev_done) { (void)hipEventDestroy(sl.ev_done); sl.ev_done = nullptr; }
    if (sl.st) { (void)hipStreamDestroy(sl.st); sl.st = nullptr; }
    return e;
}

// the slot's page-locked batch buffer made anew, `want` bytes (false: no memory, and the slot has no buffer)
bool slot_repin(DecSlot &sl, size_t want)
{
    if (sl.h_blob) { pin_free(sl.h_blob, sl.h_cap, sl.h_mapped); sl.h_blob = nullptr; sl.h_cap = 0; }
    if ((sl.h_blob = pin_alloc(want, &sl.h_mapped)) != nullptr) sl.h_cap = want;
    return sl.h_blob != nullptr;
}

// ---- pd_decode_begin's steps (the caller holds c->mu and has set the device) ----
// which contigs count and, with -b, which spans of them: the caller's arrays go up and have been read when this returns
int begin_filters(pd_ctx *c, const pd_decode_cfg *cfg)
{
    std::vector<uint8_t> on((size_t)c->n_contigs, 1);
    for (int32_t t = 0; t < c->n_contigs; ++t) on[(size_t)t] = cfg->contig_on ? (cfg->contig_on[t] != 0) : (c->len[(size_t)t] >= 2);
    if (!c->d_contig_on && hipMalloc(&c->d_contig_on, (size_t)c->n_contigs + 16) != hipSuccess) return fail(c, PD_ENOMEM, "pd_decode_begin: allocation failed");
    HIPOK(c, hipMemcpyAsync(c->d_contig_on, on.data(), on.size(), hipMemcpyHostToDevice, c->stream));
    if (c->d_span_off) { (void)hipFree(c->d_span_off); c->d_span_off = nullptr; }
    if (c->d_spans) { (void)hipFree(c->d_spans); c->d_spans = nullptr; }
    if (cfg->span_off && cfg->spans) {
        const size_t ns = cfg->span_off[c->n_contigs];
        if (hipMalloc(&c->d_span_off, ((size_t)c->n_contigs + 1) * 4) != hipSuccess || hipMalloc(&c->d_spans, ns * 8 + 16) != hipSuccess)
            return fail(c, PD_ENOMEM, "pd_decode_begin: allocation failed");
        HIPOK(c, hipMemcpyAsync(c->d_span_off, cfg->span_off, ((size_t)c->n_contigs + 1) * 4, hipMemcpyHostToDevice, c->stream));
        if (ns) HIPOK(c, hipMemcpyAsync(c->d_spans, cfg->spans, ns * 8, hipMemcpyHostToDevice, c->stream));
    }
    c->dec_cfg.contig_on = nullptr; c->dec_cfg.span_off = nullptr; c->dec_cfg.spans = nullptr;      // (the caller's arrays are not kept)
    HIPOK(c, hipStreamSynchronize(c->stream));                        // (the caller's arrays have been read)
    return PD_OK;
}

// PD_DECODE_RECORD_STATS: the session's sums and contig triples, zeroed (on c->stream, which begin_filters waits for)
int begin_record_stats(pd_ctx *c)
{
    c->rs_bins = c->dec_isize_bins;
    const size_t words = (size_t)PD_RECSTAT_FIXED + c->rs_bins + 1 + 3 * (size_t)c->n_contigs;
    if (words != c->recstat_words) {
        if (c->d_recstat) { (void)hipFree(c->d_recstat); c->d_recstat = nullptr; c->recstat_words = 0; }
        if (hipMalloc(&c->d_recstat, words * 8 + 64) != hipSuccess) { (void)hipGetLastError(); return fail(c, PD_ENOMEM, "pd_decode_begin: allocation failed"); }
        c->recstat_words = words;
    }
    HIPOK(c, hipMemsetAsync(c->d_recstat, 0, words * 8, c->stream));
    return PD_OK;
}

// PD_DECODE_ALN_STATS: the session's sums, zeroed (on c->stream, which begin_filters waits for)
int begin_aln_stats(pd_ctx *c)
{
    c->as_width = c->dec_len_bin_width;
    if (!c->d_alnstat && hipMalloc(&c->d_alnstat, (size_t)PD_ALNSTAT_WORDS * 8 + 64) != hipSuccess) { (void)hipGetLastError(); c->d_alnstat = nullptr; return fail(c, PD_ENOMEM, "pd_decode_begin: allocation failed"); }
    HIPOK(c, hipMemsetAsync(c->d_alnstat, 0, (size_t)PD_ALNSTAT_WORDS * 8, c->stream));
    return PD_OK;
}

// PD_DECODE_ROW_COUNTS: the table pd_decode_row_bins left becomes the session's — offsets and edges go up, the bins are zeroed (on c->stream,
// which begin_filters waits for; the host copies stay for the next session)
int begin_row_counts(pd_ctx *c)
{
    const size_t words = (size_t)c->rb_nbins * PD_ROWCOUNT_WORDS;
    const auto oom = [&]() { (void)hipGetLastError(); return fail(c, PD_ENOMEM, "pd_decode_begin: allocation failed"); };
    if (!c->d_rc_off && hipMalloc(&c->d_rc_off, ((size_t)c->n_contigs + 1) * 8 + 64) != hipSuccess) return oom();
    if (c->rb_edges.size() > c->rc_edges_cap) {
        if (c->d_rc_edges) { (void)hipFree(c->d_rc_edges); c->d_rc_edges = nullptr; c->rc_edges_cap = 0; }
        if (hipMalloc(&c->d_rc_edges, c->rb_edges.size() * 4 + 64) != hipSuccess) return oom();
        c->rc_edges_cap = c->rb_edges.size();
    }
    if (words != c->rowcnt_words) {
        if (c->d_rowcnt) { (void)hipFree(c->d_rowcnt); c->d_rowcnt = nullptr; c->rowcnt_words = 0; }
        if (hipMalloc(&c->d_rowcnt, words * 8 + 64) != hipSuccess) return oom();
        c->rowcnt_words = words;
    }
    c->rc_w = c->rb_w; c->rc_nbins = c->rb_nbins;
    HIPOK(c, hipMemcpyAsync(c->d_rc_off, c->rb_off.data(), c->rb_off.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (!c->rb_edges.empty()) HIPOK(c, hipMemcpyAsync(c->d_rc_edges, c->rb_edges.data(), c->rb_edges.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(c, hipMemsetAsync(c->d_rowcnt, 0, words * 8, c->stream));
    return PD_OK;
}

// A sorted file read for whole-contig statistics (PD_DECODE_COMPACT), its batches numbered 0 .. n_batches - 1: the batches' runs go
// straight to their final places in a compact sample (C8Dec).  Sized from the compressed bytes
// (>= 32 B of BGZF per record of a real file; denser files make it grow): a first run per record, a later run for every fourth.
// A session that cannot be one goes on with 12-byte runs per batch.  tb: pd_decode_begin's time marks.
int begin_compact(pd_ctx *c, const pd_decode_cfg *cfg, uint64_t *tb)
{
    std::lock_guard<std::mutex> l8(c->c8.mu);
    pd_ctx::C8Dec &x = c->c8;
    if (x.on || !x.batch.empty()) { (void)hipDeviceSynchronize(); c8_drop(c); }     // (a session that was never ended)
    x.on = false; x.n_s = x.n_o = x.turn = 0; x.n_batches = 0; x.err.clear();
    const uint64_t nb64 = (uint64_t)c->n_tiles << runs_bshift(c);
    // (any genome size: a compact run keeps the low 32 bits of its flat begin and every consumer works relative to a tile; what is bounded is
    // the number of runs — 32-bit indices — so a file that promises more than that many records keeps 12-byte runs per batch)
    if (!((cfg->flags & PD_DECODE_COMPACT) && cfg->n_batches && cfg->n_batches < (1ull << 31) && cfg->sorted && !cfg->spans && c->pend.empty() &&
          cfg->bytes_hint / 16 < DEV_BATCH_MAX && nb64 <= 0xFFFFFF00ull &&
          // (above 2^32 cells a compact session that outgrows its 32-bit run indices cannot fall back to 12-byte runs afterwards — pd_decode_end
          // would have to refuse a file already decoded — so there the caller must have said how large the file is; the executable always does)
          (c->n_cells < (1ull << 32) || cfg->bytes_hint != 0))) return PD_OK;
    x.bshift = runs_bshift(c);
    x.nbw = (size_t)nb64 + 2;
    if (x.b1) { (void)hipFree(x.b1); x.b1 = nullptr; }
    if (x.marks) { (void)hipFree(x.marks); x.marks = nullptr; }
    if (hipMalloc(&x.b1, c8_index_bytes(x.nbw, c->n_tiles)) != hipSuccess || hipMalloc(&x.marks, x.nbw * 8 + 8) != hipSuccess) { (void)hipGetLastError(); return fail(c, PD_ENOMEM, "pd_decode_begin: allocation failed"); }
    HIPOK(c, hipMemsetAsync(x.marks, 0xFF, x.nbw * 8, c->stream));
    HIPOK(c, hipMemsetAsync(x.wide(), 0, 8, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));                // (the batches' kernels run on other streams)
    if (!x.compose) HIPOK(c, hipStreamCreateWithFlags(&x.compose, hipStreamNonBlocking));
    tb[2] = tb[3] = dec_now_us();
    // (>= 32 B of BGZF per record of a real short-read file: a first run per record, a later run for every fourth; c8_reserve adds
    // half again when the sample has to GROW, not to this first estimate — a 70 GB file would otherwise ask for 50 GB up front.)
    uint64_t est = std::min<uint64_t>(cfg->bytes_hint ? cfg->bytes_hint / 32 + (1u << 20) : (uint64_t)8 << 20, DEV_BATCH_MAX);
    if (c->dec_c8_reserve) est = std::min<uint64_t>(est, c->dec_c8_reserve);
    const int rsv = c8_reserve(c, est, est / 4, /*exact=*/true);
    tb[3] = dec_now_us();
    if (rsv == PD_OK) {
        x.n_batches = cfg->n_batches;
        x.batch.assign((size_t)cfg->n_batches, pd_ctx::C8Dec::Batch());
        x.base_s.assign((size_t)cfg->n_batches, 0u);
        x.on = true;
    } else {
        // not enough memory for the compact sample's arrays: the session goes on with 12-byte runs per batch, as sessions without
        // PD_DECODE_COMPACT do (pd_decode_end then takes the general paths)
        (void)hipGetLastError();
        if (x.b1) { (void)hipFree(x.b1); x.b1 = nullptr; }
        if (x.marks) { (void)hipFree(x.marks); x.marks = nullptr; }
    }
    return PD_OK;
}

// one arena for the batches' run arrays (a hipMalloc per batch waits for the other streams): about half the compressed
// bytes is plenty for short reads (12 B per run against >= 30 B of BGZF per record); what does not fit is allocated singly
// (a compact session's segments are 8-byte first runs + 12-byte later runs: a third less)
// (round 6: a fifth in a compact session — 8 bytes per record and 12 per later run are 0.18 of a 53-bytes-per-record file — instead of a third: device
// memory a process HOLDS is wiped when it leaves, and the next process's large allocations wait for that: 1.0-1.8 s now and then in this very call when
// one run followed another within a second, tools/calls/r6_call27.sh)
void begin_arena(pd_ctx *c, const pd_decode_cfg *cfg)
{
    const size_t want = cfg->bytes_hint ? (size_t)(cfg->bytes_hint / (c->c8.on ? 5 : 2)) + ((size_t)16 << 20) : (size_t)256 << 20;
    if (c->arena_cap < want) {
        if (c->arena) { (void)hipFree(c->arena); c->arena = nullptr; c->arena_cap = 0; }
        if (hipMalloc(&c->arena, want) == hipSuccess) c->arena_cap = want; else (void)hipGetLastError();
    }
    c->arena_used = 0;
}

// "decode_warm" (measured and left off, tools/calls/r6_call26.sh): the first slots made ready by a helper thread, one after the other, while the caller
// goes on — a slot's page-locked buffer, its stream and events, and by a first, empty launch the stream's hardware queue (the runtime makes it when
// something is launched: 9 ms each, one after the other whoever asks); pd_decode_acquire hands a slot out when it is ready.  The first reader does
// start after 20 ms — and its kernels wait until the LAST queue is made: every queue the process makes stops the ones it has (first batches collected
// after 140-155 ms instead of 58-66 after a 50 ms pd_decode_begin).
void warm_slots(pd_ctx *c, uint32_t n_warm, size_t need, size_t want)
{
    (void)hipSetDevice(c->device);
    for (uint32_t k = 0; k < n_warm; ++k) {
        DecSlot &sl = c->dec[k];
        {
            DecTimer ta(1);
            if (sl.h_cap < need) { std::lock_guard<std::mutex> al(g_alloc_mu); (void)slot_repin(sl, want); }
        }
        // (dec_queue makes a stream that could not be made here and reports what cannot be made)
        if (!sl.st && slot_streams(sl) == hipSuccess && c->dec_warm_word) {
            (void)hipMemsetAsync(c->dec_warm_word, 0, 4, sl.st);      // the stream's first launch: its hardware queue is made now
            (void)hipStreamSynchronize(sl.st);
        }
        { std::lock_guard<std::mutex> l2(c->dec_mu); sl.warming = false; }
        c->dec_cv.notify_all();
    }
}

// the first batches_in_flight slots get their page-locked buffers here, or from the warm-up thread
void begin_slots(pd_ctx *c, const pd_decode_cfg *cfg)
{
    if (c->dec_warm.joinable()) c->dec_warm.join();
    if (!cfg->batch_bytes || !cfg->batches_in_flight) return;
    const size_t need = std::max<size_t>((size_t)cfg->batch_bytes + 128, (size_t)8 << 20);
    const size_t want = need + std::max<size_t>((size_t)1 << 20, need / 32);            // (room for the batch's tables behind its bytes: pd_decode_acquire)
    if (!c->dec_warm_on) {
        // the first buffers page-locked here, from ONE thread (six readers pinning at once took 75-100 ms EACH, 5-8 ms alone)
        DecTimer ta(1);
        uint32_t k = 0;
        for (auto &sl : c->dec) {
            if (k++ >= cfg->batches_in_flight) break;
            if (sl.h_cap < need) (void)slot_repin(sl, want);
        }
        return;
    }
    uint32_t n_warm = 0;
    {
        std::lock_guard<std::mutex> l2(c->dec_mu);
        for (auto &sl : c->dec) { if (n_warm >= cfg->batches_in_flight) break; sl.warming = true; ++n_warm; }
    }
    if (!c->dec_warm_word && hipMalloc(&c->dec_warm_word, 256) != hipSuccess) { (void)hipGetLastError(); c->dec_warm_word = nullptr; }
    c->dec_warm = std::thread(warm_slots, c, n_warm, need, want);
}

} // namespace

extern "C" {

int pd_decode_begin(pd_ctx *c, const pd_decode_cfg *cfg)
{
    if (!c || !cfg) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_decode_begin")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    const uint64_t tb0 = dec_now_us(); uint64_t tb[6] = {tb0, tb0, tb0, tb0, tb0, tb0};
    struct BeginMarks { const uint64_t *t; ~BeginMarks() { if (getenv("PANDEPTH_TIMING") && t[5] - t[0] > 20000) fprintf(stderr, "[timing]   pd_decode_begin: tables %.3f s, marks + compose stream %.3f s, sample arrays %.3f s, arena %.3f s, buffers %.3f s\n", (t[1] - t[0]) / 1e6, (t[2] - t[1]) / 1e6, (t[3] - t[2]) / 1e6, (t[4] - t[3]) / 1e6, (t[5] - t[4]) / 1e6); } } begin_marks{tb};
    if ((cfg->flags & PD_DECODE_RECORD_STATS) && !c->dec_isize_bins)      // (refused before anything of the context changes)
        return fail(c, PD_EINVAL, "pd_decode_begin: PD_DECODE_RECORD_STATS needs pd_set_param(\"decode_isize_bins\", N) with 1 <= N <= 65536 first");
    if ((cfg->flags & PD_DECODE_ALN_STATS) && !c->dec_len_bin_width)
        return fail(c, PD_EINVAL, "pd_decode_begin: PD_DECODE_ALN_STATS needs pd_set_param(\"decode_len_bin_width\", W) with 1 <= W <= 65536 first");
    if ((cfg->flags & PD_DECODE_ROW_COUNTS) && !c->rb_set)
        return fail(c, PD_EINVAL, "pd_decode_begin: PD_DECODE_ROW_COUNTS needs a bin table: call pd_decode_row_bins first");
    c->dec_cfg = *cfg;
    c->dec_frag_bound = c->dec_frag_max ? c->dec_frag_max : 0x7FFFFFFFu;      // ("decode_frag_max" as it stands now holds for the whole session; 0: no bound)
    c->rs_ready = false; c->rs_launches = 0; c->rs_ns = 0;
    if (cfg->flags & PD_DECODE_RECORD_STATS) if (int rc = begin_record_stats(c)) return rc;
    c->rc_ready = false; c->rc_launches = 0; c->rc_ns = 0;
    if (cfg->flags & PD_DECODE_ROW_COUNTS) if (int rc = begin_row_counts(c)) return rc;
    c->as_ready = false; c->as_launches = 0; c->as_ns = 0;
    if (cfg->flags & PD_DECODE_ALN_STATS) if (int rc = begin_aln_stats(c)) return rc;
    if (int rc = begin_filters(c, cfg)) return rc;
    tb[1] = tb[2] = tb[3] = dec_now_us();
    if (int rc = begin_compact(c, cfg, tb)) return rc;
    begin_arena(c, cfg);
    tb[4] = tb[5] = dec_now_us();
    c->dec_n_fast = 0; c->dec_n_slow = 0; c->dec_n_redo = 0;
    for (auto &n : c->dec_n) n = 0;
    for (auto &g : g_dec_us) g = 0;
    begin_slots(c, cfg);
    tb[5] = dec_now_us();
    c->dec_open = true;
    return PD_OK;
}

int pd_decode_acquire(pd_ctx *c, size_t bytes, void **host_buf)
{
    if (!c || !host_buf) return PD_EINVAL;
    *host_buf = nullptr;
    std::unique_lock<std::mutex> lk(c->dec_mu);
    if (!c->dec_open) return dec_fail(c, PD_ESTATE, "pd_decode_acquire: call pd_decode_begin first");
    DecSlot *sl = nullptr;
    { DecTimer tw(0); c->dec_cv.wait(lk, [&] { for (auto &x : c->dec) if (!x.busy && !x.warming) { sl = &x; return true; } return false; }); }
    sl->busy = true;
    lk.unlock();
    const auto give_back = [&](int code, const char *msg) {
        { std::lock_guard<std::mutex> l2(c->dec_mu); sl->busy = false; }
        c->dec_cv.notify_one();
        return dec_fail(c, code, msg);
    };
    {
        DecTimer tsd(7);
        if (hipSetDevice(c->device) != hipSuccess) return give_back(PD_EHIP, "hipSetDevice failed");
    }
    DecTimer ta(1);
    if (bytes + 64 > sl->h_cap) {
        // (room behind the caller's bytes for the batch's small tables, which then travel with them in ONE copy: dec_queue)
        const size_t want = std::max<size_t>(bytes + 64, (size_t)8 << 20) + std::max<size_t>((size_t)1 << 20, bytes / 32);
        // one allocation at a time: six feeders pinning their first buffers at once took 75-100 ms EACH (4-5 ms alone)
        std::lock_guard<std::mutex> al(g_alloc_mu);
        if (!slot_repin(*sl, want)) return give_back(PD_ENOMEM, "pinned batch buffer allocation failed");
    }
    *host_buf = sl->h_blob;
    return PD_OK;
}

} // extern "C"

namespace {

// ---- first half: everything the batch needs is put on the slot's stream; nothing is waited for -------------------------------------
// The batch is checked and its units are cut into segments (host only; J.units and J.blocks hold the caller's tables).  *guess: a unit
// begins at a guessed record start.
int dec_cut(pd_ctx *c, Job &J, const pd_decode_batch *bt, bool *guess)
{
    std::vector<pdb2::Seg> &segs = J.segs;
    J.seg0.assign(bt->n_units + 1, 0);
    for (uint32_t u = 0; u < bt->n_units; ++u) {
        const pd_decode_unit &un = J.units[u];
        if (un.start > un.stop || un.start > un.avail || un.avail > bt->inflated_bytes || (uint64_t)un.first_block + un.n_blocks > bt->n_blocks)
            return dec_fail(c, PD_EINVAL, "pd_decode_submit: unit outside the inflated buffer");
        if (un.flags & PD_UNIT_GUESS) { *guess = true; ++c->dec_n[pd_ctx::DN_GUESS]; }
        J.seg0[u] = (uint32_t)segs.size();
        for (uint64_t b = un.start; b < un.stop; b += pdb2::SEG_BYTES) {
            pdb2::Seg sg; memset(&sg, 0, sizeof sg);
            sg.begin = b; sg.end = std::min<uint64_t>(b + pdb2::SEG_BYTES, un.stop); sg.avail = un.avail;
            sg.unit_first = b == un.start;
            sg.hint = (b == un.start && !(un.flags & PD_UNIT_GUESS)) ? un.start : pdb2::NONE;
            segs.push_back(sg);
        }
    }
    J.seg0[bt->n_units] = (uint32_t)segs.size();
    for (uint32_t b = 0; b < bt->n_blocks; ++b)
        if (J.blocks[b].in_off + J.blocks[b].in_len + 8 > bt->n_bytes + 8 || J.blocks[b].out_off + J.blocks[b].out_len > bt->inflated_bytes)
            return dec_fail(c, PD_EINVAL, "pd_decode_submit: block outside its buffer");
    J.n_seg = (uint32_t)segs.size();
    return PD_OK;
}

// The batch's small tables travel through a page-locked staging area of the slot — an "asynchronous" copy from or to pageable memory
// is staged by the runtime on the calling thread, under a lock all streams share — and since round 5 as ONE copy each way: members,
// segments and the (zeroed) member counter go up together into one device buffer laid out the same way; ChainOut + the segments'
// keys (or, on the host's path, the member statuses and the segments) come back together.  -> the bytes of the staging area
size_t dec_lay_tables(Job::Tabs &o, size_t n_blocks, size_t n_seg)
{
    const auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    o.blk = 0; o.seg = o.blk + al(n_blocks * sizeof(pd_bgzf_block)); o.next = o.seg + al(n_seg * sizeof(pdb2::Seg)); o.up = o.next + 256;
    o.bst = o.up; o.co = o.bst + al(n_blocks * 4); o.so = o.co + sizeof(pdb2::ChainOut);
    o.ord = o.so + al(n_seg * sizeof(pdb2::SegOut));
    return o.ord + 256;
}

// the slot's device buffers, wave scratch and staging area are made large enough for the batch (blob_bytes: the members, with the tables where they ride along)
int dec_size_slot(pd_ctx *c, DecSlot &sl, const pd_decode_batch *bt, size_t blob_bytes, size_t small_need, unsigned n_wg)
{
    const Job &J = sl.job;
    const uint32_t n_seg = J.n_seg;
    int rc;
    if ((rc = dec_ensure(c, sl, DS_BLOB, blob_bytes)) || (rc = dec_ensure(c, sl, DS_INF, (size_t)bt->inflated_bytes + 256)) ||
        (rc = dec_ensure(c, sl, DS_BLK, J.o.up)) || (rc = dec_ensure(c, sl, DS_ST, (size_t)bt->n_blocks * 4 + 16)) ||
        (rc = dec_ensure(c, sl, DS_LANE, (size_t)n_seg * 64 * sizeof(pdb2::LaneOut))) ||
        (rc = dec_ensure(c, sl, DS_ONLY, (size_t)n_seg * 4 + 16)) || ((J.c8 || J.fast) && (rc = dec_ensure(c, sl, DS_SEGOUT, sizeof(pdb2::ChainOut) + (size_t)n_seg * sizeof(pdb2::SegOut)))) ||
        (J.fast && ((rc = dec_ensure(c, sl, DS_R8, J.c8 ? c8_seg_bytes(J.cap_first) : (size_t)J.cap_first * sizeof(pd_iv))) || (rc = dec_ensure(c, sl, DS_OTH, (size_t)J.cap_other * sizeof(pd_iv)))))) return rc;
    if (!sl.d_tok || sl.tok_wg < n_wg) {
        // (the scratch is indexed by workgroup: "inflate_waves" may have been raised since it was sized)
        std::lock_guard<std::mutex> al2(g_alloc_mu);
        if (sl.d_tok) { HIPDEC(hipStreamSynchronize(sl.st)); HIPDEC(hipFree(sl.d_tok)); sl.d_tok = nullptr; sl.tok_wg = 0; }
        if (hipMalloc(&sl.d_tok, bgzf_wave_scratch_bytes(n_wg)) != hipSuccess) { (void)hipGetLastError(); return dec_fail(c, PD_ENOMEM, "device-decode scratch allocation failed"); }
        sl.tok_wg = n_wg;
    }
    if (small_need > sl.h_small_cap) {
        std::lock_guard<std::mutex> al2(g_alloc_mu);
        if (sl.h_small) { HIPDEC(hipStreamSynchronize(sl.st)); (void)hipHostFree(sl.h_small); sl.h_small = nullptr; sl.h_small_cap = 0; }
        const size_t want = small_need + small_need / 4 + 4096;
        if (hipHostMalloc((void **)&sl.h_small, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return dec_fail(c, PD_ENOMEM, "pinned staging allocation failed"); }
        sl.h_small_cap = want;
    }
    return PD_OK;
}

// From the upload on the device may be reading the caller's buffer and the slot's staging area: a dec_queue that fails half way — in the
// upload or in the launches behind it — waits for what it has queued before the slot goes back.
struct Settle { hipStream_t st; bool armed = true; ~Settle() { if (armed) (void)hipStreamSynchronize(st); } };

// The batch's members and tables go up ("decode_h2d_fifo", "decode_h2d_lanes", "decode_h2d_kernel").  one_copy: the tables lie behind the
// members in the caller's buffer, at tab_at.  -> where the inflate kernel finds the members
// ("decode_h2d_kernel": the copy engine's transfer and the kernel behind it are ordered by a signal between two engines — 2.2 ms of idle queue per
// batch in profiles/r05_decode_timeline.txt; a copy kernel reads the pinned bytes over the link itself and the inflate kernel follows it in the same queue)
// (3: no copy at all — the inflate kernel reads the members straight out of the pinned buffer, which the slot holds until the batch is collected)
int dec_upload(pd_ctx *c, DecSlot &sl, const pd_decode_batch *bt, bool one_copy, size_t tab_at, const uint8_t **members)
{
    Job &J = sl.job;
    hipStream_t st = sl.st;
    uint8_t *const pin = sl.h_small, *const d_blob = (uint8_t *)sl.d[DS_BLOB], *const d_tab = J.d_tab;
    *members = d_blob;
    memset((uint8_t *)bt->host_buf + bt->n_bytes, 0, 64);                  // (the decoder reads up to 8 bytes past a member's end)
    uint8_t *const up = one_copy ? (uint8_t *)bt->host_buf + tab_at : pin;    // where the tables are put together
    memcpy(up + J.o.blk, J.blocks.data(), (size_t)bt->n_blocks * sizeof(pd_bgzf_block));
    memcpy(up + J.o.seg, J.segs.data(), (size_t)J.n_seg * sizeof(pdb2::Seg));
    memset(up + J.o.next, 0, 256);
    if (c->dec_h2d_kernel == 0 && c->dec_h2d_fifo) {
        // ONE batch's bytes on the link at a time, in the order the batches were queued (round 6).  Copies issued on the batches' own streams share the
        // link: six readers that happen to queue together get their bytes together, six times later than the first of them could have had them, their
        // kernels then share the GPU and finish together, and the readers come back together — a convoy in which reading, copying and decoding take
        // turns instead of overlapping (tools/feeder_trace.py, profiles/r06_feeder_trace.txt: 1.25-1.35 ms per batch whatever the readers x buffers).
        // First come, first served, the first batch decodes while the second is on the link.  The copies ride on the context's main stream, which has
        // nothing else to do while a file is decoded (a stream of their own would be one more hardware queue to make: 10 ms).
        std::lock_guard<std::mutex> lk(c->dec_copy_mu);
        hipStream_t cs = c->stream;
        if (c->dec_h2d_lanes > 1 && (c->dec_copy_seq++ & 1)) {
            if (!c->dec_copy_st2) HIPDEC(hipStreamCreateWithFlags(&c->dec_copy_st2, hipStreamNonBlocking));
            cs = c->dec_copy_st2;
        }
        if (J.timed) HIPDEC(hipEventRecord(sl.ev[0], cs));
        if (one_copy) HIPDEC(hipMemcpyAsync(d_blob, bt->host_buf, tab_at + J.o.up, hipMemcpyHostToDevice, cs));
        else {
            HIPDEC(hipMemcpyAsync(d_tab, pin, J.o.up, hipMemcpyHostToDevice, cs));
            HIPDEC(hipMemcpyAsync(d_blob, bt->host_buf, bt->n_bytes + 64, hipMemcpyHostToDevice, cs));
        }
        if (J.timed) HIPDEC(hipEventRecord(sl.ev[1], cs));
        HIPDEC(hipEventRecord(sl.ev[5], cs));
        HIPDEC(hipStreamWaitEvent(st, sl.ev[5], 0));
    } else {
        if (J.timed) HIPDEC(hipEventRecord(sl.ev[0], st));
        if (c->dec_h2d_kernel == 3) *members = (const uint8_t *)bt->host_buf;
        else if (c->dec_h2d_kernel) launch_copy_words(st, d_blob, bt->host_buf, (bt->n_bytes + 64 + 3) / 4);
        else HIPDEC(hipMemcpyAsync(d_blob, bt->host_buf, bt->n_bytes + 64, hipMemcpyHostToDevice, st));
        if (c->dec_h2d_kernel >= 2) launch_copy_words(st, d_tab, pin, (J.o.up + 3) / 4);
        else HIPDEC(hipMemcpyAsync(d_tab, pin, J.o.up, hipMemcpyHostToDevice, st));
        if (J.timed) HIPDEC(hipEventRecord(sl.ev[1], st));
    }
    return PD_OK;
}

// The records' statistics of the batch's counted segments (sessions with PD_DECODE_RECORD_STATS), on the slot's stream behind the emission.  gate:
// the chain kernel's verdict on the device (a batch it leaves to the host counts nothing here), or null behind the host's chain check.
int dec_record_stats(pd_ctx *c, DecSlot &sl, const pdb2::Seg *d_seg, const pdb2::ChainOut *gate)
{
    Job &J = sl.job;
    if (J.timed) {
        for (auto &e : sl.ev_rs) if (!e) HIPDEC(hipEventCreate(&e));
        HIPDEC(hipEventRecord(sl.ev_rs[0], sl.st));
    }
    launch_record_stats(sl.st, J.cfg, d_seg, J.n_seg, (const pdb2::LaneOut *)sl.d[DS_LANE], c->rs_bins, c->d_recstat, c->d_recstat + PD_RECSTAT_FIXED + c->rs_bins + 1, gate);
    if (J.timed) { HIPDEC(hipEventRecord(sl.ev_rs[1], sl.st)); J.rs_timed = true; }
    if (!gate) ++c->rs_launches;                                          // (a gated launch counts once its batch is known to be confirmed: dec_collect)
    return PD_OK;
}

// ... and its time, once the stream has been waited for
void dec_record_stats_time(pd_ctx *c, DecSlot &sl)
{
    if (!sl.job.rs_timed) return;
    sl.job.rs_timed = false;
    float ms = 0;
    if (hipEventElapsedTime(&ms, sl.ev_rs[0], sl.ev_rs[1]) == hipSuccess) c->rs_ns += (uint64_t)((double)ms * 1e6);
}

// The records per row of the batch's counted segments (sessions with PD_DECODE_ROW_COUNTS), at the same two places and with the same gate as
// dec_record_stats (and behind it, where a session carries both flags)
int dec_row_counts(pd_ctx *c, DecSlot &sl, const pdb2::Seg *d_seg, const pdb2::ChainOut *gate)
{
    Job &J = sl.job;
    if (J.timed) {
        for (auto &e : sl.ev_rc) if (!e) HIPDEC(hipEventCreate(&e));
        HIPDEC(hipEventRecord(sl.ev_rc[0], sl.st));
    }
    const pdrc::Bins bins{c->rc_w, c->d_rc_off, c->d_rc_edges, c->rc_nbins};
    launch_row_counts(sl.st, J.cfg, d_seg, J.n_seg, (const pdb2::LaneOut *)sl.d[DS_LANE], bins, c->d_rowcnt, gate);
    if (J.timed) { HIPDEC(hipEventRecord(sl.ev_rc[1], sl.st)); J.rc_timed = true; }
    if (!gate) ++c->rc_launches;                                          // (a gated launch counts once its batch is known to be confirmed: dec_collect)
    return PD_OK;
}

void dec_row_counts_time(pd_ctx *c, DecSlot &sl)
{
    if (!sl.job.rc_timed) return;
    sl.job.rc_timed = false;
    float ms = 0;
    if (hipEventElapsedTime(&ms, sl.ev_rc[0], sl.ev_rc[1]) == hipSuccess) c->rc_ns += (uint64_t)((double)ms * 1e6);
}

// The CIGAR operations and read lengths of the batch's counted segments (sessions with PD_DECODE_ALN_STATS), at the same two places and with the
// same gate as dec_record_stats (and behind the other two, where a session carries several of the flags)
int dec_aln_stats(pd_ctx *c, DecSlot &sl, const pdb2::Seg *d_seg, const pdb2::ChainOut *gate)
{
    Job &J = sl.job;
    if (J.timed) {
        for (auto &e : sl.ev_as) if (!e) HIPDEC(hipEventCreate(&e));
        HIPDEC(hipEventRecord(sl.ev_as[0], sl.st));
    }
    launch_aln_stats(sl.st, J.cfg, d_seg, J.n_seg, (const pdb2::LaneOut *)sl.d[DS_LANE], c->as_width, c->d_alnstat, gate);
    if (J.timed) { HIPDEC(hipEventRecord(sl.ev_as[1], sl.st)); J.as_timed = true; }
    if (!gate) ++c->as_launches;                                          // (a gated launch counts once its batch is known to be confirmed: dec_collect)
    return PD_OK;
}

void dec_aln_stats_time(pd_ctx *c, DecSlot &sl)
{
    if (!sl.job.as_timed) return;
    sl.job.as_timed = false;
    float ms = 0;
    if (hipEventElapsedTime(&ms, sl.ev_as[0], sl.ev_as[1]) == hipSuccess) c->as_ns += (uint64_t)((double)ms * 1e6);
}

// Inflate, pass 1 and — where the device confirms the record chain itself — the chain and the emission; otherwise the member statuses and
// the segments come back for the host's chain check.  *t_inflate (PANDEPTH_DEVTRACE): when the inflate kernel had been launched.
int dec_launch(pd_ctx *c, DecSlot &sl, const pd_decode_batch *bt, const uint8_t *members, unsigned n_wg, uint64_t *t_inflate)
{
    Job &J = sl.job;
    hipStream_t st = sl.st;
    const bool c8 = J.c8;
    const uint32_t n_seg = J.n_seg;
    uint8_t *const pin = sl.h_small, *const d_inf = (uint8_t *)sl.d[DS_INF], *const d_tab = J.d_tab;
    pdb2::Seg *d_seg = (pdb2::Seg *)(d_tab + J.o.seg);
    pdb2::LaneOut *d_lane = (pdb2::LaneOut *)sl.d[DS_LANE];
    pdb2::Cfg &cfg = J.cfg;
    cfg = pdb2::Cfg{};
    cfg.buf = d_inf; cfg.avail = bt->inflated_bytes; cfg.n_ref = c->n_contigs; cfg.contig_len = c->d_len; cfg.contig_on = c->d_contig_on;
    cfg.flag_mask = c->dec_cfg.flag_mask; cfg.min_mapq = c->dec_cfg.min_mapq; cfg.span_off = c->d_span_off; cfg.spans = c->d_spans;
    cfg.near_span = c8 ? 0xFFFFFFFFu : c->dec_near_span;                   // (a compact session has one stream of later runs)
    cfg.count_del = c->dec_cfg.flags & PD_DECODE_DELETIONS ? 1u : 0u;      // (`-del`: every launch of this batch takes the kernels of the group rule)
    cfg.fragments = c->dec_cfg.flags & PD_DECODE_FRAGMENTS ? 1u : 0u;      // (`-frag`: ... the kernels that class every kept record by its mate fields)
    cfg.frag_max = c->dec_frag_bound;
    cfg.c8 = pdb2::C8Out{};
    launch_bgzf_inflate_wave(st, members, (const pd_bgzf_block *)(d_tab + J.o.blk), bt->n_blocks, d_inf, (int *)sl.d[DS_ST], sl.d_tok, n_wg, c->dec_crc,
                             (uint32_t *)(d_tab + J.o.next), false);
    if (g_dec_devtrace) *t_inflate = dec_now_us();
    if (J.timed) HIPDEC(hipEventRecord(sl.ev[2], st));
    launch_walk_segments(st, cfg, d_seg, n_seg, d_lane, nullptr, 0);
    if (c->dec_spoil) launch_spoil_segments(st, cfg, d_seg, n_seg, d_lane, c->dec_spoil);     // (test hook)
    if (J.fast) {
        pd_ctx::C8Dec &x = c->c8;
        pdb2::ChainOut *d_co = (pdb2::ChainOut *)sl.d[DS_SEGOUT];
        launch_chain_segments(st, cfg, d_seg, n_seg, d_lane, (const int *)sl.d[DS_ST], bt->n_blocks, J.cap_first, J.cap_other, c->dec_max_redo, d_co);
        if (J.timed) HIPDEC(hipEventRecord(sl.ev[3], st));
        pdb2::Cfg c2 = cfg;
        if (c8) c2.c8 = pdb2::C8Out{nullptr, x.marks, c->d_off, 13u - x.bshift, (pdb2::SegOut *)(d_co + 1), (uint32_t)bt->order,
                                    (uint32_t *)sl.d[DS_R8], (uint32_t *)sl.d[DS_R8] + c8_plane_words((size_t)J.cap_first)};      // (the slot's array as two planes of cap_first words)
        else { c2.c8 = pdb2::C8Out{}; c2.c8.seg_out = (pdb2::SegOut *)(d_co + 1); }      // (12-byte runs; the order keys ride along)
        launch_emit_segments(st, c2, d_seg, n_seg, d_lane, c8 ? nullptr : (pd_iv *)sl.d[DS_R8], (pd_iv *)sl.d[DS_OTH], nullptr, d_co);
        HIPDEC(hipMemcpyAsync(pin + J.o.co, d_co, sizeof(pdb2::ChainOut) + (size_t)n_seg * sizeof(pdb2::SegOut), hipMemcpyDeviceToHost, st));
        if (J.timed) HIPDEC(hipEventRecord(sl.ev[4], st));
        if (c->dec_cfg.flags & PD_DECODE_RECORD_STATS) if (int rc = dec_record_stats(c, sl, d_seg, d_co)) return rc;
        if (c->dec_cfg.flags & PD_DECODE_ROW_COUNTS) if (int rc = dec_row_counts(c, sl, d_seg, d_co)) return rc;
        if (c->dec_cfg.flags & PD_DECODE_ALN_STATS) if (int rc = dec_aln_stats(c, sl, d_seg, d_co)) return rc;
    } else {
        HIPDEC(hipMemcpyAsync(pin + J.o.bst, sl.d[DS_ST], (size_t)bt->n_blocks * 4, hipMemcpyDeviceToHost, st));
        HIPDEC(hipMemcpyAsync(pin + J.o.seg, d_seg, (size_t)n_seg * sizeof(pdb2::Seg), hipMemcpyDeviceToHost, st));
        if (J.timed) HIPDEC(hipEventRecord(sl.ev[3], st));
    }
    return PD_OK;
}

int dec_queue(pd_ctx *c, DecSlot &sl, const pd_decode_batch *bt)
{
    Job &J = sl.job;                                                  // (claimed by dec_slot_of: J.open is set)
    J.queued = false; J.fast = false; J.timed = false; J.segs_sent = false; J.rs_timed = false; J.rc_timed = false; J.as_timed = false; J.t_q0 = dec_now_us(); J.order = bt->order; J.n_bytes = bt->n_bytes; J.inflated = bt->inflated_bytes; J.n_seg = 0;
    J.blocks.clear(); J.units.clear(); J.segs.clear(); J.seg0.clear();
    const bool c8 = J.c8 = c->c8.on;
    J.owes_count = c8 && bt->order < c->c8.n_batches;
    C8Owes owes{c, &J};
    if (c8 && bt->order >= c->c8.n_batches && bt->n_units) return dec_fail(c, PD_EINVAL, "pd_decode_submit: batch order outside [0, n_batches) of this session");
    if (!bt->n_units || !bt->n_blocks) return PD_OK;                  // (nothing to decode: the order is counted, empty)
    if (!bt->units || !bt->blocks) return dec_fail(c, PD_EINVAL, "pd_decode_submit: a batch with units needs its unit and member tables");
    if (bt->n_bytes + 64 > sl.h_cap) return dec_fail(c, PD_EINVAL, "pd_decode_submit: more bytes than were acquired");
    HIPDEC(hipSetDevice(c->device));
    uint64_t dq[6] = {};                                               // (PANDEPTH_DEVTRACE: where the call's own time goes, first batches)
    const auto dq_mark = [&](int k) { if (g_dec_devtrace) dq[k] = dec_now_us(); };
    dq_mark(0);
    if (!sl.st) HIPDEC(slot_streams(sl));
    J.units.assign(bt->units, bt->units + bt->n_units);
    J.blocks.assign(bt->blocks, bt->blocks + bt->n_blocks);
    bool guess = false;
    if (int rc = dec_cut(c, J, bt, &guess)) return rc;
    if (!J.n_seg) return PD_OK;
    // The device confirms the record chain itself — no host round trip between the two passes — in sessions whose units all start at
    // known records (index cuts and index chunks: everything but no-index streams).  A kept read has at least one CIGAR operation, so its record is at least 41 bytes (4 + 32 fixed, a name of
    // one byte, one operation): inflated / 41 first runs is a bound, not an estimate.  Later runs are bounded only by the CIGAR bytes;
    // the same number of slots (several times what real reads need) is given and the chain kernel checks that they suffice.
    J.fast = c->dec_fast && !guess && (c8 || c->dec_near_span == 0xFFFFFFFFu);      // (every session whose units start at known records and whose later runs are one stream)
    J.cap_first = J.fast ? bt->inflated_bytes / 41 + 64 : 0;
    J.cap_other = J.fast ? bt->inflated_bytes / c->dec_oth_div.load() + 64 : 0;
    // (the inflate kernel's LDS lets 20 one-wave workgroups share a CU; "inflate_waves": fewer per launch, so that several batches' launches share the GPU)
    const unsigned n_wg = (unsigned)c->n_cu * c->dec_waves;
    dq_mark(1);
    J.t_mark = dec_now_us();
    const size_t small_need = dec_lay_tables(J.o, bt->n_blocks, J.n_seg);
    // the tables behind the members in the caller's (page-locked) buffer when it has the room: one host-to-device copy per batch instead of two
    const size_t tab_at = (bt->n_bytes + 64 + 255) & ~(size_t)255;
    const bool one_copy = c->dec_h2d_kernel == 0 && c->dec_h2d_fifo && tab_at + J.o.up <= sl.h_cap;
    if (int rc = dec_size_slot(c, sl, bt, one_copy ? tab_at + J.o.up : bt->n_bytes + 64, small_need, n_wg)) return rc;
    dec_lap(J, 2);                                                        // device buffers
    dq_mark(2);
    J.d_tab = one_copy ? (uint8_t *)sl.d[DS_BLOB] + tab_at : (uint8_t *)sl.d[DS_BLK];
    J.timed = g_dec_timing;
    Settle settle{sl.st};
    const uint8_t *members = nullptr;
    if (int rc = dec_upload(c, sl, bt, one_copy, tab_at, &members)) return rc;
    dq_mark(3);
    if (int rc = dec_launch(c, sl, bt, members, n_wg, &dq[4])) return rc;
    // (what the collecting call waits for.  hipStreamSynchronize would put a marker of its own into the stream's HARDWARE queue at the time of the call — and
    // the process's streams share eight of those: the marker landed behind whatever another batch's stream had in the same queue, and a batch that had long
    // finished was "collected" 2 ms later, when the other batch was through: tools/calls/r6_call14.sh, profiles/r06_devtrace.txt)
    HIPDEC(hipEventRecord(sl.ev_done, sl.st));
    HIPDEC(hipGetLastError());
    dq_mark(5);
    if (g_dec_devtrace && bt->order < 14)
        fprintf(stderr, "[devtrace] batch %llu pd_decode_queue: stream + events + segments %llu us, buffers %llu, copies issued %llu, inflate launched %llu, the rest launched %llu\n", (unsigned long long)bt->order,
                (unsigned long long)(dq[1] - dq[0]), (unsigned long long)(dq[2] - dq[1]), (unsigned long long)(dq[3] - dq[2]), (unsigned long long)(dq[4] - dq[3]), (unsigned long long)(dq[5] - dq[4]));
    J.queued = true; J.t_q1 = dec_now_us();
    owes.armed = false;                                                   // (the second half counts the order)
    settle.armed = false;
    return PD_OK;
}

// ---- second half: wait for the batch, finish it, report what pd_decode_submit reports ------------------------------------------------
int dec_wait(pd_ctx *c, DecSlot &sl)
{
    Job &J = sl.job;
    if (g_dec_devtrace && J.timed) {
        uint64_t t[6] = {};
        for (int k = 0; k < 5; ++k) { if (k < 4 || J.fast) (void)hipEventSynchronize(sl.ev[k]); t[k] = dec_now_us(); }
        (void)hipEventSynchronize(sl.ev_done); t[5] = dec_now_us();
        fprintf(stderr, "[devtrace] batch %llu queue call %llu us; since its start: collect entered %llu, copy begun %llu, copied %llu, inflated %llu, walked %llu, emitted %llu, stream idle %llu\n",
                (unsigned long long)J.order, (unsigned long long)(J.t_q1 - J.t_q0), (unsigned long long)(J.t_mark - J.t_q0), (unsigned long long)(t[0] - J.t_q0), (unsigned long long)(t[1] - J.t_q0),
                (unsigned long long)(t[2] - J.t_q0), (unsigned long long)(t[3] - J.t_q0), (unsigned long long)(t[4] - J.t_q0), (unsigned long long)(t[5] - J.t_q0));
    }
    HIPDEC(c->dec_sync_event ? hipEventSynchronize(sl.ev_done) : hipStreamSynchronize(sl.st));
    HIPDEC(hipGetLastError());
    dec_lap(J, 3);                                                        // waiting for the device
    return PD_OK;
}

// the batch's stages as its events timed them (PANDEPTH_TIMING)
void dec_times(const DecSlot &sl, pd_decode_result *res, bool emitted)
{
    if (!res || !sl.job.timed) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, sl.ev[0], sl.ev[1]) == hipSuccess) res->ms_h2d = ms;
    if (hipEventElapsedTime(&ms, sl.ev[1], sl.ev[2]) == hipSuccess) res->ms_inflate = ms;
    if (hipEventElapsedTime(&ms, sl.ev[2], sl.ev[3]) == hipSuccess) res->ms_walk = ms;
    if (emitted && hipEventElapsedTime(&ms, sl.ev[3], sl.ev[4]) == hipSuccess) res->ms_emit = ms;
}

// the order of a batch's first runs across its segments, from the keys the emission left (inside a lane and across the lanes of a segment the emission checked it)
void order_of(const pdb2::SegOut *so, uint32_t n_seg, RunSeg *rs)
{
    uint64_t prev = 0, first = pdb2::NONE, n_long = 0; uint32_t bad = 0;
    for (uint32_t j = 0; j < n_seg; ++j) {
        bad |= so[j].unsorted; n_long += so[j].n_long;
        if (so[j].first_key == pdb2::NONE) continue;
        if (first == pdb2::NONE) first = so[j].first_key; else if (so[j].first_key < prev) bad = 1;
        prev = so[j].last_key;
    }
    rs->unsorted = bad ? 1u : 0u; rs->first_key = first; rs->last_key = prev; rs->n_long = n_long;
}

// The device has confirmed the chain and written the runs to the slot's arrays: exact arrays for them, copied behind the emission on this
// stream (the slot's arrays are free again when its next batch gets there), and the batch is counted.  12-byte runs (every mode that
// needs the arrays) go to arrays from the arena and the batch is listed for pd_decode_end; a compact session's go to its segments.
int collect_confirmed(pd_ctx *c, DecSlot &sl, const pdb2::ChainOut &co, pd_decode_result *res)
{
    Job &J = sl.job;
    ++c->dec_n_fast;
    const uint64_t nf = co.n_first, no = co.n_other;
    RunSeg rs{J.order, nullptr, nf, nullptr, no, nullptr, 0, co.max_span, 0u, 0ull, 0ull};
    Owned own{c};
    const auto copy_out = [&](void *first, size_t run_bytes, void *other) -> int {
        if (nf && J.c8) launch_copy_planes(sl.st, (uint32_t *)first, (uint32_t *)first + c8_plane_words((size_t)nf), (const uint32_t *)sl.d[DS_R8],
                                           (const uint32_t *)sl.d[DS_R8] + c8_plane_words((size_t)J.cap_first), nf);      // both planes, one launch
        else if (nf) launch_copy_words(sl.st, first, sl.d[DS_R8], nf * (run_bytes / 4));
        if (no) launch_copy_words(sl.st, other, sl.d[DS_OTH], no * (sizeof(pd_iv) / 4));
        HIPDEC(hipGetLastError());                                   // (pd_decode_end waits for the slots' streams before it reads these arrays)
        return PD_OK;
    };
    if (J.c8) {
        if (int rc = c8_hand_over(c, sl, nf, no, [&](uint32_t *seg_s, pd_iv *seg_o) { return copy_out(seg_s, sizeof(Run8), seg_o); })) return rc;
    } else if (nf + no) {
        if ((nf && !own.grab(0, (size_t)nf * sizeof(pd_iv))) || (no && !own.grab(1, (size_t)no * sizeof(pd_iv)))) return dec_fail(c, PD_ENOMEM, "run array allocation failed");
        rs.first = (pd_iv *)own.p[0]; rs.other = (pd_iv *)own.p[1];
        if (int rc = copy_out(rs.first, sizeof(pd_iv), rs.other)) return rc;
    }
    if (nf + no) order_of((const pdb2::SegOut *)(sl.h_small + J.o.so), J.n_seg, &rs);
    if (!J.c8) rs.n_long = 0;
    if (res) { res->n_first = nf; res->n_other = no; res->n_reads = co.n_rec; res->unsorted = rs.unsorted; res->first_key = rs.first_key; res->last_key = rs.last_key;
               res->first_start = co.first_start; res->next_start = co.next_start; }
    dec_times(sl, res, true);
    dec_lap(J, 5);
    if (nf + no) { std::lock_guard<std::mutex> lk(c->dec_mu); c->run_segs.push_back(rs); }
    own.kept = true;
    return PD_OK;
}

// the chain across segments on the host; segments whose guess was wrong walk again from the corrected start
int collect_chain(pd_ctx *c, DecSlot &sl)
{
    Job &J = sl.job;
    hipStream_t st = sl.st;
    std::vector<pdb2::Seg> &segs = J.segs;
    const uint32_t n_seg = J.n_seg;
    uint8_t *const pin = sl.h_small;
    pdb2::Seg *d_seg = (pdb2::Seg *)((J.d_tab ? J.d_tab : (uint8_t *)sl.d[DS_BLK]) + J.o.seg);
    memcpy(segs.data(), pin + J.o.seg, (size_t)n_seg * sizeof(pdb2::Seg));
    std::vector<uint32_t> redo;
    for (int round = 0; dec_finish(segs, &redo) > 0; ++round) {
        if (round >= 24) { for (uint32_t j : redo) segs[j].flags |= pdb2::WF_BAD; break; }
        for (uint32_t j : redo) HIPDEC(hipMemcpyAsync(&d_seg[j].hint, &segs[j].hint, 8, hipMemcpyHostToDevice, st));
        HIPDEC(hipMemcpyAsync(sl.d[DS_ONLY], redo.data(), redo.size() * 4, hipMemcpyHostToDevice, st));
        launch_walk_segments(st, J.cfg, d_seg, n_seg, (pdb2::LaneOut *)sl.d[DS_LANE], (const uint32_t *)sl.d[DS_ONLY], (uint32_t)redo.size());
        HIPDEC(hipMemcpyAsync(pin + J.o.seg, d_seg, (size_t)n_seg * sizeof(pdb2::Seg), hipMemcpyDeviceToHost, st));
        HIPDEC(hipStreamSynchronize(st));
        memcpy(segs.data(), pin + J.o.seg, (size_t)n_seg * sizeof(pdb2::Seg));
    }
    return PD_OK;
}

// does the batch have a counted unit with records?  (after unit_outcomes: the segments of a unit that is handed back carry RS_SKIP)
bool counted_records(const Job &J) { for (auto &s : J.segs) if (s.pad2 != (uint32_t)pdrs::RS_SKIP && s.n_rec) return true; return false; }

// Unit outcomes (units handed back emit nothing) and the bases of the segments' runs in the batch's arrays; host only.  bst: the members'
// statuses.  -> the batch's totals, its arrays not yet taken
RunSeg unit_outcomes(Job &J, const int *bst, int32_t *unit_status, pd_decode_result *res)
{
    std::vector<pdb2::Seg> &segs = J.segs;
    const std::vector<uint32_t> &seg0 = J.seg0;
    uint64_t nf = 0, no = 0, nfar = 0, nrec = 0; uint32_t max_span = 0;
    for (uint32_t u = 0; u < (uint32_t)J.units.size(); ++u) {
        int stt = 0;
        const pd_decode_unit &un = J.units[u];
        for (uint32_t b = 0; b < un.n_blocks; ++b) { const int v = bst[un.first_block + b]; if (v < 0) stt = 2; else if (v > 0 && stt == 0) stt = 1; }
        for (uint32_t j = seg0[u]; j < seg0[u + 1]; ++j) {
            if (segs[j].flags & pdb2::WF_BAD) { if (stt != 2) stt = 3; }
            else if ((segs[j].flags & (pdb2::WF_MORE | pdb2::WF_HOST)) && stt == 0) stt = 1;
        }
        unit_status[u] = stt;
        for (uint32_t j = seg0[u]; j < seg0[u + 1]; ++j) {
            segs[j].pad2 = stt ? (uint32_t)pdrs::RS_SKIP : 0u;          // (k_record_stats: a unit that is handed back is counted by whoever decodes it)
            if (stt) { segs[j].n_first = segs[j].n_other = segs[j].n_far = 0; } else nrec += segs[j].n_rec;
            segs[j].base_first = nf; segs[j].base_other = no; segs[j].base_far = nfar;
            nf += segs[j].n_first; no += segs[j].n_other; nfar += segs[j].n_far;
            if (!stt && segs[j].max_span > max_span) max_span = segs[j].max_span;
        }
    }
    if (res) {
        res->n_first = nf; res->n_other = no + nfar; res->n_reads = nrec;
        uint64_t fs = ~0ull, E = 0;
        for (uint32_t j = seg0[0]; j < seg0[1]; ++j) { if (fs == ~0ull && segs[j].used_start != pdb2::NONE) fs = segs[j].used_start; if (segs[j].e_last > E) E = segs[j].e_last; }
        res->first_start = fs; res->next_start = E ? E : ~0ull;
    }
    return RunSeg{J.order, nullptr, nf, nullptr, no, nullptr, nfar, max_span, 0u, 0ull, 0ull};
}

// Pass 2 behind the host's chain check: the runs.  A compact session's pass 2 writes the batch's first runs as 8-byte runs (two planes) into a segment
// of its own and marks the buckets' first runs (*have_so: the segments' keys are on their way back); otherwise the runs go to 12-byte
// arrays, which are `own`'s until the batch is listed.
int collect_emit(pd_ctx *c, DecSlot &sl, RunSeg &rs, Owned &own, bool *have_so)
{
    Job &J = sl.job;
    hipStream_t st = sl.st;
    const uint32_t n_seg = J.n_seg;
    const uint64_t nf = rs.n_first, no = rs.n_other, nfar = rs.n_far;
    uint8_t *const pin = sl.h_small;
    pdb2::Seg *d_seg = (pdb2::Seg *)((J.d_tab ? J.d_tab : (uint8_t *)sl.d[DS_BLK]) + J.o.seg);
    pdb2::LaneOut *d_lane = (pdb2::LaneOut *)sl.d[DS_LANE];
    const auto segs_up = [&]() -> int {                                   // the segments with their bases
        memcpy(pin + J.o.seg, J.segs.data(), (size_t)n_seg * sizeof(pdb2::Seg));
        HIPDEC(hipMemcpyAsync(d_seg, pin + J.o.seg, (size_t)n_seg * sizeof(pdb2::Seg), hipMemcpyHostToDevice, st));
        J.segs_sent = true;
        return PD_OK;
    };
    if (J.c8) {
        pdb2::SegOut *d_so = (pdb2::SegOut *)((uint8_t *)sl.d[DS_SEGOUT] + sizeof(pdb2::ChainOut));
        const int rc = c8_hand_over(c, sl, nf, no, [&](uint32_t *seg_s, pd_iv *seg_o) -> int {
            if (const int ru = segs_up()) return ru;
            pdb2::Cfg cfg = J.cfg;
            cfg.c8 = pdb2::C8Out{nullptr, c->c8.marks, c->d_off, 13u - c->c8.bshift, d_so, (uint32_t)J.order, seg_s, seg_s + c8_plane_words((size_t)nf)};
            launch_emit_segments(st, cfg, d_seg, n_seg, d_lane, nullptr, seg_o, nullptr, nullptr);
            return PD_OK;
        });
        if (rc) return rc;
        if (nf + no) {
            *have_so = true;
            HIPDEC(hipMemcpyAsync(pin + J.o.so, d_so, (size_t)n_seg * sizeof(pdb2::SegOut), hipMemcpyDeviceToHost, st));
        }
        dec_lap(J, 5);
    } else if (nf + no + nfar) {
        if ((nf && !own.grab(0, (size_t)nf * sizeof(pd_iv))) || (no && !own.grab(1, (size_t)no * sizeof(pd_iv))) ||
            (nfar && !own.grab(2, (size_t)nfar * sizeof(pd_iv)))) return dec_fail(c, PD_ENOMEM, "run array allocation failed");
        rs.first = (pd_iv *)own.p[0]; rs.other = (pd_iv *)own.p[1]; rs.far = (pd_iv *)own.p[2];
        if (const int ru = segs_up()) return ru;
        dec_lap(J, 5);                                                    // run array allocation
        launch_emit_segments(st, J.cfg, d_seg, n_seg, d_lane, rs.first, rs.other, rs.far, nullptr);
    }
    return PD_OK;
}

int dec_collect(pd_ctx *c, DecSlot &sl, int32_t *unit_status, pd_decode_result *res)
{
    Job &J = sl.job;                                                  // (J.open goes with the slot: dec_release)
    if (res) { memset(res, 0, sizeof *res); res->first_start = res->next_start = ~0ull; }
    if (unit_status) for (size_t u = 0; u < J.units.size(); ++u) unit_status[u] = 0;
    C8Owes owes{c, &J};
    if (!J.queued) return PD_OK;
    if (!unit_status) return dec_fail(c, PD_EINVAL, "pd_decode_collect: unit_status is required for a batch with units");
    HIPDEC(hipSetDevice(c->device));
    hipStream_t st = sl.st;
    uint8_t *const pin = sl.h_small;
    J.t_mark = dec_now_us();
    if (int rc = dec_wait(c, sl)) return rc;
    dec_record_stats_time(c, sl);
    dec_row_counts_time(c, sl);
    dec_aln_stats_time(c, sl);
    if (J.fast) {
        pdb2::ChainOut co;
        memcpy(&co, pin + J.o.co, sizeof co);
        c->dec_n_redo += co.n_redo;
        if (!co.slow) {
            if (c->dec_cfg.flags & PD_DECODE_RECORD_STATS) ++c->rs_launches;      // (the gated k_record_stats of dec_launch counted this batch; one the gate stopped is not a launch of the counter)
            if (c->dec_cfg.flags & PD_DECODE_ROW_COUNTS) ++c->rc_launches;        // (k_row_counts likewise)
            if (c->dec_cfg.flags & PD_DECODE_ALN_STATS) ++c->as_launches;         // (k_aln_stats likewise)
            return collect_confirmed(c, sl, co, res);
        }
        // ---- out of the ordinary (ChainOut::slow says why; nothing was emitted): the member statuses and the segments as they stand come
        // to the host, which goes through the batch the way it always has
        // (more later runs than the batch's array holds — reads with thousands of CIGAR operations: the batches queued from now on get
        // a slot per 8 inflated bytes, which an alternation of matches and gaps cannot exceed)
        if ((co.slow & pdb2::CH_ROOM) && co.n_first <= J.cap_first) c->dec_oth_div.store(8);
        pdb2::Seg *d_seg = (pdb2::Seg *)((J.d_tab ? J.d_tab : (uint8_t *)sl.d[DS_BLK]) + J.o.seg);
        HIPDEC(hipMemcpyAsync(pin + J.o.bst, sl.d[DS_ST], J.blocks.size() * 4, hipMemcpyDeviceToHost, st));
        HIPDEC(hipMemcpyAsync(pin + J.o.seg, d_seg, (size_t)J.n_seg * sizeof(pdb2::Seg), hipMemcpyDeviceToHost, st));
        HIPDEC(hipStreamSynchronize(st));
    }
    ++c->dec_n_slow;
    if (int rc = collect_chain(c, sl)) return rc;
    RunSeg rs = unit_outcomes(J, (const int *)(pin + J.o.bst), unit_status, res);
    const uint64_t nf = rs.n_first;
    Owned own{c};                                                         // (run arrays taken outside the arena: every early return gives them back)
    dec_lap(J, 4);                                                        // host: chain check, unit outcomes
    bool have_so = false;
    if (int rc = collect_emit(c, sl, rs, own, &have_so)) return rc;
    // are the first runs in (tid, begin) order, as the header's SO:coordinate promises?  (DS_ONLY is free again: 6 words)
    uint32_t order_words[6] = {0, 0, 0, 0, 0, 0};
    if (nf && !J.c8) {
        HIPDEC(hipMemsetAsync(sl.d[DS_ONLY], 0, 24, st));
        launch_runs_sorted(st, rs.first, nf, (uint32_t *)sl.d[DS_ONLY]);
        HIPDEC(hipMemcpyAsync(pin + J.o.ord, sl.d[DS_ONLY], 24, hipMemcpyDeviceToHost, st));
    }
    if (J.timed) HIPDEC(hipEventRecord(sl.ev[4], st));
    if ((c->dec_cfg.flags & (PD_DECODE_RECORD_STATS | PD_DECODE_ROW_COUNTS | PD_DECODE_ALN_STATS)) && counted_records(J)) {
        // the records of the counted units (the segments of the others carry RS_SKIP); the segments go up where the emission had none to send
        pdb2::Seg *d_seg = (pdb2::Seg *)((J.d_tab ? J.d_tab : (uint8_t *)sl.d[DS_BLK]) + J.o.seg);
        if (!J.segs_sent) {
            memcpy(pin + J.o.seg, J.segs.data(), (size_t)J.n_seg * sizeof(pdb2::Seg));
            HIPDEC(hipMemcpyAsync(d_seg, pin + J.o.seg, (size_t)J.n_seg * sizeof(pdb2::Seg), hipMemcpyHostToDevice, st));
            J.segs_sent = true;
        }
        if (c->dec_cfg.flags & PD_DECODE_RECORD_STATS) if (int rc = dec_record_stats(c, sl, d_seg, nullptr)) return rc;
        if (c->dec_cfg.flags & PD_DECODE_ROW_COUNTS) if (int rc = dec_row_counts(c, sl, d_seg, nullptr)) return rc;
        if (c->dec_cfg.flags & PD_DECODE_ALN_STATS) if (int rc = dec_aln_stats(c, sl, d_seg, nullptr)) return rc;
    }
    HIPDEC(hipStreamSynchronize(st));
    HIPDEC(hipGetLastError());
    dec_record_stats_time(c, sl);
    dec_row_counts_time(c, sl);
    dec_aln_stats_time(c, sl);
    if (nf && !J.c8) {
        memcpy(order_words, pin + J.o.ord, 24);
        rs.unsorted = order_words[0];
        rs.first_key = (uint64_t)order_words[2] | ((uint64_t)order_words[3] << 32);
        rs.last_key = (uint64_t)order_words[4] | ((uint64_t)order_words[5] << 32);
    }
    if (have_so) order_of((const pdb2::SegOut *)(pin + J.o.so), J.n_seg, &rs);
    if (res) { res->unsorted = rs.unsorted; res->first_key = rs.first_key; res->last_key = rs.last_key; }
    dec_lap(J, 6);                                                        // pass 2 (waiting)
    dec_times(sl, res, !J.fast);
    if (rs.n_first + rs.n_other + rs.n_far) { std::lock_guard<std::mutex> lk(c->dec_mu); c->run_segs.push_back(rs); }
    own.kept = true;
    return PD_OK;
}

DecSlot *dec_slot_of(pd_ctx *c, const void *host_buf)
{
    // (other feeders may be in pd_decode_acquire, re-allocating THEIR slots' pinned buffers: look the slot up under the lock)
    std::lock_guard<std::mutex> l0(c->dec_mu);
    for (auto &x : c->dec) if (x.busy && !x.job.open && x.h_blob == host_buf) { x.job.open = true; return &x; }      // (claimed: a batch is under way in this slot)
    return nullptr;
}
void dec_release(pd_ctx *c, DecSlot *s) { { std::lock_guard<std::mutex> l(c->dec_mu); s->busy = false; s->job.open = false; s->job.collecting = false; } c->dec_cv.notify_all(); }
struct Release { pd_ctx *c; DecSlot *s; ~Release() { dec_release(c, s); } };

} // namespace

extern "C" {

int pd_decode_submit(pd_ctx *c, const pd_decode_batch *bt, int32_t *unit_status, pd_decode_result *res)
{
    if (!c || !bt || !bt->host_buf || !unit_status) return PD_EINVAL;
    DecSlot *slp = dec_slot_of(c, bt->host_buf);
    if (!slp) return dec_fail(c, PD_EINVAL, "pd_decode_submit: buffer was not handed out by pd_decode_acquire");
    Release rel{c, slp};
    if (res) { memset(res, 0, sizeof *res); res->first_start = res->next_start = ~0ull; }
    for (uint32_t u = 0; u < bt->n_units; ++u) unit_status[u] = 0;
    // (a ticket of an earlier batch on this slot is stale from here on, and nobody else may collect or drain the batch about to be queued)
    { std::lock_guard<std::mutex> l0(c->dec_mu); ++slp->gen; slp->job.collecting = true; }
    const int rc = dec_queue(c, *slp, bt);
    if (rc) return rc;
    return dec_collect(c, *slp, unit_status, res);
}

int pd_decode_queue(pd_ctx *c, const pd_decode_batch *bt, uint64_t *ticket)
{
    if (!c || !bt || !bt->host_buf || !ticket) return PD_EINVAL;
    *ticket = 0;
    DecSlot *slp = dec_slot_of(c, bt->host_buf);
    if (!slp) return dec_fail(c, PD_EINVAL, "pd_decode_queue: buffer was not handed out by pd_decode_acquire");
    const int rc = dec_queue(c, *slp, bt);
    if (rc) { dec_release(c, slp); return rc; }
    { std::lock_guard<std::mutex> l0(c->dec_mu); *ticket = ((uint64_t)++slp->gen << 8) | (uint64_t)(slp - c->dec + 1); }
    return PD_OK;
}

int pd_decode_collect(pd_ctx *c, uint64_t ticket, int32_t *unit_status, pd_decode_result *res)
{
    if (!c) return PD_EINVAL;
    const uint64_t k = ticket & 0xff;
    DecSlot *slp = k >= 1 && k <= (uint64_t)pd_ctx::N_DEC ? &c->dec[k - 1] : nullptr;
    {
        std::lock_guard<std::mutex> l0(c->dec_mu);
        if (!slp || !slp->busy || !slp->job.open || slp->job.collecting || slp->gen != (uint32_t)(ticket >> 8)) slp = nullptr;
        else slp->job.collecting = true;
    }
    if (!slp) return dec_fail(c, PD_EINVAL, "pd_decode_collect: not the ticket of a queued batch (or the batch is being collected already)");
    Release rel{c, slp};
    return dec_collect(c, *slp, unit_status, res);
}

} // extern "C"

namespace {

// The session is over for its callers: batches that were queued and never collected are finished here (pd_decode_end: they count) or
// waited for and dropped (pd_decode_abort); then every slot has come back.
void dec_close(pd_ctx *c, bool finish)
{
    if (c->dec_warm.joinable()) c->dec_warm.join();
    for (auto &sl : c->dec) {
        bool mine = false;
        // (a slot some thread is collecting, or is inside pd_decode_submit on, is left to that thread: this call waits on dec_cv for it)
        { std::lock_guard<std::mutex> lk(c->dec_mu); mine = sl.busy && sl.job.open && !sl.job.collecting; if (mine) sl.job.collecting = true; }
        if (!mine) continue;
        if (finish) { std::vector<int32_t> st(sl.job.units.size() + 1, 0); (void)dec_collect(c, sl, st.data(), nullptr); }
        else { (void)hipSetDevice(c->device); if (sl.st) (void)hipStreamSynchronize(sl.st); C8Owes owes{c, &sl.job}; sl.job.queued = false; }
        dec_release(c, &sl);
    }
    std::unique_lock<std::mutex> lk(c->dec_mu);                           // (stragglers that still hold a slot)
    c->dec_cv.wait(lk, [&] { for (auto &x : c->dec) if (x.busy) return false; return true; });
    c->dec_open = false;
}

// ---- pd_decode_end's pieces (the caller holds c->mu) ----
// do the batches' first runs follow one another in (tid, begin) order?  (segs: by order; inside a batch its own flag says)
bool batches_in_order(const std::vector<RunSeg> &segs)
{
    uint64_t prev = 0; bool have = false;
    for (auto &r : segs) {
        if (!r.n_first) continue;
        if (r.unsorted || (have && r.first_key < prev)) return false;
        prev = r.last_key; have = true;
    }
    return true;
}

// the decoded sample as ONE compact sample: the context's single deferred batch; counter: which way it was made (pd_ctx::DN_END_*)
void install_sample(pd_ctx *c, pd_runs *r, int counter)
{
    c->dec_runs = r;
    ++c->dec_n[counter];
    Pending p{nullptr, r->n, 0u, -1};
    p.cr = r;
    c->pend.push_back(p);
}

// The sample as up to three 12-byte streams in file order (c->run_first / run_other / run_far): every read's first run (position sorted
// for a coordinate-sorted file: exact tile bounds), its later runs that trail the sorted order by at most near_dis, and the few that
// follow a long gap (N operations: they trail by up to `span`).  An unsorted file, or gaps of more than a few tiles, take the atomic path.
int scatter_streams(pd_ctx *c, bool sorted, uint64_t nf, uint64_t no, uint64_t nfar, uint32_t near_dis, uint32_t span)
{
    const bool near_sorted = sorted && near_dis <= (1u << 14), far_sorted = sorted && span <= (1u << 14);
    int rc = PD_OK;
    if (nf) rc = scatter_device(c, c->run_first, (size_t)nf, sorted ? (PD_PUSH_SORTED | PD_PUSH_MORE) : PD_PUSH_DEFAULT, -1, nullptr);
    if (rc == PD_OK && no) rc = scatter_device(c, c->run_other, (size_t)no, near_sorted ? (PD_PUSH_SORTED | PD_PUSH_MORE | PD_PUSH_DISORDER(near_dis + 1)) : PD_PUSH_DEFAULT, -1, nullptr);
    if (rc == PD_OK && nfar) rc = scatter_device(c, c->run_far, (size_t)nfar, far_sorted ? (PD_PUSH_SORTED | PD_PUSH_MORE | PD_PUSH_DISORDER(span + 1)) : PD_PUSH_DEFAULT, -1, nullptr);
    return rc;
}

// PANDEPTH_TIMING: the session's line.  head: the host-side timers under the names the kind of session gives them (eight %.3f and the
// number of batches); runs: what was decoded
void end_timing(pd_ctx *c, const char *head, size_t n_batches, const char *runs)
{
    char timers[512];
    snprintf(timers, sizeof timers, head, g_dec_us[0] / 1e6, g_dec_us[1] / 1e6, g_dec_us[2] / 1e6, g_dec_us[3] / 1e6, g_dec_us[4] / 1e6, g_dec_us[5] / 1e6, g_dec_us[6] / 1e6, g_dec_us[7] / 1e6, n_batches);
    fprintf(stderr, "%s%s; chain confirmed on the device for %llu batches, by the host for %llu; segments the device walked again: %llu\n", timers, runs,
            (unsigned long long)c->dec_n_fast.load(), (unsigned long long)c->dec_n_slow.load(), (unsigned long long)c->dec_n_redo.load());
}

// the compact session's arrays become the sample (the caller holds c8.mu; every batch's runs have reached their places); n_long: runs
// longer than a bucket that the batches' emissions counted
int compact_to_sample(pd_ctx *c, uint64_t n_long)
{
    pd_ctx::C8Dec &x = c->c8;
    pd_runs *r = new pd_runs;
    r->ctx = c; r->lo = x.lo(); r->hi = x.hi(); r->nar = x.nar(); r->own_lo = true; r->n_s = (uint32_t)x.n_s; r->n_o = (uint32_t)x.n_o; r->n = r->n_s + r->n_o; r->o_base = r->n_s;      // (the later runs go right behind the sorted stream, as in pd_runs_create: what counts is how many runs there ARE, not how many were reserved)
    r->b1 = x.b1; r->o1 = x.b1 + x.nbw; r->td = (TileDesc *)((uint8_t *)x.b1 + c8_desc_offset(x.nbw)); r->heavy_tiles = (uint32_t *)((uint8_t *)x.b1 + c8_heavy_offset(x.nbw, c->n_tiles)); r->bshift = x.bshift;
    const pd_iv *oth = x.oth(); const size_t no1 = (size_t)x.n_o;
    uint32_t *tmp = nullptr, *words = nullptr, *d_base = nullptr;
    const size_t nbw = x.nbw;
    unsigned long long *marks = x.marks;
    const std::vector<uint32_t> base_s = x.base_s;
    x.base = nullptr; x.b1 = nullptr; x.marks = nullptr; x.bytes = 0; x.cap_s = x.cap_o = 0;       // (they belong to the sample now; the marks go below)
    c8_drop(c);                                                                                        // the batches' segments and events
    if (hipMalloc(&tmp, (2 * nbw + nbw / 1024 + 8) * 4) != hipSuccess || hipMalloc(&words, 16) != hipSuccess || hipMalloc(&d_base, base_s.size() * 4 + 16) != hipSuccess) {
        (void)hipGetLastError(); for (void *q : {(void *)tmp, (void *)words, (void *)d_base, (void *)marks}) if (q) (void)hipFree(q); runs_free(r);
        return fail(c, PD_ENOMEM, "pd_decode_end: allocation failed");
    }
    uint32_t h[4] = {0, 0, 0, 0};
    hipError_t e = hipMemsetAsync(words, 0, 16, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(words + 3, marks + nbw, 4, hipMemcpyDeviceToDevice, c->stream);      // the placing copies' count of first runs longer than 255 cells (C8Dec::wide; the compose stream has been waited for)
    if (e == hipSuccess) e = hipMemcpyAsync(d_base, base_s.data(), base_s.size() * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        // the marks (batch, index in the batch) of the buckets' first runs become indices into the sorted stream
        { ProfScope ps(c, "compact_finish"); launch_c8_marks_to_index(c->stream, marks, (uint32_t)(nbw - 1), d_base, r->b1); }
        const pd_iv *o[1] = {oth}; const size_t non[1] = {no1};
        runs_finish(c, r, o, non, no1 ? 1 : 0, tmp, words);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, words, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(tmp); (void)hipFree(words); (void)hipFree(d_base); (void)hipFree(marks);
    if (e != hipSuccess) { runs_free(r); return fail(c, PD_EHIP, std::string("pd_decode_end: ") + hipGetErrorString(e)); }
    r->n_long = (uint32_t)std::min<uint64_t>(n_long + h[1], 0xFFFFFFFFull);
    r->n_heavy = h[2];
    r->n_wide_sorted = h[3];
    install_sample(c, r, pd_ctx::DN_END_COMPACT);
    return PD_OK;
}

// a compact session: the runs are where they belong already (or on their way there, on the compose stream)
int end_compact(pd_ctx *c, const std::vector<RunSeg> &segs, uint32_t span)
{
    pd_ctx::C8Dec &x = c->c8;
    std::lock_guard<std::mutex> l8(x.mu);
    x.on = false;
    if (x.turn != x.n_batches || !x.err.empty()) {
        const std::string why = x.err.empty() ? "not every batch of the compact session was submitted" : x.err;
        (void)hipDeviceSynchronize(); c8_drop(c);
        return fail(c, PD_ESTATE, "pd_decode_end: " + why);
    }
    const bool ok_order = batches_in_order(segs);
    uint64_t n_long = 0;
    for (auto &r : segs) n_long += r.n_long;
    if (getenv("PANDEPTH_TIMING")) {
        char runs[160];
        snprintf(runs, sizeof runs, "runs (compact session): %llu first, %llu later (span %u)", (unsigned long long)x.n_s, (unsigned long long)x.n_o, span);
        end_timing(c, "[timing]   decode entry points, thread-seconds: slot wait %.3f, pinned alloc %.3f, device buffers + queueing %.3f, waiting for the device %.3f, "
                      "host chain check %.3f, runs to their arrays %.3f, wait emit (host's path) %.3f, first HIP call of the feeder threads %.3f; %zu batches; ", segs.size(), runs);
    }
    if (x.n_s + x.n_o == 0) { (void)hipStreamSynchronize(x.compose); c8_drop(c); return PD_OK; }
    HIPOK(c, hipStreamSynchronize(x.compose));                 // every batch's runs have reached their places
    if (ok_order && x.n_s && x.n_s + x.n_o <= DEV_BATCH_MAX && !c->pend.empty()) {
        // the context holds other runs already (units the device handed back and the host decoded meanwhile, an earlier file of a list):
        // they go into the arrays now, and the compact sample is pushed behind them like any other deferred batch
        ++c->dec_n[pd_ctx::DN_END_PEND];
        const int rf = flush_pending(c);
        if (rf) { (void)hipDeviceSynchronize(); c8_drop(c); return rf; }
    }
    if (ok_order && x.n_s && c->pend.empty() && x.n_s + x.n_o <= DEV_BATCH_MAX) return compact_to_sample(c, n_long);
    // not usable as a compact sample after all (the records are not in the order the header promised, more than 2^32 runs):
    // back to 12-byte arrays, which take the general paths
    const uint64_t nf = x.n_s, no = x.n_o;
    ++c->dec_n[pd_ctx::DN_END_C8_FALLBACK];
    if (!ok_order) ++c->dec_n[pd_ctx::DN_END_UNSORTED];
    if (nf && c->n_cells >= (1ull << 32)) {
        // 32 bits of a flat begin name a cell only below 2^32 cells; above, it takes the sample's own bucket index to say which contig a
        // run lies in, and that index is exactly what an unordered stream does not have.  (The executable never gets here: it gives a
        // file whose records are not in the promised order to the host readers before anything is counted.)
        (void)hipDeviceSynchronize(); c8_drop(c);
        return fail(c, PD_ESTATE, "pd_decode_end: the records of this compact session are not in coordinate order (or are more than 2^32 - 256 runs) on a genome of 2^32 cells or more: "
                                  "decode it again without PD_DECODE_COMPACT");
    }
    if ((nf && hipMalloc(&c->run_first, (size_t)nf * sizeof(pd_iv)) != hipSuccess) || (no && hipMalloc(&c->run_other, (size_t)no * sizeof(pd_iv)) != hipSuccess)) {
        c8_drop(c); return fail(c, PD_ENOMEM, "pd_decode_end: run array allocation failed"); }
    if (nf) launch_r8_to_iv(c->stream, x.lo(), x.hi(), nf, tab_of(c), c->run_first);
    if (no) HIPOK(c, hipMemcpyAsync(c->run_other, x.oth(), (size_t)no * sizeof(pd_iv), hipMemcpyDeviceToDevice, c->stream));
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipStreamSynchronize(c->stream));
    c8_drop(c);
    return scatter_streams(c, ok_order, nf, no, 0, span, span);
}

// every other session: the batches' 12-byte arrays are concatenated in file order; the whole-contig modes then make ONE compact sample
// of them, everything else scatters them
int end_concat(pd_ctx *c, std::vector<RunSeg> &segs, uint64_t nf, uint64_t no, uint64_t nfar, uint32_t span)
{
    const auto drop = [&]() { for (auto &r : segs) r.release(c); };
    if ((nf && hipMalloc(&c->run_first, (size_t)nf * sizeof(pd_iv)) != hipSuccess) || (no && hipMalloc(&c->run_other, (size_t)no * sizeof(pd_iv)) != hipSuccess) ||
        (nfar && hipMalloc(&c->run_far, (size_t)nfar * sizeof(pd_iv)) != hipSuccess)) { drop(); return fail(c, PD_ENOMEM, "pd_decode_end: run array allocation failed"); }
    uint64_t of = 0, oo = 0, ofar = 0;
    for (auto &r : segs) {
        if (r.n_first) HIPOK(c, hipMemcpyAsync(c->run_first + of, r.first, (size_t)r.n_first * sizeof(pd_iv), hipMemcpyDeviceToDevice, c->stream));
        if (r.n_other) HIPOK(c, hipMemcpyAsync(c->run_other + oo, r.other, (size_t)r.n_other * sizeof(pd_iv), hipMemcpyDeviceToDevice, c->stream));
        if (r.n_far) HIPOK(c, hipMemcpyAsync(c->run_far + ofar, r.far, (size_t)r.n_far * sizeof(pd_iv), hipMemcpyDeviceToDevice, c->stream));
        of += r.n_first; oo += r.n_other; ofar += r.n_far;
    }
    HIPOK(c, hipStreamSynchronize(c->stream));
    drop();
    // sorted only if the records really are in that order (the header may lie)
    const bool sorted = c->dec_cfg.sorted != 0 && batches_in_order(segs);
    if (getenv("PANDEPTH_TIMING")) {
        char runs[160];
        snprintf(runs, sizeof runs, "runs: %llu first, %llu near, %llu far (span %u)", (unsigned long long)nf, (unsigned long long)no, (unsigned long long)nfar, span);
        end_timing(c, "[timing]   decode entry points, thread-seconds: slot wait %.3f, pinned alloc %.3f, device buffers %.3f, wait H2D+inflate+walk %.3f, "
                      "host chain check %.3f, run arrays %.3f, wait emit %.3f, first HIP call of the feeder threads %.3f; %zu batches; ", segs.size(), runs);
    }
    if (nf && sorted && (c->dec_cfg.flags & PD_DECODE_COMPACT) && c->pend.empty() && nf + no + nfar <= DEV_BATCH_MAX) {
        // the whole-contig modes: the sample stays as ONE compact sample (8 bytes per run, grouped by 512-cell bucket: the first
        // runs keep their order — checked again —, the later runs of multi-run reads are dropped into their buckets), the
        // 12-byte arrays go
        pd_runs *r = nullptr;
        const pd_iv *o[2] = {c->run_other, c->run_far}; const size_t non[2] = {(size_t)no, (size_t)nfar};
        if (runs_make(c, c->run_first, (size_t)nf, o, non, 2, &r) == PD_OK) {
            for (pd_iv **q : {&c->run_first, &c->run_other, &c->run_far}) if (*q) { (void)hipFree(*q); *q = nullptr; }
            install_sample(c, r, pd_ctx::DN_END_RUNS_MAKE);
            return PD_OK;
        }
    }
    ++c->dec_n[pd_ctx::DN_END_SCATTER];
    if (c->dec_cfg.sorted && !sorted) ++c->dec_n[pd_ctx::DN_END_UNSORTED];
    // disorder of a stream = how far its runs may trail the sorted order: the near stream by near_span (when the split is on,
    // otherwise by the longest gap seen, like the far stream)
    return scatter_streams(c, sorted, nf, no, nfar, nfar ? (c->dec_near_span < span ? c->dec_near_span : span) : span, span);
}

} // namespace

extern "C" {

int pd_decode_end(pd_ctx *c)
{
    if (!c) return PD_EINVAL;
    dec_close(c, true);
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_decode_end")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    for (auto &sl : c->dec) if (sl.st) HIPOK(c, hipStreamSynchronize(sl.st));      // (the last copies of the batches' runs to their arrays)
    c->rc_ready = (c->dec_cfg.flags & PD_DECODE_ROW_COUNTS) != 0;                  // (... and every batch's k_row_counts: pd_decode_row_counts)
    c->as_ready = (c->dec_cfg.flags & PD_DECODE_ALN_STATS) != 0;                   // (... and every batch's k_aln_stats: pd_decode_aln_stats)
    c->rs_ready = (c->dec_cfg.flags & PD_DECODE_RECORD_STATS) != 0;                // (every batch's k_record_stats is through: pd_decode_record_stats)
    std::vector<RunSeg> segs;
    { std::lock_guard<std::mutex> l2(c->dec_mu); segs.swap(c->run_segs); }
    std::sort(segs.begin(), segs.end(), [](const RunSeg &a, const RunSeg &b) { return a.order < b.order; });
    uint64_t nf = 0, no = 0, nfar = 0; uint32_t span = 0;
    for (auto &r : segs) { nf += r.n_first; no += r.n_other; nfar += r.n_far; if (r.max_span > span) span = r.max_span; }
    if (c->run_first || c->run_other || c->run_far || c->dec_runs) {
        // an earlier sample of this context (#.list: one file after another) may still be deferred on these arrays
        int rf = flush_pending(c);
        if (rf) { for (auto &r : segs) r.release(c); return rf; }
        HIPOK(c, hipStreamSynchronize(c->stream));
        for (pd_iv **q : {&c->run_first, &c->run_other, &c->run_far}) if (*q) { (void)hipFree(*q); *q = nullptr; }
        runs_free(c->dec_runs); c->dec_runs = nullptr;
    }
    const int rc = c->c8.on ? end_compact(c, segs, span) : end_concat(c, segs, nf, no, nfar, span);
    if (getenv("PANDEPTH_TIMING"))                                   // (which way the sample was made: the counters pd_profile_get reports as decode_end_*)
        fprintf(stderr, "[timing]   pd_decode_end: runs of the batches %llu first, %llu later; decode_end_compact %llu, decode_end_c8_fallback %llu, decode_end_runs_make %llu, "
                        "decode_end_scatter %llu, decode_end_unsorted %llu, decode_end_pending %llu\n", (unsigned long long)nf, (unsigned long long)(no + nfar),
                (unsigned long long)c->dec_n[pd_ctx::DN_END_COMPACT], (unsigned long long)c->dec_n[pd_ctx::DN_END_C8_FALLBACK], (unsigned long long)c->dec_n[pd_ctx::DN_END_RUNS_MAKE],
                (unsigned long long)c->dec_n[pd_ctx::DN_END_SCATTER], (unsigned long long)c->dec_n[pd_ctx::DN_END_UNSORTED], (unsigned long long)c->dec_n[pd_ctx::DN_END_PEND]);
    if (getenv("PANDEPTH_TIMING") && c->rs_ready)                    // (the records' statistics pass: decode_record_stats)
        fprintf(stderr, "[timing]   k_record_stats: %llu launches, %.3f ms summed over the batches\n", (unsigned long long)c->rs_launches.load(), (double)c->rs_ns.load() / 1e6);
    if (getenv("PANDEPTH_TIMING") && c->rc_ready)                    // (the rows' pass: decode_row_counts)
        fprintf(stderr, "[timing]   k_row_counts: %llu launches, %.3f ms summed over the batches\n", (unsigned long long)c->rc_launches.load(), (double)c->rc_ns.load() / 1e6);
    if (getenv("PANDEPTH_TIMING") && c->as_ready)                    // (the CIGAR pass: decode_aln_stats)
        fprintf(stderr, "[timing]   k_aln_stats: %llu launches, %.3f ms summed over the batches\n", (unsigned long long)c->as_launches.load(), (double)c->as_ns.load() / 1e6);
    return rc;
}

int pd_decode_abort(pd_ctx *c)
{
    if (!c) return PD_EINVAL;
    dec_close(c, false);
    (void)hipSetDevice(c->device);
    { std::lock_guard<std::mutex> lk(c->dec_mu); for (auto &r : c->run_segs) r.release(c); c->run_segs.clear(); }
    { std::lock_guard<std::mutex> l8(c->c8.mu); if (c->c8.on || c->c8.base) { (void)hipDeviceSynchronize(); c8_drop(c); } }
    c->rs_ready = false;
    if (c->d_recstat && (c->dec_cfg.flags & PD_DECODE_RECORD_STATS)) {            // (the statistics of the batches that are forgotten)
        for (auto &sl : c->dec) if (sl.st) (void)hipStreamSynchronize(sl.st);
        (void)hipMemset(c->d_recstat, 0, c->recstat_words * 8);
    }
    c->rc_ready = false;
    if (c->d_rowcnt && (c->dec_cfg.flags & PD_DECODE_ROW_COUNTS)) {               // (... and their rows)
        for (auto &sl : c->dec) if (sl.st) (void)hipStreamSynchronize(sl.st);
        (void)hipMemset(c->d_rowcnt, 0, c->rowcnt_words * 8);
    }
    c->as_ready = false;
    if (c->d_alnstat && (c->dec_cfg.flags & PD_DECODE_ALN_STATS)) {               // (... and their CIGARs)
        for (auto &sl : c->dec) if (sl.st) (void)hipStreamSynchronize(sl.st);
        (void)hipMemset(c->d_alnstat, 0, (size_t)PD_ALNSTAT_WORDS * 8);
    }
    return PD_OK;
}

int pd_decode_aln_stats(pd_ctx *c, uint64_t *sums, size_t n_sums)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!(c->dec_cfg.flags & PD_DECODE_ALN_STATS) || !c->as_ready || !c->d_alnstat)
        return fail(c, PD_EINVAL, "pd_decode_aln_stats: no session with PD_DECODE_ALN_STATS has been ended by pd_decode_end since the last pd_decode_begin");
    if (!sums || n_sums != (size_t)PD_ALNSTAT_WORDS)
        return fail(c, PD_EINVAL, "pd_decode_aln_stats: sums must hold PD_ALNSTAT_WORDS = " + std::to_string((size_t)PD_ALNSTAT_WORDS) + " words");
    HIPOK(c, hipSetDevice(c->device));
    HIPOK(c, hipMemcpy(sums, c->d_alnstat, (size_t)PD_ALNSTAT_WORDS * 8, hipMemcpyDeviceToHost));
    return PD_OK;
}

int pd_decode_record_stats(pd_ctx *c, uint64_t *sums, size_t n_sums, uint64_t *per_contig)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!(c->dec_cfg.flags & PD_DECODE_RECORD_STATS) || !c->rs_ready || !c->d_recstat)
        return fail(c, PD_EINVAL, "pd_decode_record_stats: no session with PD_DECODE_RECORD_STATS has been ended by pd_decode_end since the last pd_decode_begin");
    const size_t want = (size_t)PD_RECSTAT_FIXED + c->rs_bins + 1;
    if (!sums || n_sums != want || (!per_contig && c->n_contigs))
        return fail(c, PD_EINVAL, "pd_decode_record_stats: sums must hold PD_RECSTAT_FIXED + decode_isize_bins + 1 = " + std::to_string(want) + " words and per_contig 3 per contig");
    HIPOK(c, hipSetDevice(c->device));
    HIPOK(c, hipMemcpy(sums, c->d_recstat, want * 8, hipMemcpyDeviceToHost));
    if (c->n_contigs) HIPOK(c, hipMemcpy(per_contig, c->d_recstat + want, 3 * (size_t)c->n_contigs * 8, hipMemcpyDeviceToHost));
    return PD_OK;
}

int pd_decode_row_bins(pd_ctx *c, uint32_t w, const uint64_t *edge_off, const uint32_t *edges)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t n = (size_t)c->n_contigs;
    const uint64_t max_bins = 1ull << 28;
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<uint32_t> ed;
    uint64_t n_bins;
    if (w) {
        if (edge_off || edges) return fail(c, PD_EINVAL, "pd_decode_row_bins: w > 0 (the window form) takes no edges");
        if (int rc = pd_window_layout(c, w, off.data())) return fail(c, rc, "pd_decode_row_bins: pd_window_layout failed");
        n_bins = off[n];
    } else {
        if (edge_off) {
            if (edge_off[0] != 0) return fail(c, PD_EINVAL, "pd_decode_row_bins: edge_off must begin at 0");
            for (size_t t = 0; t < n; ++t) {
                if (edge_off[t + 1] < edge_off[t]) return fail(c, PD_EINVAL, "pd_decode_row_bins: edge_off must not descend");
                if (edge_off[t + 1] > max_bins) return fail(c, PD_EINVAL, "pd_decode_row_bins: more than 2^28 bins");
            }
            if (edge_off[n] && !edges) return fail(c, PD_EINVAL, "pd_decode_row_bins: edge_off names edges, edges is NULL");
            off.assign(edge_off, edge_off + n + 1);
            for (size_t t = 0; t < n; ++t)
                for (uint64_t k = off[t] + 1; k < off[t + 1]; ++k)
                    if (edges[k] <= edges[k - 1]) return fail(c, PD_EINVAL, "pd_decode_row_bins: the edges of contig " + std::to_string(t) + " are not strictly ascending");
            ed.assign(edges, edges + off[n]);
        }
        n_bins = off[n] + n;
    }
    if (n_bins > max_bins) return fail(c, PD_EINVAL, "pd_decode_row_bins: more than 2^28 bins");
    c->rb_w = w; c->rb_off.swap(off); c->rb_edges.swap(ed); c->rb_nbins = n_bins; c->rb_set = true;
    return PD_OK;
}

int pd_decode_row_counts(pd_ctx *c, uint64_t *counts, size_t n_bins)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!(c->dec_cfg.flags & PD_DECODE_ROW_COUNTS) || !c->rc_ready || !c->d_rowcnt)
        return fail(c, PD_EINVAL, "pd_decode_row_counts: no session with PD_DECODE_ROW_COUNTS has been ended by pd_decode_end since the last pd_decode_begin");
    if (n_bins != c->rc_nbins || (!counts && n_bins))
        return fail(c, PD_EINVAL, "pd_decode_row_counts: counts must hold PD_ROWCOUNT_WORDS words for each of the session's " + std::to_string(c->rc_nbins) + " bins");
    HIPOK(c, hipSetDevice(c->device));
    if (n_bins) HIPOK(c, hipMemcpy(counts, c->d_rowcnt, n_bins * PD_ROWCOUNT_WORDS * 8, hipMemcpyDeviceToHost));
    return PD_OK;
}

// The synchronous single-batch form (round 1's entry point, kept for its callers): one batch through the pipeline
// above, its runs scattered at once (first runs: owner tiles; the others: atomics).
int pd_push_bgzf_units(pd_ctx *c, const void *blob, size_t n_bytes, const pd_bgzf_block *blocks, uint32_t n_blocks,
                       const pd_bgzf_unit *units, uint32_t n_units, uint64_t inflated_bytes, uint32_t flag_mask,
                       int32_t min_mapq, int32_t *unit_status, uint64_t *n_records)
{
    if (!c || !blob || !blocks || !units || !unit_status) return PD_EINVAL;
    if (n_records) *n_records = 0;
    if (n_units == 0 || n_blocks == 0) return PD_OK;
    pd_decode_cfg cfg{}; cfg.flag_mask = flag_mask; cfg.min_mapq = min_mapq; cfg.sorted = 1;
    if (c->dec_deletions) cfg.flags |= PD_DECODE_DELETIONS;               // (pd_set_param "decode_deletions": this entry's signature has no room for flags)
    if (c->dec_fragments) cfg.flags |= PD_DECODE_FRAGMENTS;               // (likewise "decode_fragments"; the bound is "decode_frag_max", which pd_decode_begin reads)
    int rc = pd_decode_begin(c, &cfg);
    if (rc) return rc;
    // the session this call opens is closed on every path out of it (its batch is taken out of the list below, so the
    // abort drops nothing that was counted)
    struct Close { pd_ctx *c; ~Close() { (void)pd_decode_abort(c); } } close_session{c};
    void *hb = nullptr;
    if ((rc = pd_decode_acquire(c, n_bytes, &hb))) return rc;
    memcpy(hb, blob, n_bytes);
    std::vector<pd_decode_unit> du(n_units);
    for (uint32_t u = 0; u < n_units; ++u) du[u] = pd_decode_unit{units[u].start, units[u].stop, units[u].avail, units[u].first_block, units[u].n_blocks, 0, 0};
    static std::atomic<uint64_t> key{0};
    pd_decode_batch bt{}; bt.host_buf = hb; bt.n_bytes = n_bytes; bt.blocks = blocks; bt.n_blocks = n_blocks; bt.inflated_bytes = inflated_bytes;
    bt.units = du.data(); bt.n_units = n_units; bt.order = ((uint64_t)1 << 63) + key.fetch_add(1);
    pd_decode_result res;
    if ((rc = pd_decode_submit(c, &bt, unit_status, &res))) return rc;
    for (auto &sl : c->dec) if (sl.st) (void)hipStreamSynchronize(sl.st);           // (the batch's runs are scattered from another stream below)
    if (n_records) *n_records = res.n_reads;
    RunSeg mine{0, nullptr, 0, nullptr, 0, nullptr, 0, 0};
    {
        std::lock_guard<std::mutex> lk(c->dec_mu);
        for (size_t i = 0; i < c->run_segs.size(); ++i)
            if (c->run_segs[i].order == bt.order) { mine = c->run_segs[i]; c->run_segs.erase(c->run_segs.begin() + (long)i); break; }
    }
    if (mine.n_first + mine.n_other + mine.n_far) {
        std::unique_lock<std::mutex> lk(c->mu);
        if (int rs = need_state(c, 0, "pd_push_bgzf_units")) return rs;
        HIPOK(c, hipSetDevice(c->device));
        if (mine.n_first) { rc = scatter_device(c, mine.first, (size_t)mine.n_first, PD_PUSH_SORTED, -1, nullptr); if (rc) return rc; }
        if (mine.n_other) { rc = scatter_device(c, mine.other, (size_t)mine.n_other, PD_PUSH_DEFAULT, -1, nullptr); if (rc) return rc; }
        if (mine.n_far) { rc = scatter_device(c, mine.far, (size_t)mine.n_far, PD_PUSH_DEFAULT, -1, nullptr); if (rc) return rc; }
        HIPOK(c, hipStreamSynchronize(c->stream));
        mine.release(c);
    }
    return PD_OK;
}

} // extern "C"
