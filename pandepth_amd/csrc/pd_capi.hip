// pd_capi.hip — implementation of include/pandepth_amd.h on top of pd_kernels.hip and pd_direct.hip, all but the window calls (pd_windows.hip), the decode session (pd_decode.hip), the row statistics (pd_rows.hip) and -gcbias (pd_gcbias.hip).
//
// One context = one GPU, one compute stream, one copy stream, one int32 allocation holding all
// contig difference arrays followed by the tile sums.  Host batches go through a small pool of
// pinned staging slots (async H2D on the copy stream, scatter on the compute stream), so
// reader threads overlap decode, PCIe and the scatter kernel.  No CPU fallback exists here:
// without a gfx950 device pd_create fails.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <iostream>
#include <fcntl.h>
#include <unistd.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <thread>
#include <sys/mman.h>
#include <string>
#include <vector>
#include <map>
#include <deque>
#include "pd_local_comm.h"
#include "pd_ctx.h"            // (behind pd_local_comm.h, whose staging buffer is not one of the guarded allocations)

// ---- guarded device allocations: what pd_ctx.h declares (the bookkeeping is this file's alone) ----
namespace pdguard {
constexpr size_t G = 256;
constexpr unsigned char PAT = 0xC5;
struct Rec { size_t bytes; const char *file; int line; };
std::mutex mu;
std::map<void *, Rec> live;
std::atomic<uint64_t> n_bad{0};
std::string last_msg;
bool on() { static const bool v = [] { const char *e = getenv("PANDEPTH_GUARD"); return e && *e && strcmp(e, "0") != 0; }(); return v; }

// caller holds mu; the device is idle
uint64_t check_one(void *user, const Rec &r)
{
    unsigned char h[2 * G];
    uint8_t *raw = (uint8_t *)user - G;
    if (hipMemcpy(h, raw, G, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h + G, (uint8_t *)user + r.bytes, G, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int front = 0, back = 0, first_back = -1, last_back = -1, first_front = -1;
    for (size_t i = 0; i < G; ++i) if (h[i] != PAT) { ++front; if (first_front < 0) first_front = (int)i; }
    for (size_t i = 0; i < G; ++i) if (h[G + i] != PAT) { ++back; if (first_back < 0) first_back = (int)i; last_back = (int)i; }
    if (!front && !back) return 0;
    char m[320];
    snprintf(m, sizeof m, "[guard] device buffer of %zu bytes allocated at %s:%d was written out of bounds: %d byte(s) in front (first at -%d), "
             "%d byte(s) behind (offsets +%d .. +%d past the end)", r.bytes, r.file, r.line, front, first_front < 0 ? 0 : (int)G - first_front, back, first_back, last_back);
    fprintf(stderr, "%s\n", m);
    last_msg = m;
    // repair the canaries so that one overrun is reported once
    (void)hipMemset(raw, PAT, G); (void)hipMemset((uint8_t *)user + r.bytes, PAT, G);
    return 1;
}

hipError_t gmalloc(void **out, size_t bytes, const char *file, int line)
{
    if (!on()) return (hipMalloc)(out, bytes);              // (in parentheses: the runtime's own, not pd_ctx.h's macro)
    uint8_t *raw = nullptr;
    const hipError_t e = (hipMalloc)((void **)&raw, bytes + 2 * G);
    if (e != hipSuccess) return e;
    (void)hipMemset(raw, PAT, G);
    (void)hipMemset(raw + G + bytes, PAT, G);
    (void)hipDeviceSynchronize();
    *out = raw + G;
    std::lock_guard<std::mutex> g(mu);
    live[raw + G] = Rec{bytes, file, line};
    return hipSuccess;
}

hipError_t gfree(void *user)
{
    if (!on() || !user) return (hipFree)(user);
    std::lock_guard<std::mutex> g(mu);
    auto it = live.find(user);
    if (it == live.end()) return (hipFree)(user);          // not one of ours (cannot happen; stay safe)
    (void)hipDeviceSynchronize();
    n_bad += check_one(user, it->second);
    live.erase(it);
    return (hipFree)((uint8_t *)user - G);
}

// a sub-buffer of a larger allocation (pd_create packs the context's small buffers into one): the caller has left G bytes in front of
// and behind it; they become canaries, checked like everybody else's until drop()
void adopt(void *user, size_t bytes, const char *file, int line)
{
    if (!on()) return;
    (void)hipMemset((uint8_t *)user - G, PAT, G);
    (void)hipMemset((uint8_t *)user + bytes, PAT, G);
    (void)hipDeviceSynchronize();
    std::lock_guard<std::mutex> g(mu);
    live[user] = Rec{bytes, file, line};
}
void drop(void *user)
{
    if (!on() || !user) return;
    std::lock_guard<std::mutex> g(mu);
    auto it = live.find(user);
    if (it == live.end()) return;
    (void)hipDeviceSynchronize();
    n_bad += check_one(user, it->second);
    live.erase(it);
}

uint64_t check_all()
{
    if (!on()) return 0;
    std::lock_guard<std::mutex> g(mu);
    int dev = 0; (void)hipGetDevice(&dev);
    (void)hipDeviceSynchronize();
    for (auto &kv : live) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, kv.first) == hipSuccess && at.device != dev) { (void)hipSetDevice(at.device); (void)hipDeviceSynchronize(); }
        n_bad += check_one(kv.first, kv.second);
    }
    (void)hipSetDevice(dev);
    return n_bad.load();
}
} // namespace pdguard

extern "C" int pd_guard_check(char *msg, size_t cap)
{
    const uint64_t n = pdguard::check_all();
    if (msg && cap) { std::lock_guard<std::mutex> g(pdguard::mu); snprintf(msg, cap, "%s", pdguard::last_msg.c_str()); }
    return n > 0x7fffffff ? 0x7fffffff : (int)n;
}

// proves that the guard sees what it is there to see: a guarded buffer is allocated, ONE byte is written just behind it (and, second
// round, just in front of it), and the check must report exactly that.  Returns 0 when both are found, 1 when the guard is off, -1 when the
// guard is on and misses a write.  The findings it provokes are not counted (pd_guard_check's count is unchanged).
extern "C" int pd_guard_selftest(void)
{
    if (!pdguard::on()) return 1;
    int found = 0;
    for (int side = 0; side < 2; ++side) {
        uint8_t *p = nullptr;
        if (hipMalloc(&p, 1000) != hipSuccess) return -1;
        (void)hipMemset(side ? p - 1 : p + 1000, 0, 1);
        (void)hipDeviceSynchronize();
        const uint64_t before = pdguard::n_bad.load();
        (void)hipFree(p);
        if (pdguard::n_bad.load() == before + 1) ++found;
        pdguard::n_bad.store(before);
    }
    { std::lock_guard<std::mutex> g(pdguard::mu); pdguard::last_msg.clear(); }
    return found == 2 ? 0 : -1;
}

namespace {

std::string g_create_err;                   // why the last pd_create failed (contexts may be created on several threads at once:
std::mutex g_create_err_mu;                 // written and read under this lock, handed out as a copy of the calling thread's own)

} // namespace

namespace pdi {

int fail(pd_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else { std::lock_guard<std::mutex> lk(g_create_err_mu); g_create_err = msg; }
    return code;
}

// every entry point that needs the arrays in a given state (0 accumulating, 1 depth)
int need_state(pd_ctx *c, int want, const char *fn)
{
    if (c->state == want) return PD_OK;
    const char *why = c->state == 1 ? "depth already materialised (call pd_reset, or use the pd_reduce_* calls)"
                                    : "call pd_scan first";
    return fail(c, PD_ESTATE, std::string(fn) + ": " + why);
}

ContigTab tab_of(pd_ctx *c) { return ContigTab{c->d_off, c->d_len, c->n_contigs}; }

hipEvent_t get_event(pd_ctx *c)
{
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

} // namespace pdi

namespace {

int prof_collect(pd_ctx *c)
{
    if (c->prof_pending.empty()) return PD_OK;
    HIPOK(c, hipStreamSynchronize(c->stream));
    for (auto &r : c->prof_pending) {
        float ms = 0.f;
        HIPOK(c, hipEventElapsedTime(&ms, r.a, r.b));
        auto &acc = c->prof_acc[r.name];
        acc.first += ms; acc.second += 1;
        c->ev_pool.push_back(r.a); c->ev_pool.push_back(r.b);
    }
    c->prof_pending.clear();
    return PD_OK;
}

// Reset = forget every cell: mark all half-tiles "not written" (the owner-tile kernel stores into
// them without reading, the sweep reads them as zeros) and zero the tile sums.  No 12 GB fill.
int do_reset(pd_ctx *c)
{
    // (Skipping the launch while nobody has written the four spans since the last reset — every step of the direct path on a compact sample — was built and
    // taken out again: the launch hides behind the host's turn-around, the traced cycle and the step did not move.  profiles/r14_direct_step_ab.txt.)
    ProfScope ps(c, "reset");
    launch_reset_spans(c->stream, ResetSpans{{c->hstate, c->sums, c->chk, c->desc},
                                             {(size_t)c->n_half, (size_t)(c->n_words - c->n_cells) * 4, sizeof(CheckWords), sizeof(BatchDesc) * PD_MAXPEND}});
    HIPOK(c, hipGetLastError());
    c->all_valid_host = false;
    c->pristine = true;
    c->sums_stale = false;
    return PD_OK;
}

// every cell readable/atomically addable: zero-fill what has not been written since the reset
int ensure_all_valid(pd_ctx *c)
{
    if (c->all_valid_host) return PD_OK;
    ProfScope ps(c, "fill");
    launch_fill_invalid(c->stream, c->buf, c->hstate, c->n_half, c->chk, false, (unsigned)c->n_cu * 8);
    HIPOK(c, hipGetLastError());
    c->all_valid_host = true;
    return PD_OK;
}

} // namespace

namespace pdi {

int ensure_scratch(pd_ctx *c, size_t bytes)
{
    if (bytes <= c->scratch_bytes) return PD_OK;
    if (c->scratch) { HIPOK(c, hipStreamSynchronize(c->stream)); HIPOK(c, hipFree(c->scratch)); c->scratch = nullptr; c->scratch_bytes = 0; }
    size_t want = bytes + bytes / 4 + 4096;
    if (hipMalloc(&c->scratch, want) != hipSuccess) return fail(c, PD_ENOMEM, "scratch allocation failed");
    c->scratch_bytes = want;
    return PD_OK;
}

// a compact pending sample that has to take a path that reads 12-byte runs: expanded once (the copy stays with the sample).
// Inside a bucket the runs are in no particular order: the batch is sorted up to one bucket's cells of disorder.
static int expand_compact(pd_ctx *c, Pending &p)
{
    if (!p.cr || p.iv) return PD_OK;
    pd_runs *r = p.cr;
    if (!r->iv12) {
        if (hipMalloc(&r->iv12, (size_t)r->n * sizeof(pd_iv)) != hipSuccess) return fail(c, PD_ENOMEM, "compact sample: allocation of the expanded runs failed");
        ProfScope ps(c, "expand_runs");
        launch_c8_expand(c->stream, r->view(), c->d_tile_contig, c->d_off, (uint32_t)c->n_tiles, r->iv12);
        HIPOK(c, hipGetLastError());
    }
    p.iv = r->iv12;
    p.disorder = (uint32_t)PD_TILE >> r->bshift;
    return PD_OK;
}

// the one preparation of the pending sample for a tile pass (flush_pending, direct_windows, direct_export: pd_ctx.h says what the arguments are)
int pend_prepare(pd_ctx *c, uint32_t stride, uint32_t n_stiles, int stile, bool skip, PendSet *ps, uint64_t *all)
{
    *ps = PendSet{};
    ps->nb = (int)c->pend.size(); ps->lmax = c->lmax;
    *all = 0;
    for (auto &p : c->pend) *all += p.n;
    if (skip) return PD_OK;
    for (auto &p : c->pend) { const int re = expand_compact(c, p); if (re) return re; }
    for (int b = 0; b < ps->nb; ++b) {
        const Pending &p = c->pend[b];
        ps->b[b] = PendBatch{p.iv, c->ub_a[b], c->cand_lo[b], c->desc + b, p.n, 0};
        ProfScope sc(c, "scatter_index");
        launch_scatter_index(c->stream, p.iv, p.n, tab_of(c), c->lmax, p.disorder, stride, c->ub_a[b], c->cand_lo[b], n_stiles, stile, c->desc + b);
    }
    return PD_OK;
}

// one owner-tile pass over all pending sorted batches
int flush_pending(pd_ctx *c)
{
    if (c->pend.empty()) return PD_OK;
    if (c->sums_stale) {                      // a direct export wrote this (still deferred) sample's tile sums; the scatter adds to them
        HIPOK(c, hipMemsetAsync(c->sums, 0, (c->n_words - c->n_cells) * 4, c->stream));
        c->sums_stale = false;
    }
    uint64_t total = 0;
    for (auto &p : c->pend) total += p.n;
    if (total > OVF_MAX) total = OVF_MAX;     // more long runs than this in ONE pass is reported (err bit 4):
                                              // such data belongs on the PD_PUSH_DEFAULT path
    if (total > c->ovf_cap) {
        if (c->ovf) { HIPOK(c, hipStreamSynchronize(c->stream)); HIPOK(c, hipFree(c->ovf)); c->ovf = nullptr; c->ovf_cap = 0; }
        const uint64_t cap = total;
        if (hipMalloc(&c->ovf, (size_t)cap * 8) != hipSuccess) return fail(c, PD_ENOMEM, "overflow list allocation failed");
        c->ovf_cap = (uint32_t)cap;
    }
    const uint32_t n_stiles = (uint32_t)(c->n_cells / c->stile);
    PendSet ps{}; uint64_t all = 0;
    if (int rc = pend_prepare(c, c->sample, n_stiles, c->stile, false, &ps, &all)) return rc;
    c->pristine = false;
    const unsigned grid = pdwin::pass_grid(all, c->n_cu, c->grid_tiles, 0);
    { ProfScope sc(c, "scatter_tiles");
      launch_scatter_tiles(c->stream, ps, tab_of(c), c->d_tile_contig, n_stiles, c->stile, c->buf, c->sums, c->hstate,
                           c->ovf, c->ovf_cap, c->chk, grid); }
    { ProfScope sc(c, "scatter_finish");
      if (!c->all_valid_host) launch_fill_invalid(c->stream, c->buf, c->hstate, c->n_half, c->chk, true, (unsigned)c->n_cu * 8);
      launch_scatter_finish(c->stream, ps, c->buf, c->sums, c->ovf, c->ovf_cap, c->chk); }
    HIPOK(c, hipGetLastError());
    for (auto &p : c->pend)
        if (p.slot >= 0) {
            Stage &st = c->stage[p.slot];
            HIPOK(c, hipEventRecord(st.done, c->stream));
            st.state = 2; st.seq = ++c->seq;
        }
    c->pend.clear();
    return PD_OK;
}

// scatter a device-resident batch on the compute stream; *deferred = true when a staged slot must
// stay in flight until flush_pending records its event
int scatter_device(pd_ctx *c, const pd_iv *d, size_t n, unsigned flags, int slot, bool *deferred)
{
    if (deferred) *deferred = false;
    if (n == 0) return PD_OK;
    if (flags & PD_PUSH_SORTED) {
        const uint64_t dis64 = (uint64_t)(flags >> 8) * 256u;
        const uint32_t disorder = dis64 > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)dis64;
        for (size_t o = 0; o < n; o += DEV_BATCH_MAX) {
            const uint32_t m = (uint32_t)(n - o < DEV_BATCH_MAX ? n - o : DEV_BATCH_MAX);
            const bool last = o + m >= n;
            c->pend.push_back(Pending{d + o, m, disorder, last ? slot : -1});
            if (c->pend.size() == PD_MAXPEND || !(last && (flags & PD_PUSH_MORE))) {
                int rc = flush_pending(c);
                if (rc) return rc;
            }
        }
        if (deferred) *deferred = !c->pend.empty();
    } else {
        int rc = flush_pending(c);
        if (rc) return rc;
        rc = ensure_all_valid(c);
        if (rc) return rc;
        c->pristine = false;
        ProfScope ps(c, "scatter_atomic");
        launch_scatter_atomic(c->stream, d, n, tab_of(c), c->buf, c->sums);
    }
    HIPOK(c, hipGetLastError());
    return PD_OK;
}

int check_words(pd_ctx *c)
{
    CheckWords h;
    HIPOK(c, hipMemcpyAsync(&h, c->chk, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    if (h.unsorted_batches || h.err) {
        char m[256];
        snprintf(m, sizeof m, "%llu batch(es) pushed with PD_PUSH_SORTED were not sorted by (tid,beg), held invalid "
                 "contig ids or too many runs longer than lmax (err bits 0x%x); depth arrays are not valid",
                 (unsigned long long)h.unsorted_batches, h.err);
        return fail(c, PD_EINVAL, m);
    }
    return PD_OK;
}

} // namespace pdi

namespace {

// caller holds c->mu
int stage_acquire(pd_ctx *c, int *slot)
{
    for (;;) {
        int oldest = -1;
        for (int i = 0; i < (int)c->stage.size(); ++i) {
            Stage &s = c->stage[i];
            if (s.state == 2 && hipEventQuery(s.done) == hipSuccess) s.state = 0;
            if (s.state == 0) { *slot = i; s.state = 1; return PD_OK; }
            if (s.state == 2 && (oldest < 0 || s.seq < c->stage[oldest].seq)) oldest = i;
        }
        // a new slot while the pool may still grow and fewer than 4 batches are queued on the GPU
        int inflight = 0;
        for (auto &s : c->stage) inflight += s.state == 2;
        if ((int)c->stage.size() < N_STAGE && (oldest < 0 || inflight < 4)) {
            Stage s;
            if (hipEventCreateWithFlags(&s.copied, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess)
                return fail(c, PD_EHIP, "cannot create staging events");
            s.state = 1;
            c->stage.push_back(s);
            *slot = (int)c->stage.size() - 1;
            return PD_OK;
        }
        if (oldest < 0) {
            if (!c->pend.empty()) { int rc = flush_pending(c); if (rc) return rc; continue; }
            return fail(c, PD_ESTATE, "all staging slots are held by callers");
        }
        HIPOK(c, hipEventSynchronize(c->stage[oldest].done));
        c->stage[oldest].state = 0;
    }
}

int stage_submit(pd_ctx *c, int slot, size_t n, unsigned flags)
{
    Stage &s = c->stage[slot];
    if (n == 0) { s.state = 0; return PD_OK; }
    if (!c->copy_stream) HIPOK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    HIPOK(c, hipMemcpyAsync(s.dev, s.host, n * sizeof(pd_iv), hipMemcpyHostToDevice, c->copy_stream));
    HIPOK(c, hipEventRecord(s.copied, c->copy_stream));
    HIPOK(c, hipStreamWaitEvent(c->stream, s.copied, 0));
    bool deferred = false;
    int rc = scatter_device(c, s.dev, n, flags, slot, &deferred);
    if (rc) return rc;
    Stage &s2 = c->stage[slot];               // (the vector may not have grown, but stay safe)
    if (deferred) { s2.state = 3; return PD_OK; }          // event recorded by flush_pending
    if (s2.state != 2) { HIPOK(c, hipEventRecord(s2.done, c->stream)); s2.state = 2; s2.seq = ++c->seq; }
    return PD_OK;
}

} // namespace

namespace pdi {

// A page-locked host buffer for a decode slot.  hipHostMalloc of 34 MB takes 7-8 ms (the runtime allocates and maps it 4 KiB page by page): six of them were
// 46 ms in front of every run's first read.  Anonymous memory the kernel backs with 2 MiB pages (MADV_HUGEPAGE; where transparent huge pages are off it is
// ordinary memory), touched, then registered with the runtime (hipHostRegister) takes 1.5 ms and copies at the same 56 GB/s (tools/ubench/pin_cost.hip,
// profiles/r06_h2d_fill.txt).  Falls back to hipHostMalloc.
uint8_t *pin_alloc(size_t bytes, bool *mapped)
{
    *mapped = false;
    if (!getenv("PANDEPTH_NO_HUGE_PIN")) {
        const size_t al = (size_t)2 << 20, len = (bytes + al - 1) / al * al;
        void *m = mmap(nullptr, len + al, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m != MAP_FAILED) {
            uint8_t *q = (uint8_t *)(((uintptr_t)m + al - 1) / al * al);
            // (the unaligned head and tail go back at once: the region is exactly [q, q + len))
            if (q > (uint8_t *)m) munmap(m, (size_t)(q - (uint8_t *)m));
            if ((uint8_t *)m + len + al > q + len) munmap(q + len, (size_t)((uint8_t *)m + len + al - (q + len)));
            (void)madvise(q, len, MADV_HUGEPAGE);
            for (size_t o = 0; o < len; o += 4096) q[o] = 0;              // (fault it in before the runtime walks it)
            if (hipHostRegister(q, len, hipHostRegisterDefault) == hipSuccess) { *mapped = true; return q; }
            (void)hipGetLastError();
            munmap(q, len);
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return (uint8_t *)p;
}
void pin_free(uint8_t *p, size_t bytes, bool mapped)
{
    if (!p) return;
    if (!mapped) { (void)hipHostFree(p); return; }
    const size_t al = (size_t)2 << 20, len = (bytes + al - 1) / al * al;
    (void)hipHostUnregister(p);
    munmap(p, len);
}

} // namespace pdi

extern "C" {

int pd_abi_version(void) { return PD_ABI_VERSION; }

const char *pd_strerror(const pd_ctx *ctx)
{
    if (ctx) return ctx->err.c_str();
    static thread_local std::string mine;
    { std::lock_guard<std::mutex> lk(g_create_err_mu); mine = g_create_err; }
    return mine.c_str();
}

int pd_create(int device, int32_t n_contigs, const uint32_t *contig_len, pd_ctx **out)
{
    if (!out || n_contigs <= 0 || !contig_len) return fail(nullptr, PD_EINVAL, "pd_create: bad arguments");
    *out = nullptr;
    const bool tm_on = getenv("PANDEPTH_TIMING") != nullptr;
    const auto tm_t0 = std::chrono::steady_clock::now();
    auto tm_mark = [&](const char *what) { if (tm_on) fprintf(stderr, "[timing]   pd_create: %-28s at %.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - tm_t0).count()); };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, PD_ENODEV, "pd_create: no HIP device visible (this engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, PD_ENODEV, "pd_create: device index out of range");
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) != hipSuccess) return fail(nullptr, PD_ENODEV, "pd_create: cannot query device");
    if (!strstr(pr.gcnArchName, "gfx950"))
        return fail(nullptr, PD_ENODEV, std::string("pd_create: device is ") + pr.gcnArchName + ", kernels are built for gfx950 only");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, PD_ENODEV, "pd_create: hipSetDevice failed");
    tm_mark("runtime up, device chosen");

    pd_ctx *c = new pd_ctx;
    c->device = device;
    c->n_contigs = n_contigs;
    c->len.assign(contig_len, contig_len + n_contigs);
    c->off.resize((size_t)n_contigs + 1);
    uint64_t o = 0;
    for (int32_t i = 0; i < n_contigs; ++i) {
        c->off[i] = o;
        o += ((uint64_t)contig_len[i] + 1 + PD_TILE - 1) / PD_TILE * PD_TILE;   // room for the -1 at cell len
    }
    c->off[n_contigs] = o;
    c->n_cells = o;
    c->n_tiles = o / PD_TILE;
    if (c->n_tiles >= 0xFFFFFFF0ull) { delete c; return fail(nullptr, PD_EINVAL, "pd_create: genome too large"); }
    c->n_words = c->n_cells + (c->n_tiles + 3) / 4 * 4;
    c->n_cu = pr.multiProcessorCount;

#define CREATE_OK(call)                                                                                  \
    do { hipError_t e_ = (call); if (e_ != hipSuccess) {                                                 \
        std::string m_ = std::string("pd_create: ") + #call + ": " + hipGetErrorString(e_);            \
        pd_destroy(c); return fail(nullptr, e_ == hipErrorOutOfMemory ? PD_ENOMEM : PD_EHIP, m_); } } while (0)

    CREATE_OK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CREATE_OK(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    CREATE_OK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    CREATE_OK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    // (the copy stream of the host staging path is made by its first user: a queue costs ~15 ms, and the device-decode path
    // of the executable never stages runs from the host)
    tm_mark("streams");
    CREATE_OK(hipMalloc(&c->buf, c->n_words * 4));
    tm_mark("cell buffer");
    c->sums = c->buf + c->n_cells;
    c->n_half = (uint32_t)(c->n_cells / PD_HALF);
    {
        // the small buffers come out of ONE allocation (seventeen hipMalloc calls were 17 ms of every run's start-up), each on a 256-byte
        // boundary; with PANDEPTH_GUARD they keep a canary in front of and behind them inside the slab, like separate allocations would
        struct Want { void **pp; size_t bytes; int line; };
        std::vector<Want> wants;
#define WANT(field, bytes_) wants.push_back(Want{(void **)&(field), (size_t)(bytes_), __LINE__})
        WANT(c->carry, (c->n_tiles + 4) * 4);
        WANT(c->bsum, (c->n_tiles / 1024 + 4) * 4);
        WANT(c->d_off, ((size_t)n_contigs + 1) * 8);
        WANT(c->d_len, (size_t)n_contigs * 4);
        WANT(c->d_tile_contig, (c->n_tiles + 1) * 4);
        for (int b = 0; b < PD_MAXPEND; ++b) {
            WANT(c->ub_a[b], (c->n_tiles * 2 + 4) * 4);          // indexed by 4096-cell scatter tile
            WANT(c->cand_lo[b], (c->n_tiles * 2 + 4) * 4);
        }
        WANT(c->hstate, c->n_half + 16);
        WANT(c->slice_flags, slice_flag_bytes(c->n_tiles) + 2 * (16 + ((size_t)c->n_tiles + 4) * 4) + 16);   // flags | counter | list of flagged tiles | counter | list of the tiles the packed sweep leaves
        WANT(c->direct_words, 64 + (c->n_tiles + 4) * 4);        // [n_long, fail, heavy_count, diagnostics ... | heavy tile list at +16]
        WANT(c->desc, sizeof(BatchDesc) * PD_MAXPEND);
        WANT(c->chk, sizeof(CheckWords));
#undef WANT
        const size_t gap = pdguard::on() ? pdguard::G : 0;
        std::vector<size_t> at(wants.size());
        size_t total = 0;
        for (size_t k = 0; k < wants.size(); ++k) { total += gap; at[k] = total; total = (total + wants[k].bytes + gap + 255) / 256 * 256; }
        CREATE_OK(hipMalloc(&c->slab, total + 256));
        for (size_t k = 0; k < wants.size(); ++k) { *wants[k].pp = c->slab + at[k]; pdguard::adopt(*wants[k].pp, wants[k].bytes, __FILE_NAME__, wants[k].line); }
    }
    {
        std::vector<uint32_t> tc(c->n_tiles + 1, 0);
        for (int32_t i = 0; i < n_contigs; ++i)
            for (uint64_t t = c->off[i] / PD_TILE; t < c->off[i + 1] / PD_TILE; ++t) tc[t] = (uint32_t)i;
        // (on the context's stream, not the null stream: the process's null stream would be one more hardware queue to make — 9 ms — for three small copies)
        CREATE_OK(hipMemcpyAsync(c->d_tile_contig, tc.data(), (c->n_tiles + 1) * 4, hipMemcpyHostToDevice, c->stream));
        CREATE_OK(hipMemcpyAsync(c->d_off, c->off.data(), ((size_t)n_contigs + 1) * 8, hipMemcpyHostToDevice, c->stream));
        CREATE_OK(hipMemcpyAsync(c->d_len, c->len.data(), (size_t)n_contigs * 4, hipMemcpyHostToDevice, c->stream));
        CREATE_OK(hipStreamSynchronize(c->stream));
    }
#undef CREATE_OK
    tm_mark("other buffers + tables");
    int rc = do_reset(c);
    if (rc == PD_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = PD_EHIP;
    tm_mark("first reset (kernels loaded)");
    if (rc != PD_OK) { { std::lock_guard<std::mutex> lk(g_create_err_mu); g_create_err = c->err; } pd_destroy(c); return rc; }
    *out = c;
    return PD_OK;
}

int pd_destroy(pd_ctx *c)
{
    if (!c) return PD_OK;
    if (c->dec_warm.joinable()) c->dec_warm.join();
    const bool tm = getenv("PANDEPTH_TIMING") != nullptr;
    const uint64_t t0 = dec_now_us(); uint64_t t1 = t0, t2 = t0, t3 = t0;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (size_t i = 0; i < c->stage.size(); ++i) {
        if (c->stage[i].host) (void)hipHostFree(c->stage[i].host);
        if (c->stage[i].dev) (void)hipFree(c->stage[i].dev);
        if (c->stage[i].copied) (void)hipEventDestroy(c->stage[i].copied);
        if (c->stage[i].done) (void)hipEventDestroy(c->stage[i].done);
    }
    for (auto &r : c->prof_pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    for (void *p : {(void *)c->carry, (void *)c->bsum, (void *)c->d_off, (void *)c->d_len, (void *)c->d_tile_contig, (void *)c->ub_a[0], (void *)c->ub_a[1], (void *)c->ub_a[2],
                    (void *)c->ub_a[3], (void *)c->cand_lo[0], (void *)c->cand_lo[1], (void *)c->cand_lo[2], (void *)c->cand_lo[3], (void *)c->hstate, (void *)c->slice_flags,
                    (void *)c->direct_words, (void *)c->desc, (void *)c->chk}) pdguard::drop(p);            // (parts of the slab)
    void *ptrs[] = {c->buf, c->slab, c->ovf, c->scratch};
    t1 = dec_now_us();
    for (void *p : ptrs) if (p) (void)hipFree(p);
    c->win.release();
    t2 = dec_now_us();
    for (auto &sl : c->dec) {
        if (sl.st) (void)hipStreamSynchronize(sl.st);
        pin_free(sl.h_blob, sl.h_cap, sl.h_mapped);
        if (sl.h_small) (void)hipHostFree(sl.h_small);
        for (void *p : sl.d) if (p) (void)hipFree(p);
        if (sl.d_tok) (void)hipFree(sl.d_tok);
        for (hipEvent_t e : sl.ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : sl.ev_rs) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : sl.ev_rc) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : sl.ev_as) if (e) (void)hipEventDestroy(e);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
        if (sl.st) (void)hipStreamDestroy(sl.st);
    }
    for (auto &r : c->run_segs) r.release(c);
    for (void *p : {(void *)c->d_contig_on, (void *)c->d_span_off, (void *)c->d_spans, (void *)c->run_first, (void *)c->run_other, (void *)c->run_far, (void *)c->arena, (void *)c->d_recstat, (void *)c->d_rc_off, (void *)c->d_rc_edges, (void *)c->d_rowcnt, (void *)c->d_alnstat}) if (p) (void)hipFree(p);
    runs_free(c->dec_runs);
    for (void *p : {(void *)c->c8.base, (void *)c->c8.b1}) if (p) (void)hipFree(p);
    t3 = dec_now_us();
    for (auto &w : c->lz) { std::lock_guard<std::mutex> g(w.mu); w.release(); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    for (hipEvent_t e : {c->ev_fork, c->ev_join}) if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->dec_copy_st2) (void)hipStreamDestroy(c->dec_copy_st2);
    if (c->dec_warm_word) (void)hipFree(c->dec_warm_word);
    delete c;
    if (tm) fprintf(stderr, "[timing]   pd_destroy: sync + staging %.3f s, cells and tables %.3f s, decode slots and runs %.3f s, parse buffers and streams %.3f s\n",
                    (t1 - t0) * 1e-6, (t2 - t1) * 1e-6, (t3 - t2) * 1e-6, (dec_now_us() - t3) * 1e-6);
    return PD_OK;
}

int pd_reset(pd_ctx *c)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->win.valid = false;
    HIPOK(c, hipSetDevice(c->device));
    // deferred batches are forgotten with everything else (they used to be scattered first, a whole-genome pass for nothing);
    // their staging slots are free once the stream has passed this point
    for (auto &p : c->pend)
        if (p.slot >= 0) {
            Stage &st = c->stage[p.slot];
            HIPOK(c, hipEventRecord(st.done, c->stream));
            st.state = 2; st.seq = ++c->seq;
        }
    c->pend.clear();
    c->state = 0;
    if (pdguard::on()) (void)pdguard::check_all();
    int rc = do_reset(c);
    if (rc == PD_OK && (c->run_first || c->run_other || c->run_far || c->dec_runs)) {          // the decoded sample's runs go with it
        HIPOK(c, hipStreamSynchronize(c->stream));
        for (pd_iv **q : {&c->run_first, &c->run_other, &c->run_far}) if (*q) { (void)hipFree(*q); *q = nullptr; }
        runs_free(c->dec_runs); c->dec_runs = nullptr;
    }
    return rc;
}

int pd_keep_deferred(pd_ctx *c, int enable)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->direct_windows = enable != 0;
    return PD_OK;
}

int pd_set_param(pd_ctx *c, const char *name, uint64_t value)
{
    if (!c || !name) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!strcmp(name, "lmax")) { if (value < 1 || value > 4096) return fail(c, PD_EINVAL, "lmax must be in [1, 4096]"); c->lmax = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "sample")) { if (value < 1 || value > 65536) return fail(c, PD_EINVAL, "sample must be in [1, 65536]"); c->sample = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "scatter_tile")) {
        if (value != 4096 && value != 8192) return fail(c, PD_EINVAL, "scatter_tile must be 4096 or 8192");
        c->stile = (int)value; return PD_OK;
    }
    if (!strcmp(name, "grid_tiles")) { if (value > (1u << 20)) return fail(c, PD_EINVAL, "grid_tiles out of range"); c->grid_tiles = (unsigned)value; return PD_OK; }
    if (!strcmp(name, "accumulate_packed")) { c->accumulate_packed = value != 0; return PD_OK; }
    if (!strcmp(name, "direct_un")) { c->direct_un = (int)value; return PD_OK; }
    if (!strcmp(name, "direct_cover")) { c->direct_cover = value != 0; return PD_OK; }
    if (!strcmp(name, "cover_narrow")) { c->cover_narrow = value != 0; return PD_OK; }
    if (!strcmp(name, "cover_fast")) { c->cover_fast = value != 0; return PD_OK; }
    if (!strcmp(name, "direct_cover_min")) { c->direct_cover_min = value > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "direct_sample")) { if (value < 1 || value > 65536) return fail(c, PD_EINVAL, "direct_sample must be in [1, 65536]"); c->direct_sample = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "decode_crc")) { c->dec_crc = value != 0; return PD_OK; }
    if (!strcmp(name, "sweep_i4_fast")) { pdk::set_sweep_i4_fast(value != 0); return PD_OK; }
    if (!strcmp(name, "lz_mix")) { c->lz_mix = value != 0; return PD_OK; }
    if (!strcmp(name, "lz_group")) { if (value > pdk::LZ_GROUP_MAX) return fail(c, PD_EINVAL, "lz_group must be in [0, 16]"); c->lz_group = (unsigned)value; return PD_OK; }
    if (!strcmp(name, "inflate_waves")) { if (value < 1 || value > 24) return fail(c, PD_EINVAL, "inflate_waves must be in [1, 24]"); c->dec_waves = (unsigned)value; return PD_OK; }
    if (!strcmp(name, "decode_spoil")) { c->dec_spoil = value > 0xFFFFFFFFull ? 0u : (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "decode_fast")) { c->dec_fast = value != 0; return PD_OK; }
    if (!strcmp(name, "decode_h2d_kernel")) { c->dec_h2d_kernel = (int)value; return PD_OK; }
    if (!strcmp(name, "decode_h2d_fifo")) { c->dec_h2d_fifo = value != 0; return PD_OK; }
    if (!strcmp(name, "decode_warm")) { c->dec_warm_on = value != 0; return PD_OK; }
    if (!strcmp(name, "lz_slots")) { c->lz_slots = value >= 4 ? 4 : 2; return PD_OK; }
    if (!strcmp(name, "decode_h2d_lanes")) { c->dec_h2d_lanes = value > 1 ? 2 : 1; return PD_OK; }
    if (!strcmp(name, "decode_sync_event")) { c->dec_sync_event = value != 0; return PD_OK; }
    if (!strcmp(name, "decode_c8_reserve")) { c->dec_c8_reserve = value; return PD_OK; }
    if (!strcmp(name, "decode_max_redo")) { c->dec_max_redo = value > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "hist_variant")) { if (value > 3) return fail(c, PD_EINVAL, "hist_variant must be in [0, 3]"); c->hist_variant = (int)value; return PD_OK; }
    if (!strcmp(name, "quantile_wave_max")) { if (value > 2048) return fail(c, PD_EINVAL, "quantile_wave_max must be in [0, 2048]"); c->q_wave_max = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "threshold_wave_max")) { if (value > 0xFFFFFFFFull) return fail(c, PD_EINVAL, "threshold_wave_max must be below 2^32"); c->t_wave_max = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "gcbias_piece_cells")) { if (value < 1 || value > (1ull << 26)) return fail(c, PD_EINVAL, "gcbias_piece_cells must be in [1, 2^26]"); c->gc_piece_cells = value; return PD_OK; }
    if (!strcmp(name, "gcbias_wave_max")) { if (value > 0xFFFFFFFFull) return fail(c, PD_EINVAL, "gcbias_wave_max must be below 2^32"); c->gc_wave_max = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "quantile_split_cells")) { if (value > 0xFFFFFFFFull) return fail(c, PD_EINVAL, "quantile_split_cells must be below 2^32"); c->q_split = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "decode_deletions")) { c->dec_deletions = value != 0; return PD_OK; }
    if (!strcmp(name, "decode_fragments")) { c->dec_fragments = value != 0; return PD_OK; }
    if (!strcmp(name, "decode_frag_max")) { if (value > 0x7FFFFFFFull) return fail(c, PD_EINVAL, "decode_frag_max must be below 2^31 (0: no bound)"); c->dec_frag_max = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "decode_len_bin_width")) { if (value < 1 || value > 65536) return fail(c, PD_EINVAL, "decode_len_bin_width must be in 1 .. 65536"); c->dec_len_bin_width = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "decode_isize_bins")) { if (value < 1 || value > 65536) return fail(c, PD_EINVAL, "decode_isize_bins must be in 1 .. 65536"); c->dec_isize_bins = (uint32_t)value; return PD_OK; }
    if (!strcmp(name, "decode_near_span")) { c->dec_near_span = value > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)value; return PD_OK; }
    return fail(c, PD_EINVAL, std::string("unknown parameter ") + name);
}

} // extern "C"

namespace pdi {

void runs_free(pd_runs *r)
{
    if (!r) return;
    if (r->own_lo && r->lo) (void)hipFree(r->lo);                 // (both planes)
    for (void *q : {(void *)r->b1, (void *)r->iv12}) if (q) (void)hipFree(q);
    delete r;
}

uint32_t runs_bshift(const pd_ctx *c)
{
    // buckets as wide as the look-back bound ("lmax", a power of two between 256 and 8192 cells; default 512)
    uint32_t cells = 256; while (cells < c->lmax && cells < (uint32_t)PD_TILE) cells <<= 1;
    uint32_t bs = 0; while (((uint32_t)PD_TILE >> bs) > cells) ++bs;
    return bs;
}

// The second half of making a compact sample, shared by pd_runs_create and pd_decode_end: the sorted stream is in r->lo / r->hi[0 .. n_s) and the
// first run of every bucket has left its index in r->b1 (everything else 0xFFFFFFFF); `others` are the remaining runs as 12-byte arrays, any
// order.  Fills the bucket starts of the sorted stream (a suffix minimum over the marks), counts the other runs per bucket, places them
// behind o_base, and writes the per-tile descriptors (r->td) from the finished bucket starts.  words (device, 2 x uint32, already holding
// the sorted stream's flags): [0] bad contig id, [1] runs longer than a bucket, [2] pile-up tiles (k_c8_tile_desc), [3] sorted runs longer than 255 cells —
// left there by whoever wrote the sorted stream (k_c8_from_sorted; a decode session's placing copies, through compact_to_sample) and read with the
// others by the caller into pd_runs::n_wide_sorted.
// Only enqueues on c->stream; `tmp` must hold 2 x (nb + 2) + (nb / 1024 + 4) words.
void runs_finish(pd_ctx *c, pd_runs *r, const pd_iv *const *others, const size_t *n_others, int n_arr, uint32_t *tmp, uint32_t *words)
{
    hipStream_t st = c->stream;
    const uint32_t nb = (uint32_t)((uint64_t)c->n_tiles << r->bshift);
    const size_t nbw = (size_t)nb + 2;
    uint32_t *hist = tmp, *cursor = tmp + nbw, *bs = tmp + 2 * nbw;
    const ContigTab tab = tab_of(c);
    ProfScope ps(c, "compact_finish");
    launch_c8_fill_starts(st, r->b1, nb, r->n_s, bs);
    (void)hipMemsetAsync(hist, 0, 2 * nbw * 4, st);                       // the histogram and the buckets' cursors
    for (int k = 0; k < n_arr; ++k) launch_c8_hist(st, others[k], (uint32_t)n_others[k], tab, r->bshift, hist, words);
    launch_excl_scan_u32(st, hist, r->o1, nb + 1, bs);
    for (int k = 0; k < n_arr; ++k) launch_c8_place_other(st, others[k], (uint32_t)n_others[k], tab, r->bshift, r->o1, cursor, r->lo + r->o_base, r->hi + r->o_base);
    launch_c8_tile_desc(st, r->view(), tab, c->d_tile_contig, (uint32_t)c->n_tiles, r->td, words + 2, r->heavy_tiles);       // both streams' bucket starts are final; words[2]: the pile-up tiles, listed in r->heavy_tiles
}

// caller holds c->mu and has set the device.  `sorted` must be sorted by (tid, beg) — checked; the `others` may be in any order.
int runs_make(pd_ctx *c, const pd_iv *sorted, size_t n_sorted, const pd_iv *const *others, const size_t *n_others, int n_arr, pd_runs **out)
{
    *out = nullptr;
    size_t n = n_sorted, n_o = 0;
    for (int k = 0; k < n_arr; ++k) n_o += n_others[k];
    n += n_o;
    if (n == 0 || n > DEV_BATCH_MAX) return fail(c, PD_EINVAL, "pd_runs_create: between 1 and 2^32 - 256 runs");
    if (n_arr > 2) return PD_EINVAL;
    pd_runs *r = new pd_runs;
    r->ctx = c; r->n = (uint32_t)n; r->n_s = (uint32_t)n_sorted; r->n_o = (uint32_t)n_o; r->o_base = (uint32_t)n_sorted;
    r->bshift = runs_bshift(c);
    const uint64_t nb64 = (uint64_t)c->n_tiles << r->bshift;
    if (nb64 > 0xFFFFFF00ull) { delete r; return fail(c, PD_EINVAL, "pd_runs_create: too many buckets for this genome"); }
    const uint32_t nb = (uint32_t)nb64;
    const size_t nbw = (size_t)nb + 2;
    uint32_t *tmp = nullptr, *words = nullptr;
    if (hipMalloc(&r->lo, c8_planes_bytes(n, n_sorted)) != hipSuccess || hipMalloc(&r->b1, c8_index_bytes(nbw, c->n_tiles)) != hipSuccess ||
        hipMalloc(&tmp, (2 * nbw + nb / 1024 + 8) * 4) != hipSuccess || hipMalloc(&words, 16) != hipSuccess) {
        (void)hipGetLastError();
        for (void *q : {(void *)tmp, (void *)words}) if (q) (void)hipFree(q);
        runs_free(r);
        return fail(c, PD_ENOMEM, "pd_runs_create: allocation failed");
    }
    r->hi = r->lo + n;                                            // one allocation: lo | hi, n words each, then the sorted stream's narrow plane
    r->nar = (uint16_t *)((uint8_t *)r->lo + c8_nar_offset(n));
    r->o1 = r->b1 + nbw; r->td = (TileDesc *)((uint8_t *)r->b1 + c8_desc_offset(nbw)); r->heavy_tiles = (uint32_t *)((uint8_t *)r->b1 + c8_heavy_offset(nbw, c->n_tiles));
    uint32_t h[4] = {0, 0, 0, 0};
    hipStream_t st = c->stream;
    hipError_t e = hipMemsetAsync(words, 0, 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(r->b1, 0xFF, nbw * 4, st);
    if (e == hipSuccess) {
        // (this first pass is what the GPU decoder's emit kernel does as it writes a file's runs: 8-byte runs in file order as two planes, the buckets'
        // first runs marked)
        { ProfScope ps(c, "compact_runs"); launch_c8_from_sorted(st, sorted, (uint32_t)n_sorted, tab_of(c), r->bshift, r->lo, r->hi, r->nar, r->b1, words); }
        runs_finish(c, r, others, n_others, n_arr, tmp, words);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, words, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(tmp); (void)hipFree(words);
    if (e != hipSuccess) { runs_free(r); return fail(c, PD_EHIP, std::string("pd_runs_create: ") + hipGetErrorString(e)); }
    if (h[0]) { runs_free(r); return fail(c, PD_EINVAL, "pd_runs_create: the first batch is not sorted by (tid, beg), or a contig id is out of range"); }
    r->n_long = h[1];
    r->n_heavy = h[2];
    r->n_wide_sorted = h[3];
    *out = r;
    return PD_OK;
}

} // namespace pdi

extern "C" {

int pd_runs_create(pd_ctx *c, const pd_iv *dev_sorted, size_t n_sorted, const pd_iv *dev_other, size_t n_other, pd_runs **out)
{
    if (!c || !out || (!dev_sorted && n_sorted) || (!dev_other && n_other)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPOK(c, hipSetDevice(c->device));
    const pd_iv *o[1] = {dev_other}; const size_t no[1] = {n_other};
    return runs_make(c, dev_sorted, n_sorted, o, no, n_other ? 1 : 0, out);
}

int pd_runs_destroy(pd_runs *r)
{
    if (!r) return PD_OK;
    pd_ctx *c = r->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    for (auto &p : c->pend) if (p.cr == r) return fail(c, PD_ESTATE, "pd_runs_destroy: the sample is still deferred on its context (pd_reset first)");
    (void)hipStreamSynchronize(c->stream);
    runs_free(r);
    return PD_OK;
}

int pd_runs_pileup_tiles(pd_ctx *c, const pd_runs *r, uint32_t *tiles, uint32_t cap, uint32_t *n)
{
    if (!c || !n || (cap && !tiles) || (r && r->ctx != c)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!r) r = c->dec_runs;
    if (!r) return fail(c, PD_ESTATE, "pd_runs_pileup_tiles: the context holds no compact sample of a decode session");
    HIPOK(c, hipSetDevice(c->device));
    *n = r->n_heavy;
    const uint32_t m = r->n_heavy < cap ? r->n_heavy : cap;
    if (m) {
        HIPOK(c, hipMemcpyAsync(tiles, r->heavy_tiles, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
        HIPOK(c, hipStreamSynchronize(c->stream));
    }
    return PD_OK;
}

int pd_push_runs(pd_ctx *c, const pd_runs *runs, unsigned flags)
{
    if (!c || !runs || runs->ctx != c || (flags & ~PD_PUSH_MORE)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_push_runs")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);                 // what was deferred before it is scattered first
    if (rc) return rc;
    Pending p{nullptr, runs->n, 0u, -1};
    p.cr = const_cast<pd_runs *>(runs);
    c->pend.push_back(p);
    return (flags & PD_PUSH_MORE) ? PD_OK : flush_pending(c);
}

int pd_push_intervals_device(pd_ctx *c, const pd_iv *dev_iv, size_t n, unsigned flags)
{
    if (!c || (!dev_iv && n)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_push_intervals_device")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    return scatter_device(c, dev_iv, n, flags, -1, nullptr);
}

int pd_stage_acquire(pd_ctx *c, pd_iv **host_buf, size_t *capacity)
{
    if (!c || !host_buf || !capacity) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPOK(c, hipSetDevice(c->device));
    int slot = -1;
    int rc = stage_acquire(c, &slot);
    if (rc) return rc;
    Stage &s = c->stage[slot];
    if (!s.host) {
        if (hipHostMalloc((void **)&s.host, STAGE_CAP * sizeof(pd_iv), hipHostMallocDefault) != hipSuccess ||
            hipMalloc((void **)&s.dev, STAGE_CAP * sizeof(pd_iv)) != hipSuccess) {
            s.state = 0;
            return fail(c, PD_ENOMEM, "staging slot allocation failed");
        }
    }
    *host_buf = s.host; *capacity = STAGE_CAP;
    return PD_OK;
}

int pd_stage_submit(pd_ctx *c, pd_iv *host_buf, size_t n, unsigned flags)
{
    if (!c || !host_buf) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int slot = -1;
    for (int i = 0; i < (int)c->stage.size(); ++i) if (c->stage[i].host == host_buf && c->stage[i].state == 1) slot = i;
    if (slot < 0) return fail(c, PD_EINVAL, "pd_stage_submit: buffer was not handed out by pd_stage_acquire");
    if (n > STAGE_CAP) return fail(c, PD_EINVAL, "pd_stage_submit: more runs than the slot holds");
    if (c->state != 0) { c->stage[slot].state = 0; return fail(c, PD_ESTATE, "pd_stage_submit: depth already materialised (call pd_reset)"); }
    HIPOK(c, hipSetDevice(c->device));
    return stage_submit(c, slot, n, flags);
}

int pd_push_intervals(pd_ctx *c, const pd_iv *iv, size_t n, unsigned flags)
{
    if (!c || (!iv && n)) return PD_EINVAL;
    for (size_t o = 0; o < n; o += STAGE_CAP) {
        const size_t m = n - o < STAGE_CAP ? n - o : STAGE_CAP;
        pd_iv *hb = nullptr; size_t cap = 0;
        int rc = pd_stage_acquire(c, &hb, &cap);
        if (rc) return rc;
        memcpy(hb, iv + o, m * sizeof(pd_iv));
        rc = pd_stage_submit(c, hb, m, flags);
        if (rc) return rc;
    }
    return PD_OK;
}

int pd_scan(pd_ctx *c, unsigned wrap_bits)
{
    if (!c || wrap_bits > 32) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_scan")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc) return rc;
    rc = check_words(c);
    if (rc) return rc;
    const uint32_t mask = pdwin::wrap_mask(wrap_bits);
    { ProfScope ps(c, "tile_carry"); launch_tile_carry(c->stream, c->sums, c->bsum, c->carry, (uint32_t)c->n_tiles); }
    { ProfScope ps(c, "scan"); launch_scan_write(c->stream, c->buf, c->carry, (uint32_t)c->n_tiles, mask, c->hstate); }
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipMemsetAsync(c->hstate, 1, c->n_half, c->stream));     // the sweep wrote every cell
    launch_mark_all_valid(c->stream, c->chk);
    c->all_valid_host = true;
    c->state = 1;
    return PD_OK;
}

int pd_read_depth(pd_ctx *c, int32_t tid, uint32_t beg, size_t n, uint32_t *out)
{
    if (!c || (!out && n)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_read_depth")) return rs;
    if (tid < 0 || tid >= c->n_contigs) return fail(c, PD_EINVAL, "pd_read_depth: contig id out of range");
    if ((uint64_t)beg + n > c->off[tid + 1] - c->off[tid]) return fail(c, PD_EINVAL, "pd_read_depth: range past the contig slot");
    HIPOK(c, hipSetDevice(c->device));
    HIPOK(c, hipMemcpyAsync(out, c->buf + c->off[tid] + beg, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    return PD_OK;
}

int pd_format_sites(pd_ctx *c, int32_t tid, uint32_t beg, size_t n, const char *name, size_t name_len, char *text, size_t cap, size_t *n_bytes)
{
    if (!c || !n_bytes || (!text && cap) || (!name && name_len)) return PD_EINVAL;
    *n_bytes = 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_format_sites")) return rs;
    if (tid < 0 || tid >= c->n_contigs) return fail(c, PD_EINVAL, "pd_format_sites: contig id out of range");
    if ((uint64_t)beg + n > c->off[tid + 1] - c->off[tid]) return fail(c, PD_EINVAL, "pd_format_sites: range past the contig slot");
    if (name_len > 4096 || n > ((size_t)1 << 27)) return fail(c, PD_EINVAL, "pd_format_sites: at most 2^27 cells per call and 4096 bytes of name");
    if (n == 0) return PD_OK;
    HIPOK(c, hipSetDevice(c->device));
    const uint32_t nb = pdk::site_rows_blocks(n);
    const size_t b_name = (name_len + 15) / 16 * 16 + 16, b_cnt = ((size_t)nb * 4 + 15) / 16 * 16, b_off = ((size_t)nb + 1) * 8;
    const size_t worst = n * (name_len + 23);                  // name + 2 tabs + newline + 2 x 10 digits
    int rc = ensure_scratch(c, b_name + b_cnt + b_off + worst + 64);
    if (rc) return rc;
    unsigned char *s = (unsigned char *)c->scratch;
    char *d_name = (char *)s; uint32_t *d_cnt = (uint32_t *)(s + b_name); uint64_t *d_off = (uint64_t *)(s + b_name + b_cnt);
    char *d_text = (char *)(s + b_name + b_cnt + b_off);
    ProfScope ps(c, "format_sites");
    if (name_len) HIPOK(c, hipMemcpyAsync(d_name, name, name_len, hipMemcpyHostToDevice, c->stream));
    const uint32_t *depth = (const uint32_t *)(c->buf + c->off[tid] + beg);
    pdk::launch_site_rows(c->stream, depth, beg, n, (uint32_t)name_len, d_name, d_cnt, d_off, d_text, false);
    uint64_t total = 0;
    HIPOK(c, hipMemcpyAsync(&total, d_off + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    HIPOK(c, hipGetLastError());
    if (total > cap) return fail(c, PD_EINVAL, "pd_format_sites: the text buffer is too small");
    pdk::launch_site_rows(c->stream, depth, beg, n, (uint32_t)name_len, d_name, d_cnt, d_off, d_text, true);
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipMemcpyAsync(text, d_text, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    *n_bytes = (size_t)total;
    return PD_OK;
}

int pd_device_buffer(pd_ctx *c, void **dev_ptr, uint64_t *n_words, uint64_t *contig_off)
{
    if (!c) return PD_EINVAL;
    {   // whoever reads the raw buffer must see real zeros, not "not written since reset"
        std::lock_guard<std::mutex> lk(c->mu);
        HIPOK(c, hipSetDevice(c->device));
        int rc = flush_pending(c);
        if (rc) return rc;
        if (c->state == 0) { rc = ensure_all_valid(c); if (rc) return rc; }
    }
    if (dev_ptr) *dev_ptr = c->buf;
    if (n_words) *n_words = c->n_words;
    if (contig_off) for (int32_t i = 0; i < c->n_contigs; ++i) contig_off[i] = c->off[i];
    return PD_OK;
}

} // extern "C"


extern "C" {

int pd_device_count(int *n)
{
    if (!n) return PD_EINVAL;
    int k = 0;
    if (hipGetDeviceCount(&k) != hipSuccess) k = 0;
    *n = k;
    return k > 0 ? PD_OK : PD_ENODEV;
}

int pd_accumulate_from(pd_ctx *dst, pd_ctx *src)
{
    if (!dst || !src || dst == src) return PD_EINVAL;
    // lock both contexts in address order
    std::unique_lock<std::mutex> l1(dst < src ? dst->mu : src->mu), l2(dst < src ? src->mu : dst->mu);
    if (dst->n_words != src->n_words || dst->n_contigs != src->n_contigs || dst->len != src->len)
        return fail(dst, PD_EINVAL, "pd_accumulate_from: the contexts describe different contigs");
    if (dst->state != 0 || src->state != 0) return fail(dst, PD_ESTATE, "pd_accumulate_from: both contexts must be accumulating");
    HIPOK(src, hipSetDevice(src->device));
    int rc = flush_pending(src);
    if (rc) { dst->err = src->err; return rc; }
    rc = check_words(src);
    if (rc) { dst->err = src->err; return rc; }
    if (dst->device != src->device) {
        HIPOK(dst, hipSetDevice(dst->device));
        int can = 0;
        (void)hipDeviceCanAccessPeer(&can, dst->device, src->device);
        if (can) (void)hipDeviceEnablePeerAccess(src->device, 0);    // already enabled is fine
        (void)hipGetLastError();
        HIPOK(src, hipSetDevice(src->device));
    }
    // Packed transport (default): the source packs its cells to nibbles (d + 8) + an exception list
    // on its own GPU — 1.5 GB instead of 12 GB over the link for a 3 Gb genome; never-written
    // half-tiles need no fill.  More than EXC_CAP cells outside [-8, 7]: the int32 path below.
    constexpr uint32_t EXC_CAP = 1u << 20;
    const size_t img_bytes = dst->n_cells / 2, exc_bytes = (size_t)EXC_CAP * sizeof(pd_exc);
    bool packed = dst->accumulate_packed;
    uint32_t n_exc = 0;
    if (packed) {
        rc = ensure_scratch(src, 16 + exc_bytes + img_bytes);
        if (rc) { dst->err = src->err; return rc; }
        unsigned char *ss = (unsigned char *)src->scratch;
        HIPOK(src, hipMemsetAsync(ss, 0, 16, src->stream));
        { ProfScope ps(src, "export_i4");
          launch_export_i4(src->stream, src->buf, src->hstate, ss + 16 + exc_bytes, src->n_cells, (pd_exc *)(ss + 16), EXC_CAP,
                           (uint32_t *)ss); }
        HIPOK(src, hipMemcpyAsync(&n_exc, ss, 4, hipMemcpyDeviceToHost, src->stream));
        HIPOK(src, hipStreamSynchronize(src->stream));
        if (n_exc > EXC_CAP) packed = false;
    }
    if (!packed) {
        // int32 transport: materialise the source (zeros where nothing was written)
        rc = ensure_all_valid(src);
        if (rc) { dst->err = src->err; return rc; }
    }
    if (src->copy_stream) HIPOK(src, hipStreamSynchronize(src->copy_stream));
    HIPOK(src, hipStreamSynchronize(src->stream));
    HIPOK(dst, hipSetDevice(dst->device));
    rc = flush_pending(dst);
    if (rc) return rc;
    rc = ensure_all_valid(dst);
    if (rc) return rc;
    dst->pristine = false;
    const size_t CH = (size_t)64 << 20;                               // words per chunk (256 MiB)
    if (packed) {
        const unsigned char *ss = (const unsigned char *)src->scratch;
        const size_t CHB = CH * 4;                                    // image bytes per chunk = 512 Mi cells
        rc = ensure_scratch(dst, CHB + (size_t)n_exc * sizeof(pd_exc) + 64);
        if (rc) return rc;
        unsigned char *ds = (unsigned char *)dst->scratch;
        pd_exc *d_exc = (pd_exc *)(ds + CHB);
        if (n_exc) HIPOK(dst, hipMemcpyPeerAsync(d_exc, dst->device, ss + 16, src->device, (size_t)n_exc * sizeof(pd_exc), dst->stream));
        for (size_t o = 0; o < img_bytes; o += CHB) {
            const size_t n = img_bytes - o < CHB ? img_bytes - o : CHB;
            HIPOK(dst, hipMemcpyPeerAsync(ds, dst->device, ss + 16 + exc_bytes + o, src->device, n, dst->stream));
            ProfScope ps(dst, "accumulate_from");
            const bool last = o + CHB >= img_bytes;
            launch_add_i4(dst->stream, dst->buf + o * 2, ds, (uint32_t)(n / (PD_TILE / 2)), d_exc, last ? n_exc : 0, dst->n_cells, dst->buf);
        }
        // the int32 tile sums travel as they are (4 B per 8192 cells)
        const size_t n_sum_words = dst->n_words - dst->n_cells;
        HIPOK(dst, hipMemcpyPeerAsync(ds, dst->device, src->sums, src->device, n_sum_words * 4, dst->stream));
        launch_add_i32(dst->stream, dst->sums, (const int *)ds, n_sum_words);
    } else {
        rc = ensure_scratch(dst, CH * 4);
        if (rc) return rc;
        for (size_t o = 0; o < dst->n_words; o += CH) {
            const size_t n = dst->n_words - o < CH ? dst->n_words - o : CH;
            HIPOK(dst, hipMemcpyPeerAsync(dst->scratch, dst->device, src->buf + o, src->device, n * 4, dst->stream));
            ProfScope ps(dst, "accumulate_from");
            launch_add_i32(dst->stream, dst->buf + o, (const int *)dst->scratch, n);
        }
    }
    HIPOK(dst, hipGetLastError());
    HIPOK(dst, hipStreamSynchronize(dst->stream));
    return PD_OK;
}

int pd_device_layout(pd_ctx *c, uint64_t *n_cells, uint64_t *n_tile_sums)
{
    if (!c) return PD_EINVAL;
    if (n_cells) *n_cells = c->n_cells;
    if (n_tile_sums) *n_tile_sums = c->n_words - c->n_cells;
    return PD_OK;
}

int pd_export_i8(pd_ctx *c, int threshold, void *dev_i8, pd_exc *dev_exc, uint32_t exc_cap, uint32_t *dev_count)
{
    if (!c || !dev_i8 || !dev_count || threshold < 1 || threshold > 127 || (exc_cap && !dev_exc)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_export_i8")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc) return rc;
    HIPOK(c, hipMemsetAsync(dev_count, 0, 4, c->stream));
    { ProfScope ps(c, "export_i8");
      launch_export_i8(c->stream, c->buf, c->hstate, dev_i8, c->n_cells, threshold, dev_exc, exc_cap, dev_count); }
    HIPOK(c, hipGetLastError());
    return PD_OK;
}

int pd_import_i8(pd_ctx *c, const void *dev_i8, int bias, const pd_exc *dev_exc, uint64_t n_exc)
{
    if (!c || !dev_i8 || bias < 0 || bias > 255 || (n_exc && !dev_exc)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_import_i8")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc) return rc;
    c->pristine = false;
    { ProfScope ps(c, "import_i8");
      launch_import_i8(c->stream, dev_i8, c->buf, c->n_cells, bias, dev_exc, n_exc); }
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipMemsetAsync(c->hstate, 1, c->n_half, c->stream));      // every cell was just written
    c->all_valid_host = true;
    launch_mark_all_valid(c->stream, c->chk);
    return PD_OK;
}

int pd_slice_sweep_i4(pd_ctx *c, const void *dev_parts, uint32_t n_parts, uint64_t part_stride, uint64_t tile_first,
                      uint64_t tile_count, const int32_t *dev_tile_sums, const pd_exc *dev_exc, uint64_t exc_stride,
                      const int32_t *dev_exc_counts, uint32_t w, uint32_t min_dep, unsigned wrap_bits, void *dev_partials)
{
    if (!c || !dev_parts || !n_parts || !dev_tile_sums || !dev_partials || wrap_bits > 32) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (w < PD_TILE) return fail(c, PD_EINVAL, "pd_slice_sweep_i4: windows narrower than a tile are not sliced");
    if (tile_first > c->n_tiles || tile_count > c->n_tiles - tile_first)
        return fail(c, PD_EINVAL, "pd_slice_sweep_i4: tile range outside the buffer");
    if (n_parts > 1 && part_stride < tile_count * (PD_TILE / 2)) return fail(c, PD_EINVAL, "pd_slice_sweep_i4: parts overlap");
    if (((uintptr_t)dev_parts | part_stride) & 15) return fail(c, PD_EINVAL, "pd_slice_sweep_i4: parts must be 16-byte aligned");
    HIPOK(c, hipSetDevice(c->device));
    const uint32_t mask = pdwin::wrap_mask(wrap_bits);
    { ProfScope ps(c, "tile_carry"); launch_tile_carry(c->stream, dev_tile_sums, c->bsum, c->carry, (uint32_t)c->n_tiles); }
    { ProfScope ps(c, "slice_sweep");
      TileMap tm{c->d_tile_contig, c->d_off, c->d_len, nullptr};
      launch_sweep_i4(c->stream, dev_parts, n_parts, part_stride, (uint32_t)tile_first, (uint32_t)tile_count, dev_exc, exc_stride,
                      dev_exc_counts, c->slice_flags, slice_flag_bytes(c->n_tiles), c->carry, mask, tm, w, min_dep, (TilePart *)dev_partials, nullptr); }
    HIPOK(c, hipGetLastError());
    return PD_OK;
}

// zlib's level-6 LZ77 parse of a host text on the device (pd_deflate.hip / pd_lz77.h): positions sorted by (hash, position),
// one wave per chunk, the symbols gathered and copied back.  Buffers live for the call.
// A text stream that lives in HBM (include/pandepth_amd.h: pd_text_*): a ring of segments, each one append's bytes, contiguous.
struct pd_text {
    pd_ctx *ctx = nullptr;
    uint8_t *ring = nullptr; size_t cap = 0;
    struct Seg { uint64_t off; size_t phys, len; };
    std::deque<Seg> segs;
    uint64_t tail_off = 0; size_t phys_tail = 0;
    void *scratch = nullptr; size_t scratch_bytes = 0;         // name | block counts | block offsets of an append
    std::mutex mu;
};

// The parse of pd_deflate_parse / pd_text_parse: the text comes from the host (`text`) or from a device stream (`tx`, bytes
// [tx_off, tx_off + n_text)); crc_out (optional): CRC-32 of every chunk's first crc_span bytes.
static int lz_run(pd_ctx *c, const void *text, pd_text *tx, uint64_t tx_off, size_t n_text, const pd_lz_chunk *chunks, uint32_t n_chunks,
                  uint32_t *syms, size_t syms_cap, uint64_t *sym_off, uint32_t *crc_out, uint64_t crc_span)
{
    // The call works on its own stream and its own buffers: the context's lock is held only where the context is touched (its
    // error text, the profile), so that the per-site writer's producer (pd_format_sites on the context's stream) is not kept
    // waiting for the time a round's parse takes.  Two calls run at a time, each in its own slot (buffers + stream).
    const unsigned lz_slot = c->lz_turn.fetch_add(1) & (c->lz_slots >= 4 ? 3u : 1u);
    pd_ctx::LzWork &w = c->lz[lz_slot];
    // "lz_mix": of the two calls a stream keeps in flight, the second parses with its text in memory — a workgroup of the LDS parse fills a CU's
    // LDS, so two LDS parses run one after the other, while a parse from memory shares the CUs with either kind
    const unsigned lz_group = c->lz_mix && (lz_slot & 1u) ? 0u : c->lz_group;
    std::lock_guard<std::mutex> lz_lock(w.mu);
    auto fail = [&](pd_ctx *cc, int code, const std::string &msg) { std::lock_guard<std::mutex> lk(cc->mu); cc->err = msg; return code; };
    if (n_text < 3 || n_text > 0xFFFFFF00ull - 64) return fail(c, PD_EINVAL, "pd_deflate_parse: between 3 and 2^32 - 320 bytes of text");
    uint64_t stride = 0;
    for (uint32_t k = 0; k < n_chunks; ++k) {
        const pd_lz_chunk &ch = chunks[k];
        if (ch.origin > ch.start || ch.start > ch.end || ch.end > n_text || ch.start - ch.origin > 32768)
            return fail(c, PD_EINVAL, "pd_deflate_parse: a chunk lies outside the text or has more than 32768 bytes of history");
        stride = std::max<uint64_t>(stride, ch.end - ch.start);
    }
    sym_off[0] = 0;
    if (!n_chunks) return PD_OK;
    stride += 8;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, PD_EHIP, "pd_deflate_parse: hipSetDevice failed");
    if (!w.st && hipStreamCreateWithFlags(&w.st, hipStreamNonBlocking) != hipSuccess) { w.st = nullptr; return fail(c, PD_EHIP, "pd_deflate_parse: stream creation failed"); }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    const bool prof = c->prof;
    if (prof) for (auto &e : ev) (void)hipEventCreate(&e);
    const bool dbg = getenv("PD_LZ_DEBUG") != nullptr;
    double tm[8] = {}; int ti = 0;
    auto tick = [&]() { if (dbg && ti < 8) tm[ti++] = dec_now_us() * 1e-6; };
    tick();
    const uint32_t np = (uint32_t)(n_text - 2);
    const uint32_t n_blocks = (np + 2047) / 2048;
    // work buffers: kept from call to call (a round of 200 MB of text needs 5 GB of them; allocating and freeing them costs more
    // than the kernels), grown on demand, released by pd_destroy of the context that made them
    const size_t nh = (size_t)256 * n_blocks + 16;
    const size_t want[pd_ctx::LzWork::N] = {n_text + 64, (size_t)np * 8 + 64, (size_t)np * 8 + 64, nh * 4, (nh / 1024 + 8) * 4, (size_t)np * 4 + 64, (size_t)n_text * 4 + 64,
                                    ((size_t)32768 + 8) * 4, (size_t)n_chunks * 24, ((size_t)n_chunks + 1) * 8, (size_t)n_chunks * stride * 4, (size_t)n_chunks * 4 + 16, 0,
                                    (size_t)n_chunks * 4 + 16, (size_t)n_chunks * sizeof(pdk::LzGroup) + 16, (size_t)n_chunks * 4 + 16};
    for (int k = 0; k < pd_ctx::LzWork::N; ++k)
        if (!w.fit(k, want[k])) { (void)hipGetLastError(); return fail(c, PD_ENOMEM, "pd_deflate_parse: device allocation failed"); }
    uint8_t *d_text = (uint8_t *)w.p[0]; uint64_t *ka = (uint64_t *)w.p[1], *kb = (uint64_t *)w.p[2];
    uint32_t *hist = (uint32_t *)w.p[3], *scan_tmp = (uint32_t *)w.p[4], *S = (uint32_t *)w.p[5], *R = (uint32_t *)w.p[6], *bucket = (uint32_t *)w.p[7];
    uint64_t *d_chunks = (uint64_t *)w.p[8], *d_off = (uint64_t *)w.p[9]; uint32_t *d_syms = (uint32_t *)w.p[10], *d_cnt = (uint32_t *)w.p[11], *d_crc = (uint32_t *)w.p[13];
    auto cleanup = [&]() { for (auto &x : ev) if (x) { (void)hipEventDestroy(x); x = nullptr; } };
    // Consecutive chunks whose text — the first one's history up to the last one's end — fits a CU's LDS parse as one workgroup
    // (pd_deflate.hip: k_lz_parse_lds).  A chunk qualifies when its history is zlib's whole window or begins with the text: its
    // candidates (nearer than 32 506 bytes) then lie inside what the group holds.  The others parse with the text in memory.
    std::vector<pdk::LzGroup> groups;
    std::vector<uint32_t> loose;
    uint32_t group_waves = 0; size_t lds_bytes = 0;
    {
        int lds_max = 0;
        if (lz_group == 0 || hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) != hipSuccess) { (void)hipGetLastError(); lds_max = 0; }
        if (lds_max > (int)pdk::LZ_LDS_MAX) lds_max = (int)pdk::LZ_LDS_MAX;
        if (lds_max > 0 && !pdk::lz_parse_lds_ready((size_t)lds_max)) lds_max = 0;
        auto fits = [&](const pd_lz_chunk &ch) { return ch.origin == 0 || ch.start - ch.origin == 32768; };
        uint32_t k = 0;
        while (k < n_chunks) {
            const uint64_t base = chunks[k].origin;
            uint32_t count = 0; uint64_t hi = 0, len = 0;
            for (uint32_t j = k; lds_max > 0 && j < n_chunks && count < lz_group && fits(chunks[j]) && chunks[j].origin >= base; ++j) {
                const uint64_t nhi = std::max<uint64_t>(hi, chunks[j].end);
                const uint64_t nlen = std::min<uint64_t>(nhi + pdk::LZ_LDS_SLACK, (uint64_t)n_text + 32) - base;
                if ((base & 15) + nlen + 16 > (uint64_t)lds_max) break;
                hi = nhi; len = nlen; ++count;
            }
            if (!count) { loose.push_back(k); ++k; continue; }
            groups.push_back(pdk::LzGroup{k, count, base, len});
            group_waves = std::max(group_waves, count);
            lds_bytes = std::max<size_t>(lds_bytes, (size_t)(((base & 15) + len + 15) & ~(uint64_t)15));
            k += count;
        }
    }
    pdk::LzGroup *d_groups = (pdk::LzGroup *)w.p[14]; uint32_t *d_loose = (uint32_t *)w.p[15];
    tick();
    hipStream_t st = w.st;
    std::vector<uint32_t> counts(n_chunks);
    hipError_t e = hipMemsetAsync(d_text + n_text, 0, 64, st);
    if (tx) {
        // the stretch, segment by segment (the segments stay where they are until the caller releases them).  The stream's lock is
        // released before anything is reported: fail() takes the context's lock, and the append paths take the two in the other order.
        uint64_t got = 0;
        {
            std::lock_guard<std::mutex> tlk(tx->mu);
            for (const auto &sg : tx->segs) {
                const uint64_t lo = std::max<uint64_t>(sg.off, tx_off), hi = std::min<uint64_t>(sg.off + sg.len, tx_off + n_text);
                if (lo >= hi) continue;
                if (e == hipSuccess) e = hipMemcpyAsync(d_text + (lo - tx_off), tx->ring + sg.phys + (lo - sg.off), (size_t)(hi - lo), hipMemcpyDeviceToDevice, st);
                got += hi - lo;
            }
        }
        if (got != n_text) { (void)hipStreamSynchronize(st); cleanup(); return fail(c, PD_EINVAL, "pd_text_parse: the stretch is not (or no longer) in the stream"); }
    } else if (e == hipSuccess) e = hipMemcpyAsync(d_text, text, n_text, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_chunks, chunks, (size_t)n_chunks * 24, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !groups.empty()) e = hipMemcpyAsync(d_groups, groups.data(), groups.size() * sizeof(pdk::LzGroup), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !loose.empty()) e = hipMemcpyAsync(d_loose, loose.data(), loose.size() * 4, hipMemcpyHostToDevice, st);
    static_assert(sizeof(pd_lz_chunk) == 24, "pd_lz_chunk layout");
    if (dbg && e == hipSuccess) e = hipStreamSynchronize(st);
    tick();
    if (e == hipSuccess) {
        if (prof) (void)hipEventRecord(ev[0], st);
        launch_lz_sort(st, d_text, np, ka, kb, hist, scan_tmp, S, R, bucket);
        if (prof) (void)hipEventRecord(ev[1], st);
        if (dbg) { (void)hipStreamSynchronize(st); tick(); }
        launch_lz_parse(st, d_text, n_text, S, R, bucket, d_chunks, d_groups, (uint32_t)groups.size(), group_waves, lds_bytes, d_loose, (uint32_t)loose.size(), d_syms, stride, d_cnt);
        if (prof) (void)hipEventRecord(ev[2], st);
        if (crc_out) launch_lz_crc(st, d_text, d_chunks, n_chunks, crc_span, d_crc);
        e = hipGetLastError();
    }
    if (e == hipSuccess && crc_out) e = hipMemcpyAsync(crc_out, d_crc, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), d_cnt, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { cleanup(); return fail(c, PD_EHIP, std::string("pd_deflate_parse: ") + hipGetErrorString(e)); }
    tick();
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_chunks; ++k) {
        if (counts[k] == 0xFFFFFFFFu) { cleanup(); return fail(c, PD_EHIP, "pd_deflate_parse: a chunk's symbols did not fit its buffer"); }
        total += counts[k]; sym_off[k + 1] = total;
    }
    if (total > syms_cap) { cleanup(); return fail(c, PD_ERANGE, "pd_deflate_parse: the symbol buffer is too small"); }
    if (total) {
        if (!w.fit(12, total * 4 + 64)) { (void)hipGetLastError(); cleanup(); return fail(c, PD_ENOMEM, "pd_deflate_parse: device allocation failed"); }
        uint32_t *d_out = (uint32_t *)w.p[12];
        e = hipMemcpyAsync(d_off, sym_off, ((size_t)n_chunks + 1) * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) { launch_lz_gather(st, d_syms, stride, d_off, n_chunks, d_out); e = hipGetLastError(); }
        if (dbg && e == hipSuccess) { e = hipStreamSynchronize(st); tick(); }
        // the symbols come back through a page-locked buffer of the slot, in pieces, and are copied on from there: a large copy
        // straight into the caller's pageable memory makes the runtime lock and unlock those pages around it
        const size_t PIECE = (size_t)8 << 20;                        // bytes
        if (!w.h_stage && hipHostMalloc(&w.h_stage, 2 * PIECE, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); w.h_stage = nullptr; }
        if (w.h_stage && getenv("PD_LZ_DIRECT_COPY") == nullptr) {
            if (!w.ev_stage[0]) { (void)hipEventCreateWithFlags(&w.ev_stage[0], hipEventDisableTiming); (void)hipEventCreateWithFlags(&w.ev_stage[1], hipEventDisableTiming); }
            const size_t bytes = total * 4;
            const size_t n_pieces = (bytes + PIECE - 1) / PIECE;
            // piece k is on the wire while piece k - 1 is copied out of the other half of the buffer
            for (size_t k = 0; k <= n_pieces && e == hipSuccess; ++k) {
                if (k < n_pieces) {
                    const size_t off = k * PIECE, n = std::min(PIECE, bytes - off);
                    e = hipMemcpyAsync((uint8_t *)w.h_stage + (k & 1) * PIECE, (const uint8_t *)d_out + off, n, hipMemcpyDeviceToHost, st);
                    if (e == hipSuccess) e = hipEventRecord(w.ev_stage[k & 1], st);
                }
                if (k > 0 && e == hipSuccess) {
                    const size_t off = (k - 1) * PIECE, n = std::min(PIECE, bytes - off);
                    e = hipEventSynchronize(w.ev_stage[(k - 1) & 1]);
                    if (e == hipSuccess) memcpy((uint8_t *)syms + off, (const uint8_t *)w.h_stage + ((k - 1) & 1) * PIECE, n);
                }
            }
        } else {
            if (e == hipSuccess) e = hipMemcpyAsync(syms, d_out, total * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
    }
    tick();
    if (dbg && ti >= 7)
        fprintf(stderr, "[lz] %zu groups of up to %u chunks with their text in LDS (%zu bytes a workgroup), %zu chunks with the text in memory\n", groups.size(), group_waves, lds_bytes, loose.size());
    if (dbg && ti >= 7)
        fprintf(stderr, "[lz] %.1f MB, %u chunks, %.1f M symbols: buffers %.4f, text to the device %.4f, sort %.4f, parse %.4f, gather %.4f, symbols back %.4f s\n", n_text / 1e6,
                n_chunks, total / 1e6, tm[1] - tm[0], tm[2] - tm[1], tm[3] - tm[2], tm[4] - tm[3], tm[5] - tm[4], tm[6] - tm[5]);
    if (prof) {
        float a = 0, b = 0;
        if (e == hipSuccess && hipEventElapsedTime(&a, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev[1], ev[2]) == hipSuccess) {
            std::lock_guard<std::mutex> lk(c->mu);
            auto &s1 = c->prof_acc["lz_sort"]; s1.first += a; s1.second += 1;
            auto &s2 = c->prof_acc["lz_parse"]; s2.first += b; s2.second += 1;
        }
    }
    cleanup();
    if (e != hipSuccess) return fail(c, PD_EHIP, std::string("pd_deflate_parse: ") + hipGetErrorString(e));
    return PD_OK;
}

int pd_deflate_parse(pd_ctx *c, const void *text, size_t n_text, const pd_lz_chunk *chunks, uint32_t n_chunks,
                     uint32_t *syms, size_t syms_cap, uint64_t *sym_off)
{
    if (!c || !text || !chunks || !syms || !sym_off) return PD_EINVAL;
    return lz_run(c, text, nullptr, 0, n_text, chunks, n_chunks, syms, syms_cap, sym_off, nullptr, 0);
}

// (the callers hold the context's lock)
static int text_scratch(pd_text *t, size_t bytes)
{
    pd_ctx *c = t->ctx;
    if (t->scratch_bytes >= bytes) return PD_OK;
    if (t->scratch) { HIPOK(c, hipStreamSynchronize(c->stream)); HIPOK(c, hipFree(t->scratch)); t->scratch = nullptr; t->scratch_bytes = 0; }
    const size_t want = bytes * 2;
    if (hipMalloc(&t->scratch, want) != hipSuccess) { (void)hipGetLastError(); return fail(c, PD_ENOMEM, "pd_text: device allocation failed"); }
    t->scratch_bytes = want;
    return PD_OK;
}
// a place for `total` bytes in the ring: behind the last segment, or at the ring's start once that end is free again
static int text_place(pd_text *t, uint64_t total, size_t *phys, const char *who)
{
    pd_ctx *c = t->ctx;
    std::lock_guard<std::mutex> tlk(t->mu);
    if (total > t->cap) return fail(c, PD_EINVAL, std::string(who) + ": more bytes than the stream's capacity");
    if (t->segs.empty()) { t->phys_tail = 0; *phys = 0; return PD_OK; }
    const size_t head = t->segs.front().phys;
    if (t->phys_tail >= head) {                                // live bytes in [head, tail)
        if (t->phys_tail + total <= t->cap) { *phys = t->phys_tail; return PD_OK; }
        if (total < head) { *phys = 0; return PD_OK; }
    } else if (t->phys_tail + total < head) { *phys = t->phys_tail; return PD_OK; }   // wrapped: live bytes in [head, ...) and [0, tail)
    return fail(c, PD_ERANGE, std::string(who) + ": the stream is full (release what has been consumed)");
}
static void text_commit(pd_text *t, size_t phys, uint64_t total)
{
    std::lock_guard<std::mutex> tlk(t->mu);
    t->segs.push_back(pd_text::Seg{t->tail_off, phys, (size_t)total});
    t->tail_off += total; t->phys_tail = phys + (size_t)total;
}

// ---- a text stream in HBM: the per-site rows are formatted, parsed and check-summed where the cells are ----
int pd_text_open(pd_ctx *c, size_t capacity, pd_text **out)
{
    if (!c || !out || capacity < ((size_t)1 << 20)) return PD_EINVAL;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPOK(c, hipSetDevice(c->device));
    pd_text *t = new pd_text;
    t->ctx = c; t->cap = capacity;
    if (hipMalloc(&t->ring, capacity + 64) != hipSuccess) { (void)hipGetLastError(); delete t; return fail(c, PD_ENOMEM, "pd_text_open: device allocation failed"); }
    *out = t;
    return PD_OK;
}

int pd_text_close(pd_text *t)
{
    if (!t) return PD_OK;
    pd_ctx *c = t->ctx;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        (void)hipSetDevice(c->device);
        for (auto &w : c->lz) { std::lock_guard<std::mutex> g(w.mu); if (w.st) (void)hipStreamSynchronize(w.st); }
        (void)hipStreamSynchronize(c->stream);
        if (t->ring) (void)hipFree(t->ring);
        if (t->scratch) (void)hipFree(t->scratch);
    }
    delete t;
    return PD_OK;
}

int pd_text_append_sites(pd_text *t, int32_t tid, uint32_t beg, size_t n, const char *name, size_t name_len, uint64_t *n_bytes)
{
    if (!t || !n_bytes || (!name && name_len)) return PD_EINVAL;
    *n_bytes = 0;
    pd_ctx *c = t->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_text_append_sites")) return rs;
    if (tid < 0 || tid >= c->n_contigs) return fail(c, PD_EINVAL, "pd_text_append_sites: contig id out of range");
    if ((uint64_t)beg + n > c->off[tid + 1] - c->off[tid]) return fail(c, PD_EINVAL, "pd_text_append_sites: range past the contig slot");
    if (name_len > 4096 || n > ((size_t)1 << 27)) return fail(c, PD_EINVAL, "pd_text_append_sites: at most 2^27 cells per call and 4096 bytes of name");
    if (n == 0) return PD_OK;
    HIPOK(c, hipSetDevice(c->device));
    const uint32_t nb = pdk::site_rows_blocks(n);
    const size_t b_name = (name_len + 15) / 16 * 16 + 16, b_cnt = ((size_t)nb * 4 + 15) / 16 * 16, b_off = ((size_t)nb + 1) * 8;
    if (int rs = text_scratch(t, b_name + b_cnt + b_off)) return rs;
    unsigned char *s = (unsigned char *)t->scratch;
    char *d_name = (char *)s; uint32_t *d_cnt = (uint32_t *)(s + b_name); uint64_t *d_off = (uint64_t *)(s + b_name + b_cnt);
    ProfScope ps(c, "format_sites");
    if (name_len) HIPOK(c, hipMemcpyAsync(d_name, name, name_len, hipMemcpyHostToDevice, c->stream));
    const uint32_t *depth = (const uint32_t *)(c->buf + c->off[tid] + beg);
    // pass 1: the rows' lengths and where each workgroup's rows begin
    pdk::launch_site_rows(c->stream, depth, beg, n, (uint32_t)name_len, d_name, d_cnt, d_off, nullptr, false);
    uint64_t total = 0;
    HIPOK(c, hipMemcpyAsync(&total, d_off + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    HIPOK(c, hipGetLastError());
    size_t phys = 0;
    if (int rp = text_place(t, total, &phys, "pd_text_append_sites")) return rp;
    // pass 2: the bytes
    pdk::launch_site_rows(c->stream, depth, beg, n, (uint32_t)name_len, d_name, d_cnt, d_off, (char *)t->ring + phys, true);
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipStreamSynchronize(c->stream));
    text_commit(t, phys, total);
    *n_bytes = total;
    return PD_OK;
}

int pd_text_append_window_rows(pd_text *t, int32_t tid, uint32_t w, uint64_t row_first, size_t n_rows, const char *name, size_t name_len, uint64_t *n_bytes)
{
    if (!t || !n_bytes || (!name && name_len) || !w) return PD_EINVAL;
    *n_bytes = 0;
    pd_ctx *c = t->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->win.valid || c->win.w != w) return fail(c, PD_ESTATE, "pd_text_append_window_rows: the last window call (pd_scan_reduce_windows / pd_reduce_windows) was not for this width");
    if (tid < 0 || tid >= c->n_contigs) return fail(c, PD_EINVAL, "pd_text_append_window_rows: contig id out of range");
    const uint64_t rows_here = c->win.n_rows(tid);
    if (row_first > rows_here || n_rows > rows_here - row_first) return fail(c, PD_EINVAL, "pd_text_append_window_rows: rows beyond the contig's windows");
    if (name_len > 4096 || n_rows > ((size_t)1 << 27)) return fail(c, PD_EINVAL, "pd_text_append_window_rows: at most 2^27 rows per call and 4096 bytes of name");
    if (n_rows == 0) return PD_OK;
    HIPOK(c, hipSetDevice(c->device));
    const uint32_t nb = pdk::window_rows_blocks(n_rows);
    const size_t b_name = (name_len + 15) / 16 * 16 + 16, b_cnt = ((size_t)nb * 4 + 15) / 16 * 16, b_off = ((size_t)nb + 1) * 8;
    if (int rs = text_scratch(t, b_name + b_cnt + b_off)) return rs;
    unsigned char *s = (unsigned char *)t->scratch;
    char *d_name = (char *)s; uint32_t *d_cnt = (uint32_t *)(s + b_name); uint64_t *d_off = (uint64_t *)(s + b_name + b_cnt);
    ProfScope ps(c, "format_window_rows");
    if (name_len) HIPOK(c, hipMemcpyAsync(d_name, name, name_len, hipMemcpyHostToDevice, c->stream));
    const unsigned long long *d_sum = nullptr; const uint32_t *d_cov = nullptr;
    c->win.rows(tid, row_first, &d_sum, &d_cov);
    pdk::launch_window_rows(c->stream, d_cov, d_sum, row_first, n_rows, w, c->len[(size_t)tid], (uint32_t)name_len, d_name, d_cnt, d_off, nullptr, false);
    uint64_t total = 0;
    HIPOK(c, hipMemcpyAsync(&total, d_off + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    HIPOK(c, hipGetLastError());
    size_t phys = 0;
    if (int rp = text_place(t, total, &phys, "pd_text_append_window_rows")) return rp;
    pdk::launch_window_rows(c->stream, d_cov, d_sum, row_first, n_rows, w, c->len[(size_t)tid], (uint32_t)name_len, d_name, d_cnt, d_off, (char *)t->ring + phys, true);
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipStreamSynchronize(c->stream));
    text_commit(t, phys, total);
    *n_bytes = total;
    return PD_OK;
}

int pd_text_append_bytes(pd_text *t, const void *bytes, size_t n)
{
    if (!t || (!bytes && n)) return PD_EINVAL;
    if (!n) return PD_OK;
    pd_ctx *c = t->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPOK(c, hipSetDevice(c->device));
    size_t phys = 0;
    if (int rp = text_place(t, n, &phys, "pd_text_append_bytes")) return rp;
    HIPOK(c, hipMemcpyAsync(t->ring + phys, bytes, n, hipMemcpyHostToDevice, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    text_commit(t, phys, n);
    return PD_OK;
}

int pd_text_parse(pd_text *t, uint64_t off, size_t n_text, const pd_lz_chunk *chunks, uint32_t n_chunks, uint32_t *syms, size_t syms_cap,
                  uint64_t *sym_off, uint32_t *crc, uint64_t crc_span)
{
    if (!t || !chunks || !syms || !sym_off) return PD_EINVAL;
    return lz_run(t->ctx, nullptr, t, off, n_text, chunks, n_chunks, syms, syms_cap, sym_off, crc, crc_span);
}

int pd_text_read(pd_text *t, uint64_t off, size_t n, void *out)
{
    if (!t || (!out && n)) return PD_EINVAL;
    pd_ctx *c = t->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPOK(c, hipSetDevice(c->device));
    std::lock_guard<std::mutex> tlk(t->mu);
    uint64_t got = 0;
    for (const auto &sg : t->segs) {
        const uint64_t lo = std::max<uint64_t>(sg.off, off), hi = std::min<uint64_t>(sg.off + sg.len, off + n);
        if (lo >= hi) continue;
        HIPOK(c, hipMemcpyAsync((uint8_t *)out + (lo - off), t->ring + sg.phys + (lo - sg.off), (size_t)(hi - lo), hipMemcpyDeviceToHost, c->stream));
        got += hi - lo;
    }
    HIPOK(c, hipStreamSynchronize(c->stream));
    if (got != n) return fail(c, PD_EINVAL, "pd_text_read: the stretch is not (or no longer) in the stream");
    return PD_OK;
}

int pd_text_release(pd_text *t, uint64_t off)
{
    if (!t) return PD_EINVAL;
    std::lock_guard<std::mutex> tlk(t->mu);
    while (!t->segs.empty() && t->segs.front().off + t->segs.front().len <= off) t->segs.pop_front();
    return PD_OK;
}

int pd_host_register(pd_ctx *c, void *ptr, size_t bytes)
{
    if (!c || !ptr || !bytes) return PD_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess || hipHostRegister(ptr, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(c->mu);
        return fail(c, PD_EHIP, "pd_host_register: hipHostRegister failed");
    }
    return PD_OK;
}

int pd_host_unregister(pd_ctx *c, void *ptr)
{
    if (!c || !ptr) return PD_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess || hipHostUnregister(ptr) != hipSuccess) {
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(c->mu);
        return fail(c, PD_EHIP, "pd_host_unregister: hipHostUnregister failed");
    }
    return PD_OK;
}

void *pd_stream(pd_ctx *c) { return c ? (void *)c->stream : nullptr; }

int pd_synchronize(pd_ctx *c)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPOK(c, hipSetDevice(c->device));
    // a whole deferred sample in an otherwise empty context stays deferred when the direct window path may still take it
    const bool keep_deferred = c->direct_windows && c->pristine && !c->pend.empty() && c->state == 0;
    int rc = keep_deferred ? PD_OK : flush_pending(c);
    if (rc) return rc;
    if (c->copy_stream) HIPOK(c, hipStreamSynchronize(c->copy_stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    return PD_OK;
}

int pd_profile(pd_ctx *c, int enable)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPOK(c, hipSetDevice(c->device));
    int rc = prof_collect(c);
    c->prof_acc.clear();
    c->prof = enable != 0;
    return rc;
}

int pd_profile_get(pd_ctx *c, const char *name, double *ms, uint64_t *launches)
{
    if (!c || !name) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPOK(c, hipSetDevice(c->device));
    int rc = prof_collect(c);
    if (rc) return rc;
    {   // the decode session's counters (launches only; counted whether or not profiling is on)
        static const struct { const char *name; int k; } dn[] = {
            {"decode_c8_grow", pd_ctx::DN_GROW}, {"decode_end_compact", pd_ctx::DN_END_COMPACT}, {"decode_end_c8_fallback", pd_ctx::DN_END_C8_FALLBACK},
            {"decode_end_runs_make", pd_ctx::DN_END_RUNS_MAKE}, {"decode_end_scatter", pd_ctx::DN_END_SCATTER}, {"decode_end_unsorted", pd_ctx::DN_END_UNSORTED},
            {"decode_end_pending", pd_ctx::DN_END_PEND}, {"decode_guess_units", pd_ctx::DN_GUESS}};
        uint64_t v = 0; bool hit = false;
        for (auto &d : dn) if (!strcmp(name, d.name)) { v = c->dec_n[d.k].load(); hit = true; }
        if (!strcmp(name, "direct_cover_narrow")) { v = c->direct_narrow; hit = true; }       // 1: the last direct window call's k_direct_c8 swept the narrow plane
        if (!strcmp(name, "direct_cover_fast")) { v = c->direct_fast; hit = true; }           // chunks of the last direct window call that the narrow sweep accepted as fast chunks
        if (!strcmp(name, "direct_cover_settled")) { v = c->direct_settled; hit = true; }     // tiles of the last direct window call that k_direct_c8 settled without a window
        if (!strcmp(name, "direct_pileup_tiles")) { v = c->direct_pileup; hit = true; }       // ... and the tiles it left to the pile-up pass (k_c8_heavy)
        if (!strcmp(name, "decode_chain_device")) { v = c->dec_n_fast.load(); hit = true; }
        if (!strcmp(name, "decode_chain_host")) { v = c->dec_n_slow.load(); hit = true; }
        if (!strcmp(name, "decode_segments_redone")) { v = c->dec_n_redo.load(); hit = true; }
        if (!strcmp(name, "decode_record_stats")) {                                             // k_record_stats: launches of the last session, and their time where its batches were timed
            if (ms) *ms = (double)c->rs_ns.load() / 1e6;
            if (launches) *launches = c->rs_launches.load();
            return PD_OK;
        }
        if (!strcmp(name, "decode_row_counts")) {                                               // k_row_counts, likewise
            if (ms) *ms = (double)c->rc_ns.load() / 1e6;
            if (launches) *launches = c->rc_launches.load();
            return PD_OK;
        }
        if (!strcmp(name, "decode_aln_stats")) {                                                // k_aln_stats, likewise
            if (ms) *ms = (double)c->as_ns.load() / 1e6;
            if (launches) *launches = c->as_launches.load();
            return PD_OK;
        }
        if (hit) { if (ms) *ms = 0.0; if (launches) *launches = v; return PD_OK; }
    }
    auto it = c->prof_acc.find(name);
    if (ms) *ms = it == c->prof_acc.end() ? 0.0 : it->second.first;
    if (launches) *launches = it == c->prof_acc.end() ? 0 : it->second.second;
    return PD_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Multi-sample sum over several GPUs with RCCL called from here (include/pandepth_amd.h: pd_comm_*, pd_sliced_window_sum):
// the C++ form of pandepth_amd/multi.py's SlicedSum, for the CLI's `#.list` mode and for any host that is not Python.
// ---------------------------------------------------------------------------------------------------------------
namespace { struct Rccl; }
struct pd_comm {
    pd_ctx *ctx = nullptr;
    const Rccl *tp = nullptr;                     // the transport's entry points: librccl's (between processes) or the in-process peer-copy one
    ncclComm_t nccl = nullptr;
    int rank = 0, world = 1;
    uint64_t n_tiles = 0, slice_tiles = 0, slice_bytes = 0, tile_first = 0, tile_count = 0, n_sums = 0;
    // two slots of exchange buffers: sample k+1 is scattered and packed while sample k's image is on the links
    struct Slot {
        uint8_t *send = nullptr, *recv = nullptr;
        int32_t *meta = nullptr;                  // tile sums | exception counts per rank
        pd_exc *exc = nullptr, *exc_all = nullptr;
        uint32_t *count = nullptr;
        hipEvent_t packed = nullptr, landed = nullptr;
        bool busy = false;
    } slot[2];
    uint8_t *part_mine = nullptr, *part_all = nullptr;
    int *slice_depth = nullptr;                   // the summed depth of this rank's slice (narrow windows, intervals), made on demand
    hipStream_t links = nullptr;                  // every RCCL call is issued on this stream, ordered against the context's by events
    hipEvent_t swept = nullptr, gathered = nullptr;
    std::string err;
};

namespace {
// RCCL is loaded on first use (dlopen): librccl.so is half a gigabyte of code objects that a single-GPU run never needs,
// and the executable's start-up time is part of its end-to-end figure.
struct Rccl {
    void *h = nullptr;
    decltype(&::ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&::ncclCommInitRank) CommInitRank = nullptr;
    decltype(&::ncclCommInitAll) CommInitAll = nullptr;
    decltype(&::ncclCommDestroy) CommDestroy = nullptr;
    decltype(&::ncclGroupStart) GroupStart = nullptr;
    decltype(&::ncclGroupEnd) GroupEnd = nullptr;
    decltype(&::ncclSend) Send = nullptr;
    decltype(&::ncclRecv) Recv = nullptr;
    decltype(&::ncclAllReduce) AllReduce = nullptr;
    decltype(&::ncclAllGather) AllGather = nullptr;
    decltype(&::ncclGetErrorString) GetErrorString = nullptr;
    bool ok = false, alt = false;
};
Rccl &rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        // PANDEPTH_RCCL_LIB names another library with RCCL's entry points (tests: a loopback transport between contexts that
        // share one GPU, tests/harness/loopback_nccl.hip — the only way to run N > 1 ranks of this code on a 1-GPU box)
        if (const char *alt = getenv("PANDEPTH_RCCL_LIB")) { if (alt[0]) r.h = dlopen(alt, RTLD_NOW | RTLD_LOCAL); if (r.h) r.alt = true; }
        if (!r.h) for (const char *p : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) if ((r.h = dlopen(p, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!r.h) return;
#define PD_SYM(name) r.name = (decltype(r.name))dlsym(r.h, "nccl" #name)
        PD_SYM(GetUniqueId); PD_SYM(CommInitRank); PD_SYM(CommInitAll); PD_SYM(CommDestroy); PD_SYM(GroupStart); PD_SYM(GroupEnd);
        PD_SYM(Send); PD_SYM(Recv); PD_SYM(AllReduce); PD_SYM(AllGather); PD_SYM(GetErrorString);
#undef PD_SYM
        r.ok = r.GetUniqueId && r.CommInitRank && r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.AllReduce &&
               r.AllGather && r.GetErrorString;
    });
    return r;
}
// (RCCL 2.27 prints a version banner on stdout when the first communicator is made, whatever NCCL_DEBUG says.  The library leaves
// descriptor 1 alone — until round 6 it pointed it at /dev/null meanwhile, which in a multi-threaded process can eat somebody else's
// line; a caller whose stdout is a contract keeps its own lines on a descriptor of its own: host/pipeline.cpp, OwnStdout.)
//
// The in-process transport (pd_local_comm.h) behind the same table: pd_comm_init_local.
Rccl &local_tp()
{
    static Rccl r = [] {
        Rccl t;
        t.CommInitAll = pdlocal::CommInitAll; t.CommDestroy = pdlocal::CommDestroy; t.GroupStart = pdlocal::GroupStart; t.GroupEnd = pdlocal::GroupEnd;
        t.Send = pdlocal::Send; t.Recv = pdlocal::Recv; t.AllReduce = pdlocal::AllReduce; t.AllGather = pdlocal::AllGather; t.GetErrorString = pdlocal::GetErrorString;
        t.ok = true; t.alt = true;                 // (alt: ranks may share a device)
        return t;
    }();
    return r;
}
// Communicators made ahead of their contexts (pd_comm_preinit): ncclCommInitAll wants device numbers only, and a short-lived process
// wants librccl's load and bootstrap over BEFORE its contexts load code objects and its readers launch kernels (see pd_comm_preinit).
struct ParkedComms { std::mutex mu; std::vector<int> devs; std::vector<ncclComm_t> nc; } g_parked;
constexpr uint32_t COMM_EXC_BLOCK = 1u << 18;       // exceptions (cells outside the 4-bit range) per rank
constexpr size_t COMM_MSG_BYTES = (size_t)1 << 28;  // RCCL 2.26 delivers only the first half of a send/recv above 1 GiB: stay far below

int comm_fail(pd_comm *m, int code, const std::string &msg) { m->err = msg; if (m->ctx) { std::lock_guard<std::mutex> lk(m->ctx->mu); m->ctx->err = msg; } return code; }
#define NCCLOK(m, call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) return comm_fail(m, PD_EHIP, std::string(#call) + ": " + (m)->tp->GetErrorString(r_)); } while (0)
#define HIPCM(m, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return comm_fail(m, PD_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// a slot's exchange buffers, on first use (the calling rank's thread; its device is current)
int slot_setup(pd_comm *m, pd_comm::Slot &s)
{
    if (s.send) return PD_OK;
    pd_ctx *c = m->ctx;
    const size_t W = (size_t)m->world, img = (size_t)(c->n_cells / 2), all = W * (size_t)m->slice_bytes + 256;
    // one rank: nothing is received — the "received" slices are the image itself
    if (hipMalloc(&s.send, all) != hipSuccess || (W > 1 && hipMalloc(&s.recv, all) != hipSuccess) ||
        hipMalloc(&s.meta, (m->n_sums + W + 16) * 4) != hipSuccess || hipMalloc(&s.exc, (size_t)COMM_EXC_BLOCK * sizeof(pd_exc)) != hipSuccess ||
        hipMalloc(&s.exc_all, W * COMM_EXC_BLOCK * sizeof(pd_exc)) != hipSuccess || hipMalloc(&s.count, 64) != hipSuccess) {
        (void)hipGetLastError();
        return comm_fail(m, PD_ENOMEM, "pd_comm: buffer allocation failed");
    }
    if (W == 1) s.recv = s.send;
    HIPCM(m, hipEventCreateWithFlags(&s.packed, hipEventDisableTiming));
    HIPCM(m, hipEventCreateWithFlags(&s.landed, hipEventDisableTiming));
    // (the export writes every byte of the image every time: only the padding behind it — the last slice's tail — must be, and stay, zero)
    if (all > img) HIPCM(m, hipMemsetAsync(s.send + img, 0, all - img, c->stream));
    HIPCM(m, hipMemsetAsync(s.exc, 0, (size_t)COMM_EXC_BLOCK * sizeof(pd_exc), c->stream));
    return PD_OK;
}

int comm_setup(pd_comm *m)
{
    pd_ctx *c = m->ctx;
    m->n_tiles = c->n_tiles; m->n_sums = c->n_words - c->n_cells;
    m->slice_tiles = std::max<uint64_t>(1, (m->n_tiles + (uint64_t)m->world - 1) / (uint64_t)m->world);
    m->slice_bytes = m->slice_tiles * (PD_TILE / 2);
    m->tile_first = std::min<uint64_t>((uint64_t)m->rank * m->slice_tiles, m->n_tiles);
    m->tile_count = std::min<uint64_t>(m->slice_tiles, m->n_tiles - m->tile_first);
    const size_t W = (size_t)m->world;
    HIPCM(m, hipSetDevice(c->device));
    HIPCM(m, hipStreamCreateWithFlags(&m->links, hipStreamNonBlocking));
    HIPCM(m, hipEventCreateWithFlags(&m->swept, hipEventDisableTiming));
    HIPCM(m, hipEventCreateWithFlags(&m->gathered, hipEventDisableTiming));
    // (the slots' exchange buffers — twice the 4-bit image per slot, 3 GB for a 3 Gb genome — are made by the first pd_sliced_sum_start that
    // uses the slot: a device allocation of that size costs tenths of a second, and the executable only ever uses slot 0)
    if (hipMalloc(&m->part_mine, m->slice_tiles * PD_TILE_PARTIAL_BYTES + 64) != hipSuccess ||
        hipMalloc(&m->part_all, W * m->slice_tiles * PD_TILE_PARTIAL_BYTES + 64) != hipSuccess)
        return comm_fail(m, PD_ENOMEM, "pd_comm: buffer allocation failed");
    HIPCM(m, hipMemsetAsync(m->part_mine, 0, m->slice_tiles * PD_TILE_PARTIAL_BYTES + 64, c->stream));
    HIPCM(m, hipStreamSynchronize(c->stream));
    return PD_OK;
}
} // namespace

extern "C" {

int pd_comm_unique_id(void *id128)
{
    if (!id128) return PD_EINVAL;
    if (!rccl().ok) return PD_ENODEV;
    ncclUniqueId id;
    if (rccl().GetUniqueId(&id) != ncclSuccess) return PD_EHIP;
    static_assert(sizeof(id) == PD_UNIQUE_ID_BYTES, "unique id size");
    memcpy(id128, &id, sizeof id);
    return PD_OK;
}

int pd_comm_init(pd_ctx *ctx, const void *id128, int rank, int n_ranks, pd_comm **out)
{
    if (!ctx || !id128 || !out || rank < 0 || rank >= n_ranks) return PD_EINVAL;
    *out = nullptr;
    if (!rccl().ok) { std::lock_guard<std::mutex> lk(ctx->mu); ctx->err = "pd_comm_init: librccl.so.1 cannot be loaded"; return PD_ENODEV; }
    pd_comm *m = new pd_comm; m->ctx = ctx; m->tp = &rccl(); m->rank = rank; m->world = n_ranks;
    ncclUniqueId id; memcpy(&id, id128, sizeof id);
    const bool made = hipSetDevice(ctx->device) == hipSuccess && rccl().CommInitRank(&m->nccl, n_ranks, id, rank) == ncclSuccess;
    if (!made) {
        { std::lock_guard<std::mutex> lk(ctx->mu); ctx->err = "pd_comm_init: ncclCommInitRank failed"; }
        delete m; return PD_EHIP;
    }
    const int rc = comm_setup(m);
    if (rc) { pd_comm_destroy(m); return rc; }
    *out = m;
    return PD_OK;
}

// librccl loaded and an n-rank communicator bootstrapped over `devices` NOW, before any context exists; the next pd_comm_init_all
// over contexts on exactly these devices adopts it.  For a short-lived process: the load registers half a gigabyte of code objects
// under the runtime lock every kernel launch needs, so behind a running decode it costs the decode (profiles/r05_comm_init.txt:
// 0.68 -> 2.19 s); ahead of pd_create it overlaps header and index reads and slows nothing down.  devices == NULL: load only.
int pd_comm_preinit(const int *devices, int n)
{
    if (!rccl().ok) return PD_ENODEV;
    if (!devices || n < 1) return PD_OK;
    std::vector<int> devs(devices, devices + n);
    if (!rccl().alt)
        for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) if (devs[(size_t)i] == devs[(size_t)j]) return PD_EINVAL;
    std::vector<ncclComm_t> nc((size_t)n, nullptr);
    if (rccl().CommInitAll(nc.data(), n, devs.data()) != ncclSuccess) return PD_EHIP;
    std::lock_guard<std::mutex> lk(g_parked.mu);
    for (ncclComm_t old : g_parked.nc) if (old) (void)rccl().CommDestroy(old);         // (made, never adopted)
    g_parked.devs = devs; g_parked.nc = nc;
    return PD_OK;
}

static int comm_init_over(Rccl &tp, const char *what, pd_ctx **ctxs, int n, pd_comm **comms)
{
    if (!ctxs || !comms || n < 1) return PD_EINVAL;
    std::vector<int> devs((size_t)n);
    for (int i = 0; i < n; ++i) { if (!ctxs[i]) return PD_EINVAL; devs[(size_t)i] = ctxs[i]->device; comms[i] = nullptr; }
    if (!tp.ok) { std::lock_guard<std::mutex> lk(ctxs[0]->mu); ctxs[0]->err = std::string(what) + ": librccl.so.1 cannot be loaded"; return PD_ENODEV; }
    if (!tp.alt)
        for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) if (devs[(size_t)i] == devs[(size_t)j]) {
            std::lock_guard<std::mutex> lk(ctxs[0]->mu); ctxs[0]->err = std::string(what) + ": two contexts share a GPU (RCCL wants one rank per device)"; return PD_EINVAL; }
    std::vector<ncclComm_t> nc((size_t)n, nullptr);
    bool made = false;
    // (NOT `&tp == &rccl()`: rccl() LOADS librccl — round 6's first in-process communicators spent 1.1 s doing exactly that, and slowed the decode
    // beside them the way round 5's side thread had: profiles/r06_comm_transports.txt)
    const bool is_local = &tp == &local_tp();
    if (!is_local) {               // a communicator made ahead of the contexts (pd_comm_preinit) over the same devices
        std::lock_guard<std::mutex> lk(g_parked.mu);
        if (g_parked.devs == devs && !g_parked.nc.empty()) { nc = g_parked.nc; g_parked.nc.clear(); g_parked.devs.clear(); made = true; }
    }
    if (!made) made = tp.CommInitAll(nc.data(), n, devs.data()) == ncclSuccess;
    if (!made) {
        std::lock_guard<std::mutex> lk(ctxs[0]->mu);
        ctxs[0]->err = !is_local ? std::string("ncclCommInitAll failed") : std::string(what) + ": no peer access between the contexts' GPUs";
        return PD_EHIP;
    }
    // every rank's buffers side by side (one thread per rank: allocations on eight devices in a row were most of a list run's start-up)
    std::vector<int> rcs((size_t)n, PD_OK);
    for (int i = 0; i < n; ++i) {
        pd_comm *m = new pd_comm; m->ctx = ctxs[i]; m->tp = &tp; m->rank = i; m->world = n; m->nccl = nc[(size_t)i];
        comms[i] = m;
    }
    if (n == 1) rcs[0] = comm_setup(comms[0]);
    else {
        std::vector<std::thread> th;
        for (int i = 0; i < n; ++i) th.emplace_back([&, i] { rcs[(size_t)i] = comm_setup(comms[i]); });
        for (auto &t : th) t.join();
    }
    int rc = PD_OK;
    for (int i = 0; i < n; ++i) if (rcs[(size_t)i] != PD_OK && rc == PD_OK) { rc = rcs[(size_t)i]; std::lock_guard<std::mutex> lk(ctxs[0]->mu); ctxs[0]->err = comms[i]->err; }
    if (rc) for (int i = 0; i < n; ++i) { pd_comm_destroy(comms[i]); comms[i] = nullptr; }
    return rc;
}

int pd_comm_init_all(pd_ctx **ctxs, int n, pd_comm **comms) { return comm_init_over(rccl(), "pd_comm_init_all", ctxs, n, comms); }

int pd_comm_init_local(pd_ctx **ctxs, int n, pd_comm **comms) { return comm_init_over(local_tp(), "pd_comm_init_local", ctxs, n, comms); }

int pd_comm_destroy(pd_comm *m)
{
    if (!m) return PD_OK;
    if (m->ctx) (void)hipSetDevice(m->ctx->device);
    if (m->links) (void)hipStreamSynchronize(m->links);
    if (m->ctx && m->ctx->stream) (void)hipStreamSynchronize(m->ctx->stream);
    if (m->nccl && m->tp) (void)m->tp->CommDestroy(m->nccl);
    for (pd_comm::Slot &s : m->slot) {
        for (void *p : {(void *)s.send, (void *)(s.recv == s.send ? nullptr : s.recv), (void *)s.meta, (void *)s.exc, (void *)s.exc_all, (void *)s.count}) if (p) (void)hipFree(p);
        if (s.packed) (void)hipEventDestroy(s.packed);
        if (s.landed) (void)hipEventDestroy(s.landed);
    }
    if (m->part_mine) (void)hipFree(m->part_mine);
    if (m->part_all) (void)hipFree(m->part_all);
    if (m->slice_depth) (void)hipFree(m->slice_depth);
    if (m->swept) (void)hipEventDestroy(m->swept);
    if (m->gathered) (void)hipEventDestroy(m->gathered);
    if (m->links) (void)hipStreamDestroy(m->links);
    delete m;
    return PD_OK;
}

const char *pd_comm_strerror(const pd_comm *m) { return m ? m->err.c_str() : ""; }

// The slot's exchange buffers now instead of at its first pd_sliced_sum_start: not collective, any thread (the executable calls it on a
// side thread while the rank's file is being decoded: 3 GB of device allocations per rank for a 3 Gb genome are tenths of a second).
int pd_comm_prepare(pd_comm *m, int slot)
{
    if (!m || slot < 0 || slot > 1) return PD_EINVAL;
    HIPCM(m, hipSetDevice(m->ctx->device));
    return slot_setup(m, m->slot[slot]);
}

// Collective, first half: packs the context's sample (pd_export_i4) into `slot` and puts it on the links.  Only enqueues: the
// context may be reset and refilled right away, and the other slot may be started before this one is finished.
int pd_sliced_sum_start(pd_comm *m, int slot)
{
    if (!m || slot < 0 || slot > 1) return PD_EINVAL;
    pd_comm::Slot &s = m->slot[slot];
    if (s.busy) return comm_fail(m, PD_EINVAL, "pd_sliced_sum_start: the slot has not been finished");
    pd_ctx *c = m->ctx;
    const size_t W = (size_t)m->world, sb = (size_t)m->slice_bytes;
    HIPCM(m, hipSetDevice(c->device));
    hipStream_t st = c->stream, ln = m->links;
    // 1. this rank's 4-bit image (straight from the tile windows in LDS when the sample is still deferred), its own slice in place
    int rc = slot_setup(m, s);
    if (rc) return rc;
    rc = pd_export_i4(c, s.send, s.exc, COMM_EXC_BLOCK, s.count);
    if (rc) return comm_fail(m, rc, std::string("pd_export_i4: ") + c->err);
    HIPCM(m, hipMemcpyAsync(s.meta, c->sums, (size_t)m->n_sums * 4, hipMemcpyDeviceToDevice, st));
    HIPCM(m, hipMemsetAsync(s.meta + m->n_sums, 0, W * 4, st));
    HIPCM(m, hipMemcpyAsync(s.meta + m->n_sums + m->rank, s.count, 4, hipMemcpyDeviceToDevice, st));
    if (W > 1) HIPCM(m, hipMemcpyAsync(s.recv + (size_t)m->rank * sb, s.send + (size_t)m->rank * sb, sb, hipMemcpyDeviceToDevice, st));
    HIPCM(m, hipEventRecord(s.packed, st));
    HIPCM(m, hipStreamWaitEvent(ln, s.packed, 0));
    // 2. the all-to-all: every pair of GPUs moves 1/world of the image over its own xGMI link, all links at once
    for (size_t c0 = 0; c0 < sb && W > 1; c0 += COMM_MSG_BYTES) {
        const size_t n = std::min(COMM_MSG_BYTES, sb - c0);
        NCCLOK(m, m->tp->GroupStart());
        for (int p = 0; p < m->world; ++p) {
            if (p == m->rank) continue;
            NCCLOK(m, m->tp->Send(s.send + (size_t)p * sb + c0, n, ncclUint8, p, m->nccl, ln));
            NCCLOK(m, m->tp->Recv(s.recv + (size_t)p * sb + c0, n, ncclUint8, p, m->nccl, ln));
        }
        NCCLOK(m, m->tp->GroupEnd());
    }
    // 3. tile sums (+ exception counts) summed over the ranks; everybody's exception block to everybody
    NCCLOK(m, m->tp->AllReduce(s.meta, s.meta, (size_t)m->n_sums + W, ncclInt32, ncclSum, m->nccl, ln));
    NCCLOK(m, m->tp->AllGather(s.exc, s.exc_all, (size_t)COMM_EXC_BLOCK * sizeof(pd_exc), ncclUint8, m->nccl, ln));
    HIPCM(m, hipEventRecord(s.landed, ln));
    s.busy = true;
    return PD_OK;
}

// Collective, second half: on `root`, cover / sum receive what pd_scan_reduce_windows would give on a context holding the sum
// of all ranks' samples started in `slot` (windows of w >= 8192 cells).  Blocks until this rank's part is complete.
int pd_sliced_sum_finish(pd_comm *m, int slot, uint32_t w, uint32_t min_dep, unsigned wrap_bits, int root, uint32_t *cover, uint64_t *sum)
{
    if (!m || slot < 0 || slot > 1 || root < 0 || root >= m->world || w < PD_TILE || wrap_bits > 32) return PD_EINVAL;
    if (m->rank == root && (!cover || !sum)) return PD_EINVAL;
    pd_comm::Slot &s = m->slot[slot];
    if (!s.busy) return comm_fail(m, PD_EINVAL, "pd_sliced_sum_finish: the slot has not been started");
    s.busy = false;
    pd_ctx *c = m->ctx;
    const size_t W = (size_t)m->world, sb = (size_t)m->slice_bytes;
    HIPCM(m, hipSetDevice(c->device));
    hipStream_t st = c->stream, ln = m->links;
    // 4. this rank's slice: sum of the images, prefix sum, wrap, per-tile partials of the windows
    HIPCM(m, hipStreamWaitEvent(st, s.landed, 0));
    int rc = pd_slice_sweep_i4(c, s.recv, (uint32_t)W, sb, m->tile_first, m->tile_count, s.meta, s.exc_all, COMM_EXC_BLOCK, s.meta + m->n_sums, w, min_dep,
                               wrap_bits, m->part_mine);
    if (rc) return comm_fail(m, rc, std::string("pd_slice_sweep_i4: ") + c->err);
    // 5. 24 bytes per tile to the root
    const size_t pb = (size_t)m->slice_tiles * PD_TILE_PARTIAL_BYTES;
    if (m->rank == root) HIPCM(m, hipMemcpyAsync(m->part_all + (size_t)root * pb, m->part_mine, pb, hipMemcpyDeviceToDevice, st));
    if (W > 1) {
        HIPCM(m, hipEventRecord(m->swept, st));
        HIPCM(m, hipStreamWaitEvent(ln, m->swept, 0));
        NCCLOK(m, m->tp->GroupStart());
        if (m->rank == root) { for (int p = 0; p < m->world; ++p) if (p != root) NCCLOK(m, m->tp->Recv(m->part_all + (size_t)p * pb, pb, ncclUint8, p, m->nccl, ln)); }
        else NCCLOK(m, m->tp->Send(m->part_mine, pb, ncclUint8, root, m->nccl, ln));
        NCCLOK(m, m->tp->GroupEnd());
        HIPCM(m, hipEventRecord(m->gathered, ln));
        HIPCM(m, hipStreamWaitEvent(st, m->gathered, 0));
    }
    std::vector<int32_t> counts(W);
    HIPCM(m, hipMemcpyAsync(counts.data(), s.meta + m->n_sums, W * 4, hipMemcpyDeviceToHost, st));
    HIPCM(m, hipStreamSynchronize(st));
    // (every rank holds the same all-reduced counts, so every rank leaves here with the same code; the samples are intact —
    // an export that overflows never consumes a deferred sample, it leaves it in the rank's difference arrays)
    for (int32_t k : counts) if (k < 0 || (uint32_t)k > COMM_EXC_BLOCK)
        return comm_fail(m, PD_ERANGE, "a sample has more cells outside the 4-bit range than the exception block holds: the sliced sum does not apply, "
                                       "every context still holds its sample (pd_accumulate_from adds them up)");
    if (m->rank == root) {
        rc = pd_gather_windows(c, m->part_all, w, cover, sum);
        if (rc) return comm_fail(m, rc, std::string("pd_gather_windows: ") + c->err);
    }
    return PD_OK;
}

// Collective: after pd_sliced_sum_start(slot) — this rank's slice of the SUMMED sample as int32 depth cells (prefix-summed, wrapped) in
// m->slice_depth: what pd_scan would leave in cells [tile_first, tile_first + tile_count) x 8192 of a context holding every rank's sample.
// The statistics that need the cells themselves (narrow windows, annotation intervals) then run on the rank that owns them.
static int sliced_depth(pd_comm *m, int slot, unsigned wrap_bits)
{
    pd_comm::Slot &s = m->slot[slot];
    if (!s.busy) return comm_fail(m, PD_EINVAL, "sliced statistics: the slot has not been started");
    s.busy = false;
    pd_ctx *c = m->ctx;
    const size_t W = (size_t)m->world, sb = (size_t)m->slice_bytes;
    HIPCM(m, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCM(m, hipStreamWaitEvent(st, s.landed, 0));
    std::vector<int32_t> counts(W);
    HIPCM(m, hipMemcpyAsync(counts.data(), s.meta + m->n_sums, W * 4, hipMemcpyDeviceToHost, st));
    HIPCM(m, hipStreamSynchronize(st));
    for (int32_t k : counts) if (k < 0 || (uint32_t)k > COMM_EXC_BLOCK)
        return comm_fail(m, PD_ERANGE, "a sample has more cells outside the 4-bit range than the exception block holds: the sliced sum does not apply, "
                                       "every context still holds its sample (pd_accumulate_from adds them up)");
    if (!m->slice_depth && hipMalloc(&m->slice_depth, (size_t)m->slice_tiles * PD_TILE * 4 + 64) != hipSuccess) {
        (void)hipGetLastError();
        return comm_fail(m, PD_ENOMEM, "sliced statistics: the slice's depth cells could not be allocated");
    }
    {
        std::lock_guard<std::mutex> lk(c->mu);          // (comm_fail takes this lock: nothing below fails under it)
        const uint32_t mask = pdwin::wrap_mask(wrap_bits);
        { ProfScope ps(c, "tile_carry"); launch_tile_carry(st, s.meta, c->bsum, c->carry, (uint32_t)c->n_tiles); }
        { ProfScope ps(c, "slice_depth");
          TileMap tm{c->d_tile_contig, c->d_off, c->d_len, nullptr};
          launch_sweep_i4(st, s.recv, (uint32_t)W, sb, (uint32_t)m->tile_first, (uint32_t)m->tile_count, s.exc_all, COMM_EXC_BLOCK, s.meta + m->n_sums,
                          c->slice_flags, slice_flag_bytes(c->n_tiles), c->carry, mask, tm, PD_TILE, 0, nullptr, m->slice_depth); }
    }
    HIPCM(m, hipGetLastError());
    return PD_OK;
}

// windows of w < 8192 cells: every rank reduces the windows of its slice's cells; the window arrays are merged (each window has one
// writer: an all-reduce of the words adds zeros to it), the windows across tile edges are put together from the tiles' shares
static int sliced_narrow_windows(pd_comm *m, uint32_t w, uint32_t min_dep, unsigned wrap_bits, int root, uint32_t *cover, uint64_t *sum)
{
    int rc = pd_sliced_sum_start(m, 0);
    if (rc) return rc;
    rc = sliced_depth(m, 0, wrap_bits);
    if (rc) return rc;
    pd_ctx *c = m->ctx;
    hipStream_t st = c->stream, ln = m->links;
    // (the collective is the context's only user while it runs — one thread per rank; the context's lock is taken only where its
    // shared scratch and profile records are touched, never across a comm_fail, which takes it itself)
    std::vector<uint64_t> wo;
    const pdwin::WinLayout l = win_table(c, w, &wo);
    const size_t b_off = wo.size() * 8;
    std::string emsg;
    { std::lock_guard<std::mutex> lk(c->mu);
      rc = ensure_scratch(c, b_off + 64);
      if (!rc) rc = c->win.fit(c, l.b_all);
      if (rc) emsg = c->err; }
    if (rc) return comm_fail(m, rc, emsg);
    uint64_t *d_wo = (uint64_t *)c->scratch;
    unsigned long long *d_sum = c->win.sums();
    uint32_t *d_cov = c->win.covers(l);
    HIPCM(m, hipMemcpyAsync(d_wo, wo.data(), b_off, hipMemcpyHostToDevice, st));
    HIPCM(m, hipStreamSynchronize(st));                 // wo is a local
    HIPCM(m, hipMemsetAsync(d_sum, 0, l.b_res, st));
    TileMap tm{c->d_tile_contig, c->d_off, c->d_len, d_wo};
    TilePart *parts = (TilePart *)m->part_all;           // indexed by tile of the genome: the ranks' slices are consecutive blocks of it
    int e_lds = 0;
    { std::lock_guard<std::mutex> lk(c->mu);
      ProfScope ps(c, "slice_windows");
      e_lds = launch_sweep_windows_slice(st, m->slice_depth, (uint32_t)m->tile_first, (uint32_t)m->tile_count, tm, w, min_dep, d_cov, d_sum, parts); }
    if (e_lds) return comm_fail(m, PD_EHIP, "window sweep: cannot reserve LDS");
    HIPCM(m, hipGetLastError());
    if (m->world > 1) {
        HIPCM(m, hipEventRecord(m->swept, st));
        HIPCM(m, hipStreamWaitEvent(ln, m->swept, 0));
        const size_t pb = (size_t)m->slice_tiles * PD_TILE_PARTIAL_BYTES;
        NCCLOK(m, m->tp->AllGather(m->part_all + (size_t)m->rank * pb, m->part_all, pb, ncclUint8, m->nccl, ln));
        NCCLOK(m, m->tp->AllReduce(d_sum, d_sum, l.b_res / 4, ncclInt32, ncclSum, m->nccl, ln));
        HIPCM(m, hipEventRecord(m->gathered, ln));
        HIPCM(m, hipStreamWaitEvent(st, m->gathered, 0));
    }
    launch_window_edges(st, parts, tm, (uint32_t)c->n_tiles, w, d_cov, d_sum);
    HIPCM(m, hipGetLastError());
    if (m->rank == root) {
        HIPCM(m, hipMemcpyAsync(sum, d_sum, l.b_sum, hipMemcpyDeviceToHost, st));
        HIPCM(m, hipMemcpyAsync(cover, d_cov, (size_t)l.nw * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCM(m, hipStreamSynchronize(st));
    { std::lock_guard<std::mutex> lk(c->mu); c->win.commit(w, l, wo); }   // (every rank holds the merged statistics)
    return PD_OK;
}

int pd_sliced_window_sum(pd_comm *m, uint32_t w, uint32_t min_dep, unsigned wrap_bits, int root, uint32_t *cover, uint64_t *sum)
{
    if (!m || root < 0 || root >= m->world || w == 0 || wrap_bits > 32) return PD_EINVAL;
    if (m->rank == root && (!cover || !sum)) return PD_EINVAL;
    if (w < PD_TILE) return sliced_narrow_windows(m, w, min_dep, wrap_bits, root, cover, sum);
    const int rc = pd_sliced_sum_start(m, 0);
    return rc ? rc : pd_sliced_sum_finish(m, 0, w, min_dep, wrap_bits, root, cover, sum);
}

// Collective: pd_reduce_intervals (PD:329-348 over the CDS / BED regions) on the sum of every rank's sample without any GPU holding the
// summed arrays: a rank reduces the stretches of the regions that lie in its slice, the per-region partial results of all ranks are
// gathered and added on `root`.
int pd_sliced_interval_sum(pd_comm *m, const pd_region *regs, size_t n, uint32_t min_dep, unsigned wrap_bits, int root, int32_t *cover, uint64_t *sum)
{
    if (!m || root < 0 || root >= m->world || wrap_bits > 32 || (n && !regs)) return PD_EINVAL;
    if (m->rank == root && n && (!cover || !sum)) return PD_EINVAL;
    if (n > 0xFFFFFFF0ull) return comm_fail(m, PD_EINVAL, "too many regions");
    int rc = pd_sliced_sum_start(m, 0);
    if (rc) return rc;
    rc = sliced_depth(m, 0, wrap_bits);
    if (rc) return rc;
    if (n == 0) return PD_OK;
    pd_ctx *c = m->ctx;
    hipStream_t st = c->stream, ln = m->links;
    constexpr uint32_t PIECE = 16384;
    const uint64_t lo_cell = m->tile_first * PD_TILE, hi_cell = (m->tile_first + m->tile_count) * PD_TILE;
    std::vector<Piece> pieces;
    for (size_t i = 0; i < n; ++i) {
        const pd_region &r = regs[i];
        if (r.tid < 0 || r.tid >= c->n_contigs) return comm_fail(m, PD_EINVAL, "pd_sliced_interval_sum: contig id out of range");
        int64_t b = (int64_t)r.first - 1, e = r.second;          // cells [first - 1, second), clipped to the slot
        const int64_t slot = (int64_t)(c->off[r.tid + 1] - c->off[r.tid]);
        if (b < 0) b = 0;
        if (e > slot) e = slot;
        if (b >= e) continue;
        uint64_t gb = c->off[r.tid] + (uint64_t)b, ge = c->off[r.tid] + (uint64_t)e;
        if (gb < lo_cell) gb = lo_cell;
        if (ge > hi_cell) ge = hi_cell;
        for (uint64_t p = gb; p < ge; p += PIECE) {
            Piece pc; pc.start = p - lo_cell; pc.count = (uint32_t)std::min<uint64_t>(PIECE, ge - p); pc.region = (uint32_t)i;
            pieces.push_back(pc);
        }
    }
    const size_t W = (size_t)m->world;
    const size_t b_sum = n * 8, b_cov = (n * 4 + 7) / 8 * 8, blk = b_sum + b_cov, b_p = (pieces.size() * sizeof(Piece) + 15) / 16 * 16;
    std::string emsg;
    { std::lock_guard<std::mutex> lk(c->mu); rc = ensure_scratch(c, b_p + blk * (W + 1) + 64); if (rc) emsg = c->err; }
    if (rc) return comm_fail(m, rc, emsg);
    unsigned char *sc = (unsigned char *)c->scratch;
    Piece *d_p = (Piece *)sc;
    unsigned char *mine = sc + b_p, *all = mine + blk;
    unsigned long long *d_sum = (unsigned long long *)mine;
    int *d_cov = (int *)(mine + b_sum);
    if (!pieces.empty()) HIPCM(m, hipMemcpyAsync(d_p, pieces.data(), pieces.size() * sizeof(Piece), hipMemcpyHostToDevice, st));
    HIPCM(m, hipMemsetAsync(mine, 0, blk, st));
    HIPCM(m, hipStreamSynchronize(st));                 // pieces is a local
    { std::lock_guard<std::mutex> lk(c->mu);
      ProfScope ps(c, "slice_intervals");
      launch_reduce_pieces(st, m->slice_depth, d_p, (uint32_t)pieces.size(), min_dep, d_cov, d_sum); }
    HIPCM(m, hipGetLastError());
    if (m->world > 1) {
        HIPCM(m, hipEventRecord(m->swept, st));
        HIPCM(m, hipStreamWaitEvent(ln, m->swept, 0));
        NCCLOK(m, m->tp->AllGather(mine, all, blk, ncclUint8, m->nccl, ln));
        HIPCM(m, hipEventRecord(m->gathered, ln));
        HIPCM(m, hipStreamWaitEvent(st, m->gathered, 0));
    } else HIPCM(m, hipMemcpyAsync(all, mine, blk, hipMemcpyDeviceToDevice, st));
    if (m->rank == root) {
        std::vector<unsigned char> host(blk * W);
        HIPCM(m, hipMemcpyAsync(host.data(), all, blk * W, hipMemcpyDeviceToHost, st));
        HIPCM(m, hipStreamSynchronize(st));
        for (size_t i = 0; i < n; ++i) { cover[i] = 0; sum[i] = 0; }
        for (size_t k = 0; k < W; ++k) {
            const uint64_t *hs = (const uint64_t *)(host.data() + k * blk);
            const int32_t *hc = (const int32_t *)(host.data() + k * blk + b_sum);
            for (size_t i = 0; i < n; ++i) { cover[i] += hc[i]; sum[i] += hs[i]; }
        }
    } else HIPCM(m, hipStreamSynchronize(st));
    return PD_OK;
}

} // extern "C"
