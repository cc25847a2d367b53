// pd_windows.hip — the window calls: the owner of their result buffer (WinKeep), the arrays path (windows_common), the direct whole-sample
// paths (direct_windows, direct_export) and the gather of sliced partials.  What they decide by arithmetic is pd_win_rule.h's; what crosses
// to pd_capi.hip is declared in pd_ctx.h.
#include "pd_ctx.h"

using namespace pdwin;

static_assert(STATUS_BYTES == PD_STATUS_WORDS * 4, "the gather zeroes a whole set of status words");
static_assert(pdwin::TILE == PD_TILE, "pd_win_rule.h's tile");
static_assert(sizeof(TilePart) == PD_TILE_PARTIAL_BYTES, "pd_gather_windows' partial layout");
static_assert(PD_TILE == PD_TILE_CELLS, "tile size in the public header");

// ---- WinKeep: the one owner of the window result buffer --------------------------------------------------------------------------------

int WinKeep::fit(pd_ctx *c, size_t need)
{
    valid = false;
    words = words_unknown(words);                        // whoever calls writes the buffer: the direct call's status words are no longer known to be zero
    if (need <= bytes) return PD_OK;
    if (buf) { HIPOK(c, hipStreamSynchronize(c->stream)); HIPOK(c, hipFree(buf)); buf = nullptr; bytes = 0; }
    const size_t want = need + need / 8 + 4096;
    if (hipMalloc(&buf, want) != hipSuccess) { (void)hipGetLastError(); return fail(c, PD_ENOMEM, "window statistics: device allocation failed"); }
    bytes = want;
    return PD_OK;
}

// The device's copy of the window offsets `wo` of width w.  The offsets follow from the contig table, which is fixed at pd_create, and w, so the copy
// is kept from call to call and uploaded only for another width — queued, from the context's page-locked copy: the call's final sync covers it.
// (Until round 11 every window call uploaded a local vector and synchronised the stream before it queued anything else: in the traced bench step, 48 us
// from the reset's last fill to the direct kernel's start, 29 us without the copy and the sync — profiles/r11_direct_call_ab.txt, sections 0 and 4.)
int WinKeep::offsets(pd_ctx *c, uint32_t width, const std::vector<uint64_t> &wo, const uint64_t **d_wo)
{
    const size_t b_off = wo.size() * 8;
    if (!d_woff) {
        if (hipMalloc(&d_woff, b_off) != hipSuccess) { (void)hipGetLastError(); d_woff = nullptr; return fail(c, PD_ENOMEM, "window offsets: device allocation failed"); }
        if (hipHostMalloc((void **)&woff_host, b_off, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); (void)hipFree(d_woff); d_woff = nullptr; woff_host = nullptr;
            return fail(c, PD_ENOMEM, "window offsets: page-locked allocation failed");
        }
    }
    if (woff_w != width) {
        woff_w = 0;                                      // (every call that used woff_host has synchronised the stream behind its upload)
        memcpy(woff_host, wo.data(), b_off);
        HIPOK(c, hipMemcpyAsync(d_woff, woff_host, b_off, hipMemcpyHostToDevice, c->stream));
        woff_w = width;
    }
    *d_wo = d_woff;
    return PD_OK;
}

int WinKeep::pin_fit(pd_ctx *c)
{
    if (pin) return PD_OK;
    if (hipHostMalloc((void **)&pin, PIN_BYTES, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void **)&pin_dev, pin, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (pin) (void)hipHostFree(pin);
        pin = pin_dev = nullptr;
        return fail(c, PD_ENOMEM, "window statistics: page-locked allocation failed");
    }
    return PD_OK;
}

void WinKeep::release()
{
    for (void *p : {(void *)buf, (void *)d_woff}) if (p) (void)hipFree(p);
    for (void *p : {(void *)woff_host, (void *)pin}) if (p) (void)hipHostFree(p);
    buf = pin = pin_dev = nullptr; d_woff = woff_host = nullptr; bytes = 0; woff_w = 0; valid = false; words = WordsState{};
}

namespace pdi {

WinLayout win_table(const pd_ctx *c, uint32_t w, std::vector<uint64_t> *wo)
{
    wo->resize((size_t)c->n_contigs + 1);
    pd_window_layout(c, w, wo->data());
    return WinLayout(wo->back());
}

} // namespace pdi

namespace {

int windows_common(pd_ctx *c, uint32_t w, uint32_t min_dep, uint32_t mask, bool from_depth, uint32_t *cover, uint64_t *sum)
{
    WinKeep &k = c->win;
    std::vector<uint64_t> wo;
    const WinLayout l = win_table(c, w, &wo);
    const size_t b_part = (size_t)c->n_tiles * sizeof(TilePart);      // wide windows: every tile's shares; narrow ones: the shares of the windows across tile boundaries
    int rc = ensure_scratch(c, b_part + 64);
    if (rc) return rc;
    rc = k.fit(c, l.b_all);
    if (rc) return rc;
    const uint64_t *d_wo = nullptr;
    rc = k.offsets(c, w, wo, &d_wo);
    if (rc) return rc;
    unsigned long long *d_sum = k.sums();
    uint32_t *d_cov = k.covers(l);
    TilePart *d_part = (TilePart *)c->scratch;
    if (w < PD_TILE) HIPOK(c, hipMemsetAsync(d_sum, 0, l.b_res, c->stream));   // windows nobody writes stay zero
    if (!from_depth) { ProfScope ps(c, "tile_carry"); launch_tile_carry(c->stream, c->sums, c->bsum, c->carry, (uint32_t)c->n_tiles); }
    {
        ProfScope ps(c, from_depth ? "reduce_windows" : "scan_reduce_windows");
        TileMap tm{c->d_tile_contig, c->d_off, c->d_len, d_wo};
        int e = launch_sweep_windows(c->stream, c->buf, c->carry, (uint32_t)c->n_tiles, mask, tm, w, min_dep,
                                     d_cov, d_sum, d_part, l.nw, c->n_contigs, from_depth, c->hstate);
        if (e) return fail(c, PD_EHIP, "window sweep: cannot reserve LDS");
    }
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipMemcpyAsync(sum, d_sum, l.b_sum, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipMemcpyAsync(cover, d_cov, (size_t)l.nw * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    k.commit(w, l, wo);
    return PD_OK;
}

// ---- the direct window call ------------------------------------------------------------------------------------------------------------
// Every run of the sample is still pending and the arrays hold nothing, so the windows are computed from the runs without ever materialising
// the difference arrays: k_direct_c8 (with k_c8_heavy beside it) for a lone compact sample and wide windows, k_direct_tiles (12-byte runs)
// anywhere else, then k_window_gather for wide windows.  direct_windows below is the list of steps; DirectCall is what they hand on.
struct DirectCall {
    uint32_t w, min_dep, mask;
    std::vector<uint64_t> wo; WinLayout lay;
    bool gathered; WordsTurn wt; ReadBack rb;
    const uint64_t *d_wo; unsigned long long *d_sum; uint32_t *d_cov; TilePart *d_part;
    uint32_t *d_words, *d_words_next;                    // [n_long, fail, heavy_count, diagnostics ..., [12] tiles settled by the cover pass]; the heavy tile list: c->direct_words + 16
    bool c8; PendSet ps; uint64_t all; unsigned grid;
    uint32_t words[PD_STATUS_READ];                      // ... as read back; [12]: heavy_count[PD_HEAVY_SETTLED], [13]: [PD_HEAVY_FAST]
};

// step 1: the layout, the buffers it needs and the pointers into them
int direct_buffers(pd_ctx *c, DirectCall &d)
{
    WinKeep &k = c->win;
    d.lay = win_table(c, d.w, &d.wo);
    int rc = ensure_scratch(c, (size_t)c->n_tiles * sizeof(TilePart) + 64);
    if (rc) return rc;
    d.gathered = gathered(d.w, d.lay.nw);
    d.wt = words_turn(k.words, d.gathered, d.lay.b_res);                // (asked before fit(), which forgets the words like every other user's)
    rc = k.fit(c, d.lay.b_all + STATUS_BYTES);
    if (rc) return rc;
    rc = k.offsets(c, d.w, d.wo, &d.d_wo);
    if (rc) return rc;
    d.d_sum = k.sums(); d.d_cov = k.covers(d.lay);
    d.d_words = k.status(d.lay, d.wt.turn); d.d_words_next = k.status(d.lay, d.wt.turn ^ 1u);
    d.d_part = (TilePart *)c->scratch;
    d.rb = read_back(d.lay, d.gathered);                                 // (k.buf still gets the windows of a call that comes back through the page-locked buffer: the text rows)
    return d.rb.pinned ? k.pin_fit(c) : PD_OK;
}

// step 2: narrow windows are accumulated, so everything is zeroed; wide ones fill both sets of status words unless the last gather left them
int direct_zero(pd_ctx *c, const DirectCall &d)
{
    if (d.w < PD_TILE) HIPOK(c, hipMemsetAsync(d.d_sum, 0, d.lay.b_all, c->stream));   // edge windows are accumulated; the status words with them
    else if (!d.wt.kept) HIPOK(c, hipMemsetAsync(c->win.status(d.lay, 0), 0, 2 * STATUS_BYTES, c->stream));
    return PD_OK;
}

// step 3: the sample as the kernel of step 4 reads it
int direct_pending(pd_ctx *c, DirectCall &d)
{
    const Pending &p0 = c->pend[0];
    d.c8 = c8_windows((int)c->pend.size(), p0.cr != nullptr, p0.iv != nullptr, p0.cr ? p0.cr->n_long : 0, d.w);
    // a 4x sparser index than the arrays path's: measured neutral for the tile kernel, 0.43 -> 0.13 ms of index
    const int rc = pend_prepare(c, c->direct_sample, (uint32_t)c->n_tiles, PD_TILE, d.c8, &d.ps, &d.all);
    d.grid = pass_grid(d.all, c->n_cu, c->grid_tiles, c->n_tiles);
    return rc;
}

// The pile-up pass runs BESIDE k_direct_c8 on the context's side stream: its list and count are the sample's (k_c8_tile_desc), it writes the
// TileParts of exactly the tiles k_direct_c8 skips, and neither touches what the other reads.  heavy_fork: an event on main in front of k_direct_c8
// (the pass must not overtake what is queued before the call: the fills, an upload of the offsets, the sample's making).  heavy_join: main waits for
// the pass before the section's end event, so "direct_tiles" still times both, and before the gather.
// THE INVARIANT: every exit behind the fork is behind the join, or has synchronised the side stream — whoever syncs main afterwards is behind the pass.
hipError_t heavy_fork(pd_ctx *c) { return hipEventRecord(c->ev_fork, c->stream); }
hipError_t heavy_join(pd_ctx *c)
{
    hipError_t e = hipEventRecord(c->ev_join, c->side_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->ev_join, 0);
    if (e != hipSuccess) (void)hipStreamSynchronize(c->side_stream);   // (the pass may be in the side stream without main waiting for it: wait here)
    return e;
}

// step 4, compact: k_direct_c8 in the form pdwin::cover_plan picks, and the int-window pass for the pile-up tiles it lists, launched only for a sample
// that has some: the sample knows from its making (pd_runs::n_heavy, counted by k_c8_tile_desc from the records k_direct_c8 reads), so no round trip
// decides.  The bench's 1e9-record sample HAS pile-up tiles (12): the pass's 0.028 ms per call there (k_c8_heavy; 0.099 as the compact branch of
// k_direct_tiles_heavy, profiles/r12_pileup_gather_ab.txt) are its work; on the empty lists of the 1e8- and 3e8-record samples a launch took 0.004 ms, and
// deciding by the count that comes back with the results (a second gather, copy and sync) gained a 1e9-record step 0.024 ms where this form gains
// 0.069 (profiles/r11_direct_call_ab.txt, sections 2 and 3).
int direct_c8(pd_ctx *c, const DirectCall &d)
{
    const pd_runs *cr = c->pend[0].cr;
    const CoverPlan cp = cover_plan(CoverIn{c->direct_cover, c->cover_narrow, cr->nar != nullptr, c->direct_cover_min, cr->n_wide_sorted, d.all, c->n_tiles,
                                            c->n_cu, c->grid_tiles, c->direct_un}, d.grid);
    if (cr->n_heavy) HIPOK(c, heavy_fork(c));
    DirectC8Launch L{};
    L.st = c->stream; L.cs = cr->view(); L.desc = cr->td; L.n_tiles = (uint32_t)c->n_tiles;
    L.heavy_list = c->direct_words + 16; L.heavy_count = d.d_words + 2; L.grid_tiles = cp.grid;
    L.wrap_mask = d.mask; L.w = d.w; L.min_dep = d.min_dep; L.part = d.d_part;
    L.un = c->direct_un; L.cover = cp.cover; L.cover_min = c->direct_cover_min; L.narrow = cp.narrow; L.fast = c->cover_fast;
    c->direct_narrow = launch_direct_c8(L) ? 1 : 0;
    if (!cr->n_heavy) return PD_OK;
    hipError_t e = hipStreamWaitEvent(c->side_stream, c->ev_fork, 0);
    if (e == hipSuccess) {
        launch_direct_c8_heavy(c->side_stream, cr->view(), tab_of(c), c->d_tile_contig, (uint32_t)c->n_tiles, d.mask, d.w, d.min_dep, d.d_part, cr->heavy_tiles, cr->n_heavy);
        e = heavy_join(c);
    }
    if (e != hipSuccess) return fail(c, PD_EHIP, std::string("direct windows: the pile-up pass's stream: ") + hipGetErrorString(e));
    return PD_OK;
}

// step 4: the tile kernel ("direct_tiles" times the pile-up pass with it)
int direct_launch(pd_ctx *c, const DirectCall &d)
{
    ProfScope sc(c, "direct_tiles");
    if (d.c8) return direct_c8(c, d);
    launch_direct_tiles(c->stream, d.ps, tab_of(c), c->d_tile_contig, (uint32_t)c->n_tiles, d.mask, d.w, d.min_dep, d.d_part, d.d_wo,
                        d.d_cov, d.d_sum, d.d_words, d.d_words + 1, c->direct_words + 16, d.d_words + 2, d.grid, c->direct_un);
    return PD_OK;
}

// step 5: wide windows from the tiles' shares; the gather zeroes the next call's status words and, where the plan says so, stores the results to the host
int direct_gather(pd_ctx *c, const DirectCall &d)
{
    WinKeep &k = c->win;
    if (d.w >= PD_TILE) {
        ProfScope sc(c, "gather_windows");
        TileMap tm{c->d_tile_contig, c->d_off, c->d_len, d.d_wo};
        GatherCall gc{d.gathered ? d.d_words_next : nullptr, d.d_words, nullptr, nullptr, nullptr};
        if (d.rb.pin_stores) { gc.pin_sum = (unsigned long long *)k.pin_dev; gc.pin_cover = (uint32_t *)(k.pin_dev + d.lay.b_sum); gc.pin_words = (uint32_t *)(k.pin_dev + d.lay.b_res); }
        launch_window_gather(c->stream, d.d_part, tm, c->n_contigs, d.w, d.lay.nw, d.d_cov, d.d_sum, gc);
    }
    HIPOK(c, hipGetLastError());
    k.words = d.wt.after;                                // (the gather is in the stream: the other set is zero for whoever comes behind it)
    return PD_OK;
}

// step 6: the status words to d.words and — large results only — the windows to the caller's arrays; small ones wait in the page-locked buffer
int direct_read_back(pd_ctx *c, DirectCall &d, uint32_t *cover, uint64_t *sum)
{
    WinKeep &k = c->win;
    memset(d.words, 0, sizeof d.words);
    if (d.rb.pinned) { if (!d.rb.pin_stores) HIPOK(c, hipMemcpyAsync(k.pin, k.buf, d.lay.b_all, hipMemcpyDeviceToHost, c->stream)); }
    else {
        HIPOK(c, hipMemcpyAsync(d.words, d.d_words, sizeof d.words, hipMemcpyDeviceToHost, c->stream));
        HIPOK(c, hipMemcpyAsync(sum, d.d_sum, d.lay.b_sum, hipMemcpyDeviceToHost, c->stream));
        HIPOK(c, hipMemcpyAsync(cover, d.d_cov, (size_t)d.lay.nw * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPOK(c, hipStreamSynchronize(c->stream));
    if (d.rb.pinned) memcpy(d.words, k.pin + d.lay.b_res, sizeof d.words);
    return PD_OK;
}

// step 8: not applicable — the batches stay pending, the caller materialises the arrays
void direct_decline_note(const uint32_t *words)
{
    if (!getenv("PANDEPTH_TIMING")) return;
    fprintf(stderr, "[timing]   direct window path declined: begins owned %llu of %llu runs, runs with cells %u vs ends owned %u (difference), index error bits 0x%x, "
                    "long runs %u: the arrays are materialised\n", (unsigned long long)words[3] | ((unsigned long long)words[4] << 32),
            (unsigned long long)words[5] | ((unsigned long long)words[6] << 32), words[7], words[8], words[9], words[10]);
}

// *done = false (and nothing consumed) when the device found a run longer than the look-back or a batch that was not sorted: the caller then takes
// the materialising path, which reports real errors.
int direct_windows(pd_ctx *c, uint32_t w, uint32_t min_dep, uint32_t mask, uint32_t *cover, uint64_t *sum, bool *done)
{
    *done = false;
    DirectCall d{};
    d.w = w; d.min_dep = min_dep; d.mask = mask;
    if (int rc = direct_buffers(c, d)) return rc;
    if (int rc = direct_zero(c, d)) return rc;
    if (int rc = direct_pending(c, d)) return rc;
    if (int rc = direct_launch(c, d)) return rc;
    if (int rc = direct_gather(c, d)) return rc;
    if (int rc = direct_read_back(c, d, cover, sum)) return rc;
    const uint32_t *words = d.words;
    if (d.c8 && words[2] != c->pend[0].cr->n_heavy)      // step 7 (k_direct_c8's own count of the tiles it listed: the same candidates, the same threshold)
        return fail(c, PD_ESTATE, "direct windows: the kernel listed " + std::to_string(words[2]) + " pile-up tiles, the sample was made with " + std::to_string(c->pend[0].cr->n_heavy));
    c->direct_settled = words[2 + pdk::PD_HEAVY_SETTLED];
    c->direct_fast = words[2 + pdk::PD_HEAVY_FAST];
    c->direct_pileup = d.c8 ? words[2] : 0;
    if (words[1]) { direct_decline_note(words); return PD_OK; }
    if (d.rb.pinned) { memcpy(sum, c->win.pin, d.lay.b_sum); memcpy(cover, c->win.pin + d.lay.b_sum, (size_t)d.lay.nw * 4); }
    // the call READ the sample: it stays deferred (like pd_export_i4's direct form), every other call still works on it
    *done = true;
    c->win.commit(w, d.lay, d.wo);
    return PD_OK;
}

// ---- the direct export -----------------------------------------------------------------------------------------------------------------
// pd_export_i4 without the arrays (pd_keep_deferred, sample entirely deferred, context pristine): the tile windows leave as the 4-bit image
// straight from LDS (k_direct_c8's export form for a lone compact sample, k_direct_wide3's for 12-byte runs), the tile sums are written beside it.

// the kernel, behind the zeroing of what it counts into and the sample's preparation
int export_launch(pd_ctx *c, void *dev_i4, pd_exc *dev_exc, uint32_t exc_cap, uint32_t *dev_count)
{
    HIPOK(c, hipMemsetAsync(dev_count, 0, 4, c->stream));
    HIPOK(c, hipMemsetAsync(c->direct_words, 0, 64, c->stream));
    const Pending &p0 = c->pend[0];
    const bool c8 = c8_sample((int)c->pend.size(), p0.cr != nullptr, p0.iv != nullptr, p0.cr ? p0.cr->n_long : 0);
    PendSet ps{}; uint64_t all = 0;
    if (int rc = pend_prepare(c, c->sample < 256 ? 256 : c->sample, (uint32_t)c->n_tiles, PD_TILE, c8, &ps, &all)) return rc;
    const unsigned grid = pass_grid(all, c->n_cu, c->grid_tiles, c->n_tiles);
    { ProfScope sc(c, "direct_export");
      if (c8) {
          DirectC8Launch L{};
          L.st = c->stream; L.cs = p0.cr->view(); L.desc = p0.cr->td; L.n_tiles = (uint32_t)c->n_tiles;
          L.heavy_list = c->direct_words + 16; L.heavy_count = c->direct_words + 2; L.grid_tiles = grid;
          L.tab = tab_of(c); L.tile_contig = c->d_tile_contig; L.img = dev_i4; L.exc = dev_exc; L.cap = exc_cap; L.count = dev_count; L.sums = c->sums;
          L.n_heavy = p0.cr->n_heavy;
          launch_direct_c8_export(L);
      } else launch_direct_export(c->stream, ps, tab_of(c), c->d_tile_contig, (uint32_t)c->n_tiles, dev_i4, dev_exc, exc_cap, dev_count,
                                c->sums, c->direct_words, c->direct_words + 1, c->direct_words + 16, c->direct_words + 2, grid); }
    HIPOK(c, hipGetLastError());
    return PD_OK;
}

// *done = false (tile sums re-zeroed, batches still pending) when a tile was too heavy, a run too long or a batch not sorted.
int direct_export(pd_ctx *c, void *dev_i4, pd_exc *dev_exc, uint32_t exc_cap, uint32_t *dev_count, bool *done)
{
    *done = false;
    if (int rc = export_launch(c, dev_i4, dev_exc, exc_cap, dev_count)) return rc;
    uint32_t words[2] = {0, 0}, n_exc = 0;
    HIPOK(c, hipMemcpyAsync(words, c->direct_words, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipMemcpyAsync(&n_exc, dev_count, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    // more cells outside the 4-bit range than the caller's exception block holds (amplicon / very deep data): the image is
    // not usable, and the sample must stay whole for whatever the caller does instead — it is materialised below like any
    // other declined export, the arrays keep it
    if (n_exc > exc_cap) words[1] = 1;
    if (words[1]) {
        HIPOK(c, hipMemsetAsync(c->sums, 0, (c->n_words - c->n_cells) * 4, c->stream));      // the kernel wrote them
        c->sums_stale = false;
        char m[160];
        snprintf(m, sizeof m, "direct export declined (heavy tiles / long runs: %u; cells outside the 4-bit range: %u); the materialising path was used", words[0], n_exc);
        c->err = m;                                          // informational: the call still succeeds
        return PD_OK;
    }
    // The sample STAYS deferred: an export reads it.  (A caller that finds out later that the image is of no use — another
    // rank's sample did not fit its exception block, pd_sliced_sum_finish -> PD_ERANGE — still has every context's sample and
    // adds them up the general way.)  The tile sums now hold this sample's sums although the arrays hold nothing:
    // flush_pending zeroes them before it scatters, pd_reset forgets them with everything else.
    c->sums_stale = true;
    *done = true;
    return PD_OK;
}

} // namespace

extern "C" {

int pd_window_layout(const pd_ctx *c, uint32_t w, uint64_t *win_off)
{
    if (!c || !win_off || w == 0) return PD_EINVAL;
    uint64_t o = 0;
    for (int32_t i = 0; i < c->n_contigs; ++i) { win_off[i] = o; o += ((uint64_t)c->len[i] + w - 1) / w; }
    win_off[c->n_contigs] = o;
    return PD_OK;
}

int pd_scan_reduce_windows(pd_ctx *c, uint32_t w, uint32_t min_dep, unsigned wrap_bits, uint32_t *cover, uint64_t *sum)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->win.valid = false;                                // the kept windows are the LAST window call's: this one's once it commits, nobody's if it fails
    if (!cover || !sum || w == 0 || wrap_bits > 32) return PD_EINVAL;
    if (int rs = need_state(c, 0, "pd_scan_reduce_windows")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    c->direct_settled = 0; c->direct_pileup = 0; c->direct_narrow = 0; c->direct_fast = 0;
    const uint32_t mask = wrap_mask(wrap_bits);
    if (c->direct_windows && c->pristine && !c->pend.empty() && w >= 64 && c->stile == PD_TILE) {
        bool done = false;
        int rd = direct_windows(c, w, min_dep, mask, cover, sum, &done);
        if (rd || done) return rd;
    }
    int rc = flush_pending(c);
    if (rc) return rc;
    rc = check_words(c);
    if (rc) return rc;
    return windows_common(c, w, min_dep, mask, false, cover, sum);
}

int pd_reduce_windows(pd_ctx *c, uint32_t w, uint32_t min_dep, uint32_t *cover, uint64_t *sum)
{
    if (!c) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->win.valid = false;                                // (as in pd_scan_reduce_windows)
    if (!cover || !sum || w == 0) return PD_EINVAL;
    if (int rs = need_state(c, 1, "pd_reduce_windows")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    return windows_common(c, w, min_dep, 0xFFFFFFFFu, true, cover, sum);
}

int pd_export_i4(pd_ctx *c, void *dev_i4, pd_exc *dev_exc, uint32_t exc_cap, uint32_t *dev_count)
{
    if (!c || !dev_i4 || !dev_count || (exc_cap && !dev_exc)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_export_i4")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    if (c->direct_windows && c->pristine && !c->pend.empty() && c->stile == PD_TILE) {
        bool done = false;
        const int rd = direct_export(c, dev_i4, dev_exc, exc_cap, dev_count, &done);
        if (rd || done) return rd;
    }
    int rc = flush_pending(c);
    if (rc) return rc;
    HIPOK(c, hipMemsetAsync(dev_count, 0, 4, c->stream));
    { ProfScope ps(c, "export_i4");
      launch_export_i4(c->stream, c->buf, c->hstate, dev_i4, c->n_cells, dev_exc, exc_cap, dev_count); }
    HIPOK(c, hipGetLastError());
    return PD_OK;
}

// (The call does not commit: the kept windows, if any, are still an earlier call's — DESIGN.md 3.)
int pd_gather_windows(pd_ctx *c, const void *dev_partials, uint32_t w, uint32_t *cover, uint64_t *sum)
{
    if (!c || !dev_partials || !cover || !sum) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (w < PD_TILE) return fail(c, PD_EINVAL, "pd_gather_windows: windows narrower than a tile are not sliced");
    HIPOK(c, hipSetDevice(c->device));
    std::vector<uint64_t> wo;
    const WinLayout l = win_table(c, w, &wo);
    const size_t b_off = wo.size() * 8;
    int rc = ensure_scratch(c, b_off + l.b_res + 64);
    if (rc) return rc;
    unsigned char *s = (unsigned char *)c->scratch;
    uint64_t *d_wo = (uint64_t *)s;
    unsigned long long *d_sum = (unsigned long long *)(s + b_off);
    uint32_t *d_cov = (uint32_t *)(s + b_off + l.b_sum);
    HIPOK(c, hipMemcpyAsync(d_wo, wo.data(), b_off, hipMemcpyHostToDevice, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));          // wo is a local
    { ProfScope ps(c, "gather_windows");
      TileMap tm{c->d_tile_contig, c->d_off, c->d_len, d_wo};
      launch_window_gather(c->stream, (const TilePart *)dev_partials, tm, c->n_contigs, w, l.nw, d_cov, d_sum); }
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipMemcpyAsync(sum, d_sum, l.b_sum, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipMemcpyAsync(cover, d_cov, (size_t)l.nw * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    return PD_OK;
}

} // extern "C"
