// pd_win_rule.h — the arithmetic of a window call: where its results lie, which set of status words it counts into, how they come back,
// and the grids and kernel forms of the passes over the pending sample.
//
// pd_windows.hip and pd_capi.hip (the product) and tests/harness/win_rule_check.cpp (the CPU check of the edges) share this code.  Plain C++17,
// no HIP types: every function here decides from numbers, the callers queue the work.  The measurement notes stand once, next to their rule.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pdwin {

constexpr uint32_t TILE = 8192;                      // cells per tile (PD_TILE; pd_windows.hip asserts it): windows of at least a tile are put together by a gather
constexpr size_t STATUS_BYTES = 64;                  // one set of the direct call's status words (PD_STATUS_WORDS words)
constexpr size_t PIN_BYTES = (size_t)1 << 20;        // the page-locked buffer a direct call's results come back through

// depths wrap at 2^wrap_bits (0 and 32: no wrap)
inline uint32_t wrap_mask(unsigned wrap_bits) { return (wrap_bits == 0 || wrap_bits == 32) ? 0xFFFFFFFFu : ((1u << wrap_bits) - 1u); }

// The result buffer of a window call over nw windows: [sums, 8 B per window | covers, 4 B per window, padded to 16 B | the direct path's status words],
// so that all a call hands back is one contiguous range.  b_res: where the results end; b_all: with one set of status words behind them.
struct WinLayout {
    uint64_t nw = 0;
    size_t b_sum = 0, b_cov = 0, b_res = 0, b_all = 0;
    WinLayout() = default;
    explicit WinLayout(uint64_t n) : nw(n), b_sum((size_t)n * 8), b_cov(((size_t)n * 4 + 15) / 16 * 16), b_res(b_sum + b_cov), b_all(b_res + STATUS_BYTES) {}
};

// windows of at least a tile are put together from the tiles' shares by k_window_gather; narrower ones are accumulated where they lie
inline bool gathered(uint32_t w, uint64_t nw) { return w >= TILE && nw > 0; }

// Wide windows have TWO sets of status words behind the results, used in turn: the gather of one call zeroes the set the next call counts into, so
// that no call fills its own (a 64-byte fill was 2.5 us of every step and a boundary of its own in the stream).  The sets are known to be as a gather
// left them only while nothing else has been at the buffer since (words_unknown: every user that fits the buffer says so) and the results end where
// they did; any other call — the first, another width, one behind a call that failed, returned early or took another path — fills both.
struct WordsState { bool ok = false; size_t at = 0; unsigned turn = 0; };        // ok: the last call's gather left set `turn` zeroed, `at` bytes into the buffer
struct WordsTurn { bool kept; unsigned turn; WordsState after; };                // kept: nothing to fill; turn: the set this call counts into; after: once its gather is queued
inline WordsState words_unknown(WordsState s) { s.ok = false; return s; }
inline WordsTurn words_turn(WordsState s, bool gath, size_t b_res)
{
    const bool kept = gath && s.ok && s.at == b_res;
    const unsigned turn = kept ? s.turn : 0u;
    return WordsTurn{kept, turn, WordsState{gath, b_res, gath ? (turn ^ 1u) : s.turn}};
}

// Up to PIN_BYTES the call's results come back in one copy through the context's page-locked buffer (three copies into the caller's pageable arrays
// were three staged round trips: 53 us from the gather's end to the last copy's, 10 us with the one copy — profiles/r11_direct_call_ab.txt, sections 0
// and 4); a larger result goes straight to the caller's arrays, so that no call pins memory in proportion to its output.
// Where a gather ends the call it stores every window to that buffer itself, through the buffer's device address, and one of its lanes copies the status
// words there: no copy is queued at all, and the call's sync is what makes the stores visible to the host.  Narrow windows (no gather) keep the one copy.
struct ReadBack { bool pinned, pin_stores; };
inline ReadBack read_back(const WinLayout &l, bool gath)
{
    const bool pinned = l.b_all <= PIN_BYTES;
    return ReadBack{pinned, pinned && gath};
}

// Grid of a tile pass over `all` pending runs: measured best is ~64 K workgroups for a whole-genome pass (each walks a handful of tiles; the
// hardware overlaps their load/flush phases); small streaming batches touch few tiles and get a proportionally smaller grid.  "grid_tiles"
// overrides it.  The direct passes walk tiles one by one and never get more workgroups than tiles (n_tiles_max; 0: no such bound, the arrays path).
inline unsigned pass_grid(uint64_t all, int n_cu, unsigned grid_tiles, uint64_t n_tiles_max)
{
    uint64_t g = grid_tiles;
    if (!g) {
        g = all / 256;
        if (g < (uint64_t)n_cu * 4) g = (uint64_t)n_cu * 4;
        if (g > 65536) g = 65536;
    }
    if (n_tiles_max && g > n_tiles_max) g = n_tiles_max;
    return (unsigned)g;
}

// a compact sample that is ALL there is goes through k_direct_c8 as it is; anywhere else it goes on as 12-byte runs.  Windows: wide ones only.
inline bool c8_sample(int nb, bool compact, bool expanded, uint32_t n_long) { return nb == 1 && compact && !expanded && !n_long; }
inline bool c8_windows(int nb, bool compact, bool expanded, uint32_t n_long, uint32_t w) { return c8_sample(nb, compact, expanded, n_long) && w >= TILE; }

// The form of k_direct_c8 a window call launches, and its grid.
struct CoverIn {
    bool direct_cover, cover_narrow, has_nar;        // "direct_cover", "cover_narrow", the sample has a narrow plane
    uint32_t cover_min, n_wide_sorted;               // "direct_cover_min"; sorted runs longer than 255 cells
    uint64_t all, n_tiles;
    int n_cu; unsigned grid_tiles; int direct_un;
};
struct CoverPlan { bool cover, narrow; unsigned grid; };
inline CoverPlan cover_plan(const CoverIn &in, unsigned grid)
{
    CoverPlan p{false, false, grid};
    p.cover = in.direct_cover && in.all >= (uint64_t)in.cover_min * in.n_tiles;    // a thin sample: the form without the pass (launch_direct_c8)
    // ... and the pass sweeps the sorted stream's narrow plane, half the bytes, when every sorted run fits a half-word (counted when the sample was made)
    p.narrow = p.cover && in.cover_narrow && in.has_nar && in.n_wide_sorted == 0;
    // The cover form walks GROUPS of four tiles and a settled group costs a workgroup little more than its start, so its default grid is 64 workgroups
    // per CU, not one per 256 runs: on the bench sample (91 623 groups; ms per launch with the pile-up pass) 65 536 workgroups 0.985, one per group
    // 1.352, 32 768: 0.798, 16 384: 0.806, 7 168: 0.797 (profiles/r13_cover_wave_ab.txt).  "grid_tiles" still overrides it.
    if (p.cover && !in.grid_tiles && !in.direct_un) {
        const uint64_t groups = (in.n_tiles + 3) / 4, g = (uint64_t)in.n_cu * 64;
        p.grid = (unsigned)(g < groups ? g : groups);
    }
    return p;
}

} // namespace pdwin
