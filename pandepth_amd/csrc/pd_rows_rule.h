// pd_rows_rule.h — the arithmetic of the row statistics (histograms of regions, interval sums, quantiles, thresholds): how a segment is clipped,
// how a cell span is cut into pieces and fed to the device, where a batch of rows ends, which launch shape a row takes and with which numbers.
// pd_rows.hip (the product) and tests/harness/rows_rule_check.cpp (the CPU check of the edges) share this code.  Plain C++17, no HIP types:
// every function here decides from numbers, the callers queue the work.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace pdrows {

constexpr uint32_t PIECE_CELLS = 16384;              // a cell span goes to the piece kernels in pieces of at most this many cells
constexpr size_t FLUSH_PIECES = (size_t)1 << 21;     // pieces the feed holds before it flushes (32 MiB of scratch)
constexpr size_t ROW_BATCH = (size_t)1 << 20, SEG_BATCH = (size_t)1 << 21;     // rows and segments that go up together (SEG_BATCH: also the most segments a row may have)
constexpr uint32_t WIDE_ROWS = 1024;                 // histogram rows (4096 x 8 B each) of one pieces + pick launch
inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }     // every scratch region of the quantiles and thresholds is rounded to this

// cells [first - 1, second) of a 1-based inclusive segment, clipped to [0, limit): `start` inside the contig, `count` cells (0: empty; start is
// first - 1 even then).  limit is the contig's LENGTH for histograms, quantiles and thresholds and its SLOT for pd_reduce_intervals, which reads
// the zero padding as the reference reads its own.
struct Span { uint64_t start, count; };
inline Span seg_clip(int64_t first, int64_t second, uint64_t limit)
{
    int64_t b = first - 1, e = second;
    if (b < 0) b = 0;
    if (e > (int64_t)limit) e = (int64_t)limit;
    return Span{(uint64_t)b, e > b ? (uint64_t)(e - b) : 0};
}

// [start, start + count) in pieces of at most `piece` cells, in order: the piece that begins p cells into the span has piece_cells() cells; cut_pieces
// hands every one to f(piece start, piece cells, slot), which returns 0 to go on; anything else ends the cut and is returned.
inline uint32_t piece_cells(uint64_t count, uint64_t p, uint32_t piece) { return (uint32_t)(count - p < piece ? count - p : piece); }
template <class F> inline int cut_pieces(uint64_t start, uint64_t count, uint32_t slot, uint32_t piece, F &&f)
{
    for (uint64_t p = 0; p < count; p += piece)
        if (int rc = f(start + p, piece_cells(count, p, piece), slot)) return rc;
    return 0;
}
inline uint64_t piece_count(uint64_t count) { return (count + PIECE_CELLS - 1) / PIECE_CELLS; }

// The feed: spans are cut into pieces P{start, cells, slot}; whenever `cap` are held, and once at the end (finish; not for an empty feed), they go to
// flush(held), which returns 0 or the error that ends the feed.  A flush in the middle of a span does not change the slot of what follows.
template <class P> struct Feed {
    std::vector<P> held; size_t cap;
    explicit Feed(size_t c) : cap(c) {}
    template <class Flush> int finish(Flush &&flush)
    {
        if (held.empty()) return 0;
        const int rc = flush(held);
        held.clear();
        return rc;
    }
    template <class Flush> int add(uint64_t start, uint64_t count, uint32_t slot, Flush &&flush)
    {
        for (uint64_t p = 0; p < count; p += PIECE_CELLS) {
            held.push_back(P{start + p, piece_cells(count, p, PIECE_CELLS), slot});     // (a flat loop, one test a piece: a window call makes ten million of them on the host)
            if (held.size() == cap) if (int rc = finish(flush)) return rc;
        }
        return 0;
    }
};

// the batch that begins at row r0 ends in front of the first row with which it would hold more than max_rows rows or max_segs segments; a row alone is
// always a batch (the entry points refuse a row of more than SEG_BATCH segments)
inline size_t batch_end(const uint64_t *row_off, size_t n_rows, size_t r0, size_t max_rows, uint64_t max_segs)
{
    size_t r1 = r0 + 1;
    while (r1 < n_rows && r1 - r0 < max_rows && row_off[r1 + 1] - row_off[r0] <= max_segs) ++r1;
    return r1;
}

// The launch shape of a row of C cells: 0 a group of lanes, up to wave_max cells; 1 a workgroup, up to split cells; 2 cut into pieces over many
// workgroups.  Quantiles: "quantile_wave_max" / "quantile_split_cells".  Thresholds have no workgroup shape: both are "threshold_wave_max".
inline int row_shape(uint64_t C, uint32_t wave_max, uint32_t split) { return C <= wave_max ? 0 : C <= split ? 1 : 2; }

// k_quant_narrow: a group of 8 .. 64 lanes, a lane per cell of the widest row (rows of segments: always 64)
inline uint32_t quant_gshift(uint32_t weff) { uint32_t g = 3; while (g < 6 && (1u << g) < weff) ++g; return g; }
// k_thr_narrow: a lane takes 8 cells of the largest row before the group grows
inline uint32_t thr_gshift(uint32_t cells) { uint32_t g = 3; while (g < 6 && (8u << g) < cells) ++g; return g; }
// ... and a group takes this many windows one after the other (rows of segments: 1)
inline uint32_t thr_rpg(uint32_t weff) { const uint32_t r = weff ? 8192u / weff : 16u; return r > 16u ? 16u : r < 1u ? 1u : r; }     // (weff = 0: no window has cells)
// windows a batch of a window call holds, n_val results each (the wide quantile shape: WIDE_ROWS)
inline uint64_t win_batch_rows(uint32_t n_val) { const uint64_t r = ((uint64_t)1 << 24) / n_val; return r < ((uint64_t)1 << 22) ? r : (uint64_t)1 << 22; }

// window g of pd_window_layout(w), wo[t] = the first window of contig t: *t steps up to g's contig (callers walk g upwards), the span is inside it
inline Span win_span(const uint64_t *wo, const uint32_t *len, uint32_t w, uint64_t g, int32_t *t)
{
    while (wo[*t + 1] <= g) ++*t;
    const uint64_t b = (g - wo[*t]) * w, e = b + w < len[*t] ? b + w : len[*t];
    return Span{b, e - b};
}

} // namespace pdrows
