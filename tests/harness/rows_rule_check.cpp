// rows_rule_check — the arithmetic of the row statistics (pandepth_amd/csrc/pd_rows_rule.h) at its edges: the segment clip in its two forms, the
// piece cutter, the feed with a small cap (a flush at a row's end and in the middle of a row), where a batch of rows ends, the launch shape of a row,
// the group shifts / rows per group / rows per batch, and the cell span of a window.  The limits the product passes (2^20 rows, 2^21 segments,
// 2^21 pieces a flush) are out of any test's reach on a device; here the same code runs with a handful.  Every expected number is written out, none is
// computed by the header's own code.  Stand-alone: own main, no GPU; built by tests/test_rows_rule.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../pandepth_amd/csrc/pd_rows_rule.h"

using namespace pdrows;

static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

struct P3 { uint64_t start; uint32_t count; uint32_t region; };
static bool same(const P3 &p, uint64_t s, uint32_t n, uint32_t r) { return p.start == s && p.count == n && p.region == r; }

static void check_constants()
{
    CHECK(PIECE_CELLS == 16384); CHECK(FLUSH_PIECES == 2097152); CHECK(ROW_BATCH == 1048576); CHECK(SEG_BATCH == 2097152); CHECK(WIDE_ROWS == 1024);
    CHECK(al256(0) == 0); CHECK(al256(1) == 256); CHECK(al256(256) == 256); CHECK(al256(257) == 512);
    CHECK(FLUSH_PIECES * sizeof(P3) == 33554432);                // 32 MiB of pieces, a multiple of 256 as it stands
}

static void check_clip()
{
    Span s = seg_clip(0, 100, 1000); CHECK(s.start == 0 && s.count == 100);            // first = 0 and first = 1: the same start
    s = seg_clip(1, 100, 1000); CHECK(s.start == 0 && s.count == 100);
    s = seg_clip(-5, 3, 1000); CHECK(s.start == 0 && s.count == 3);
    s = seg_clip(2, 2, 1000); CHECK(s.start == 1 && s.count == 1);                     // a single cell
    s = seg_clip(901, 2000, 1000); CHECK(s.start == 900 && s.count == 100);            // second past the end
    s = seg_clip(1000, 1000, 1000); CHECK(s.start == 999 && s.count == 1);             // the last cell
    s = seg_clip(1001, 1100, 1000); CHECK(s.start == 1000 && s.count == 0);            // wholly past the end
    s = seg_clip(5, 4, 1000); CHECK(s.start == 4 && s.count == 0);                     // second < first: empty
    s = seg_clip(5, 3, 1000); CHECK(s.count == 0);
    s = seg_clip(1, 0, 1000); CHECK(s.start == 0 && s.count == 0);
    s = seg_clip(1, 1, 1); CHECK(s.start == 0 && s.count == 1);                        // a contig of one cell
    s = seg_clip(1, 5, 1); CHECK(s.start == 0 && s.count == 1);
    s = seg_clip(2, 5, 1); CHECK(s.count == 0);
    s = seg_clip(1, 2147483647, 700001); CHECK(s.start == 0 && s.count == 700001);
    // a contig of 8191 cells in a slot of 8192: the length form (histograms, quantiles, thresholds) against the slot form (pd_reduce_intervals)
    s = seg_clip(8000, 9000, 8191); CHECK(s.start == 7999 && s.count == 192);
    s = seg_clip(8000, 9000, 8192); CHECK(s.start == 7999 && s.count == 193);
    s = seg_clip(8192, 8192, 8191); CHECK(s.count == 0);
    s = seg_clip(8192, 8192, 8192); CHECK(s.start == 8191 && s.count == 1);
}

static std::vector<P3> cut(uint64_t start, uint64_t count, uint32_t slot, uint32_t piece = PIECE_CELLS)
{
    std::vector<P3> v;
    const int rc = cut_pieces(start, count, slot, piece, [&](uint64_t s, uint32_t n, uint32_t sl) { v.push_back(P3{s, n, sl}); return 0; });
    CHECK(rc == 0);
    return v;
}

static void check_cutter()
{
    CHECK(cut(100, 0, 7).empty());
    std::vector<P3> v = cut(100, 1, 7); CHECK(v.size() == 1 && same(v[0], 100, 1, 7));
    v = cut(100, 16383, 7); CHECK(v.size() == 1 && same(v[0], 100, 16383, 7));
    v = cut(100, 16384, 7); CHECK(v.size() == 1 && same(v[0], 100, 16384, 7));
    v = cut(100, 16385, 7); CHECK(v.size() == 2 && same(v[0], 100, 16384, 7) && same(v[1], 16484, 1, 7));       // the last one is short
    v = cut(100, 32768, 7); CHECK(v.size() == 2 && same(v[0], 100, 16384, 7) && same(v[1], 16484, 16384, 7));
    v = cut(5000000000ull, 40000, 3);                                                                            // a flat cell above 2^32
    CHECK(v.size() == 3 && same(v[0], 5000000000ull, 16384, 3) && same(v[1], 5000016384ull, 16384, 3) && same(v[2], 5000032768ull, 7232, 3));
    v = cut(0, 10, 1, 4); CHECK(v.size() == 3 && same(v[0], 0, 4, 1) && same(v[1], 4, 4, 1) && same(v[2], 8, 2, 1));
    CHECK(piece_count(0) == 0); CHECK(piece_count(1) == 1); CHECK(piece_count(16384) == 1); CHECK(piece_count(16385) == 2); CHECK(piece_count(32768) == 2);
    CHECK(piece_count(34359738368ull) == 2097152); CHECK(piece_count(34359738369ull) == 2097153);     // (2^35 cells: what a flush inside one row takes)
    // an error from the callback ends the cut and is returned
    int calls = 0;
    CHECK(cut_pieces(0, 50000, 0, PIECE_CELLS, [&](uint64_t, uint32_t, uint32_t) { return ++calls == 2 ? -7 : 0; }) == -7); CHECK(calls == 2);
}

struct Flushes { std::vector<std::vector<P3>> got; int fail_at = -1; };
static int feed_all(Feed<P3> &f, Flushes &fl, const std::vector<P3> &spans /* start, cells (< 2^32 here), slot */)
{
    auto flush = [&](std::vector<P3> &held) { fl.got.push_back(held); return (int)fl.got.size() == fl.fail_at ? -3 : 0; };
    for (const P3 &s : spans) if (int rc = f.add(s.start, s.count, s.region, flush)) return rc;
    return f.finish(flush);
}

static void check_feed()
{
    {   // an empty feed: no flush at all
        Feed<P3> f(4); Flushes fl;
        CHECK(feed_all(f, fl, {}) == 0); CHECK(fl.got.empty());
        CHECK(feed_all(f, fl, {P3{10, 0, 0}, P3{20, 0, 1}}) == 0); CHECK(fl.got.empty());             // rows without cells
    }
    {   // a row that ends exactly at the cap: one flush of four, and the final flush has nothing to do
        Feed<P3> f(4); Flushes fl;
        CHECK(feed_all(f, fl, {P3{0, 16384 * 4, 5}}) == 0);
        CHECK(fl.got.size() == 1 && fl.got[0].size() == 4);
        CHECK(same(fl.got[0][0], 0, 16384, 5) && same(fl.got[0][3], 49152, 16384, 5));
        CHECK(f.held.empty());
    }
    {   // two rows, the second crosses the cap: the flush in the middle of the row keeps the row's slot; the final flush happens once
        Feed<P3> f(4); Flushes fl;
        CHECK(feed_all(f, fl, {P3{1000, 16384 * 2 + 1, 0}, P3{200000, 16384 * 3, 1}}) == 0);
        CHECK(fl.got.size() == 2 && fl.got[0].size() == 4 && fl.got[1].size() == 2);
        CHECK(same(fl.got[0][0], 1000, 16384, 0) && same(fl.got[0][1], 17384, 16384, 0) && same(fl.got[0][2], 33768, 1, 0));
        CHECK(same(fl.got[0][3], 200000, 16384, 1));
        CHECK(same(fl.got[1][0], 216384, 16384, 1) && same(fl.got[1][1], 232768, 16384, 1));
        CHECK(f.held.empty());
    }
    {   // fewer than the cap: the one final flush
        Feed<P3> f(4); Flushes fl;
        CHECK(feed_all(f, fl, {P3{0, 5, 0}, P3{9, 5, 1}, P3{30, 16385, 2}}) == 0);
        CHECK(fl.got.size() == 1 && fl.got[0].size() == 4 && same(fl.got[0][3], 16414, 1, 2));       // (exactly the cap again: flushed by add, not by finish)
    }
    {   // nine pieces of one row at cap 4: 4 + 4 + 1
        Feed<P3> f(4); Flushes fl;
        CHECK(feed_all(f, fl, {P3{0, 16384 * 8 + 100, 9}}) == 0);
        CHECK(fl.got.size() == 3 && fl.got[0].size() == 4 && fl.got[1].size() == 4 && fl.got[2].size() == 1);
        CHECK(same(fl.got[1][0], 65536, 16384, 9) && same(fl.got[2][0], 131072, 100, 9));
    }
    {   // a failing flush ends the feed with its code; nothing is flushed after it
        Feed<P3> f(4); Flushes fl; fl.fail_at = 1;
        CHECK(feed_all(f, fl, {P3{0, 16384 * 9, 0}}) == -3); CHECK(fl.got.size() == 1);
        Feed<P3> g(4); Flushes gl; gl.fail_at = 1;
        CHECK(feed_all(g, gl, {P3{0, 7, 0}}) == -3); CHECK(gl.got.size() == 1);                      // ... the final one as well
    }
    {   // the product's cap: one piece short of it holds, the next one flushes
        Feed<P3> f(FLUSH_PIECES); int n = 0;
        auto flush = [&](std::vector<P3> &held) { ++n; return held.size() == 2097152 ? 0 : -1; };
        for (uint32_t i = 0; i < 2097151; ++i) f.add(i, 1, i, flush);
        CHECK(n == 0 && f.held.size() == 2097151);
        CHECK(f.add(7, 1, 7, flush) == 0); CHECK(n == 1 && f.held.empty());
        CHECK(f.finish(flush) == 0); CHECK(n == 1);
    }
}

// the batches of a row list at limits of 4 rows and 6 segments
static std::vector<size_t> batches(const std::vector<uint64_t> &row_off)
{
    std::vector<size_t> ends;
    const size_t n = row_off.size() - 1;
    for (size_t r0 = 0; r0 < n;) {
        const size_t r1 = batch_end(row_off.data(), n, r0, 4, 6);
        CHECK(r1 > r0 && r1 <= n);                               // the batches tile [0, n_rows)
        if (r1 <= r0) break;
        ends.push_back(r1); r0 = r1;
    }
    return ends;
}

static void check_batch_end()
{
    typedef std::vector<size_t> V;
    CHECK(batches({0, 1, 2, 3, 4, 5, 6, 7, 8, 9}) == V({4, 8, 9}));                  // a stop on rows; the last batch is short
    CHECK(batches({0, 1, 2, 3, 4}) == V({4}));                                       // exactly one full batch
    CHECK(batches({0, 3, 6, 9, 12}) == V({2, 4}));                                   // a stop on segments: 3 + 3 fit, the third row does not
    CHECK(batches({0, 6, 7}) == V({1, 2}));                                          // a row of exactly the limit, alone
    CHECK(batches({0, 5, 7, 8}) == V({1, 3}));                                       // 5 + 2 > 6
    CHECK(batches({0, 2, 11, 12}) == V({1, 2, 3}));                                  // a row of 9 segments (more than the limit) forms a batch alone
    CHECK(batches({0, 9}) == V({1}));
    CHECK(batches({0, 0, 0, 0, 0, 0, 0}) == V({4, 6}));                              // rows without segments stop on rows
    CHECK(batches({0, 0, 6, 6, 6, 7}) == V({4, 5}));                                 // empty rows around a full one
    CHECK(batches({0, 1}) == V({1}));
    CHECK(batches({0}).empty());                                                     // no rows, no batch
    // the product's limits: 2^20 + 5 single-segment rows are a batch of 2^20 and one of 5
    std::vector<uint64_t> ro(1048576 + 5 + 1);
    for (size_t i = 0; i < ro.size(); ++i) ro[i] = i;
    CHECK(batch_end(ro.data(), ro.size() - 1, 0, ROW_BATCH, SEG_BATCH) == 1048576);
    CHECK(batch_end(ro.data(), ro.size() - 1, 1048576, ROW_BATCH, SEG_BATCH) == 1048581);
}

static void check_shape()
{
    // the defaults of the quantiles: 512 / 262144
    CHECK(row_shape(0, 512, 262144) == 0); CHECK(row_shape(512, 512, 262144) == 0); CHECK(row_shape(513, 512, 262144) == 1);
    CHECK(row_shape(262144, 512, 262144) == 1); CHECK(row_shape(262145, 512, 262144) == 2); CHECK(row_shape(34000000000ull, 512, 262144) == 2);
    // the REGIMES of tests/test_depth_quantiles_gpu.py on rows of 0, 100, 5000 and 700001 cells
    const uint64_t C[4] = {0, 100, 5000, 700001};
    const uint32_t reg[6][2] = {{512, 262144}, {0, 0xFFFFFFFFu}, {0, 0}, {2048, 0}, {0, 4999}, {2048, 0xFFFFFFFFu}};
    const int want[6][4] = {{0, 0, 1, 2}, {0, 1, 1, 1}, {0, 2, 2, 2}, {0, 0, 2, 2}, {0, 1, 2, 2}, {0, 0, 1, 1}};
    const int wide[6] = {1, 0, 3, 2, 2, 0};                      // the rows of shape 2: what the wide launches are sized for
    for (int r = 0; r < 6; ++r) {
        int n2 = 0;
        for (int k = 0; k < 4; ++k) {
            CHECK(row_shape(C[k], reg[r][0], reg[r][1]) == want[r][k]);
            n2 += C[k] > reg[r][0] && C[k] > reg[r][1];          // (the count as pd_depth_quantiles used to spell it)
        }
        CHECK(n2 == wide[r]);
        int s2 = 0;
        for (int k = 0; k < 4; ++k) s2 += row_shape(C[k], reg[r][0], reg[r][1]) == 2;
        CHECK(s2 == wide[r]);
    }
    CHECK(row_shape(0, 0, 0) == 0); CHECK(row_shape(1, 0, 0) == 2); CHECK(row_shape(1, 0, 0xFFFFFFFFu) == 1);
    CHECK(row_shape(0xFFFFFFFFull, 0, 0xFFFFFFFFu) == 1); CHECK(row_shape(0x100000000ull, 0, 0xFFFFFFFFu) == 2);
    CHECK(row_shape(2048, 2048, 0) == 0); CHECK(row_shape(2049, 2048, 0) == 2);     // a split below the wave bound: no workgroup shape
    // the thresholds: both bounds are "threshold_wave_max", the shapes 0 and 2
    CHECK(row_shape(65536, 65536, 65536) == 0); CHECK(row_shape(65537, 65536, 65536) == 2); CHECK(row_shape(1, 0, 0) == 2);
}

static void check_formulas()
{
    CHECK(quant_gshift(1) == 3); CHECK(quant_gshift(8) == 3); CHECK(quant_gshift(9) == 4); CHECK(quant_gshift(16) == 4); CHECK(quant_gshift(17) == 5);
    CHECK(quant_gshift(32) == 5); CHECK(quant_gshift(33) == 6); CHECK(quant_gshift(512) == 6); CHECK(quant_gshift(0) == 3);
    CHECK(thr_gshift(0) == 3); CHECK(thr_gshift(64) == 3); CHECK(thr_gshift(65) == 4); CHECK(thr_gshift(128) == 4); CHECK(thr_gshift(129) == 5);
    CHECK(thr_gshift(256) == 5); CHECK(thr_gshift(257) == 6); CHECK(thr_gshift(512) == 6); CHECK(thr_gshift(513) == 6); CHECK(thr_gshift(65536) == 6);
    CHECK(thr_rpg(0) == 16); CHECK(thr_rpg(1) == 16); CHECK(thr_rpg(512) == 16); CHECK(thr_rpg(513) == 15); CHECK(thr_rpg(4096) == 2); CHECK(thr_rpg(4097) == 1);
    CHECK(thr_rpg(8192) == 1); CHECK(thr_rpg(8193) == 1); CHECK(thr_rpg(65536) == 1);
    CHECK(win_batch_rows(1) == 4194304); CHECK(win_batch_rows(4) == 4194304); CHECK(win_batch_rows(5) == 3355443); CHECK(win_batch_rows(16) == 1048576);
}

static void check_win_span()
{
    // contigs of 25, 3, 20 and 1 cells at w = 10: 3 + 1 + 2 + 1 windows
    const uint32_t len[4] = {25, 3, 20, 1};
    const uint64_t wo[5] = {0, 3, 4, 6, 7};
    const uint64_t want[7][3] = {{0, 0, 10}, {0, 10, 10}, {0, 20, 5}, {1, 0, 3}, {2, 0, 10}, {2, 10, 10}, {3, 0, 1}};     // contig, start, cells
    int32_t t = 0;
    for (uint64_t g = 0; g < 7; ++g) {                           // g walks upwards across the contigs; t follows
        const Span s = win_span(wo, len, 10, g, &t);
        CHECK((uint64_t)t == want[g][0]); CHECK(s.start == want[g][1]); CHECK(s.count == want[g][2]);
    }
    t = 0;                                                       // a walk may begin anywhere
    Span s = win_span(wo, len, 10, 5, &t); CHECK(t == 2 && s.start == 10 && s.count == 10);     // the last window of a contig of exactly 2 w cells
    s = win_span(wo, len, 10, 6, &t); CHECK(t == 3 && s.start == 0 && s.count == 1);
    // a contig without cells has no window: the walk steps over it
    const uint32_t len2[3] = {10, 0, 7};
    const uint64_t wo2[4] = {0, 1, 1, 2};
    t = 0;
    s = win_span(wo2, len2, 10, 0, &t); CHECK(t == 0 && s.start == 0 && s.count == 10);
    s = win_span(wo2, len2, 10, 1, &t); CHECK(t == 2 && s.start == 0 && s.count == 7);
    // one window wider than every contig
    const uint64_t wo3[5] = {0, 1, 2, 3, 4};
    t = 0;
    s = win_span(wo3, len, 10000000, 2, &t); CHECK(t == 2 && s.start == 0 && s.count == 20);
    // far into a long contig: the start is a 64-bit product
    const uint32_t len4[1] = {4000000000u};
    const uint64_t wo4[2] = {0, 4000000};
    t = 0;
    s = win_span(wo4, len4, 1000, 3999999, &t); CHECK(t == 0 && s.start == 3999999000ull && s.count == 1000);
}

int main()
{
    check_constants();
    check_clip();
    check_cutter();
    check_feed();
    check_batch_end();
    check_shape();
    check_formulas();
    check_win_span();
    printf("rows_rule_check: %d checks, %d failed\n", checks, failures);
    if (!failures) printf("rows_rule_check: ok\n");
    return failures ? 1 : 0;
}
