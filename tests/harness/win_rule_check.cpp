// win_rule_check — the arithmetic of a window call (pandepth_amd/csrc/pd_win_rule.h) at its edges: the wrap mask, the result layout and the
// 1 MiB boundary of the page-locked read-back, the turn of the two sets of status words as a SEQUENCE of calls, the grids of the tile passes
// and which form of k_direct_c8 a call launches.  Every expected number is written out here, none is computed by the header's own code.
// Stand-alone: own main, no GPU; built by tests/test_win_rule.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>

#include "../../pandepth_amd/csrc/pd_win_rule.h"

using namespace pdwin;

static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

static void check_mask()
{
    CHECK(wrap_mask(0) == 0xFFFFFFFFu);
    CHECK(wrap_mask(32) == 0xFFFFFFFFu);
    CHECK(wrap_mask(1) == 1u);
    CHECK(wrap_mask(18) == 0x3FFFFu);
    CHECK(wrap_mask(31) == 0x7FFFFFFFu);
}

static void check_layout()
{
    // nw, b_sum, b_cov (4 nw padded to 16), b_res, b_all
    const uint64_t want[][5] = {{0, 0, 0, 0, 64}, {1, 8, 16, 24, 88}, {3, 24, 16, 40, 104}, {4, 32, 16, 48, 112}, {5, 40, 32, 72, 136},
                                {87376, 699008, 349504, 1048512, 1048576}, {87377, 699016, 349520, 1048536, 1048600}, {87400, 699200, 349600, 1048800, 1048864}};
    for (const auto &r : want) {
        const WinLayout l(r[0]);
        CHECK(l.nw == r[0]); CHECK(l.b_sum == r[1]); CHECK(l.b_cov == r[2]); CHECK(l.b_res == r[3]); CHECK(l.b_all == r[4]);
        CHECK(l.b_cov % 16 == 0 && l.b_cov >= l.nw * 4 && l.b_cov < l.nw * 4 + 16);
    }
    CHECK(STATUS_BYTES == 64); CHECK(PIN_BYTES == 1048576);
    // the 1 MiB boundary of the page-locked buffer
    CHECK(read_back(WinLayout(87376), true).pinned);
    CHECK(!read_back(WinLayout(87377), true).pinned);
    CHECK(!read_back(WinLayout(87400), true).pinned && !read_back(WinLayout(87400), true).pin_stores);
    // the gather stores there itself only where there is a gather: windows of at least a tile
    const WinLayout l(43700);
    CHECK(read_back(l, gathered(8192, l.nw)).pinned && read_back(l, gathered(8192, l.nw)).pin_stores);
    CHECK(read_back(l, gathered(8191, l.nw)).pinned && !read_back(l, gathered(8191, l.nw)).pin_stores);
    CHECK(read_back(l, gathered(4096, l.nw)).pinned && !read_back(l, gathered(4096, l.nw)).pin_stores);
    CHECK(gathered(8192, 1) && gathered(1u << 30, 5) && !gathered(8191, 1) && !gathered(64, 100));
    CHECK(!gathered(8192, 0) && !gathered(1u << 30, 0));                                         // no windows: never gathered
}

// one call: the rule's answer, then the state it leaves
static WordsTurn call(WordsState &s, uint32_t w, uint64_t nw)
{
    const WordsTurn t = words_turn(s, gathered(w, nw), WinLayout(nw).b_res);
    s = words_unknown(s);                                // (the call fits the buffer like every user)
    s = t.after;                                         // (... and its gather is queued)
    return t;
}

static void check_turn()
{
    const size_t r100 = WinLayout(100).b_res, r101 = WinLayout(101).b_res;
    CHECK(r100 == 1200 && r101 == 1224);
    WordsState s;
    WordsTurn t = call(s, 10000, 100);                   // the first call
    CHECK(!t.kept && t.turn == 0); CHECK(s.ok && s.at == r100 && s.turn == 1);
    t = call(s, 10000, 100);                             // the same again: nothing to fill, the other set
    CHECK(t.kept && t.turn == 1); CHECK(s.ok && s.at == r100 && s.turn == 0);
    t = call(s, 10000, 100);
    CHECK(t.kept && t.turn == 0); CHECK(s.ok && s.turn == 1);
    t = call(s, 9900, 101);                              // another width: the results end elsewhere
    CHECK(!t.kept && t.turn == 0); CHECK(s.ok && s.at == r101 && s.turn == 1);
    t = call(s, 9900, 101);
    CHECK(t.kept && t.turn == 1);
    t = call(s, 4096, 101);                              // a narrow call between two wide ones: no gather
    CHECK(!t.kept && t.turn == 0); CHECK(!s.ok);
    t = call(s, 9900, 101);
    CHECK(!t.kept && t.turn == 0); CHECK(s.ok && s.turn == 1);
    s = words_unknown(s);                                // a call of another kind fitted the buffer (the arrays path, the sliced narrow windows)
    CHECK(!s.ok);
    t = call(s, 9900, 101);
    CHECK(!t.kept && t.turn == 0); CHECK(s.ok && s.at == r101 && s.turn == 1);
    t = call(s, 9900, 101);
    CHECK(t.kept && t.turn == 1);
    t = call(s, 10000, 0);                               // no windows at all
    CHECK(!t.kept && t.turn == 0); CHECK(!s.ok);
    t = call(s, 10000, 0);
    CHECK(!t.kept && t.turn == 0); CHECK(!s.ok);
    // a call that returned before its gather was queued leaves what fit() left: unknown
    s = WordsState{true, r100, 1};
    t = words_turn(s, true, r100);
    CHECK(t.kept && t.turn == 1);
    s = words_unknown(s);
    CHECK(!words_turn(s, true, r100).kept && words_turn(s, true, r100).turn == 0);
}

static void check_grids()
{
    CHECK(pass_grid(1000, 256, 0, 0) == 1024);           // at least four workgroups per CU
    CHECK(pass_grid(1000000000ull, 256, 0, 0) == 65536);
    CHECK(pass_grid(10000000ull, 256, 0, 0) == 39062);
    CHECK(pass_grid(0, 256, 0, 0) == 1024);
    CHECK(pass_grid(262144, 256, 0, 0) == 1024 && pass_grid(262400, 256, 0, 0) == 1025);
    CHECK(pass_grid(1000, 256, 777, 0) == 777);          // "grid_tiles" as it is
    CHECK(pass_grid(1000000000ull, 256, 1u << 20, 0) == (1u << 20));
    // the bound by the tiles only where asked: the arrays path passes none
    CHECK(pass_grid(1000, 256, 0, 26) == 26);
    CHECK(pass_grid(10000000ull, 256, 0, 50000) == 39062);
    CHECK(pass_grid(1000000000ull, 256, 0, 50000) == 50000);
    CHECK(pass_grid(1000, 256, 777, 26) == 26 && pass_grid(1000, 256, 20, 26) == 20);
}

static CoverIn cin(uint64_t all, uint64_t n_tiles)
{
    return CoverIn{true, true, true, 2048, 0, all, n_tiles, 256, 0, 0};
}

static void check_cover()
{
    // the threshold: cover_min candidates per tile on average
    CoverPlan p = cover_plan(cin(2048ull * 1000 - 1, 1000), 4000);
    CHECK(!p.cover && !p.narrow && p.grid == 4000);
    p = cover_plan(cin(2048ull * 1000, 1000), 4000);
    CHECK(p.cover && p.narrow && p.grid == 250);          // ceil(1000 / 4) groups, fewer than 64 per CU
    p = cover_plan(cin(1000000000ull, 366491), 65536);
    CHECK(p.cover && p.grid == 16384);                    // 64 per CU; 91 623 groups
    p = cover_plan(cin(1000000000ull, 65533), 65533);
    CHECK(p.cover && p.grid == 16384);                    // 16 384 groups (65 533 tiles): both bounds meet
    p = cover_plan(cin(1000000000ull, 65532), 65532);
    CHECK(p.cover && p.grid == 16383);
    p = cover_plan(cin(1000000000ull, 26), 26);
    CHECK(p.cover && p.grid == 7);
    CoverIn in = cin(0, 1000);                            // a threshold of 0: every sample
    in.cover_min = 0;
    CHECK(cover_plan(in, 1000).cover);
    in = cin(2048ull * 1000, 1000); in.direct_cover = false;
    p = cover_plan(in, 4000);
    CHECK(!p.cover && !p.narrow && p.grid == 4000);
    // the cover grid yields to "grid_tiles" and to a form of the menu
    in = cin(1000000000ull, 366491); in.grid_tiles = 5000;
    p = cover_plan(in, 5000);
    CHECK(p.cover && p.narrow && p.grid == 5000);
    in = cin(1000000000ull, 366491); in.direct_un = 3;
    p = cover_plan(in, 65536);
    CHECK(p.cover && p.grid == 65536);
    // narrow: off when any of its four conditions fails
    in = cin(1000000000ull, 366491);
    CHECK(cover_plan(in, 1).narrow);
    in.cover_narrow = false;  CHECK(cover_plan(in, 1).cover && !cover_plan(in, 1).narrow);
    in = cin(1000000000ull, 366491); in.has_nar = false;       CHECK(cover_plan(in, 1).cover && !cover_plan(in, 1).narrow);
    in = cin(1000000000ull, 366491); in.n_wide_sorted = 1;     CHECK(cover_plan(in, 1).cover && !cover_plan(in, 1).narrow);
    in = cin(1000, 366491);                                    CHECK(!cover_plan(in, 1).cover && !cover_plan(in, 1).narrow);
    // k_direct_c8 reads a lone compact sample that nobody expanded and that has no long run; windows: of at least a tile
    CHECK(c8_sample(1, true, false, 0) && c8_windows(1, true, false, 0, 8192) && c8_windows(1, true, false, 0, 10000000));
    CHECK(!c8_sample(1, true, false, 1) && !c8_windows(1, true, false, 1, 8192));
    CHECK(!c8_sample(2, true, false, 0) && !c8_windows(2, true, false, 0, 8192));
    CHECK(!c8_sample(1, true, true, 0) && !c8_windows(1, true, true, 0, 8192));
    CHECK(!c8_sample(1, false, false, 0) && !c8_windows(1, false, false, 0, 8192));
    CHECK(c8_sample(1, true, false, 0) && !c8_windows(1, true, false, 0, 8191));                 // the export has no width
}

int main()
{
    check_mask();
    check_layout();
    check_turn();
    check_grids();
    check_cover();
    printf("win_rule_check: %d checks, %d failed\n", checks, failures);
    if (!failures) printf("win_rule_check: ok\n");
    return failures ? 1 : 0;
}
