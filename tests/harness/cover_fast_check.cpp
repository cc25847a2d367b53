// cover_fast_check — the FAST CHUNK of the narrow cover sweep (pandepth_amd/csrc/pd_cover_rule.h: nar_pair_steps, nar_lane_summary,
// chunk_fast_entry / _lane_ok / _ok, chunk_fast: a full chunk of 512 sorted runs, eight per lane, settled from a summary per lane) against the rule
// run by run (seg_sweep_nar), on the CPU.  Built with -fsanitize=address,undefined by tests/test_cover_fast_rule.py.
// A stream of sorted runs is swept in chunks of 512 as the kernel's narrow form sweeps a tile: every full chunk is offered to chunk_fast, a chunk it
// refuses and the partial chunk go through the rule.  Checked for crafted and random streams:
//   * an accepted chunk leaves exactly the state seg_sweep_nar has behind the same runs: the last run's begin, the largest end, the sum, no new gap
//   * a chunk that holds a gap, a begin < 0 or an end > tile is never accepted
//   * a refused chunk has changed nothing
//   * the packed step and the lane summary equal nar_step / nar_len run by run
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../pandepth_amd/csrc/pd_cover_rule.h"

static const int TILE = 8192;
static const uint32_t CW = 512;
struct Run { int b, len; };                              // tile-relative begin (>= -8192), cells (<= 255)

static int g_fail = 0;
static unsigned long g_chunks = 0, g_accepted = 0, g_ref_gap = 0, g_ref_neg = 0, g_ref_beyond = 0, g_ref_other = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; if (g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

// the rule, run by run, on the sweep's own state (what the kernel's general path computes for a chunk); says what the runs held
struct Held { bool gap, neg, beyond; };
static Held rule_runs(const uint16_t *nar, uint32_t n, pdcover::NarState &st)
{
    Held h{false, false, false};
    for (uint32_t i = 0; i < n; ++i) {
        const int b = st.base + pdcover::nar_step(nar[i], st.pb), e = b + pdcover::nar_len(nar[i]);
        if (b > st.reach) { st.gap = 1; h.gap = true; }
        if (b < 0) h.neg = true;
        if (e > TILE) h.beyond = true;
        st.reach = std::max(st.reach, e);
        st.sum += pdcover::run_clipped(b, e, TILE);
        st.base = b; st.pb = nar[i];
    }
    return h;
}

// want[c]: 1 / 0 the full chunk c must be accepted / refused, -1 (or beyond the list): whatever the runs say
static void check_stream(const std::string &name, const std::vector<Run> &v, const std::vector<int> &want = {})
{
    const uint32_t n = (uint32_t)v.size();
    if (!n) return;
    for (uint32_t i = 1; i < n; ++i) CHECK(v[i].b >= v[i - 1].b, "%s: the case is not sorted", name.c_str());
    for (uint32_t flat : {0u, 57344u, 65536u + 8192u}) {
        const uint32_t p0 = flat & 0xFFFFu;
        std::vector<uint32_t> lo; std::vector<uint16_t> nar;
        for (const Run &r : v) {
            lo.push_back(((flat + (uint32_t)r.b) & 0xFFFFu) | ((uint32_t)r.len << 16));
            nar.push_back((uint16_t)pdcover::nar_of_lo(lo.back()));
        }
        pdcover::NarState st{pdcover::run_begin(lo[0], p0), 0, lo[0] & 0xFFFFu, 0u, 0};     // as the kernel starts a tile's sweep
        std::vector<int> begins(n, 0);
        for (uint32_t c = 0; c * CW < n; ++c) {
            const uint32_t at = c * CW, cnt = std::min(CW, n - at);
            pdcover::NarState by_rule = st;
            const Held h = rule_runs(nar.data() + at, cnt, by_rule);
            if (cnt == CW) {
                ++g_chunks;
                const pdcover::NarState was = st;
                const bool ok = pdcover::chunk_fast(nar.data() + at, st, TILE);
                if (c < want.size() && want[c] >= 0)
                    CHECK((int)ok == want[c], "%s at flat %u: chunk %u accepted %d, expected %d", name.c_str(), flat, c, (int)ok, want[c]);
                if (ok) {
                    ++g_accepted;
                    CHECK(!h.gap && !h.neg && !h.beyond, "%s at flat %u: chunk %u accepted with a gap %d, a begin < 0 %d, an end > tile %d", name.c_str(), flat, c, (int)h.gap, (int)h.neg, (int)h.beyond);
                    CHECK(st.base == by_rule.base && st.reach == by_rule.reach && st.sum == by_rule.sum && st.gap == by_rule.gap && (st.pb & 255u) == (by_rule.pb & 255u),
                          "%s at flat %u: chunk %u leaves base %d reach %d sum %u gap %d, the rule %d %d %u %d", name.c_str(), flat, c, st.base, st.reach, st.sum, st.gap,
                          by_rule.base, by_rule.reach, by_rule.sum, by_rule.gap);
                    CHECK(st.gap == was.gap, "%s: an accepted chunk changed the gap", name.c_str());
                } else {
                    CHECK(st.base == was.base && st.reach == was.reach && st.sum == was.sum && st.gap == was.gap && st.pb == was.pb, "%s at flat %u: refused chunk %u changed the state", name.c_str(), flat, c);
                    if (h.gap) ++g_ref_gap; else if (h.neg) ++g_ref_neg; else if (h.beyond) ++g_ref_beyond; else ++g_ref_other;
                    st = by_rule;
                }
            } else st = by_rule;
            // ... and the state behind the chunk is seg_sweep_nar's behind the same runs
            bool end_ok = false;
            const pdcover::Seg s = pdcover::seg_sweep_nar(nar.data(), at + cnt, lo[0], lo[at + cnt - 1], p0, TILE, &end_ok, begins.data());
            CHECK(st.base == begins[at + cnt - 1], "%s at flat %u: behind chunk %u the last begin is %d, seg_sweep_nar's %d", name.c_str(), flat, c, st.base, begins[at + cnt - 1]);
            CHECK(st.reach == std::max(s.maxend, 0), "%s at flat %u: behind chunk %u the reach is %d, seg_sweep_nar's largest end %d", name.c_str(), flat, c, st.reach, s.maxend);
            // (a segment does not judge its own first begin, combine() does: first > 0 is the gap the kernel's sweep, whose reach starts at 0, meets at once)
            const int seg_gap = (s.gap || s.first > 0) ? 1 : 0;
            CHECK(st.sum == s.sum && st.gap == seg_gap, "%s at flat %u: behind chunk %u sum %u gap %d, seg_sweep_nar's %u %d", name.c_str(), flat, c, st.sum, st.gap, s.sum, seg_gap);
        }
    }
}

// n runs from b0 on: a run of `len` cells every `step` cells
static std::vector<Run> dense(int b0, uint32_t n, int step = 3, int len = 150)
{
    std::vector<Run> v;
    for (uint32_t i = 0; i < n; ++i) v.push_back(Run{b0 + (int)i * step, len});
    return v;
}
// every run from index i on moved by d cells
static std::vector<Run> moved(std::vector<Run> v, uint32_t i, int d) { for (; i < v.size(); ++i) v[i].b += d; return v; }

static void crafted()
{
    // The streams begin in the look-back bucket, so chunk 0 is never tried (base < 0) and what a case is about stands in chunk 1 (runs 512 .. 1023) or at
    // its border with chunk 2.  (A chunk whose first lane is not within the reach is refused whatever follows: a tile's first chunk behind cell 0.)
    const uint32_t o = CW;
    const std::vector<Run> D = dense(-600, 1700);          // run 511 begins at cell 933
    check_stream("three dense chunks and a rest", D, {0, 1, 1});
    check_stream("a dense stream from cell 0: the first lane's last begin is beyond the reach", dense(0, 1100), {0, 1});
    // a gap between lane 7's last run and lane 8's first
    check_stream("a gap at a lane boundary", moved(D, o + 64, 148), {0, 0, 1});
    check_stream("no gap at a lane boundary: the run abuts (the lane's last begin is beyond the lanes before: refused, by the rule no gap)", moved(D, o + 64, 147), {0, 0, 1});
    check_stream("the lane's last begin one beyond the ends of the lanes before", moved(D, o + 64, 127), {0, 0, 1});
    check_stream("the lane's last begin at the largest end of the lanes before", moved(D, o + 64, 126), {0, 1, 1});
    // a gap inside a lane, behind a long run of an earlier lane: none by the rule
    {
        std::vector<Run> v = dense(-100, 1700, 1, 20);
        v = moved(v, o + 43, 30);                        // lane 5's run 3 begins 31 cells behind its predecessor
        check_stream("a step of 31 inside a lane behind runs of 20 cells", v, {0, 0, 1});
        v[o + 30].len = 255;                             // ... within the 255 cells of run 30, lane 3's
        check_stream("the same behind a long run of an earlier lane", v, {0, 1, 1});
    }
    check_stream("a gap in the middle of a lane", moved(D, o + 8 * 20 + 3, 200), {0, 0, 1});
    check_stream("a gap at a lane's last run", moved(D, o + 8 * 20 + 7, 200), {0, 0, 1});
    check_stream("a gap at the chunk's last run", moved(D, o + 511, 200), {0, 0, 1});
    check_stream("a gap at the chunk's first run", moved(D, o, 200), {0, 0, 1});
    // a gap that only lane 0's predecessor reveals
    check_stream("a gap at a chunk boundary", moved(D, 2 * o, 148), {0, 1, 0});
    check_stream("lane 0's last begin one beyond the reach", moved(D, 2 * o, 127), {0, 1, 0});
    check_stream("lane 0's last begin at the reach", moved(D, 2 * o, 126), {0, 1, 1});
    // differences of 255, 256 and 257 across a word boundary, a lane boundary and a chunk boundary (runs of 255 cells: 255 is no gap; 256 rebuilds as 0):
    // whatever the test says, the state must be the rule's; behind a long run (run 590: 255 cells, the others 3) a difference of 255 must be accepted
    for (int d : {255, 256, 257})
        for (uint32_t at : {o + 8u * 11u + 2u, o + 8u * 11u + 1u, o + 8u * 11u, 2u * o, 2u * o + 8u * 63u, 3u * o - 1u}) {
            const std::vector<Run> v = moved(dense(-600, 1700, 3, 255), at, d - 3);
            check_stream("a difference of " + std::to_string(d) + " at run " + std::to_string(at), v);
        }
    for (uint32_t at : {o + 8u * 11u + 2u, o + 8u * 11u + 1u, o + 8u * 11u}) {
        std::vector<Run> v = dense(100, 1700, 0, 3);
        v[o + 78].len = 255;
        for (uint32_t i = o + 79; i < v.size(); ++i) v[i].len = 0;       // (nothing else reaches that far)
        check_stream("a difference of 255 at run " + std::to_string(at) + " behind a run of 255 cells", moved(v, at, 255), {0, 1, 1});
        check_stream("a difference of 256 at run " + std::to_string(at) + " behind a run of 255 cells", moved(v, at, 256), {0, 1, 1});      // (rebuilt as 0: the end check is what finds it)
    }
    // lengths 0 and 255
    check_stream("empty runs at cell 0", dense(0, 1100, 0, 0), {1, 1});
    check_stream("empty runs, a begin per cell", dense(-100, 1100, 1, 0), {0, 0});
    check_stream("runs of 255 cells every 255", dense(-255 * 600, 1700, 255, 255), {});
    check_stream("runs of 255 cells every 5", dense(-2500, 1700, 5, 255), {0, 1, 1});
    check_stream("runs of 255 cells every 15: the second chunk ends beyond the tile", dense(-7000, 1100, 15, 255), {0, 0});
    // the chunk's largest end at the tile's last cell exactly, and one beyond (1023 * 3 + 150 = 3219)
    check_stream("the largest end equals the tile", dense(TILE - 3219, 1024), {0, 1});
    check_stream("the largest end one beyond the tile", dense(TILE - 3218, 1024), {0, 0});
    for (int c : {TILE - 255, TILE - 254}) {             // ... as the end of a long run of an early lane, every other run ends before it
        std::vector<Run> v = dense(c, 1024, 0, 20);
        v[o + 9].len = 255;
        check_stream("a long run of an early lane ends at cell " + std::to_string(c + 255), v, {0, c + 255 <= TILE ? 1 : 0});
    }
    // base -1 and 0
    check_stream("every run at cell 0", dense(0, 600, 0, 150), {1});
    check_stream("every run at cell -1", dense(-1, 600, 0, 150), {0});
    check_stream("the first chunk's last run begins at cell -1", dense(-1 - 511 * 3, 1100), {0, 0});
    check_stream("the first chunk's last run begins at cell 0", dense(-511 * 3, 1100), {0, 1});
    check_stream("the look-back bucket's first cell", dense(-8192, 1100, 1, 200), {0, 0});
}

static std::vector<Run> random_stream(std::mt19937_64 &rng, int kind)
{
    std::vector<Run> v;
    std::uniform_int_distribution<int> small(0, kind % 3 == 0 ? 5 : (kind % 3 == 1 ? 8 : 20)), len(0, 255), rare(0, kind < 4 ? 1 << 30 : 3000), pick(0, 5), from(-600, 600);
    static const int JUMPS[] = {151, 255, 256, 257, 300, 512};
    int x = kind % 4 == 3 ? from(rng) : (kind % 4 == 2 ? -1500 : 0);
    while (x < TILE) {
        v.push_back(Run{x, kind % 2 ? len(rng) : 150});
        x += rare(rng) < 3 ? JUMPS[pick(rng)] : small(rng);
    }
    return v;
}

static void arithmetic(std::mt19937_64 &rng)
{
    for (int i = 0; i < 20000; ++i) {
        uint32_t x[4], h[9];
        for (uint32_t &w : x) w = (uint32_t)rng();
        const uint32_t before = (uint32_t)rng();
        h[0] = before >> 16;
        for (int k = 0; k < 8; ++k) h[k + 1] = (x[k / 2] >> (16 * (k % 2))) & 0xFFFFu;
        int rb = 0, m = pdcover::NONE; uint32_t lens = 0;
        for (int k = 0; k < 8; ++k) { rb += pdcover::nar_step(h[k + 1], h[k]); m = std::max(m, rb + pdcover::nar_len(h[k + 1])); lens += (uint32_t)pdcover::nar_len(h[k + 1]); }
        const pdcover::NarLane s = pdcover::nar_lane_summary(x, before);
        CHECK(s.T == rb && s.Mrel == m && s.lens == lens, "the lane summary is (%d, %d, %u), run by run (%d, %d, %u)", s.T, s.Mrel, s.lens, rb, m, lens);
        const uint32_t d = pdcover::nar_pair_steps(x[1], pdcover::nar_pred_word(x[1], x[0]));
        CHECK((int)(d & 255u) == pdcover::nar_step(h[3], h[2]) && (int)((d >> 16) & 255u) == pdcover::nar_step(h[4], h[3]), "the packed steps differ from nar_step");
    }
    CHECK(pdcover::chunk_fast_entry(512u, 0) && !pdcover::chunk_fast_entry(512u, -1) && !pdcover::chunk_fast_entry(511u, 0), "the entry test is off");
    CHECK(pdcover::chunk_fast_lane_ok(5, pdcover::NONE, 5) && !pdcover::chunk_fast_lane_ok(6, pdcover::NONE, 5) && pdcover::chunk_fast_lane_ok(6, 6, 0), "the lane test is off");
    CHECK(pdcover::chunk_fast_ok(true, TILE, TILE) && !pdcover::chunk_fast_ok(true, TILE + 1, TILE) && !pdcover::chunk_fast_ok(false, 0, TILE), "the acceptance test is off");
}

int main()
{
    std::mt19937_64 rng(20250611);
    arithmetic(rng);
    crafted();
    for (int i = 0; i < 900; ++i) check_stream("random stream " + std::to_string(i), random_stream(rng, i % 12));
    printf("full chunks checked: %lu, accepted: %lu, refused with a gap: %lu, with a begin < 0: %lu, with an end > tile: %lu, otherwise: %lu\n",
           g_chunks, g_accepted, g_ref_gap, g_ref_neg, g_ref_beyond, g_ref_other);
    CHECK(g_accepted >= 1000 && g_ref_gap >= 300 && g_ref_neg >= 100 && g_ref_beyond >= 20, "the generator is off: every outcome must be well represented");
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("cover_fast_check: ok\n");
    return 0;
}
