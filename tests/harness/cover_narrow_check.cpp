// cover_narrow_check — the narrow plane of the sorted stream (pandepth_amd/csrc/pd_cover_rule.h: nar_pack, nar_step, nar_end_ok, seg_sweep_nar:
// two bytes per run, begins rebuilt from the differences of their low bytes) against the lo words and a per-cell union, on the CPU.
// Built with -fsanitize=address,undefined by tests/test_cover_narrow_rule.py.  For crafted and random SORTED tiles at the flat offsets of
// cover_rule_check.cpp (the 16-bit seams 57344, 65536 and 131072 among them):
//   * "the end check passes" is equivalent to "every consecutive difference of begins is below 256"
//   * when it passes, the rebuilt begins, the clipped-length sum, the carry and "covered" equal seg_sweep's on the lo words
//   * a tile is never reported covered (no gap, reach >= tile, end check passed) when the per-cell union says otherwise
//   * a gap the narrow sweep meets is a true gap (the sweep on the lo words meets one too), whatever the end check would say
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../pandepth_amd/csrc/pd_cover_rule.h"

static const int TILE = 8192;
struct Run { int b, len; };                              // tile-relative begin (>= -8192: the look-back bucket), cells (<= 255)

static int g_fail = 0;
static unsigned long g_checked = 0, g_passed_check = 0, g_failed_check = 0, g_covered = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; if (g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static const uint64_t FLATS[] = {0, 8192, 57344, 65536, 65536 + 57344, 131072, 3000000000ull / 8192 * 8192};

static bool union_covers(const std::vector<Run> &v)
{
    std::vector<char> c((size_t)TILE, 0);
    for (const Run &r : v)
        for (int x = std::max(r.b, 0); x < std::min(r.b + r.len, TILE); ++x) c[(size_t)x] = 1;
    for (int x = 0; x < TILE; ++x) if (!c[(size_t)x]) return false;
    return true;
}

static void check_tile(const std::string &name, const std::vector<Run> &v, int want_ok /* 1 / 0 / -1: whatever the differences say */, int want_covered /* likewise */)
{
    bool all_small = true;
    for (size_t i = 1; i < v.size(); ++i) {
        CHECK(v[i].b >= v[i - 1].b, "%s: the case is not sorted", name.c_str());
        if (v[i].b - v[i - 1].b >= 256) all_small = false;
    }
    const bool truly = union_covers(v);
    for (uint64_t flat : FLATS) {
        const uint32_t p0 = (uint32_t)flat & 0xFFFFu;
        std::vector<uint32_t> lo; std::vector<uint16_t> nar;
        for (const Run &r : v) {
            CHECK(!pdcover::nar_is_wide((uint32_t)r.len), "%s: a run of %d cells in a narrow case", name.c_str(), r.len);
            lo.push_back((uint32_t)((flat + (uint64_t)(int64_t)r.b) & 0xFFFFu) | ((uint32_t)r.len << 16));
            nar.push_back((uint16_t)pdcover::nar_of_lo(lo.back()));
            CHECK(nar.back() == (uint16_t)pdcover::nar_pack((uint32_t)(flat + (uint64_t)(int64_t)r.b), (uint32_t)r.len), "%s: the two packings differ", name.c_str());
        }
        const uint32_t n = (uint32_t)v.size();
        std::vector<int> begins(n + 1, 0);
        bool ok = false;
        const pdcover::Seg sn = pdcover::seg_sweep_nar(nar.data(), n, n ? lo.front() : 0u, n ? lo.back() : 0u, p0, TILE, &ok, begins.data());
        const pdcover::Seg sw = pdcover::seg_sweep(lo.data(), n, p0, TILE);
        const pdcover::Tile tn = pdcover::combine(&sn, 1, nullptr, 0, TILE), tw = pdcover::combine(&sw, 1, nullptr, 0, TILE);
        ++g_checked;
        CHECK(ok == all_small, "%s at flat %llu: the end check says %d, the differences %d", name.c_str(), (unsigned long long)flat, (int)ok, (int)all_small);
        if (want_ok >= 0) CHECK((int)ok == want_ok, "%s at flat %llu: the end check says %d, expected %d", name.c_str(), (unsigned long long)flat, (int)ok, want_ok);
        for (uint32_t i = 0; i < n; ++i) CHECK(begins[i] <= v[i].b, "%s: run %u rebuilt at %d, beyond its begin %d", name.c_str(), i, begins[i], v[i].b);
        if (ok) {
            ++g_passed_check;
            for (uint32_t i = 0; i < n; ++i) CHECK(begins[i] == v[i].b, "%s at flat %llu: run %u rebuilt at %d, begins at %d", name.c_str(), (unsigned long long)flat, i, begins[i], v[i].b);
            CHECK(sn.sum == sw.sum && sn.carry == sw.carry, "%s at flat %llu: sum %u / carry %u, from the lo words %u / %u", name.c_str(), (unsigned long long)flat, sn.sum, sn.carry, sw.sum, sw.carry);
            CHECK(tn.covered == tw.covered, "%s at flat %llu: covered %d, from the lo words %d", name.c_str(), (unsigned long long)flat, (int)tn.covered, (int)tw.covered);
            CHECK(sn.first == sw.first && sn.maxend == sw.maxend && sn.gap == sw.gap, "%s at flat %llu: the summaries differ", name.c_str(), (unsigned long long)flat);
            CHECK(tw.covered == truly, "%s at flat %llu: the sweep of the lo words says %d, per cell %d", name.c_str(), (unsigned long long)flat, (int)tw.covered, (int)truly);
            if (tn.covered) ++g_covered;
        } else ++g_failed_check;
        CHECK(!(ok && tn.covered) || truly, "%s at flat %llu: reported covered, a cell is not", name.c_str(), (unsigned long long)flat);
        CHECK(!sn.gap || sw.gap, "%s at flat %llu: the narrow sweep met a gap that is none", name.c_str(), (unsigned long long)flat);
        if (want_covered >= 0) CHECK((int)(ok && tn.covered) == want_covered, "%s at flat %llu: settled %d, expected %d", name.c_str(), (unsigned long long)flat, (int)(ok && tn.covered), want_covered);
    }
}

// a dense background: a 150-cell run every `step` cells from `from` until `to` is passed
static std::vector<Run> dense(int from, int to, int step = 3, int len = 150)
{
    std::vector<Run> v;
    for (int x = from; x < to; x += step) v.push_back(Run{x, len});
    return v;
}
static std::vector<Run> join(std::vector<Run> a, const std::vector<Run> &b) { a.insert(a.end(), b.begin(), b.end()); return a; }

static void crafted()
{
    check_tile("no candidates", {}, 1, 0);
    check_tile("one run", {{0, 255}}, 1, 0);
    check_tile("a dense tile", dense(-100, TILE), 1, 1);
    check_tile("a dense tile from the look-back bucket's first cell", dense(-8192, TILE), 1, 1);
    // a difference d among the runs in front of cell 0 (the tile itself is covered: only the end check stands between the rebuild and a wrong sum)
    for (int d : {0, 1, 255, 256, 257, 512, 511, 768, 1024}) {
        std::vector<Run> v = join(join({{-2000, 100}}, {{-2000 + d, 100}}), dense(-2000 + d, TILE));
        if (d >= 256) v = join({{-2000, 100}}, dense(-2000 + d, TILE));      // (nothing between the two: the difference stands)
        check_tile("a difference of " + std::to_string(d) + " before cell 0", v, d < 256, d < 256);
        // ... and inside the tile, where it is a true gap once it exceeds the run before it
        const std::vector<Run> front = dense(-100, 3000);
        const std::vector<Run> w = join(front, dense(front.back().b + d, TILE));
        check_tile("a difference of " + std::to_string(d) + " inside the tile", w, d < 256, d <= 150);
    }
    // a difference of exactly 256 whose gap only the rebuild would close: run of 255 cells, the next 256 behind it — one uncovered cell
    check_tile("a one-cell gap behind a difference of 256", join(join(dense(-100, 3000), {{3000, 255}}), dense(3256, TILE)), 0, 0);
    check_tile("two differences of 256", join(join(dense(-300, 1000), dense(1255, 5000)), dense(5255, TILE)), 0, 0);
    // lengths 0, 1, 254, 255
    for (int len : {0, 1, 254, 255}) {
        check_tile("every run " + std::to_string(len) + " cells, a begin per cell", dense(-300, TILE, 1, len), 1, len >= 1);
        check_tile("every run " + std::to_string(len) + " cells, a begin every 255", dense(-255, TILE, 255, len), 1, len == 255);
    }
    check_tile("empty runs at a gap's edges", join(join(dense(-100, 4000, 3, 150), {{4200, 0}, {4201, 0}}), dense(4201, TILE)), 1, 0);
    // the span at its largest: the first candidate a whole bucket before the tile, the last at cell 8191
    check_tile("the largest span", join(join({{-8192, 255}}, dense(-8000, TILE - 1, 2)), {{8191, 1}}), 1, 1);
    check_tile("the largest span with one hidden difference", join(join({{-8192, 255}}, dense(-7936, TILE - 1, 2)), {{8191, 1}}), 0, 0);
    check_tile("differences of 255 all the way", dense(-8192, TILE, 255, 255), 1, 1);
    check_tile("all runs at one cell", std::vector<Run>(600, Run{17, 30}), 1, 0);
}

static std::vector<Run> random_tile(std::mt19937_64 &rng, int kind)
{
    std::vector<Run> v;
    std::uniform_int_distribution<int> small(0, kind % 3 == 0 ? 6 : 40), len(0, 255), rare(0, kind < 4 ? 1 << 30 : 2000), pick(0, 5);
    static const int JUMPS[] = {255, 256, 257, 511, 512, 1000};
    int x = -(256 << (kind % 6));
    while (x < TILE) {
        v.push_back(Run{x, kind % 2 ? len(rng) : 150});
        x += rare(rng) < 3 ? JUMPS[pick(rng)] : small(rng);
    }
    return v;
}

int main()
{
    crafted();
    CHECK(pdcover::nar_pack(0x1234u, 300u) == (0x34u | (255u << 8)), "a long run is not clamped to 255");
    CHECK(pdcover::nar_is_wide(256u) && !pdcover::nar_is_wide(255u), "the width threshold is off");
    std::mt19937_64 rng(20250117);
    for (int i = 0; i < 600; ++i) check_tile("random tile " + std::to_string(i), random_tile(rng, i % 12), -1, -1);
    printf("tiles x offsets checked: %lu, end check passed: %lu, failed: %lu, settled: %lu\n", g_checked, g_passed_check, g_failed_check, g_covered);
    CHECK(g_passed_check >= 1000 && g_failed_check >= 500 && g_covered >= 500, "the generator is off: every outcome must be well represented");
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("cover_narrow_check: ok\n");
    return 0;
}
