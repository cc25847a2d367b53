// cover_rule_check — pandepth_amd/csrc/pd_cover_rule.h (the rule by which k_direct_c8 settles a tile from its runs alone) against a
// per-cell union, on the CPU.  Built with -fsanitize=address,undefined by tests/test_direct_cover_rule.py.
//   * whenever the rule says "covered", every cell of the tile has depth >= 1;  sum and carry always equal the per-cell figures
//   * with ONE segment and a sorted stream the rule is exact
//   * crafted tiles: every split of the sorted candidates into 1 to 4 segments (empty ones included); random tiles: the kernel's
//     quarters and random unequal cuts
//   * prints the share of covered random 50x-like tiles that the kernel's quarters decline; main() fails above 1 in 100
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../pandepth_amd/csrc/pd_cover_rule.h"

static const int TILE = 8192;
struct Run { int b, len; };                              // tile-relative begin (>= -8192: the look-back bucket), cells
struct Case { std::string name; std::vector<Run> sorted, other; };

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; if (g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static std::vector<uint32_t> words(const std::vector<Run> &v, uint64_t flat)
{
    std::vector<uint32_t> w;
    for (const Run &r : v) w.push_back((uint32_t)((flat + (uint64_t)(int64_t)r.b) & 0xFFFFu) | ((uint32_t)r.len << 16));
    return w;
}

struct Brute { bool covered_all, covered_sorted; uint64_t sum; uint32_t carry; };
static Brute brute(const Case &c, uint64_t flat)
{
    std::vector<int> d_all(TILE, 0), d_sorted(TILE, 0);
    Brute out{true, true, 0, 0};
    for (int pass = 0; pass < 2; ++pass)
        for (const Run &r : pass ? c.other : c.sorted) {
            const int64_t fb = (int64_t)flat + r.b, fe = fb + r.len;       // flat cells, full width
            if (fb < (int64_t)flat && fe >= (int64_t)flat) ++out.carry;
            for (int64_t x = std::max<int64_t>(fb, (int64_t)flat); x < std::min<int64_t>(fe, (int64_t)flat + TILE); ++x) {
                ++d_all[(size_t)(x - (int64_t)flat)];
                if (!pass) ++d_sorted[(size_t)(x - (int64_t)flat)];
            }
        }
    for (int x = 0; x < TILE; ++x) {
        out.sum += (uint64_t)d_all[x];
        if (!d_all[x]) out.covered_all = false;
        if (!d_sorted[x]) out.covered_sorted = false;
    }
    return out;
}

// the rule with the sorted candidates cut at cuts[] (ascending, any may coincide: empty segments) and the other stream in n_other pieces
static pdcover::Tile rule(const std::vector<uint32_t> &ws, const std::vector<uint32_t> &wo, const std::vector<size_t> &cuts, int n_other, uint32_t p0)
{
    std::vector<pdcover::Seg> s, o;
    size_t at = 0;
    for (size_t k = 0; k <= cuts.size(); ++k) {
        const size_t end = k < cuts.size() ? cuts[k] : ws.size();
        s.push_back(pdcover::seg_sweep(ws.data() + at, (uint32_t)(end - at), p0, TILE));
        at = end;
    }
    for (int k = 0; k < n_other; ++k) {
        const size_t a = wo.size() * (size_t)k / (size_t)n_other, b = wo.size() * (size_t)(k + 1) / (size_t)n_other;
        o.push_back(pdcover::seg_sweep(wo.data() + a, (uint32_t)(b - a), p0, TILE));
    }
    return pdcover::combine(s.data(), (int)s.size(), o.data(), (int)o.size(), TILE);
}

// the kernel's cut: four quarters of ceil(n / 4) runs
static std::vector<size_t> quarters(size_t n)
{
    const size_t q = (n + 3) / 4;
    return {std::min(q, n), std::min(2 * q, n), std::min(3 * q, n)};
}

static void check_one(const Case &c, uint64_t flat, const Brute &br, const std::vector<size_t> &cuts, int n_other, bool *said_covered = nullptr)
{
    const uint32_t p0 = (uint32_t)flat & 0xFFFFu;
    const pdcover::Tile t = rule(words(c.sorted, flat), words(c.other, flat), cuts, n_other, p0);
    CHECK(!t.covered || br.covered_all, "%s at flat %llu: the rule says covered, a cell is not", c.name.c_str(), (unsigned long long)flat);
    CHECK(!t.covered || br.covered_sorted, "%s at flat %llu: covered, but not by the sorted stream", c.name.c_str(), (unsigned long long)flat);
    CHECK((uint64_t)t.sum == br.sum, "%s at flat %llu: sum %u, per cell %llu", c.name.c_str(), (unsigned long long)flat, t.sum, (unsigned long long)br.sum);
    CHECK(t.carry == br.carry, "%s at flat %llu: carry %u, per cell %u", c.name.c_str(), (unsigned long long)flat, t.carry, br.carry);
    if (said_covered) *said_covered = t.covered;
}

static bool is_sorted_by_begin(const std::vector<Run> &v)
{
    for (size_t i = 1; i < v.size(); ++i) if (v[i].b < v[i - 1].b) return false;
    return true;
}

// a tile of few runs: every split into 1 .. 4 segments; one segment must be exact
static void check_crafted(const Case &c, int want /* 1 covered by ONE sweep, 0 declined, -1 whatever the per-cell union of the sorted stream says */)
{
    static const uint64_t FLATS[] = {0, 8192, 57344, 65536, 65536 + 57344, 131072, 3000000000ull / 8192 * 8192};
    for (uint64_t flat : FLATS) {
        const Brute br = brute(c, flat);
        const size_t n = c.sorted.size();
        bool one = false;
        check_one(c, flat, br, {}, 1, &one);
        if (is_sorted_by_begin(c.sorted)) CHECK(one == br.covered_sorted, "%s: one sweep of a sorted stream says %d, per cell %d", c.name.c_str(), (int)one, (int)br.covered_sorted);
        if (want >= 0) CHECK((int)one == want, "%s: one sweep says %d, expected %d", c.name.c_str(), (int)one, want);
        for (size_t a = 0; a <= n; ++a) {
            check_one(c, flat, br, {a}, 2);
            for (size_t b = a; b <= n; ++b) {
                check_one(c, flat, br, {a, b}, 3);
                for (size_t d = b; d <= n; ++d) check_one(c, flat, br, {a, b, d}, 4);
            }
        }
    }
}

static std::vector<Run> chain(int from, int to, int len, int step)      // abutting / overlapping runs from `from` until `to` is reached
{
    std::vector<Run> v;
    for (int x = from; x < to; x += step) v.push_back(Run{x, std::min(len, 8192)});
    return v;
}

static void crafted()
{
    auto full = [] { return chain(0, TILE, 2048, 2048); };                // four runs cover the tile exactly
    { Case c{"covered by four runs", full(), {}}; check_crafted(c, 1); }
    { Case c{"a one-cell gap at cell 0", {{1, 4096}, {4000, 4192}}, {}}; check_crafted(c, 0); }
    { Case c{"cell 0 by a look-back run only", {{-5, 6}, {1, 4096}, {4000, 4192}}, {}}; check_crafted(c, 1); }
    { Case c{"a one-cell gap at cell TILE - 1", {{0, 4096}, {4096, 4095}}, {}}; check_crafted(c, 0); }
    { Case c{"reach ends at TILE", {{0, 4096}, {4096, 4096}}, {}}; check_crafted(c, 1); }
    { Case c{"reach ends past TILE", {{0, 4096}, {4096, 4200}}, {}}; check_crafted(c, 1); }
    { Case c{"a one-cell gap between two runs (every cut falls on it once)", {{0, 2048}, {2048, 2048}, {4097, 2047}, {6144, 2048}}, {}}; check_crafted(c, 0); }
    { Case c{"no gap between the same runs", {{0, 2048}, {2048, 2049}, {4097, 2047}, {6144, 2048}}, {}}; check_crafted(c, 1); }
    { Case c{"a one-cell gap among the last runs, the other stream behind them", {{0, 4096}, {4096, 4000}, {8090, 50}, {8141, 60}},
             {{8000, 90}, {8142, 10}, {-20, 10}, {-20, 30}}}; check_crafted(c, 0); }
    { Case c{"a look-back run ending exactly at the tile's first cell", {{-100, 100}, {1, 8191}}, {}}; check_crafted(c, 0); }
    { Case c{"a look-back run ending one cell into the tile", {{-100, 101}, {1, 8191}}, {}}; check_crafted(c, 1); }
    { Case c{"look-back runs only, the longest a whole bucket", {{-8192, 8192}, {-8191, 8192}, {-1, 8192}}, {}}; check_crafted(c, 0); }
    { Case c{"look-back runs and one own run", {{-8192, 8192}, {-8191, 8192}, {-1, 8192}, {8191, 1}}, {}}; check_crafted(c, 1); }
    { Case c{"a short run, then a begin beyond its end that an earlier long run covers", {{0, 3000}, {10, 10}, {50, 4096}, {60, 5}, {4100, 4092}}, {}}; check_crafted(c, 1); }
    { Case c{"empty runs at a gap's edges", {{0, 4096}, {4096, 0}, {4097, 0}, {4097, 4095}}, {}}; check_crafted(c, 0); }
    { Case c{"empty runs where there is no gap", {{0, 0}, {0, 4096}, {4096, 0}, {4096, 4096}, {8191, 0}}, {}}; check_crafted(c, 1); }
    { Case c{"empty runs only", {{0, 0}, {100, 0}, {8191, 0}}, {{5, 0}}}; check_crafted(c, 0); }
    { Case c{"an empty run beyond the reach must not extend it", {{0, 100}, {8192 - 1, 0}}, {}}; check_crafted(c, 0); }
    { Case c{"an empty look-back run", {{-10, 0}, {0, 8192}}, {}}; check_crafted(c, 1); }
    { Case c{"a gap that only a run of the other stream covers", {{0, 4096}, {4100, 4092}}, {{4090, 20}, {-3, 3}, {-3, 4}, {8190, 100}}}; check_crafted(c, 0); }
    { Case c{"no candidates", {}, {}}; check_crafted(c, 0); }
    { Case c{"the other stream alone covers", {}, {{0, 8192}}}; check_crafted(c, 0); }
    { Case c{"one run, one bucket long", {{0, 8192}}, {}}; check_crafted(c, 1); }
    { Case c{"not sorted after all: declined or right", {{4096, 4096}, {0, 4096}}, {}}; check_crafted(c, -1); }
    { Case c{"not sorted, covered in this order too", {{0, 4096}, {4000, 4192}, {100, 50}}, {}}; check_crafted(c, 1); }
}

// read starts at `rate` per cell from the look-back bucket on, lengths len_lo .. len_hi; a fifth of the reads has a later run in the other stream
static Case random_tile(std::mt19937_64 &rng, double rate, int len_lo, int len_hi, int bucket)
{
    Case c{"random", {}, {}};
    std::bernoulli_distribution start(rate > 1.0 ? 1.0 : rate), later(0.2);
    std::uniform_int_distribution<int> len(len_lo, len_hi), skip(1, 400);
    const int per_cell = rate > 1.0 ? (int)rate : 1;
    for (int x = -bucket; x < TILE; ++x)
        for (int k = 0; k < per_cell; ++k)
            if (start(rng)) {
                const Run r{x, len(rng)};
                c.sorted.push_back(r);
                if (later(rng)) {
                    const int ob = r.b + r.len + skip(rng);
                    if (ob >= -bucket && ob < TILE) c.other.push_back(Run{ob, len(rng)});
                }
            }
    std::shuffle(c.other.begin(), c.other.end(), rng);
    return c;
}

int main()
{
    crafted();
    std::mt19937_64 rng(20240611);
    uint64_t flat = 0;
    // 50x-like: a begin every 3 cells, 150-base reads (and reads of 30 .. 150 cells); what the kernel's quarters decline
    unsigned covered = 0, declined = 0;
    for (int i = 0; i < 300; ++i) {
        const Case c = i % 2 ? random_tile(rng, 1.0 / 3.0, 30, 150, 256 << (i % 6)) : random_tile(rng, 1.0 / 3.0, 150, 150, 256 << (i % 6));
        flat = (flat + 8192ull * (uint64_t)(1 + i % 9)) % (1ull << 32);
        const Brute br = brute(c, flat);
        bool one = false, four = false;
        check_one(c, flat, br, {}, 1, &one);
        CHECK(one == br.covered_sorted, "random tile %d: one sweep says %d, per cell %d", i, (int)one, (int)br.covered_sorted);
        check_one(c, flat, br, quarters(c.sorted.size()), 4, &four);
        if (br.covered_all) { ++covered; if (!four) ++declined; }
        for (int k = 0; k < 6; ++k) {                                    // random unequal cuts, 2 .. 4 segments
            std::vector<size_t> cuts;
            for (int j = 0; j < 1 + k % 3; ++j) cuts.push_back((size_t)(rng() % (c.sorted.size() + 1)));
            std::sort(cuts.begin(), cuts.end());
            check_one(c, flat, br, cuts, 1 + k % 4);
        }
    }
    // thin and uneven tiles: gaps everywhere, the rule must never be optimistic
    unsigned thin_covered = 0;
    for (int i = 0; i < 300; ++i) {
        const double rate = 1.0 / (double)(8 + 7 * (i % 12));
        const Case c = random_tile(rng, rate, 1, 40 + 30 * (i % 10), 256 << (i % 6));
        flat = (flat + 8192ull * 7) % (1ull << 32);
        const Brute br = brute(c, flat);
        bool one = false;
        check_one(c, flat, br, {}, 1, &one);
        CHECK(one == br.covered_sorted, "thin tile %d: one sweep says %d, per cell %d", i, (int)one, (int)br.covered_sorted);
        check_one(c, flat, br, quarters(c.sorted.size()), 4);
        std::vector<size_t> cuts{(size_t)(rng() % (c.sorted.size() + 1))};
        check_one(c, flat, br, cuts, 3);
        thin_covered += br.covered_sorted;
    }
    // a pile: 20 reads per cell
    {
        const Case c = random_tile(rng, 3.0, 100, 150, 4096);
        const Brute br = brute(c, 65536);
        check_one(c, 65536, br, quarters(c.sorted.size()), 4);
    }
    const double share = covered ? (double)declined / (double)covered : 1.0;
    printf("covered 50x-like tiles: %u, declined by the four quarters: %u, share %.4f\n", covered, declined, share);
    printf("thin tiles covered by the sorted stream: %u of 300\n", thin_covered);
    CHECK(covered >= 290, "only %u of 300 dense tiles are covered: the generator is off", covered);
    CHECK(share <= 0.01, "the rule declines %.4f of the covered 50x-like tiles", share);
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("cover_rule_check: ok\n");
    return 0;
}
