// pile_rule_check — the grouping rule of the pile-up pass (pandepth_amd/csrc/pd_pile_rule.h) against a window built run by run.
//
// A "wave" is 64 candidate words r = (b & 0xFFFF) | (len << 16) of a tile whose first flat cell has the low 16 bits p0.  The kernel's way:
// events() gives every lane its begin cell sb and end cell se16 and says whether they lie in the tile; group() over the begin cells (valid:
// the run has cells and begins in the tile) and, on its own, over the end cells (valid: the run has cells and ends in the tile) gives heads
// and multiplicities; a head adds its multiplicity to win[sb], takes it from win[se16].  The reference adds and subtracts 1 per run.
// Both windows, and the carry-in counts, must be equal for every wave; a head's
// multiplicity must be >= 1 and the multiplicities of a wave must add up to its valid lanes; every lane that is not a head must be valid-and-equal to its left neighbour or not valid.
// Stand-alone: own main, no GPU; built by tests/test_pile_rule.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pandepth_amd/csrc/pd_pile_rule.h"

static const uint32_t TILE = 8192;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static int failures = 0;
static uint64_t total_lanes = 0, total_heads = 0;

// a run that begins `rel` cells from the tile's first cell (negative: in the bucket before) and has `len` cells
static uint32_t run_word(uint32_t p0, int rel, uint32_t len) { return ((p0 + (uint32_t)rel) & 0xFFFFu) | (len << 16); }

// returns the heads of the begin grouping
static uint64_t check_wave(const char *what, const uint32_t (&r)[64], uint32_t p0)
{
    std::vector<int> ref(TILE, 0), win(TILE, 0);
    uint32_t carry_ref = 0, carry = 0;
    uint32_t sb[64], se[64];
    uint64_t vb = 0, ve = 0;
    for (int l = 0; l < 64; ++l) {
        // the reference: the run's two events from its begin and length as signed tile-relative numbers, one run at a time
        const int b = (int)(int16_t)(uint16_t)(r[l] - p0);
        const int len = (int)(r[l] >> 16), e = b + len;
        if (len) {
            if (b >= 0 && b < (int)TILE) ref[b] += 1;
            if (e >= 0 && e < (int)TILE) ref[e] -= 1;
            if (b < 0 && e >= 0) ++carry_ref;
        }
        const pdpile::Events ev = pdpile::events(r[l], p0);
        sb[l] = ev.sb; se[l] = ev.se16;
        if (ev.has && ev.sb < TILE) vb |= 1ull << l;
        if (ev.has && ev.se16 < TILE) ve |= 1ull << l;
        if (ev.has && ev.carry) ++carry;
    }
    uint64_t heads_b = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const uint32_t (&v)[64] = pass ? se : sb;
        const uint64_t valid = pass ? ve : vb;
        uint32_t mult[64];
        const uint64_t heads = pdpile::group(v, valid, mult);
        if (!pass) heads_b = heads;
        uint32_t msum = 0;
        for (int l = 0; l < 64; ++l) {
            const bool is_valid = (valid >> l) & 1u, head = (heads >> l) & 1u;
            if (head) {
                if (!is_valid || mult[l] < 1u) { printf("FAIL %s: head at lane %d without a valid run or a size\n", what, l); ++failures; }
                else win[v[l]] += pass ? -(int)mult[l] : (int)mult[l];
                msum += mult[l];
            } else {
                if (mult[l]) { printf("FAIL %s: lane %d is no head but has a multiplicity\n", what, l); ++failures; }
                if (is_valid && (l == 0 || !((valid >> (l - 1)) & 1u) || v[l - 1] != v[l])) { printf("FAIL %s: lane %d begins a group and is no head\n", what, l); ++failures; }
            }
        }
        if (msum != (uint32_t)__builtin_popcountll(valid)) { printf("FAIL %s: multiplicities %u, valid lanes %d\n", what, msum, __builtin_popcountll(valid)); ++failures; }
        total_lanes += (uint64_t)__builtin_popcountll(valid); total_heads += (uint64_t)__builtin_popcountll(heads);
    }
    if (win != ref) { printf("FAIL %s: the grouped window differs from the run-by-run window\n", what); ++failures; }
    if (carry != carry_ref) { printf("FAIL %s: carry-in %u, run by run %u\n", what, carry, carry_ref); ++failures; }
    return heads_b;
}

int main()
{
    const uint32_t p0s[] = {0u, 57344u, 8192u, 32768u, 0xE000u};
    uint32_t r[64];
    for (uint32_t p0 : p0s) {
        // a pile of identical runs: ONE head for the begins, one for the ends
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, 4000, 150);
        uint64_t hb = check_wave("all equal", r, p0);
        if (hb != 1ull) { printf("FAIL all equal: heads %016llx\n", (unsigned long long)hb); ++failures; }
        // all different
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, 100 + 3 * l, 1 + l);
        hb = check_wave("all different", r, p0);
        if (hb != ~0ull) { printf("FAIL all different: heads %016llx\n", (unsigned long long)hb); ++failures; }
        // groups that start at lane 0 and end at lane 63, a group of one between them
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, l < 20 ? 7 : l == 20 ? 9 : 11, 150);
        hb = check_wave("three groups", r, p0);
        if (hb != ((1ull << 0) | (1ull << 20) | (1ull << 21))) { printf("FAIL three groups: heads %016llx\n", (unsigned long long)hb); ++failures; }
        // a group of one at lane 63, and one at lane 0
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, l == 0 ? 1 : l == 63 ? 3 : 2, 10);
        hb = check_wave("singles at the rims", r, p0);
        if (hb != ((1ull << 0) | (1ull << 1) | (1ull << 63))) { printf("FAIL singles at the rims: heads %016llx\n", (unsigned long long)hb); ++failures; }
        // alternating validity on one cell: runs without cells between the pile's
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, 500, (l & 1) ? 0u : 150u);
        hb = check_wave("alternating validity", r, p0);
        if (hb != 0x5555555555555555ull) { printf("FAIL alternating validity: heads %016llx\n", (unsigned long long)hb); ++failures; }
        // alternating between two cells
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, (l & 1) ? 600 : 500, 150);
        check_wave("two cells in turn", r, p0);
        // one begin, lengths cycling
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, 700, 1 + (uint32_t)(l % 150));
        check_wave("one begin, many lengths", r, p0);
        // a pile in the bucket before the tile that reaches into it (carry-in), and one that ends exactly at the tile's first cell
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, -100, l < 32 ? 150u : 100u);
        check_wave("pile before the tile", r, p0);
        // ends exactly at the tile's last cell, at its end, and one past it
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, (int)TILE - 150, l < 20 ? 149u : l < 40 ? 150u : 151u);
        check_wave("ends at the tile's end", r, p0);
        // the tile's first and last cell
        for (int l = 0; l < 64; ++l) r[l] = run_word(p0, l < 32 ? 0 : (int)TILE - 1, 1);
        check_wave("first and last cell", r, p0);
        // nothing valid at all: padding runs
        for (int l = 0; l < 64; ++l) r[l] = (p0 + TILE) & 0xFFFFu;
        hb = check_wave("padding", r, p0);
        if (hb) { printf("FAIL padding: heads %016llx\n", (unsigned long long)hb); ++failures; }
    }
    // random waves: few distinct begins and lengths (long groups), many (short groups), with runs without cells and look-back runs mixed in
    for (int it = 0; it < 20000; ++it) {
        const uint32_t p0 = ((rnd() % 8u) * TILE) & 0xFFFFu;
        const uint32_t nb = 1u + rnd() % (it % 3 == 0 ? 3u : it % 3 == 1 ? 16u : 3000u), nl = 1u + rnd() % 4u;
        const int base = (int)(rnd() % (TILE + 600u)) - 500;      // from the bucket before (at most 512 cells back here) to the tile's end
        int cur = base;
        for (int l = 0; l < 64; ++l) {
            if (rnd() % nb == 0u) cur = base + (int)(rnd() % 40u);
            int b = cur; if (b >= (int)TILE) b = (int)TILE - 1; if (b < -512) b = -512;
            uint32_t len = 140u + rnd() % nl; if (rnd() % 9u == 0u) len = rnd() % 512u;
            if (rnd() % 13u == 0u) len = 0u;
            r[l] = run_word(p0, b, len);
        }
        check_wave("random", r, p0);
    }
    // the share of lanes that are heads on a pile of identical runs, over whole waves: it must be 1/64
    {
        total_lanes = total_heads = 0;
        for (int wv = 0; wv < 500; ++wv) {
            for (int l = 0; l < 64; ++l) r[l] = run_word(0u, 1234, 150);
            check_wave("pile", r, 0u);
        }
        printf("pile of identical runs: lanes %llu, heads %llu, share 1/%llu\n", (unsigned long long)total_lanes, (unsigned long long)total_heads,
               (unsigned long long)(total_heads ? total_lanes / total_heads : 0));
        if (total_heads * 64u != total_lanes) { printf("FAIL pile: share of heads is not 1/64\n"); ++failures; }
    }
    if (failures) { printf("pile_rule_check: %d failures\n", failures); return 1; }
    printf("pile_rule_check: ok\n");
    return 0;
}
