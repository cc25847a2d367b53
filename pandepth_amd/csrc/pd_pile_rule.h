// pd_pile_rule.h — neighbouring lanes of a wave that add to the SAME cell add once: the grouping rule of the pile-up pass.
//
// k_c8_heavy (pd_direct.hip) and tests/harness/pile_rule_check.cpp (against a window built run by run, on the CPU) share this code.
//
// A wave holds 64 values (the window cells its lanes would add 1 to, or take 1 from) and 64 validity bits (a lane whose run has no cells,
// or whose cell lies outside the tile, adds nothing).  A GROUP is a maximal stretch of consecutive valid lanes with equal values; its first
// lane is its HEAD and the group's size is the head's MULTIPLICITY.  The heads add their multiplicity, every other lane does nothing: the
// sum each cell receives is the number of valid lanes that name it, whatever the order of the values — equal values that are not
// neighbours are simply two groups, two additions to one cell.  On a pile of identical runs the 64 lanes are one group: one addition of 64.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PD_PILE_HD __host__ __device__
#else
#define PD_PILE_HD
#endif

namespace pdpile {

// A lane's KEY is its value (below 2^31) with bit 31 set when the lane is not valid; lane 0's left neighbour has the key NO_LANE.  A valid lane
// is a head when its left neighbour's key differs from its own: another value, or no valid lane at all.
constexpr uint32_t NO_LANE = 0x80000000u;
PD_PILE_HD inline uint32_t lane_key(uint32_t v, bool valid) { return valid ? v : (v | 0x80000000u); }
PD_PILE_HD inline bool is_head(uint32_t key, uint32_t prev_key) { return !(key >> 31) && key != prev_key; }

// the size of the group that head `lane` leads: up to the next head or the next lane that is not valid
PD_PILE_HD inline uint32_t multiplicity(uint64_t heads, uint64_t valid, int lane)
{
    const uint64_t stop = ((heads | ~valid) >> 1) >> lane;       // bit i: lane + 1 + i ends the group
    return stop ? (uint32_t)__builtin_ctzll(stop) + 1u : (uint32_t)(64 - lane);
}

// the whole wave at once: returns the head mask, mult[lane] = the multiplicity of a head, 0 for every other lane
PD_PILE_HD inline uint64_t group(const uint32_t (&v)[64], uint64_t valid, uint32_t (&mult)[64])
{
    uint64_t heads = 0;
    for (int l = 0; l < 64; ++l)
        if (is_head(lane_key(v[l], (valid >> l) & 1u), l ? lane_key(v[l - 1], (valid >> (l - 1)) & 1u) : NO_LANE)) heads |= 1ull << l;
    for (int l = 0; l < 64; ++l) mult[l] = ((heads >> l) & 1u) ? multiplicity(heads, valid, l) : 0u;
    return heads;
}

// a candidate's two events in the pile-up pass's 16-bit arithmetic (k_direct_c8's): r = (b & 0xFFFF) | (len << 16), p0 the low 16 bits of
// the tile's first flat cell.  sb < tile: the run begins in the tile; se16 < tile: it ends there; se >= 2^16: it begins before the tile and
// reaches its first cell (the carry-in).  A run without cells takes no part.
struct Events { uint32_t sb, se16; bool has, carry; };
PD_PILE_HD inline Events events(uint32_t r, uint32_t p0)
{
    const uint32_t sb = (r - p0) & 0xFFFFu, se = sb + (r >> 16);
    return Events{sb, se & 0xFFFFu, (r >> 16) != 0u, se >= 0x10000u};
}

} // namespace pdpile
