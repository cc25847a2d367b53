// pd_dev.h — what the kernels of pd_kernels.hip, pd_direct.hip and pd_rows.hip share: device code and its launch helpers, included by those three files alone.
#ifndef PD_DEV_H_
#define PD_DEV_H_
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pd_kernels.h"

namespace pdk {

static constexpr int WG = 256;
static constexpr int TILE = PD_TILE;            // cells per tile (8192 -> 32 KiB of LDS)
static_assert(TILE % (WG * 4) == 0, "tile must be a multiple of one int4 row per workgroup");

// ------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------
struct Ev { uint64_t gb, ge; bool valid, has; uint32_t len; };

__device__ __forceinline__ Ev expand(const pd_iv v, const ContigTab tab)
{
    Ev e; e.valid = (v.tid >= 0 && v.tid < tab.n); e.has = false; e.gb = e.ge = 0; e.len = 0;
    if (e.valid) {
        const uint32_t len = tab.len[v.tid];
        const uint64_t off = tab.off[v.tid];
        uint32_t b = v.beg < 0 ? 0u : (uint32_t)v.beg; if (b > len) b = len;
        uint32_t x = v.end < 0 ? 0u : (uint32_t)v.end; if (x > len) x = len;
        e.gb = off + b; e.ge = off + x; e.has = b < x; e.len = e.has ? x - b : 0u;
    }
    return e;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// inclusive prefix sum across the 64 lanes of a wave with DPP row shifts / row broadcasts (pure
// VALU, no LDS crossbar traffic): Hillis-Steele inside each 16-lane row, then row 0->1 and
// 2->3 (row_bcast:15), then lanes 0-31 -> 32-63 (row_bcast:31).
__device__ __forceinline__ int wave_incl_scan(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1,3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2,3
    return x;
}

// the same for a running maximum of signed values (a lane without a source takes INT_MIN, the maximum's identity)
__device__ __forceinline__ int wave_incl_scan_max(int x)
{
    constexpr int ID = (int)0x80000000u;
    auto mx = [](int a, int b) { return a > b ? a : b; };
    x = mx(x, __builtin_amdgcn_update_dpp(ID, x, 0x111, 0xf, 0xf, false));   // row_shr:1
    x = mx(x, __builtin_amdgcn_update_dpp(ID, x, 0x112, 0xf, 0xf, false));   // row_shr:2
    x = mx(x, __builtin_amdgcn_update_dpp(ID, x, 0x114, 0xf, 0xf, false));   // row_shr:4
    x = mx(x, __builtin_amdgcn_update_dpp(ID, x, 0x118, 0xf, 0xf, false));   // row_shr:8
    x = mx(x, __builtin_amdgcn_update_dpp(ID, x, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1,3
    x = mx(x, __builtin_amdgcn_update_dpp(ID, x, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2,3
    return x;
}
typedef int v4i_nt __attribute__((ext_vector_type(4)));

// the first n (0..4) of a lane's four consecutive cells, as bins, into LDS counters h (wave-uniform call)
template <bool FOLD>
__device__ __forceinline__ void hist_lane4(uint32_t *h, const uint32_t (&b)[4], uint32_t n, int lane)
{
    const uint32_t b0 = __builtin_amdgcn_readfirstlane(b[0]);
    const bool uni = n == 4 && b[0] == b0 && b[1] == b0 && b[2] == b0 && b[3] == b0;
    if (__all(uni)) { if (lane == 0) atomicAdd(&h[b0], 256u); return; }
    if (!FOLD) {
#pragma unroll
        for (int q = 0; q < 4; ++q) if ((uint32_t)q < n) atomicAdd(&h[b[q]], 1u);
        return;
    }
    if (!n) return;
    uint32_t cur = b[0], c = 1;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
        if ((uint32_t)q >= n) break;
        if (b[q] == cur) ++c; else { atomicAdd(&h[cur], c); cur = b[q]; c = 1; }
    }
    atomicAdd(&h[cur], c);
}

// Before the barrier that hands the LDS counters to hist_flush: every ds_add this wave issued has completed (s_waitcnt
// lgkmcnt(0); vmcnt / expcnt left alone).  The compiler put no such wait in front of the barrier on the contig-change path, and
// the workgroup-wide copy lost adds of other waves there (tools/dist_bench.py on the 3 Gb sample: profiles/r07_dist_bench_before_lds_wait.json).
__device__ __forceinline__ void lds_drain() { __builtin_amdgcn_s_waitcnt(0xC07F); }

template <typename K>
static int hist_lds_reserve(K kern, size_t lds)
{
    if (lds <= 48 * 1024) return 0;
    return (int)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// lane i takes lane i - 1's value, lane 0 takes `first` (wave_shr:1)
__device__ __forceinline__ int wave_shift_up(int x, int first) { return __builtin_amdgcn_update_dpp(first, x, 0x138, 0xf, 0xf, false); }
// wave totals through the DPP scan (no LDS crossbar): the last lane holds the sum
__device__ __forceinline__ int wave_total(int v) { return __builtin_amdgcn_readlane(wave_incl_scan(v), 63); }

struct WinArgs {
    uint32_t w;              // window width in cells
    uint32_t min_dep;
    float inv_w;
    uint32_t *cover;         // per window (global index = win_off[contig] + k)
    unsigned long long *sum;
    TilePart *part;          // w >= TILE: per-tile partials for the (at most two) windows it touches
};

// ---- narrow windows (4 <= w < TILE): one row of a wave (64 lanes x 4 consecutive cells) into the tile's LDS accumulators ----
// A window's share of a row is a difference of two row-prefix values, so only the lanes that hold a window's last cell touch LDS:
// the (cover << 48 | depth sum) words of the lanes are prefix-summed over the wave, the lane holding the cell before a window
// start adds the prefix there to the window that ends and subtracts it from the one that begins (the fields borrow from each other
// in between; the finished word is exact), and lane 63 adds the row's total to the window of the row's last cell.  About 2 w / 256 + 1
// LDS atomics per row on distinct addresses, where one atomic per lane and window piece (64-128 per row, on 3-4 addresses) was
// what bound these sweeps.
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long x)
{
#define PD_SCAN64_STEP(ctrl, rmask)                                                                                       \
    {                                                                                                                    \
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, ctrl, rmask, 0xf, false);          \
        const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), ctrl, rmask, 0xf, false);  \
        x += ((unsigned long long)hi_ << 32) | lo_;                                                                       \
    }
    PD_SCAN64_STEP(0x111, 0xf) PD_SCAN64_STEP(0x112, 0xf) PD_SCAN64_STEP(0x114, 0xf) PD_SCAN64_STEP(0x118, 0xf)
    PD_SCAN64_STEP(0x142, 0xa) PD_SCAN64_STEP(0x143, 0xc)
#undef PD_SCAN64_STEP
    return x;
}

// (x / w by a multiplication: x = cell + phase < 2^14 and w < 2^13, so floor(x * ceil(2^32 / w) / 2^32) is exact — one instruction per
// row where a float reciprocal with its two corrections took a dozen; these sweeps are bound by their vector instructions, a
// wave64 instruction occupying its SIMD for four cycles, not by HBM)
__device__ __forceinline__ uint32_t narrow_magic(uint32_t w) { return (uint32_t)((0x100000000ull + w - 1) / w); }

__device__ __forceinline__ void narrow_window_row(const uint32_t (&d)[4], uint32_t pos, uint32_t phase, uint32_t w, uint32_t magic, uint32_t min_dep,
                                                  uint32_t cells_left /* cells of the contig from the tile's first, at most TILE */, unsigned long long *acc, int lane)
{
    const uint32_t x = pos + phase;
    const uint32_t q = __umulhi(x, magic);
    const uint32_t k = (q + 1u) * w - x;                          // window q + 1 starts k cells behind this lane's first (k >= 1)
    unsigned long long v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (pos + e < cells_left && d[e] >= min_dep) ? ((1ull << 48) | d[e]) : 0ull;
    const unsigned long long T = v[0] + v[1] + v[2] + v[3];
    const unsigned long long L = wave_incl_scan_u64(T);
    if (k <= 4u && !(lane == 63 && k == 4u)) {
        const unsigned long long I = L - T + v[0] + (k >= 2u ? v[1] : 0ull) + (k >= 3u ? v[2] : 0ull) + (k >= 4u ? v[3] : 0ull);
        if (I) { atomicAdd(&acc[q], I); atomicAdd(&acc[q + 1], 0ull - I); }
    }
    if (lane == 63 && L) atomicAdd(&acc[k <= 3u ? q + 1 : q], L);
}

// The tile's finished accumulators go out with plain stores: windows inside the tile to the window arrays, the share of a window
// that began in the previous tile or goes on in the next one to the tile's TilePart (c0 / s0: first window, c1 / s1: last);
// k_window_edges adds the two halves.  (Global atomics for those two windows kept every workgroup resident for the atomics' round trip
// at its very end: 2.16 ms against 1.49 ms for widths that divide the tile, 2.0e9 cells.)
__device__ __forceinline__ void narrow_write_out(const unsigned long long *acc, uint32_t nacc, uint64_t k0, uint32_t w, uint64_t local0, uint32_t clen,
                                                 uint64_t wbase, const WinArgs &wa, TilePart *pt)
{
    for (uint32_t j = threadIdx.x; j < nacc; j += WG) {
        const unsigned long long a = acc[j];
        const uint32_t c = (uint32_t)(a >> 48);
        const unsigned long long sm = a & 0xFFFFFFFFFFFFull;
        const uint64_t k = k0 + j;
        const bool before = k * w < local0;                                                       // began in the previous tile
        const bool after = (k + 1) * (uint64_t)w > local0 + TILE && local0 + TILE < (uint64_t)clen;   // goes on in the next tile
        if (before) { pt->c0 = c; pt->s0 = sm; }
        else if (after) { pt->c1 = c; pt->s1 = sm; }
        else if (c) { wa.cover[wbase + k] = c; wa.sum[wbase + k] = sm; }
    }
}

} // namespace pdk
#endif
