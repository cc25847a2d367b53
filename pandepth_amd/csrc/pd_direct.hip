// pd_direct.hip — the direct depth pass and nothing else: the kernels that turn a sample's runs into window statistics (or the
// multi-GPU sum's 4-bit image) without a difference array in HBM, and their launchers.  k_direct_tiles / k_direct_wide3 read 12-byte
// runs of pending sorted batches, k_direct_c8 a compact sample (C8Sample in pd_kernels.h); k_direct_tiles_heavy / k_c8_heavy take the
// pile-up tiles they list.  The scatter, the sweeps and everything else are pd_kernels.hip's; what both use is pd_dev.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pd_kernels.h"
#include "pd_dev.h"
#include "pd_cover_rule.h"
#include "pd_pile_rule.h"

namespace pdk {

// The DIRECT whole-sample path (windows of >= TILE cells, i.e. whole-chromosome mode): when every
// run of the sample is still pending as sorted batches and the context holds nothing else, the
// difference array never needs to exist in HBM.  One workgroup per tile builds the tile's
// difference window in LDS exactly as k_scatter_tiles does, but instead of flushing it:
//   * the carry into the tile — the depth just before its first cell — is counted from the same
//     candidates: runs that begin before the tile and end at or after its first cell (every such
//     run is among the candidates as long as no run is longer than the look-back `lmax`; longer
//     runs are counted in *n_long and the caller falls back to the materialising path);
//   * the window is prefix-summed from LDS (same row layout / wave scans as k_sweep), wrapped, and
//     reduced to the tile's share of the (at most two) windows it touches.
// HBM traffic: the runs, once (+ the look-back overlap), and 24 bytes per tile.  No inter-workgroup
// dependency, no atomics outside LDS.

// Narrow windows (64 <= w < TILE) for the direct kernels: k_sweep's LDS accumulators (one packed
// 64-bit word per window overlapping the tile: cover in the top 16 bits, depth sum below), fed from
// the registers that hold the tile's local prefix sums.  Called by the whole workgroup.
template <int ROWS>
__device__ __forceinline__ void direct_small_windows(const int4 (&v)[ROWS], const int (&rowex)[ROWS], int base,
                                                     uint32_t wrap_mask, uint32_t local0, uint32_t clen, const WinArgs &wa,
                                                     uint64_t wbase, unsigned long long *acc, TilePart *pt)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t w = wa.w;
    const uint32_t k0 = local0 / w;                              // first window touching the tile
    const uint32_t nacc = (uint32_t)(((uint64_t)local0 + TILE - 1) / w - k0 + 1);
    for (uint32_t j = threadIdx.x; j < nacc; j += WG) acc[j] = 0;
    __syncthreads();
    const uint32_t phase = local0 - k0 * w;                      // offset of the tile inside window k0
    const uint32_t magic = narrow_magic(w);
    const uint32_t left = clen > local0 ? (clen - local0 < (uint32_t)TILE ? clen - local0 : (uint32_t)TILE) : 0u;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int bsum = base + rowex[r];
        const uint32_t pos = (uint32_t)(wv * (ROWS * 256) + r * 256 + lane * 4);
        const uint32_t d[4] = {(uint32_t)(v[r].x + bsum) & wrap_mask, (uint32_t)(v[r].y + bsum) & wrap_mask,
                               (uint32_t)(v[r].z + bsum) & wrap_mask, (uint32_t)(v[r].w + bsum) & wrap_mask};
        narrow_window_row(d, pos, phase, w, magic, wa.min_dep, left, acc, lane);
    }
    __syncthreads();
    narrow_write_out(acc, nacc, k0, w, local0, clen, wbase, wa, pt);
}

// One candidate run of the direct pass; per-lane counters (summed over the wave by the caller).
struct DirectCnt { uint32_t n_beg; int open; int carry; };

__device__ __forceinline__ void direct_candidate(const pd_iv v, int32_t ctg, uint32_t clen, uint32_t p0, unsigned *win,
                                                 DirectCnt &c)
{
    constexpr uint32_t ST = TILE;
    uint32_t bb = v.beg < 0 ? 0u : (uint32_t)v.beg; if (bb > clen) bb = clen;
    uint32_t x = v.end < 0 ? 0u : (uint32_t)v.end; if (x > clen) x = clen;
    // tile-relative begin / end in 32-bit arithmetic: a position before the tile wraps to a huge value
    // (candidates lie within lmax + D cells of the tile, far from 2^32)
    const uint32_t sb = bb - p0, se = x - p0;
    const bool mine = v.tid == ctg, nonempty = bb < x;
    const bool pb = mine && sb < ST;                              // owns the begin (an empty run still has an owner)
    const bool eb = pb && nonempty, ee = mine && nonempty && se < ST;
    if (eb) atomicAdd(&win[sb >> 1], 1u + (sb & 1u) * 0xFFFFu);
    if (ee) atomicSub(&win[se >> 1], 1u + (se & 1u) * 0xFFFFu);
    // selects of values, not increments under the conditions: conditional increments of the three counters were
    // compiled to ONE indexed read-modify-write of a scratch slot (12 bytes of private memory in every direct kernel)
    c.n_beg += pb ? 1u : 0u;
    c.open += (eb ? 1 : 0) - (ee ? 1 : 0);
    c.carry += (mine && nonempty && bb < p0 && x >= p0) ? 1 : 0;  // covers the cell just before the tile
}

struct DirectWide { static constexpr bool narrow = false, exporting = false; uint32_t w, min_dep; TilePart *part; uint32_t cover_min = 0; /* k_direct_c8's cover pass: tiles with fewer candidates are left to the window */
                    uint32_t cover_fast = 0; /* ... and its narrow sweep tries the fast chunk (pd_cover_rule.h) */ };
struct DirectNarrow { static constexpr bool narrow = true, exporting = false; WinArgs wa; const uint64_t *win_off; };
struct DirectExport {                  // the multi-GPU sum's 4-bit image straight from the tile windows (pd_export_i4)
    static constexpr bool narrow = false, exporting = true;
    unsigned short *img; pd_exc *exc; uint32_t cap; uint32_t *count; int *sums;
};

// A = DirectWide: windows >= TILE, per-tile partials (the bench's instantiation);
// A = DirectNarrow: 64 <= w < TILE, LDS accumulators, results straight into the window arrays;
// A = DirectExport: no statistics — the tile's difference window leaves as nibbles (k_export_i4's image), its cells
//                   outside [-8, 7] as exceptions, its sum as the tile sum: what a rank puts on the links.
template <int UN, int WPE, class A>
__global__ __launch_bounds__(WG, WPE) void k_direct_tiles(const PendSet ps, uint32_t n_tiles, ContigTab tab,
                                                        const uint32_t *tile_contig, uint32_t wrap_mask, const A args,
                                                        uint32_t *n_long, uint32_t *heavy_list, uint32_t *heavy_count)
{
    constexpr bool NARROW = A::narrow, EXPORT = A::exporting;
    uint32_t w = (uint32_t)TILE, min_dep = 1; TilePart *part = nullptr;
    if constexpr (NARROW) { w = args.wa.w; min_dep = args.wa.min_dep; }
    else if constexpr (!EXPORT) { w = args.w; min_dep = args.min_dep; part = args.part; }
    __shared__ unsigned long long acc[NARROW ? TILE / 64 + 2 : 1];
    constexpr int ST = TILE;
    constexpr int ROWS = TILE / (WG * 4);                        // 8
    // two signed 16-bit counters per word, kept as ONE 32-bit sum 65536 * H + L: half the LDS of an
    // int window, twice the resident workgroups.  L = sign-extended low half and H = (word - L) >> 16
    // are exact while both stay within +-32767, which holds when the tile has fewer candidates than
    // that; heavier tiles (pile-ups) go on the heavy list and are done by k_direct_tiles_heavy with
    // an int window.
    __shared__ __attribute__((aligned(16))) unsigned win[ST / 2];
    __shared__ int s_carry;
    __shared__ int wtot[4];
    __shared__ unsigned long long red_s[4][2];
    __shared__ int red_c[4][2];
    __shared__ uint32_t s_lo[PD_MAXPEND], s_hi[PD_MAXPEND];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // summed over the batches: begins that found their owner tile; runs with cells whose begin was owned
    // minus ends that were owned (must cancel: a run that reaches into a tile without being one of its
    // candidates — longer than the look-back — leaves its end unowned, so this also catches long runs)
    uint32_t n_beg = 0; int open = 0;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t a = t * ST;
        if (threadIdx.x < PD_MAXPEND) {
            const int b = threadIdx.x;
            uint32_t lo = 0, hi = 0;
            if (b < ps.nb) {
                const uint32_t tf = ps.b[b].desc->t_first, na = ps.b[b].desc->n_active;
                if (t >= tf && t < (uint64_t)tf + na) {
                    const uint32_t n = ps.b[b].n;
                    hi = ps.b[b].ub_a[t + 1]; if (hi > n) hi = n;
                    lo = ps.b[b].cand_lo[t]; if (lo > hi) lo = hi;
                }
            }
            s_lo[b] = lo; s_hi[b] = hi;
        }
        uint4 *w4 = reinterpret_cast<uint4 *>(win);
        for (int j = threadIdx.x; j < ST / 8; j += WG) w4[j] = make_uint4(0u, 0u, 0u, 0u);
        if (threadIdx.x == 0) s_carry = 0;
        const int32_t ctg = (int32_t)tile_contig[t];
        const uint32_t clen = tab.len[ctg];
        const uint32_t p0 = (uint32_t)(a - tab.off[ctg]);         // tile start inside the contig (slots are < 2^32 cells)
        __syncthreads();
        uint32_t cand = 0;
        for (int b = 0; b < ps.nb; ++b) cand += s_hi[b] - s_lo[b];
        if (cand > 32000u) {                                      // workgroup-uniform
            if (threadIdx.x == 0) heavy_list[atomicAdd(heavy_count, 1u)] = (uint32_t)t;
            __syncthreads();
            continue;
        }
        DirectCnt cnt{0u, 0, 0};
#pragma unroll 1
        for (int b = 0; b < ps.nb; ++b) {
            const uint32_t lo = s_lo[b], hi = s_hi[b];
            if (lo >= hi) continue;
            const pd_iv *__restrict__ iv = ps.b[b].iv;
            uint32_t i = lo;                                      // uniform
            // full chunks: scalar base + constant per-lane offsets, no bounds tests
            for (; i + UN * WG <= hi; i += UN * WG) {
                const pd_iv *__restrict__ p = iv + i;
                pd_iv vv[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) vv[u] = p[threadIdx.x + u * WG];
#pragma unroll
                for (int u = 0; u < UN; ++u) direct_candidate(vv[u], ctg, clen, p0, win, cnt);
            }
            if (i < hi) {                                         // the tail chunk
                const pd_iv *__restrict__ p = iv + i;
                const uint32_t left = hi - i;
                pd_iv vv[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const uint32_t j = threadIdx.x + u * WG;
                    vv[u] = p[j < left ? j : left - 1];
                    if (j >= left) vv[u].tid = -1;                // never equals a contig id
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) direct_candidate(vv[u], ctg, clen, p0, win, cnt);
            }
        }
        n_beg += cnt.n_beg; open += cnt.open;
        const int carry = wave_sum(cnt.carry);
        if (lane == 0 && carry != 0) atomicAdd(&s_carry, carry);
        __syncthreads();
        if constexpr (EXPORT) {
            // k_export_i4's layout: one ushort (4 cells, nibble d + 8) per lane and row, 128 contiguous bytes per wave store
            const uint64_t cw = a + (uint64_t)wv * (ROWS * 256);
            unsigned short *o = args.img + cw / 4 + lane;
            int tsum = 0;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const uint2 q = reinterpret_cast<const uint2 *>(win)[wv * (ROWS * 64) + r * 64 + lane];
                const int l0 = (int)(short)(q.x & 0xffffu), l1 = (int)(short)(q.y & 0xffffu);
                int x[4] = {l0, ((int)q.x - l0) >> 16, l1, ((int)q.y - l1) >> 16};
                unsigned wb = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    tsum += x[k];
                    if (x[k] > 7 || x[k] < -8) {
                        const uint32_t slot = atomicAdd(args.count, 1u);
                        if (slot < args.cap) { args.exc[slot].cell = cw + (uint64_t)(r * 256 + lane * 4 + k); args.exc[slot].value = x[k]; args.exc[slot].pad = 0; }
                        x[k] = 0;
                    }
                    wb |= (unsigned)((x[k] + 8) & 0xf) << (4 * k);
                }
                o[r * 64] = (unsigned short)wb;
            }
            tsum = wave_sum(tsum);
            if (lane == 0) wtot[wv] = tsum;
            __syncthreads();
            if (threadIdx.x == 0) args.sums[t] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
            __syncthreads();
            continue;
        }
        // ---- prefix sum of the window, straight from LDS (k_sweep's layout) ----
        int4 v[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint2 q = reinterpret_cast<const uint2 *>(win)[wv * (ROWS * 64) + r * 64 + lane];
            const int l0 = (int)(short)(q.x & 0xffffu), l1 = (int)(short)(q.y & 0xffffu);
            v[r] = make_int4(l0, ((int)q.x - l0) >> 16, l1, ((int)q.y - l1) >> 16);
        }
        int tot[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            v[r].y += v[r].x; v[r].z += v[r].y; v[r].w += v[r].z;
            tot[r] = v[r].w;
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) tot[r] = wave_incl_scan(tot[r]);
        int run = 0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int e = run + tot[r] - v[r].w;                  // exclusive prefix of this lane's group in the wave
            run += __builtin_amdgcn_readlane(tot[r], 63);
            tot[r] = e;
        }
        if (lane == 0) wtot[wv] = run;
        __syncthreads();
        int base = s_carry;
        for (int k = 0; k < wv; ++k) base += wtot[k];
        if constexpr (NARROW) {                                   // narrow windows: LDS accumulators
            if (p0 < clen) direct_small_windows<ROWS>(v, tot, base, wrap_mask, p0, clen, args.wa, args.win_off[ctg], acc, args.wa.part + t);
            __syncthreads();
            continue;
        }
        // ---- the tile's share of windows k0 and k0 + 1 ----
        const uint64_t local0 = p0;
        int c0 = 0, c1 = 0; unsigned long long s0 = 0, s1 = 0;
        if (local0 < clen) {
            const uint64_t k0 = local0 / w;
            const uint64_t nb64 = (k0 + 1) * (uint64_t)w - local0;   // tile-local start of window k0+1
            const uint32_t nb = nb64 > (uint64_t)ST ? (uint32_t)ST : (uint32_t)nb64;
            const uint64_t left = (uint64_t)clen - local0;           // cells of the contig from the tile start on
            const uint32_t lim = left > (uint64_t)ST ? (uint32_t)ST : (uint32_t)left;
            const uint64_t dmax = (uint64_t)(uint32_t)s_carry + cand;     // no depth in this tile exceeds carry + begins
            if (nb >= (uint32_t)ST && lim >= (uint32_t)ST && min_dep <= 1u && dmax < (1u << 27) && dmax <= wrap_mask) {
                // the common tile — inside one window, inside the contig, no wrap possible, threshold <= 1:
                // the depths need not be formed: sum = sum of the local prefixes + 4 x base per row,
                // covered cells = those whose local prefix differs from -base (all of them for threshold 0)
                uint32_t s32 = 0;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int bsum = base + tot[r];
                    s32 += (uint32_t)(v[r].x + v[r].y + v[r].z + v[r].w) + 4u * (uint32_t)bsum;
                    if (min_dep) {
                        const int z = -bsum;
                        c0 += (v[r].x != z ? 1 : 0) + (v[r].y != z ? 1 : 0) + (v[r].z != z ? 1 : 0) + (v[r].w != z ? 1 : 0);
                    } else c0 += 4;
                }
                s0 = s32;
            } else if (nb >= (uint32_t)ST && lim >= (uint32_t)ST && dmax < (1u << 27)) {
                // the common tile: inside one window and inside the contig — no position tests; no depth
                // exceeds carry + begins in the tile < 2^27, so a lane's 32 cells add up in 32 bits
                uint32_t s32 = 0;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int bsum = base + tot[r];
                    const uint32_t d[4] = {(uint32_t)(v[r].x + bsum) & wrap_mask, (uint32_t)(v[r].y + bsum) & wrap_mask,
                                           (uint32_t)(v[r].z + bsum) & wrap_mask, (uint32_t)(v[r].w + bsum) & wrap_mask};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool ok = d[q] >= min_dep;
                        c0 += ok ? 1 : 0;
                        s32 += ok ? d[q] : 0u;
                    }
                }
                s0 = s32;
            } else if (nb >= (uint32_t)ST && lim >= (uint32_t)ST) {
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int bsum = base + tot[r];
                    const uint32_t d[4] = {(uint32_t)(v[r].x + bsum) & wrap_mask, (uint32_t)(v[r].y + bsum) & wrap_mask,
                                           (uint32_t)(v[r].z + bsum) & wrap_mask, (uint32_t)(v[r].w + bsum) & wrap_mask};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool ok = d[q] >= min_dep;
                        c0 += ok ? 1 : 0;
                        s0 += ok ? d[q] : 0u;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int bsum = base + tot[r];
                    const uint32_t pos = (uint32_t)(wv * (ROWS * 256) + r * 256 + lane * 4);
                    const uint32_t d[4] = {(uint32_t)(v[r].x + bsum) & wrap_mask, (uint32_t)(v[r].y + bsum) & wrap_mask,
                                           (uint32_t)(v[r].z + bsum) & wrap_mask, (uint32_t)(v[r].w + bsum) & wrap_mask};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool ok = pos + q < lim && d[q] >= min_dep;
                        if (ok) { if (pos + q < nb) { ++c0; s0 += d[q]; } else { ++c1; s1 += d[q]; } }
                    }
                }
            }
        }
        c0 = wave_sum(c0); c1 = wave_sum(c1);
#pragma unroll
        for (int o = 32; o; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
        if (lane == 0) { red_c[wv][0] = c0; red_c[wv][1] = c1; red_s[wv][0] = s0; red_s[wv][1] = s1; }
        __syncthreads();
        if (threadIdx.x == 0) {
            TilePart tp;
            tp.c0 = (uint32_t)(red_c[0][0] + red_c[1][0] + red_c[2][0] + red_c[3][0]);
            tp.c1 = (uint32_t)(red_c[0][1] + red_c[1][1] + red_c[2][1] + red_c[3][1]);
            tp.s0 = red_s[0][0] + red_s[1][0] + red_s[2][0] + red_s[3][0];
            tp.s1 = red_s[0][1] + red_s[1][1] + red_s[2][1] + red_s[3][1];
            part[t] = tp;
        }
        __syncthreads();
    }
    // every begin and every end must have found its owner tile: totals over all batches go to batch 0's
    // counters (k_finish_direct compares sums, which is as strict: no run can be counted twice)
    __shared__ unsigned s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    {
        const int hb = wave_sum((int)n_beg), ho = wave_sum(open);
        if (lane == 0) {
            if (hb) atomicAdd(&s_cnt[0], (unsigned)hb);
            if (ho) atomicAdd(&s_cnt[1], (unsigned)ho);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        BatchDesc *desc = ps.b[0].desc;
        if (s_cnt[0]) atomicAdd((unsigned long long *)desc->handled + (blockIdx.x & (PD_CNT_SLOTS - 1)), (unsigned long long)s_cnt[0]);
        // signed total of (owned begins with cells) - (owned ends), as a 64-bit two's complement sum in `has`
        if (s_cnt[1]) atomicAdd((unsigned long long *)desc->has + (blockIdx.x & (PD_CNT_SLOTS - 1)), (unsigned long long)(long long)(int)s_cnt[1]);
    }
    (void)n_long;
}

// The 4-bit image of one tile straight from its packed window (pd_export_i4's layout: one nibble d + 8 per cell, cell 2k in the
// low half of byte k; cells outside [-8, 7] leave as exceptions and are 0 in the image), and the tile's sum.  A lane packs the 4
// cells of each of its 4 rows to 16 bits per half-tile; the halfwords go through a KiB of LDS per wave and come back as ONE
// 16-byte piece per lane — lanes 0..31 the wave's 512 bytes of the low half-tile's image, lanes 32..63 those of the high
// half-tile's: a wave stores its KiB with one 16-byte store per lane (it was eight 2-byte stores per lane).  Exceptions are
// rare: the hot loop only notes which rows have one, a second look at those words emits them.
template <int ROWS>
__device__ __forceinline__ void export_packed_tile(const unsigned *win, const uint64_t a, const uint64_t t, const DirectExport &ex, int *wtot)
{
    constexpr uint32_t HT = TILE / 2;
    __shared__ __attribute__((aligned(16))) unsigned short stage[4][2 * ROWS * 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint4 *w4 = reinterpret_cast<const uint4 *>(win);
    unsigned short *stg = stage[wv];
    int tsum = 0;                                             // packed: sum over the lane's words
    unsigned odd = 0;                                         // bit r: row r of this lane has a cell outside [-8, 7]
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint4 q = w4[wv * (ROWS * 64) + r * 64 + lane];
        const unsigned wq[4] = {q.x, q.y, q.z, q.w};
        unsigned wl = 0, wh = 0, bad = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tsum += (int)wq[k];
            const int xl = (int)(short)(wq[k] & 0xffffu), xh = ((int)wq[k] - xl) >> 16;
            const unsigned nl = (unsigned)(xl + 8), nh = (unsigned)(xh + 8);
            bad |= (nl | nh) >> 4;                            // nonzero: out of the nibble's range
            wl |= (nl < 16u ? nl : 8u) << (4 * k);
            wh |= (nh < 16u ? nh : 8u) << (4 * k);
        }
        odd |= (bad ? 1u : 0u) << r;
        stg[r * 64 + lane] = (unsigned short)wl;
        stg[ROWS * 64 + r * 64 + lane] = (unsigned short)wh;
    }
    if (__builtin_amdgcn_ballot_w64(odd != 0)) {              // rare
#pragma unroll 1
        for (int idx = 0; idx < ROWS * 4; ++idx) {
            const int r = idx >> 2, k = idx & 3;
            if (!((odd >> r) & 1u)) continue;
            const unsigned wd = win[wv * (ROWS * 256) + r * 256 + lane * 4 + k];
            const int xl = (int)(short)(wd & 0xffffu), xh = ((int)wd - xl) >> 16;
            const uint64_t cell = a + (uint64_t)(wv * (ROWS * 256) + r * 256 + lane * 4 + k);
            if ((unsigned)(xl + 8) > 15u) {
                const uint32_t slot = atomicAdd(ex.count, 1u);
                if (slot < ex.cap) { ex.exc[slot].cell = cell; ex.exc[slot].value = xl; ex.exc[slot].pad = 0; }
            }
            if ((unsigned)(xh + 8) > 15u) {
                const uint32_t slot = atomicAdd(ex.count, 1u);
                if (slot < ex.cap) { ex.exc[slot].cell = cell + HT; ex.exc[slot].value = xh; ex.exc[slot].pad = 0; }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint4 piece = reinterpret_cast<const uint4 *>(stg)[lane];
    unsigned char *img = reinterpret_cast<unsigned char *>(ex.img);
    const uint64_t at = a / 2 + (uint64_t)wv * (ROWS * 128) + (lane < 32 ? (uint64_t)lane * 16 : (uint64_t)(HT / 2) + (uint64_t)(lane - 32) * 16);
    *reinterpret_cast<uint4 *>(img + at) = piece;
    tsum = wave_total(tsum);                                  // packed 65536 * H + L over the wave (|H|, |L| <= 32 000)
    if (lane == 0) wtot[wv] = tsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tp = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        const int tl2 = (int)(short)(tp & 0xffff);
        ex.sums[t] = tl2 + ((tp - tl2) >> 16);
    }
    __syncthreads();
}

// k_direct_wide3 — the wide-window (w >= TILE) direct kernel, second form.  Same results as k_direct_tiles<.., DirectWide>
// (TilePart per tile, owner / open counters for k_finish_direct, heavy list); the SIMDs were 65 % busy with vector ALU work
// in that kernel (SQ_ACTIVE_INST_VALU), so this one does the same job in fewer instructions:
//   * SPLIT-HALF window: word j of the 16 KB window holds cell j in its low and cell j + TILE/2 in its high 16 bits (the
//     same "one 32-bit sum 65536 * H + L" arithmetic).  Both half-tiles go through the prefix sum in the SAME registers —
//     additions are linear in that packing — so the scan is over 4096 words, not 8192 cells: 4 row scans per lane, not 8;
//     the halves are only taken apart where depths are formed.  The event address is a mask and a shift.
//   * covered cells are counted with wave ballots of the compare masks (scalar popcounts), not per-lane adds + a reduction;
//     the remaining wave totals go through the DPP scan instead of the LDS crossbar.
//   * tiles that are not at a contig's first cell and lie entirely inside it skip the clamps of run begin / end — they cannot
//     change which cells of the tile a run touches; owner / open / carry counts are ballots accumulated in scalar registers.
//   * the tail chunk of a candidate range issues its loads together, as before, and skips the empty load slots.
#ifdef PD_WIDE3_TICKS                     /* development build only (tools/ubench/wide3_ticks.sh): shader-clock cycles per phase of a tile, summed over waves */
__device__ unsigned long long g_wide3_ticks[16];
#define W3_TICK(k) do { const long long now_ = (long long)clock64(); tk[k] += now_ - t_prev; t_prev = now_; } while (0)
#else
#define W3_TICK(k) do { } while (0)
#endif
template <int UN, int WPE, bool EXPORT>
__global__ __launch_bounds__(WG, WPE) void k_direct_wide3(const PendSet ps, uint32_t n_tiles, ContigTab tab,
                                                        const uint32_t *tile_contig, uint32_t wrap_mask, const DirectWide args,
                                                        uint32_t *heavy_list, uint32_t *heavy_count, const DirectExport ex)
{
    const uint32_t w = args.w, min_dep = args.min_dep; TilePart *const part = args.part;
    constexpr uint32_t ST = TILE, HT = TILE / 2;                 // cells per tile, per half-tile (= words of the window)
    constexpr int ROWS = (int)(HT / (WG * 4));                   // 4 rows of 4 words per lane
    __shared__ __attribute__((aligned(16))) unsigned win[HT];
    __shared__ int s_carry;
    __shared__ int wtot[4];
    __shared__ unsigned long long red_s[4][2];
    __shared__ int red_c[4][2];
    __shared__ uint32_t s_lo[PD_MAXPEND], s_hi[PD_MAXPEND];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t n_beg_s = 0; int open_s = 0;                        // owner / open counts: wave-uniform (scalar popcounts of compare masks)
    // the batches' active tile ranges and run arrays do not change from tile to tile; the candidate bounds of the NEXT tile
    // are fetched while this one is worked on (two dependent loads off the critical path)
    __shared__ uint32_t s_tf[PD_MAXPEND], s_te[PD_MAXPEND], s_n[PD_MAXPEND];
    __shared__ const pd_iv *s_iv[PD_MAXPEND];
    if (threadIdx.x < PD_MAXPEND) {
        const int b = threadIdx.x;
        uint32_t tf = 0, na = 0, n = 0; const pd_iv *ivp = nullptr;
        if (b < ps.nb) { tf = ps.b[b].desc->t_first; na = ps.b[b].desc->n_active; n = ps.b[b].n; ivp = ps.b[b].iv; }
        s_tf[b] = tf; s_te[b] = tf + na; s_n[b] = n; s_iv[b] = ivp;
    }
    __syncthreads();
    auto bounds = [&](const uint64_t t, uint32_t &lo, uint32_t &hi) {       // threads < PD_MAXPEND: batch threadIdx.x, tile t
        lo = 0; hi = 0;
        const int b = threadIdx.x;
        if (b < ps.nb && t < n_tiles && t >= s_tf[b] && t < s_te[b]) {
            const uint32_t n = s_n[b];
            hi = ps.b[b].ub_a[t + 1]; if (hi > n) hi = n;
            lo = ps.b[b].cand_lo[t]; if (lo > hi) lo = hi;
        }
    };
    uint32_t nlo = 0, nhi = 0;
    if (threadIdx.x < PD_MAXPEND) bounds(blockIdx.x, nlo, nhi);
#ifdef PD_WIDE3_TICKS
    long long tk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_prev = (long long)clock64();
#endif
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t a = t * ST;
        if (threadIdx.x < PD_MAXPEND) { s_lo[threadIdx.x] = nlo; s_hi[threadIdx.x] = nhi; }
        uint4 *w4 = reinterpret_cast<uint4 *>(win);
        for (uint32_t j = threadIdx.x; j < HT / 4; j += WG) w4[j] = make_uint4(0u, 0u, 0u, 0u);
        if (threadIdx.x == 0) s_carry = 0;
        const int32_t ctg = (int32_t)tile_contig[t];
        const uint32_t clen = tab.len[ctg];
        const uint32_t p0 = (uint32_t)(a - tab.off[ctg]);         // tile start inside the contig (slots are < 2^32 cells)
        W3_TICK(0);                                               // bounds to LDS, window zeroed
        __syncthreads();
        W3_TICK(1);                                               // barrier 1
        if (threadIdx.x < PD_MAXPEND) bounds(t + gridDim.x, nlo, nhi);
        uint32_t cand = 0;
        for (int b = 0; b < ps.nb; ++b) cand += s_hi[b] - s_lo[b];
        if (cand > 32000u) {                                      // workgroup-uniform: the int-window kernel does this tile
            if (threadIdx.x == 0) heavy_list[atomicAdd(heavy_count, 1u)] = (uint32_t)t;
            __syncthreads();
            continue;
        }
        const bool interior = p0 > 0u && clen < 0x7FFFFFFFu && clen > p0 && clen - p0 >= ST;
        int carry_s = 0;                                          // wave-uniform
        // one candidate.  The predicates are single compares whose wave masks (ballots of the compares themselves: no
        // extra vector work) are combined and counted in scalar registers; only the two LDS events are per-lane work.
#define PD_B(x) __builtin_amdgcn_ballot_w64(x)
        auto one = [&](const pd_iv v, const bool fast) {
            uint32_t sb, se;
            unsigned long long m_ne, m_cov;
            bool nonempty;
            if (fast) {
                sb = (uint32_t)v.beg - p0; se = (uint32_t)v.end - p0;
                nonempty = v.beg < v.end;
                m_ne = PD_B(v.beg < v.end);
                m_cov = PD_B(v.beg < (int32_t)p0) & PD_B(v.end >= (int32_t)p0);   // begins before the tile, reaches its first cell or further
            } else {
                uint32_t bb = v.beg < 0 ? 0u : (uint32_t)v.beg; if (bb > clen) bb = clen;
                uint32_t x = v.end < 0 ? 0u : (uint32_t)v.end; if (x > clen) x = clen;
                sb = bb - p0; se = x - p0;
                nonempty = bb < x;
                m_ne = PD_B(bb < x);
                m_cov = PD_B(bb < p0) & PD_B(x >= p0);
            }
            const unsigned long long m_mine = PD_B(v.tid == ctg), m_sb = PD_B(sb < ST), m_se = PD_B(se < ST);
            const unsigned long long m_pb = m_mine & m_sb;        // owns the begin (an empty run still has an owner)
            const unsigned long long m_eb = m_pb & m_ne, m_ee = m_mine & m_ne & m_se;
            if (v.tid == ctg && nonempty) {
                if (sb < ST) atomicAdd(&win[sb & (HT - 1u)], 1u + (sb >> 12) * 0xFFFFu);
                if (se < ST) atomicSub(&win[se & (HT - 1u)], 1u + (se >> 12) * 0xFFFFu);
            }
            n_beg_s += (uint32_t)__builtin_popcountll(m_pb);
            open_s += __builtin_popcountll(m_eb) - __builtin_popcountll(m_ee);
            carry_s += __builtin_popcountll(m_mine & m_ne & m_cov);
        };
#undef PD_B
        // chunks of UN x WG candidates, stream after stream; the loads of chunk k + 1 (same stream or the next one) are in
        // flight while chunk k is worked on
        {
            auto load_chunk = [&](pd_iv (&dst)[UN], const int b, const uint32_t i) {
                const pd_iv *__restrict__ p = s_iv[b];
                const uint32_t last = s_hi[b] - 1u;
#pragma unroll
                for (int k = 0; k < UN; ++k) { const uint32_t j = i + threadIdx.x + k * WG; dst[k] = p[j < last ? j : last]; }
            };
            int b = 0;
            while (b < ps.nb && s_lo[b] >= s_hi[b]) ++b;
            uint32_t i = b < ps.nb ? s_lo[b] : 0u;
            pd_iv cur[UN];
            if (b < ps.nb) load_chunk(cur, b, i);
#pragma unroll 1
            while (b < ps.nb) {
                int nb2 = b; uint32_t ni = i + UN * WG;
                if (ni >= s_hi[b]) { nb2 = b + 1; while (nb2 < ps.nb && s_lo[nb2] >= s_hi[nb2]) ++nb2; ni = nb2 < ps.nb ? s_lo[nb2] : 0u; }
                pd_iv nx[UN];
                if (nb2 < ps.nb) load_chunk(nx, nb2, ni);
                const uint32_t left = s_hi[b] - i;
                if (left >= UN * WG) {
                    if (interior) {
#pragma unroll
                        for (int k = 0; k < UN; ++k) one(cur[k], true);
                    } else {
#pragma unroll
                        for (int k = 0; k < UN; ++k) one(cur[k], false);
                    }
                } else {                                          // the tail chunk of a stream: empty slots skipped
                    const int nu = (int)((left + WG - 1) / WG);   // uniform, 1 .. UN
#pragma unroll
                    for (int k = 0; k < UN; ++k) if (k < nu) {
                        pd_iv v = cur[k];
                        if (threadIdx.x + k * WG >= left) v.tid = -1;       // never equals a contig id
                        one(v, interior);
                    }
                }
                if (nb2 < ps.nb) {
#pragma unroll
                    for (int k = 0; k < UN; ++k) cur[k] = nx[k];
                }
                b = nb2; i = ni;
            }
        }
        if (lane == 0 && carry_s != 0) atomicAdd(&s_carry, carry_s);
        W3_TICK(2);                                               // candidates
        __syncthreads();
        W3_TICK(3);                                               // barrier 2
        if constexpr (EXPORT) {                                   // the multi-GPU sum's 4-bit image (pd_export_i4)
            export_packed_tile<ROWS>(win, a, t, ex, wtot);
            continue;
        }
        // ---- prefix sum of the packed window: both half-tiles at once ----
        int4 v[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint4 q = w4[wv * (ROWS * 64) + r * 64 + lane];
            v[r] = make_int4((int)q.x, (int)q.x + (int)q.y, 0, 0);
            v[r].z = v[r].y + (int)q.z; v[r].w = v[r].z + (int)q.w;
        }
        int ex[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) ex[r] = wave_incl_scan(v[r].w);
        int run = 0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int e = run + ex[r] - v[r].w;                   // exclusive prefix of this lane's group in the wave
            run += __builtin_amdgcn_readlane(ex[r], 63);
            ex[r] = e;
        }
        if (lane == 0) wtot[wv] = run;
        W3_TICK(4);                                               // window read + scans
        __syncthreads();
        W3_TICK(5);                                               // barrier 3
        int basep = 0;                                            // packed: words of the waves before this one
        for (int k = 0; k < wv; ++k) basep += wtot[k];
        const int totp = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        const int tl = (int)(short)(totp & 0xffff);               // begins - ends over the low half-tile
        const int carry_l = s_carry, carry_h = carry_l + tl;      // depth just before cell 0 / cell HT of the tile
        // ---- the tile's share of windows k0 and k0 + 1 ----
        const uint64_t local0 = p0;
        int c0 = 0, c1 = 0; unsigned long long s0 = 0, s1 = 0;
        bool uniform_counts = false;                              // c0 is a wave count (ballots), s0 a 32-bit lane sum
        if (local0 < clen) {
            const uint64_t k0 = local0 / w;
            const uint64_t nb64 = (k0 + 1) * (uint64_t)w - local0;   // tile-local start of window k0+1
            const uint32_t nb = nb64 > (uint64_t)ST ? ST : (uint32_t)nb64;
            const uint64_t left = (uint64_t)clen - local0;
            const uint32_t lim = left > (uint64_t)ST ? ST : (uint32_t)left;
            const uint64_t dmax = (uint64_t)(uint32_t)carry_l + cand;     // no depth in this tile exceeds carry + begins
            if (nb >= ST && lim >= ST && min_dep <= 1u && dmax < (1u << 27) && dmax <= wrap_mask) {
                // the common tile — inside one window, inside the contig, no wrap possible, threshold <= 1: the sum is the
                // sum of the local prefixes + 16 x (carry_l + carry_h) per lane; a cell is covered unless its prefix = -carry
                int sl = 0; int cnt = 0;
                const int zl = -carry_l, zh = -carry_h;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int add = basep + ex[r];
                    const int pw[4] = {v[r].x + add, v[r].y + add, v[r].z + add, v[r].w + add};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int L = (int)(short)(pw[q] & 0xffff), H = (pw[q] - L) >> 16;
                        sl += L + H;
                        if (min_dep) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(L != zl)) + __builtin_popcountll(__builtin_amdgcn_ballot_w64(H != zh));
                    }
                }
                c0 = min_dep ? cnt : (int)(ROWS * 8 * 64);
                s0 = (uint32_t)sl + (uint32_t)(ROWS * 4) * ((uint32_t)carry_l + (uint32_t)carry_h);
                uniform_counts = true;
            } else if (nb >= ST && lim >= ST && dmax < (1u << 27)) {
                uint32_t s32 = 0; int cnt = 0;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int add = basep + ex[r];
                    const int pw[4] = {v[r].x + add, v[r].y + add, v[r].z + add, v[r].w + add};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int L = (int)(short)(pw[q] & 0xffff), H = (pw[q] - L) >> 16;
                        const uint32_t dl = (uint32_t)(L + carry_l) & wrap_mask, dh = (uint32_t)(H + carry_h) & wrap_mask;
                        const bool okl = dl >= min_dep, okh = dh >= min_dep;
                        cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(okl)) + __builtin_popcountll(__builtin_amdgcn_ballot_w64(okh));
                        s32 += (okl ? dl : 0u) + (okh ? dh : 0u);
                    }
                }
                c0 = cnt; s0 = s32; uniform_counts = true;
            } else {
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int add = basep + ex[r];
                    const uint32_t pos = (uint32_t)(wv * (ROWS * 256) + r * 256 + lane * 4);
                    const int pw[4] = {v[r].x + add, v[r].y + add, v[r].z + add, v[r].w + add};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int L = (int)(short)(pw[q] & 0xffff), H = (pw[q] - L) >> 16;
                        const uint32_t dl = (uint32_t)(L + carry_l) & wrap_mask, dh = (uint32_t)(H + carry_h) & wrap_mask;
                        const uint32_t pl = pos + q, ph = pl + HT;
                        if (pl < lim && dl >= min_dep) { if (pl < nb) { ++c0; s0 += dl; } else { ++c1; s1 += dl; } }
                        if (ph < lim && dh >= min_dep) { if (ph < nb) { ++c0; s0 += dh; } else { ++c1; s1 += dh; } }
                    }
                }
            }
        }
        if (uniform_counts) {                                     // workgroup-uniform
            const uint32_t s32 = (uint32_t)s0;
            const unsigned long long lo16 = (unsigned long long)(uint32_t)wave_total((int)(s32 & 0xffffu));
            const unsigned long long hi16 = (unsigned long long)(uint32_t)wave_total((int)(s32 >> 16));
            s0 = (hi16 << 16) + lo16;
        } else {
            c0 = wave_sum(c0); c1 = wave_sum(c1);
#pragma unroll
            for (int o = 32; o; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
        }
        if (lane == 0) { red_c[wv][0] = c0; red_c[wv][1] = c1; red_s[wv][0] = s0; red_s[wv][1] = s1; }
        W3_TICK(6);                                               // statistics
        __syncthreads();
        W3_TICK(7);                                               // barrier 4
        if (threadIdx.x == 0) {
            TilePart tp;
            tp.c0 = (uint32_t)(red_c[0][0] + red_c[1][0] + red_c[2][0] + red_c[3][0]);
            tp.c1 = (uint32_t)(red_c[0][1] + red_c[1][1] + red_c[2][1] + red_c[3][1]);
            tp.s0 = red_s[0][0] + red_s[1][0] + red_s[2][0] + red_s[3][0];
            tp.s1 = red_s[0][1] + red_s[1][1] + red_s[2][1] + red_s[3][1];
            part[t] = tp;
        }
        // (no barrier here: everything the next tile overwrites — bounds, window, carry, wave totals, partials — is last read
        // before one of the three barriers that precede the overwriting store)
    }
#ifdef PD_WIDE3_TICKS
    if (lane == 0) for (int k = 0; k < 8; ++k) atomicAdd(&g_wide3_ticks[k], (unsigned long long)tk[k]);
#endif
    // every begin and every end must have found its owner tile (k_finish_direct compares the sums over all batches)
    __shared__ unsigned s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if (lane == 0) {
        if (n_beg_s) atomicAdd(&s_cnt[0], n_beg_s);
        if (open_s) atomicAdd(&s_cnt[1], (unsigned)open_s);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        BatchDesc *desc = ps.b[0].desc;
        if (s_cnt[0]) atomicAdd((unsigned long long *)desc->handled + (blockIdx.x & (PD_CNT_SLOTS - 1)), (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd((unsigned long long *)desc->has + (blockIdx.x & (PD_CNT_SLOTS - 1)), (unsigned long long)(long long)(int)s_cnt[1]);
    }
}

// The int-window pass of the pile-up tiles — k_direct_tiles_heavy on 12-byte runs, k_c8_heavy on a compact sample — keeps a tile's window as
// 8192 ints in LDS; the two kernels differ only in how the candidates reach it and share what follows.
struct HeavyLds {
    alignas(16) int win[TILE];
    unsigned long long acc[TILE / 64 + 2];
    unsigned long long red_s[16][2];                             // (per wave: up to 16 of them)
    int red_c[16][2];
    int wtot[16];
    int s_carry;
};

template <int NT = WG>
__device__ __forceinline__ void heavy_tile_clear(HeavyLds &L)
{
    int4 *w4 = reinterpret_cast<int4 *>(L.win);
    for (int j = threadIdx.x; j < TILE / 4; j += NT) w4[j] = make_int4(0, 0, 0, 0);
    if (threadIdx.x == 0) L.s_carry = 0;
}

// Tile t's window is complete but for this thread's share `carry` of the runs that cover the cell before the tile: export it (ex.img != null,
// workgroup-uniform) or take the prefix sum and the tile's shares of its windows.  Ends behind a barrier: the window may be cleared again.
// NT: the workgroup's threads (256: k_direct_tiles_heavy, with narrow windows too; 1024: k_c8_heavy, whose windows are never narrower than a tile).
template <int NT = WG>
__device__ __forceinline__ void heavy_tile_finish(HeavyLds &L, int carry, const uint64_t t, const int32_t ctg, const uint32_t clen, const ContigTab tab,
                                                  const uint32_t wrap_mask, const WinArgs &wa, const uint64_t *win_off, const DirectExport &ex)
{
    constexpr int ST = TILE;
    constexpr int NW = NT / 64;                                   // waves
    constexpr int ROWS = TILE / (NT * 4);                        // 8, or 2
    static_assert(NW <= 16 && ROWS >= 1 && ROWS * NT * 4 == TILE, "the window is split evenly over at most 16 waves");
    const uint32_t w = wa.w, min_dep = wa.min_dep;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t a = t * ST;
    int4 *w4 = reinterpret_cast<int4 *>(L.win);
    carry = wave_sum(carry);
    if (lane == 0 && carry != 0) atomicAdd(&L.s_carry, carry);
    __syncthreads();
    if (ex.img) {                                                 // workgroup-uniform: the window leaves as nibbles (k_export_i4's layout)
        const uint64_t cw = a + (uint64_t)wv * (ROWS * 256);
        unsigned short *o = ex.img + cw / 4 + lane;
        int tsum = 0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int4 q = w4[wv * (ROWS * 64) + r * 64 + lane];
            int x[4] = {q.x, q.y, q.z, q.w};
            unsigned wb = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tsum += x[k];
                if (x[k] > 7 || x[k] < -8) {
                    const uint32_t slot = atomicAdd(ex.count, 1u);
                    if (slot < ex.cap) { ex.exc[slot].cell = cw + (uint64_t)(r * 256 + lane * 4 + k); ex.exc[slot].value = x[k]; ex.exc[slot].pad = 0; }
                    x[k] = 0;
                }
                wb |= (unsigned)((x[k] + 8) & 0xf) << (4 * k);
            }
            o[r * 64] = (unsigned short)wb;
        }
        tsum = wave_sum(tsum);
        if (lane == 0) L.wtot[wv] = tsum;
        __syncthreads();
        if (threadIdx.x == 0) { int ts = 0; for (int k = 0; k < NW; ++k) ts += L.wtot[k]; ex.sums[t] = ts; }
        __syncthreads();
        return;
    }
    // ---- prefix sum of the window, straight from LDS (k_sweep's layout) ----
    int4 v[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) v[r] = w4[wv * (ROWS * 64) + r * 64 + lane];
    int tot[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        v[r].y += v[r].x; v[r].z += v[r].y; v[r].w += v[r].z;
        tot[r] = v[r].w;
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) tot[r] = wave_incl_scan(tot[r]);
    int run = 0;
    int excl[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        excl[r] = run + tot[r] - v[r].w;
        run += __builtin_amdgcn_readlane(tot[r], 63);
    }
    if (lane == 0) L.wtot[wv] = run;
    __syncthreads();
    int base = L.s_carry;
    for (int k = 0; k < wv; ++k) base += L.wtot[k];
    if constexpr (NT == WG) {
        if (w < (uint32_t)ST) {                                   // narrow windows: LDS accumulators (uniform branch)
            const uint32_t p0 = (uint32_t)(a - tab.off[ctg]);
            if (p0 < clen) direct_small_windows<ROWS>(v, excl, base, wrap_mask, p0, clen, wa, win_off[ctg], L.acc, wa.part + t);
            __syncthreads();
            return;
        }
    }
    // ---- the tile's share of windows k0 and k0 + 1 ----
    const uint64_t local0 = a - tab.off[ctg];
    int c0 = 0, c1 = 0; unsigned long long s0 = 0, s1 = 0;
    if (local0 < clen) {
        const uint64_t k0 = local0 / w;
        const uint64_t nb = (k0 + 1) * (uint64_t)w - local0;     // tile-local start of window k0+1
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int bsum = base + excl[r];
            const uint32_t pos = (uint32_t)(wv * (ROWS * 256) + r * 256 + lane * 4);
            const uint32_t d[4] = {(uint32_t)(v[r].x + bsum) & wrap_mask, (uint32_t)(v[r].y + bsum) & wrap_mask,
                                   (uint32_t)(v[r].z + bsum) & wrap_mask, (uint32_t)(v[r].w + bsum) & wrap_mask};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool ok = local0 + pos + q < clen && d[q] >= min_dep;
                if (ok) { if (pos + q < nb) { ++c0; s0 += d[q]; } else { ++c1; s1 += d[q]; } }
            }
        }
    }
    c0 = wave_sum(c0); c1 = wave_sum(c1);
#pragma unroll
    for (int o = 32; o; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
    if (lane == 0) { L.red_c[wv][0] = c0; L.red_c[wv][1] = c1; L.red_s[wv][0] = s0; L.red_s[wv][1] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        TilePart tp; tp.c0 = tp.c1 = 0u; tp.s0 = tp.s1 = 0ull;
        for (int k = 0; k < NW; ++k) { tp.c0 += (uint32_t)L.red_c[k][0]; tp.c1 += (uint32_t)L.red_c[k][1]; tp.s0 += L.red_s[k][0]; tp.s1 += L.red_s[k][1]; }
        wa.part[t] = tp;
    }
    __syncthreads();
}

__global__ __launch_bounds__(WG) void k_direct_tiles_heavy(const PendSet ps, uint32_t n_tiles, ContigTab tab,
                                                     const uint32_t *tile_contig, uint32_t wrap_mask, const WinArgs wa,
                                                     const uint64_t *win_off, uint32_t *n_long,
                                                     const uint32_t *heavy_list, const uint32_t *heavy_count,
                                                     const DirectExport ex)          // ex.img != null: export instead of statistics
{
    constexpr int ST = TILE;
    __shared__ HeavyLds L;
    int *const win = L.win;
    const int lane = threadIdx.x & 63;
    uint32_t tf[PD_MAXPEND], na[PD_MAXPEND];
    uint32_t n_beg[PD_MAXPEND], n_has[PD_MAXPEND], n_end[PD_MAXPEND];
    uint32_t longs = 0;
#pragma unroll
    for (int b = 0; b < PD_MAXPEND; ++b) {
        n_beg[b] = n_has[b] = n_end[b] = 0; tf[b] = 0; na[b] = 0;
        if (b < ps.nb) { tf[b] = ps.b[b].desc->t_first; na[b] = ps.b[b].desc->n_active; }
    }
    const uint32_t lmax = ps.lmax;
    const uint32_t n_heavy = *heavy_count < n_tiles ? *heavy_count : n_tiles;
    for (uint32_t hi_ = blockIdx.x; hi_ < n_heavy; hi_ += gridDim.x) {
        const uint64_t t = heavy_list[hi_];
        const uint64_t a = t * ST;
        heavy_tile_clear(L);
        const int32_t ctg = (int32_t)tile_contig[t];
        const uint32_t clen = tab.len[ctg];
        const int64_t rel = (int64_t)(tab.off[ctg] - a);          // slot start relative to the tile (<= 0)
        __syncthreads();
        int carry = 0;
#pragma unroll
        for (int b = 0; b < PD_MAXPEND; ++b) {
            if (b >= ps.nb || t < tf[b] || t >= (uint64_t)tf[b] + na[b]) continue;
            const uint32_t n = ps.b[b].n;
            uint32_t hi = ps.b[b].ub_a[t + 1]; if (hi > n) hi = n;
            uint32_t lo = ps.b[b].cand_lo[t]; if (lo > hi) lo = hi;
            const pd_iv *__restrict__ iv = ps.b[b].iv;
            constexpr int UN = 4;
            for (uint32_t i0 = lo + threadIdx.x; i0 < hi; i0 += UN * WG) {
                pd_iv vv[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const uint32_t i = i0 + u * WG;
                    vv[u] = iv[i < hi ? i : hi - 1];
                    if (i >= hi) vv[u].tid = -1;
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const pd_iv v = vv[u];
                    if (v.tid != ctg) continue;
                    uint32_t bb = v.beg < 0 ? 0u : (uint32_t)v.beg; if (bb > clen) bb = clen;
                    uint32_t x = v.end < 0 ? 0u : (uint32_t)v.end; if (x > clen) x = clen;
                    const bool has = bb < x;
                    const int64_t sb = rel + (int64_t)bb, se = rel + (int64_t)x;     // tile-relative begin / end
                    if (sb >= 0 && sb < ST) {
                        ++n_beg[b];
                        if (has) { ++n_has[b]; atomicAdd(&win[sb], 1); if (x - bb > lmax) ++longs; }
                    }
                    if (has) {
                        if (se >= 0 && se < ST) { atomicAdd(&win[se], -1); ++n_end[b]; }
                        if (sb < 0 && se >= 0) ++carry;           // covers the cell just before the tile
                    }
                }
            }
        }
        heavy_tile_finish(L, carry, t, ctg, clen, tab, wrap_mask, wa, win_off, ex);
    }
    // the same accounting as k_scatter_tiles: every begin and every end must have found its owner tile
    __shared__ unsigned s_cnt[PD_MAXPEND][3];
    __shared__ unsigned s_long;
    if (threadIdx.x < PD_MAXPEND * 3) s_cnt[threadIdx.x / 3][threadIdx.x % 3] = 0;
    if (threadIdx.x == 0) s_long = 0;
    __syncthreads();
#pragma unroll
    for (int b = 0; b < PD_MAXPEND; ++b) {
        if (b >= ps.nb) continue;
        const int hb = wave_sum((int)n_beg[b]), hh = wave_sum((int)n_has[b]), he = wave_sum((int)n_end[b]);
        if (lane == 0) {
            if (hb) atomicAdd(&s_cnt[b][0], (unsigned)hb);
            if (hh) atomicAdd(&s_cnt[b][1], (unsigned)hh);
            if (he) atomicAdd(&s_cnt[b][2], (unsigned)he);
        }
    }
    const int hl = wave_sum((int)longs);
    if (lane == 0 && hl) atomicAdd(&s_long, (unsigned)hl);
    __syncthreads();
    if (threadIdx.x < ps.nb * 3) {
        const int b = threadIdx.x / 3, k = threadIdx.x % 3;
        const unsigned v = s_cnt[b][k];
        if (v) {
            BatchDesc *desc = ps.b[b].desc;
            unsigned long long *dst = (unsigned long long *)(k == 0 ? desc->handled : k == 1 ? desc->has : desc->ends);
            atomicAdd(dst + (blockIdx.x & (PD_CNT_SLOTS - 1)), (unsigned long long)v);
        }
    }
    if (threadIdx.x == 0 && s_long) atomicAdd(n_long, s_long);
}

// k_c8_heavy — the pile-up pass of a compact sample: the tiles k_direct_c8 put on heavy_list (more than PD_C8_HEAVY_CAND candidates: tens of
// thousands of reads that begin on one cell), one workgroup per tile, the window as ints in LDS (HeavyLds).  A tile's candidates are those of
// k_direct_c8 — its own buckets and the one before them, in both streams, 16-bit arithmetic on the lo plane (pdpile::events) — and reach the window so:
//   * chunks of UN * WG consecutive runs, the sorted stream's and then the other stream's as ONE sequence of chunks, lane after lane (slot k of a
//     thread is run threadIdx.x + k * WG of its chunk); a chunk's UN loads per thread are issued before the chunk in front of it is worked on
//     (two register buffers in turn, as in k_direct_c8).  Indices are clamped to the stream's last run and the slots past it become a run
//     without cells, which takes no part;
//   * for every slot, neighbouring lanes that name the same begin cell add ONCE (pd_pile_rule.h): the first lane of such a group adds the group's
//     size, the others do nothing — a pile's 64 begins in a wave are one LDS atomic, not 64 to one word in turn; the same, grouped on their own,
//     for the end cells (equal where the pile's reads have one length).  Integer additions commute: the window is the one a run-by-run walk leaves;
//   * the carry-in (runs of the bucket before that reach the tile's first cell) is counted with a ballot per slot.
// A tile's cost stays linear in its candidates: one workgroup walks them all.
template <bool EXPORT, int UN, int NT>
__global__ __launch_bounds__(NT) void k_c8_heavy(const C8Sample cs, uint32_t n_tiles, ContigTab tab, const uint32_t *tile_contig, uint32_t wrap_mask,
                                                  const WinArgs wa, const uint32_t *heavy_list, const uint32_t *heavy_count, uint32_t n_list, const DirectExport ex)
{
    constexpr uint32_t ST = TILE, C = UN * NT;
    __shared__ HeavyLds L;
    int *const win = L.win;
    const int lane = threadIdx.x & 63;
    const uint32_t *__restrict__ const p = cs.lo;
    // the export form walks what k_direct_c8 listed in front of it (heavy_count: the call's); the statistics form the SAMPLE's list, n_list tiles
    // by value (heavy_count unused), so that it depends on nothing k_direct_c8 writes
    const uint32_t listed = EXPORT ? *heavy_count : n_list;
    const uint32_t n_heavy = listed < n_tiles ? listed : n_tiles;
    for (uint32_t hi_ = blockIdx.x; hi_ < n_heavy; hi_ += gridDim.x) {
        const uint64_t t = heavy_list[hi_];
        const uint64_t a = t * ST;
        const int32_t ctg = (int32_t)tile_contig[t];
        const uint32_t clen = tab.len[ctg];
        const uint32_t k0 = (uint32_t)t << cs.bshift, kl = tab.off[ctg] < a ? k0 - 1 : k0;   // (a contig's first tile has nothing before it)
        const uint32_t kh = k0 + (1u << cs.bshift);
        const uint32_t s_at = cs.b1[kl], ns = cs.b1[kh] - s_at;   // the tile's candidates in the sorted stream
        const uint32_t olo = cs.o1[kl], no = cs.o1[kh] - olo;     // ... and in the other stream
        const uint32_t o_at = cs.o_base + olo;
        const uint32_t p0 = (uint32_t)a & 0xFFFFu;
        const uint32_t none = (p0 + ST) & 0xFFFFu;                // a run without cells
        const uint32_t c1 = (ns + C - 1) / C, nq = c1 + (no + C - 1) / C;
        int carry_s = 0;                                          // wave-uniform
        auto load = [&](uint32_t (&dst)[UN], const uint32_t q) {
            const bool second = q >= c1;
            const uint32_t at = second ? o_at : s_at, i = (second ? q - c1 : q) * C + threadIdx.x, last = (second ? no : ns) - 1u;
#pragma unroll
            for (int k = 0; k < UN; ++k) { const uint32_t j = i + (uint32_t)k * NT; dst[k] = p[at + (j < last ? j : last)]; }
        };
        // the wave's lanes with `valid` add sign to win[v], neighbours that name one cell as one addition (pd_pile_rule.h)
        auto add_grouped = [&](const uint32_t v, const bool valid, const unsigned long long m_valid, const int sign) {
            if (!m_valid) return;                                 // wave-uniform
            const uint32_t key = pdpile::lane_key(v, valid);
            const bool head = pdpile::is_head(key, (uint32_t)wave_shift_up((int)key, (int)pdpile::NO_LANE));
            const unsigned long long m_h = __builtin_amdgcn_ballot_w64(head);
            if (head) atomicAdd(&win[v], sign * (int)pdpile::multiplicity(m_h, m_valid, lane));
        };
        auto work = [&](const uint32_t (&c)[UN], const uint32_t q) {
            const bool second = q >= c1;
            const uint32_t i = (second ? q - c1 : q) * C + threadIdx.x, n = second ? no : ns;
            const uint32_t left = n - (second ? q - c1 : q) * C;  // >= 1
            const int nu = left >= C ? UN : (int)((left + NT - 1) / NT);      // workgroup-uniform, 1 .. UN: the slots that hold a run at all
#pragma unroll
            for (int k = 0; k < UN; ++k) {
                if (k >= nu) continue;
                const uint32_t r = i + (uint32_t)k * NT < n ? c[k] : none;
                const pdpile::Events e = pdpile::events(r, p0);
                const bool vb = e.has && e.sb < ST, ve = e.has && e.se16 < ST;
                const unsigned long long m_vb = __builtin_amdgcn_ballot_w64(vb), m_ve = __builtin_amdgcn_ballot_w64(ve);
                carry_s += __builtin_popcountll(__builtin_amdgcn_ballot_w64(e.carry && e.has));
                add_grouped(e.sb, vb, m_vb, 1);
                add_grouped(e.se16, ve, m_ve, -1);
            }
        };
        uint32_t A[UN], B[UN];
        if (nq) load(A, 0);                                       // the first chunk is on its way before the window is cleared
        heavy_tile_clear<NT>(L);
        __syncthreads();
        if (nq) {
            uint32_t q = 0;
#pragma unroll 1
            for (;;) {                                            // two buffers: B is in flight while A is worked on
                if (q + 1 < nq) load(B, q + 1);
                work(A, q);
                if (++q >= nq) break;
                if (q + 1 < nq) load(A, q + 1);
                work(B, q);
                if (++q >= nq) break;
            }
        }
        heavy_tile_finish<NT>(L, lane == 0 ? carry_s : 0, t, ctg, clen, tab, wrap_mask, wa, nullptr, EXPORT ? ex : DirectExport{});
    }
}

// k_direct_c8 — the wide-window direct kernel on a compact sample: exact bounds, nothing to test but where the two
// events of a run fall.  It reads the LO plane only — 4 bytes per run, r = (b & 0xFFFF) | (len << 16) —: every candidate of a tile begins in
// the tile or in the one bucket before it and is no longer than a bucket (at most 8192 cells), so with p0 the tile's first flat cell
//   sb = (r - p0) & 0xFFFF: < TILE exactly for the tile's own runs (a run of the bucket before lands in [2^16 - bucket, 2^16));
//   se = sb + (r >> 16):    its low 16 bits are < TILE exactly when the end lies in the tile;  se >= 2^16 exactly when the run begins
//   before the tile and reaches its first cell or further (the carry-in)
// — the same three answers as b - p0, + len and the carry of the full 32 + 32 bits, on half the bytes (k_direct_wide3: 26 vector instructions
// per run, on 12-byte runs with a contig compare and clamps).
// A run without cells adds and subtracts at the same cell.  The tile's candidates are its own buckets and the one before them, in
// BOTH streams of the sample (the file's sorted first runs as the decoder wrote them, and the later runs counting-sorted by bucket):
// one loop over the two ranges laid end to end.  Same window arithmetic and prefix sum as k_direct_wide3; the statistics of an interior tile
// take a packed minimum and a packed sum per word (exact loops for the waves that hold a cell below the threshold, and for edge tiles); tiles
// with more than 32 000 candidates go to the int-window kernel through the same list.
// LW (JOIN only, a divisor of UN8): runs per lane and load in the full chunks of the sorted stream — 1, 2 (8-byte loads) or 4 (16-byte loads; the
// stream's words are 4-byte aligned, the loads are not); which thread works on which run changes, nothing else (the window's updates commute).
// COVER (statistics form only): the cover pass in front of the window path — see it below.  The form walks GROUPS of four consecutive tiles (group
// blockIdx.x + k * gridDim.x): each wave sweeps ONE tile of the group by itself, one barrier follows, and the tiles the pass did not settle take
// the window path, all four waves together, in tile order.  Its gate is a score per workgroup, played over the tiles in their order: a declined tile adds
// COVER_DECLINE, a settled one takes 1 off (not below 0); at COVER_CLOSE the workgroup leaves the pass out for COVER_SKIP tiles, tries one, and goes on
// so while the score stays there.  Four declined tiles in a row close it; so does, in the long run, any mix in which fewer than two tiles in three
// settle (a declined tile costs a sweep on top of its window: launch_direct_c8).  A workgroup that walks consecutive tiles settles exactly the tiles it
// would settle taking them one by one: a tile swept in a group in which an earlier tile's decline closed the gate is not counted and takes the window.
constexpr uint32_t COVER_DECLINE = 2, COVER_CLOSE = 8, COVER_SKIP = 15;
// NARROW (COVER only): the pass sweeps a tile's sorted candidates from the nar plane, two bytes per run, and checks at the end that it could (cover_sweep_narrow).
// The kernel is a walk over named phases — cover pass: cover_eligible, cover_sweep_narrow / cover_sweep_wide (both on the chunk stream, sweep3 and
// cover_rule_chunk), cover_gate — each taking what it reads and returning what it leaves; the window path (fill, prefix sum, statistics) stands in the kernel's body:
// as functions its three phases compiled to other, slower instruction streams in all 30 instantiations (profiles/r18_direct_split_ab.txt).

// a tile's outcome in the cover pass (wave-uniform)
constexpr uint32_t COV_NONE = 0u /* no tile here, or a pile-up tile */, COV_WINDOW = 1u /* not swept */, COV_DECLINED = 2u, COV_SETTLED = 3u;
struct CoverResult { uint32_t outcome, wsum; };                   // wave-uniform: a swept tile's outcome and the sum of its candidates' clipped lengths
struct CoverGate { uint32_t miss = 0, skip = 0, settled = 0; };   // workgroup-uniform: the gate's score, the tiles it still leaves out, the tiles settled so far
struct GateOut { uint32_t todo; bool write_mine; };               // workgroup-uniform: bit k: tile k of the group takes the window path; wave-uniform: this wave writes its tile
struct CoverSweep { int reach = 0; bool gap = false; uint32_t sum = 0; };   // wave-uniform: [0, reach) is covered by the runs swept so far, a gap was met; this lane's clipped lengths

// ---- cover pass: whether a tile is swept, from its descriptor and the arguments (wave-uniform) ----
// Inside the contig, inside one window, no depth above the candidate count, enough candidates for the sweep to be the cheaper way (cover_min), the gate
// possibly open when the walk reaches the tile (skip at the group's start <= the wave's number).  A stream of the tile that ends inside the first eight words of
// the sample's array — fewer than eight runs in all up to there — has no eight words to load: the window path does such a tile.
__device__ __forceinline__ bool cover_eligible(const TileDesc &mine, const C8Sample &cs, const DirectWide &args, const uint32_t wrap_mask, const uint32_t skip, const uint32_t wvu)
{
    constexpr uint32_t ST = TILE;
    const uint32_t ns = mine.shi - mine.slo, no = mine.ohi - mine.olo, cand = ns + no, pc = mine.pc, clen = mine.clen, w = args.w;
    bool eligible = false;
    if (skip <= wvu && args.min_dep <= 1u && cand <= wrap_mask && cand >= args.cover_min && pc < clen && clen - pc >= ST)
        eligible = ((uint64_t)(pc / w) + 1u) * (uint64_t)w - pc >= (uint64_t)ST;
    if ((ns && mine.shi < 8u) || (no && cs.o_base + mine.ohi < 8u)) eligible = false;
    return eligible;
}

// ---- cover pass: the chunk stream of both sweeps ----
// A tile's candidates are ONE sequence of chunks, `per` consecutive runs to a lane (8 of the sorted stream and 4 of the other in the narrow sweep, 8 in the wide).
// EVERY chunk is loaded the same way, no branch around the loads, so that the wait in front of a chunk's work counts exactly the loads issued behind it.
// The lane's first element, counted from `back` elements before the chunk: in a partial chunk of cnt runs a lane's load begins at run min(per * lane, cnt - per)
// — still inside the sample's array, not before its first element.
__device__ __forceinline__ uint32_t chunk_lane_rel(const uint32_t ln, const uint32_t cnt, const uint32_t back, const uint32_t per)
{
    const int off = (int)(ln * per) < (int)cnt - (int)per ? (int)(ln * per) : (int)cnt - (int)per;
    const int rel = off + (int)back;
    return (uint32_t)(rel > 0 ? rel : 0) & 1023u;                 // (at most 512: said so that the loads take a 32-bit offset, not an address pair)
}
// ... and how many of the lane's places are not its own there: place 0 should be run per * lane, and is a run at or before it (the lane before has those);
// all of them, for a lane behind the chunk's end
__device__ __forceinline__ int chunk_skip(const uint32_t ln, const uint32_t cnt, const uint32_t back, const uint32_t per)
{
    const int mine0 = (int)(ln * per), got0 = (int)chunk_lane_rel(ln, cnt, back, per) - (int)back;
    return mine0 < (int)cnt ? mine0 - got0 : (int)per;
}
// ... which become a run that changes nothing
template <int N>
__device__ __forceinline__ void chunk_keep_own(uint32_t (&x)[N], const int skip, const uint32_t neutral)
{
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = k >= skip ? x[k] : neutral;
}
// The chunks go through pdcover::sweep3 (pd_cover_rule.h): three register buffers of N words in turn, no copies, two chunks in flight behind the one worked on
// (one wave streams a tile by itself, and a CU's 28 waves must keep HBM's latency covered).  load(x, q) also serves q >= nq, all lanes to one place.
using pdcover::sweep3;

// ---- cover pass: the rule on one chunk of eight runs per lane, tile-relative begins b and ends e (pd_cover_rule.h, ONE segment) ----
// sorted: a run that begins beyond the reach is a gap; one max-scan and one wave_shr:1 give a lane the largest end of the lanes before it, eight compares are
// joined on the scalar side.  Lengths are clipped only where needed (wave-uniform): when a run of the chunk begins before the tile or one ends behind it;
// otherwise the lane adds unclipped().  A chunk of the other stream (sorted = false) adds its clipped lengths and nothing else.
template <class Lens>
__device__ __forceinline__ void cover_rule_chunk(const int (&b)[8], const int (&e)[8], const bool sorted, const Lens &unclipped, CoverSweep &s)
{
    constexpr int ST = TILE;
    if (sorted) {
        int m = e[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) m = m > e[k] ? m : e[k];
        const int incl = wave_incl_scan_max(m);
        const int before = wave_shift_up(incl, pdcover::NONE);      // the largest end of the lanes before this one
        int P = before > s.reach ? before : s.reach;
        unsigned long long g = 0ull;
        uint32_t neg = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { g |= __builtin_amdgcn_ballot_w64(b[k] > P); P = P > e[k] ? P : e[k]; neg |= (uint32_t)b[k]; }
        if (g != 0ull) s.gap = true;
        const int top = __builtin_amdgcn_readlane(incl, 63);
        s.reach = top > s.reach ? top : s.reach;
        if (top <= ST && __builtin_amdgcn_ballot_w64((int)neg < 0) == 0ull) { s.sum += unclipped(); return; }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s.sum += pdcover::run_clipped(b[k], e[k], ST);
}

// ---- cover pass: the NARROW sweep of one tile by one wave ----
// The sorted candidates come from the nar plane, two bytes per run (pd_cover_rule.h), the other stream's from lo as in the wide sweep, behind them in the same
// sequence.  A chunk of the sorted stream is 512 runs, eight consecutive runs per lane; a chunk of the other stream is 256 runs, four per lane.  So EVERY chunk is
// ONE 16-byte load per lane (a uniform choice of where it points): 2 KB per wave in flight, in 12 registers (with a fourth buffer, or with chunks of two loads,
// the form needs 65 - 69 VGPRs: profiles/r15_cover_narrow_ab.txt, section 7).
// Begins are REBUILT: within a lane d[k] = (c[k] - c[k-1]) & 255 over the runs' low bytes, the predecessor of a lane's first run being the lane before's last
// (lane 0: the chunk before's last, carried wave-uniform in pb); the lane totals go through a wave scan and `base`, the rebuilt begin of the last run swept so far
// (at first the tile-relative begin of the tile's first sorted candidate, from its lo word).  Ends are begin + the high byte: exact, the launcher takes this form
// only for a sample without a sorted run above 255 cells.  The rebuilt begins are right exactly when no consecutive difference reached 256, and the END CHECK says
// so without any help from whoever made the sample: the stream is sorted (words[0] refuses a sample that is not), every rebuilt difference is <= the true one, so
// `base` behind the last chunk equals the last candidate's true begin (its lo word) if and only if every difference was rebuilt as it is.  That is enough: every
// rebuilt begin is <= its true one, so a wrong begin alone could only CLOSE a true gap, never open one — a gap met is a true gap and declines the tile as in the
// wide form, without the check — and the equality at the end rules the closed gap out.  A tile is settled only when the check passed; where it did not, the tile
// was NOT TRIED (COV_WINDOW: nothing for the gate's score).  In a partial chunk the places that are not the lane's own become the lane's predecessor byte with
// length 0 (a difference of 0, an empty run: pdcover::nar_neutral); for the lanes behind the chunk's last run the predecessor is that run.
// The FAST CHUNK (pd_cover_rule.h, where the proof stands): a full chunk behind a run that begins at or behind cell 0, judged by lanes — a lane whose LAST begin
// lies within P = max(reach, the ends of the lanes before it) has no gap (its other begins are no larger, and the rule would compare them with no less than P);
// base >= 0 and top <= TILE mean that nothing is clipped, so the sum is the sum of the length bytes.  An accepted chunk leaves reach, base, pb, sum and gap
// exactly as the rule would; a refused one has changed nothing and goes through the rule.  n_fast (wave-uniform) counts the accepted ones.
__device__ __forceinline__ CoverResult cover_sweep_narrow(const C8Sample &cs, const TileDesc &mine, const DirectWide &args, const uint32_t p0, const uint32_t ln, uint32_t &n_fast)
{
    constexpr uint32_t ST = TILE, CWS = 512u, CWO = 256u;
    const uint32_t ns = mine.shi - mine.slo, no = mine.ohi - mine.olo;
    const bool any_gap_ends = args.min_dep != 0u;
    const uint32_t c_s = (ns + CWS - 1u) / CWS, nq = c_s + (no + CWO - 1u) / CWO;
    const uint32_t neutral = pdcover::run_neutral(p0);
    const uint32_t o_at = cs.o_base + mine.olo;
    uint32_t lo_first = 0u, lo_last = 0u;                         // the lo words of the tile's first and last sorted candidate: issued in front of the first chunk's loads
    if (ns) { lo_first = cs.lo[mine.slo]; lo_last = cs.lo[mine.shi - 1u]; }
    // the runs of chunk q (wave-uniform)
    auto sorted_cnt = [&](const uint32_t q) -> uint32_t { const uint32_t left = ns - q * CWS; return left < CWS ? left : CWS; };
    auto other_cnt = [&](const uint32_t q) -> uint32_t { const uint32_t left = no - (q - c_s) * CWO; return left < CWO ? left : CWO; };
    typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(2)));     // (the half-words are 2-byte aligned, the 16-byte loads are not)
    auto load = [&](uint32_t (&x)[4], const uint32_t q) {
        const uint32_t qq = q < nq ? q : nq - 1u;
        const char *pq;                                           // wave-uniform
        uint32_t r;                                               // the lane's byte offset from it
        if (qq < c_s) {
            uint32_t cnt = sorted_cnt(qq);
            if (q >= nq && cnt > 8u) cnt = 8u;                    // behind the last chunk: one place for all lanes
            const uint32_t at = mine.slo + qq * CWS, back = at < 8u ? at : 8u;
            pq = reinterpret_cast<const char *>(cs.nar + (at - back)); r = chunk_lane_rel(ln, cnt, back, 8u) * 2u;
        } else {
            uint32_t cnt = other_cnt(qq);
            if (q >= nq && cnt > 4u) cnt = 4u;
            const uint32_t at = o_at + (qq - c_s) * CWO, back = at < 4u ? at : 4u;
            pq = reinterpret_cast<const char *>(cs.lo + (at - back)); r = chunk_lane_rel(ln, cnt, back, 4u) * 4u;
        }
        const u32x4_u u = *reinterpret_cast<const u32x4_u *>(pq + r);
        x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w;
    };
    CoverSweep s;
    int base = 0;                                                 // wave-uniform: the rebuilt begin of the last sorted run swept
    uint32_t pb = 0u;                                             // wave-uniform: that run's half-word (its low byte is what counts)
    auto work = [&](uint32_t (&x)[4], const uint32_t q) {
        if (q >= c_s) {                                           // the other stream: clipped lengths only, 4 runs per lane
            const uint32_t cnt = other_cnt(q);
            if (cnt < CWO) {
                const uint32_t at = o_at + (q - c_s) * CWO, back = at < 4u ? at : 4u;
                chunk_keep_own(x, chunk_skip(ln, cnt, back, 4u), neutral);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int b = pdcover::run_begin(x[k], p0); s.sum += pdcover::run_clipped(b, pdcover::run_end(x[k], b), (int)ST); }
            return;
        }
        const uint32_t cnt = sorted_cnt(q);
        if (args.cover_fast && pdcover::chunk_fast_entry(cnt, base)) {
            const uint32_t before_w = (uint32_t)wave_shift_up((int)x[3], (int)(pb << 16));
            const pdcover::NarLane nl = pdcover::nar_lane_summary(x, before_w);
            const int lane_last = base + wave_incl_scan(nl.T);
            const int incl = wave_incl_scan_max(lane_last - nl.T + nl.Mrel);
            const int before = wave_shift_up(incl, pdcover::NONE);
            const int top = __builtin_amdgcn_readlane(incl, 63);
            const bool every = __builtin_amdgcn_ballot_w64(!pdcover::chunk_fast_lane_ok(lane_last, before, s.reach)) == 0ull;
            if (pdcover::chunk_fast_ok(every, top, (int)ST)) {
                s.reach = top > s.reach ? top : s.reach;
                base = __builtin_amdgcn_readlane(lane_last, 63);
                pb = (uint32_t)__builtin_amdgcn_readlane((int)x[3], 63) >> 16;
                s.sum += nl.lens;
                ++n_fast;
                return;
            }
        }
        uint32_t h[8] = {x[0] & 0xFFFFu, x[0] >> 16, x[1] & 0xFFFFu, x[1] >> 16, x[2] & 0xFFFFu, x[2] >> 16, x[3] & 0xFFFFu, x[3] >> 16};
        const uint32_t last_lane = (cnt - 1u) >> 3;               // the lane that holds the chunk's last run, in its last place
        const uint32_t lastb = (uint32_t)__builtin_amdgcn_readlane((int)h[7], (int)last_lane);
        uint32_t pred = (uint32_t)wave_shift_up((int)h[7], (int)pb);
        if (cnt < CWS) {                                          // a partial chunk (wave-uniform): keep this lane's own runs
            const uint32_t at = mine.slo + q * CWS, back = at < 8u ? at : 8u;
            const int skip = chunk_skip(ln, cnt, back, 8u);
            if (ln > last_lane) pred = lastb;
            chunk_keep_own(h, skip, pdcover::nar_neutral(pred));
        }
        pb = lastb;
        // begins and ends relative to the lane's predecessor first (the half-words are done with before the scan), then moved by the lane's base
        int b[8], e[8];
        uint32_t lens = 0;
        b[0] = pdcover::nar_step(h[0], pred);
#pragma unroll
        for (int k = 1; k < 8; ++k) b[k] = b[k - 1] + pdcover::nar_step(h[k], h[k - 1]);
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int len = pdcover::nar_len(h[k]); e[k] = b[k] + len; lens += (uint32_t)len; }
        const int tot = wave_incl_scan(b[7]);
        const int lane_base = base + tot - b[7];
        base += __builtin_amdgcn_readlane(tot, 63);
#pragma unroll
        for (int k = 0; k < 8; ++k) { b[k] += lane_base; e[k] += lane_base; }
        cover_rule_chunk(b, e, true, [&]() -> uint32_t { return lens; }, s);
    };
    bool end_ok = true;
    if (nq) {
        uint32_t lo_last_u = 0u;
        sweep3<4>(load, work, nq, [&]() -> bool { return s.gap && any_gap_ends; }, [&]() {
            base = __builtin_amdgcn_readfirstlane(pdcover::run_begin(lo_first, p0));
            pb = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo_first);
            lo_last_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo_last);
        });
        // the end check, for a sweep that reached the stream's end (one a gap ended declines the tile whatever the check would say)
        if (ns && !(s.gap && any_gap_ends)) end_ok = pdcover::nar_end_ok(base, lo_last_u, p0);
    }
    CoverResult r; r.wsum = (uint32_t)wave_total((int)s.sum);
    if (s.gap && any_gap_ends) r.outcome = COV_DECLINED;
    else if (!end_ok) r.outcome = COV_WINDOW;
    else r.outcome = ((!s.gap && s.reach >= (int)ST) || !any_gap_ends) ? COV_SETTLED : COV_DECLINED;
    return r;
}

// ---- cover pass: the WIDE sweep of one tile by one wave ----
// Chunks of CW = 512 runs, eight consecutive lo words per lane as two 16-byte loads (the words are 4-byte aligned, the loads are not): the sorted stream's full
// chunks, its last, partial chunk, then the other stream's (their order does not matter: what they cover is ignored, their lengths count) — 12 KB a tile.
__device__ __forceinline__ CoverResult cover_sweep_wide(const C8Sample &cs, const TileDesc &mine, const DirectWide &args, const uint32_t p0, const uint32_t ln)
{
    constexpr uint32_t ST = TILE, CW = 512u;
    const uint32_t ns = mine.shi - mine.slo, no = mine.ohi - mine.olo;
    const bool any_gap_ends = args.min_dep != 0u;                 // min_dep = 0 counts every cell: only the sum is needed, never stop early
    const uint32_t n_full = ns / CW, n_rem = ns % CW, c_s = n_full + (n_rem ? 1u : 0u), nq = c_s + (no + CW - 1u) / CW;
    const uint32_t neutral = pdcover::run_neutral(p0);
    const uint32_t o_at = cs.o_base + mine.olo;
    // chunk q (wave-uniform): its first run's index in the array, its runs, and how far before it the loads may reach (8 words, or to the array's first)
    auto chunk_at = [&](const uint32_t q) -> uint32_t { return q < c_s ? mine.slo + q * CW : o_at + (q - c_s) * CW; };
    auto chunk_cnt = [&](const uint32_t q) -> uint32_t {
        if (q < n_full) return CW;
        if (q < c_s) return n_rem;
        const uint32_t left = no - (q - c_s) * CW;
        return left < CW ? left : CW;
    };
    auto load = [&](uint32_t (&x)[8], const uint32_t q) {
        const uint32_t qq = q < nq ? q : nq - 1u;
        uint32_t cnt = chunk_cnt(qq);
        if (q >= nq && cnt > 8u) cnt = 8u;                        // behind the last chunk: one place for all lanes
        const uint32_t at = chunk_at(qq), back = at < 8u ? at : 8u;
        const uint32_t *const cb = cs.lo + (at - back);
        const uint32_t rel = chunk_lane_rel(ln, cnt, back, 8u);
        const uint4 u0 = *reinterpret_cast<const uint4 *>(cb + rel), u1 = *reinterpret_cast<const uint4 *>(cb + (rel + 4u));
        x[0] = u0.x; x[1] = u0.y; x[2] = u0.z; x[3] = u0.w; x[4] = u1.x; x[5] = u1.y; x[6] = u1.z; x[7] = u1.w;
    };
    CoverSweep s;
    auto work = [&](uint32_t (&x)[8], const uint32_t q) {
        if (q >= n_full) {                                        // a partial chunk (wave-uniform): keep this lane's own runs
            const uint32_t cnt = chunk_cnt(q), at = chunk_at(q), back = at < 8u ? at : 8u;
            chunk_keep_own(x, chunk_skip(ln, cnt, back, 8u), neutral);
        }
        int b[8], e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { b[k] = pdcover::run_begin(x[k], p0); e[k] = pdcover::run_end(x[k], b[k]); }
        cover_rule_chunk(b, e, q < c_s, [&]() -> uint32_t {
            uint32_t lens = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) lens += x[k] >> 16;
            return lens; }, s);
    };
    if (nq) sweep3<8>(load, work, nq, [&]() -> bool { return s.gap && any_gap_ends; } /* a gap ends the sweep: the tile is declined, its sum is not used */, []() {});
    CoverResult r; r.wsum = (uint32_t)wave_total((int)s.sum);
    r.outcome = ((!s.gap && s.reach >= (int)ST) || !any_gap_ends) ? COV_SETTLED : COV_DECLINED;
    return r;
}

// ---- cover pass: the gate, played over the group's four outcomes in tile order as one workgroup walking them would play it ----
// Every thread reads the four outcomes, so what follows is workgroup-uniform and the same whatever each wave met: a swept tile the gate had closed on by then (an
// earlier tile of the group declined) counts as not tried; a tile settled and tried is written by its wave; every other tile takes the window path.
__device__ __forceinline__ GateOut cover_gate(const uint32_t (&set)[4] /* LDS */, const uint32_t wvu, CoverGate &g)
{
    const uint4 oc4 = *reinterpret_cast<const uint4 *>(&set[0]);
    const uint32_t oc[4] = {(uint32_t)__builtin_amdgcn_readfirstlane((int)oc4.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)oc4.y),
                            (uint32_t)__builtin_amdgcn_readfirstlane((int)oc4.z), (uint32_t)__builtin_amdgcn_readfirstlane((int)oc4.w)};
    GateOut o; o.todo = 0u; o.write_mine = false;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (oc[k] == COV_NONE) continue;
        if (g.skip) { --g.skip; o.todo |= 1u << k; }              // closed: not tried, whatever its wave found
        else if (oc[k] == COV_SETTLED) { ++g.settled; g.miss -= g.miss ? 1u : 0u; if (k == wvu) o.write_mine = true; }
        else {
            o.todo |= 1u << k;
            if (oc[k] == COV_DECLINED) { g.miss += COVER_DECLINE; if (g.miss >= COVER_CLOSE) { g.miss = COVER_CLOSE; g.skip = COVER_SKIP; } }
        }
    }
    return o;
}

// REGISTER DISCIPLINE (what keeps the cover forms at 63 / 64 VGPRs without scratch; the asm volatile lines stand where the values are formed):
//  * what the cover pass derives from the lane (`ln`) and what the window path derives from the thread's number (`tix`) is formed INSIDE that part, from a number
//    made opaque there, not kept in registers across the other part — hoisted out of the walk those values went to scratch;
//  * the tile size a settled tile is written with (`all`) is set where it is written: as a constant it is kept in a register pair from the kernel's top, and spilled;
//  * a sweep's three run buffers live inside pdcover::sweep3, the window fill's two in the branch that uses them: never at the kernel's top;
//  * sweep3 (pd_cover_rule.h) is whole rotations with ONE exit and a tail that works on the last one or two chunks from A and B without a load: the loop
//    holds three copies of a sweep's work and the tail two more, in the same 61 / 64 registers (the buffers are the loop's; the tail declares none);
//  * sweep3 ends with vmcnt(0), so that no sweep's loads are counted by the next one's waits.
template <int WPE, int UN8, bool EXPORT, bool JOIN = false, int LW = 1, bool COVER = false, bool NARROW = false>
__global__ __launch_bounds__(WG, WPE) void k_direct_c8(const C8Sample cs, const TileDesc *__restrict__ desc, uint32_t n_tiles,
                                                     uint32_t wrap_mask, const DirectWide args, uint32_t *__restrict__ heavy_list,
                                                     uint32_t *__restrict__ heavy_count, const DirectExport ex)
{
    static_assert(LW == 1 || (JOIN && (LW == 2 || LW == 4) && UN8 % LW == 0), "wide loads: JOIN form, LW runs per load");
    static_assert(!(COVER && EXPORT), "the cover pass settles statistics, the export form needs every cell");
    static_assert(COVER || !NARROW, "the narrow plane is the cover pass's");
    const uint32_t w = args.w, min_dep = args.min_dep; TilePart *const part = args.part;
    constexpr uint32_t ST = TILE, HT = TILE / 2;
    constexpr int ROWS = (int)(HT / (WG * 4));
    __shared__ __attribute__((aligned(16))) unsigned win[HT];
    __shared__ int s_carry;
    __shared__ int wtot[4];
    __shared__ unsigned long long red_s[4][2];
    __shared__ int red_c[4][2];
    __shared__ __attribute__((aligned(16))) uint32_t s_cov[2][4];  // COVER: the outcome of each wave's tile (COV_*), two sets in turn
    uint32_t cov_flip = 0; CoverGate gate;                        // COVER, workgroup-uniform
    uint32_t cov_fast = 0;                                        // NARROW, wave-uniform: the chunks this wave's sweeps accepted as fast chunks
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // COVER: a step of the walk is a GROUP of four consecutive tiles, one per wave in the cover pass, and the window path for those the pass left
    constexpr uint32_t GT = COVER ? 4u : 1u;
    const uint32_t wvu = COVER ? (uint32_t)__builtin_amdgcn_readfirstlane(wv) : 0u;
    const uint32_t n_steps = COVER ? (n_tiles >> 2) + ((n_tiles & 3u) ? 1u : 0u) : n_tiles;
    // a tile's bounds, its place in its contig and the contig's length are ONE record of the sample's descriptor table (TileDesc), read
    // through a pointer nothing is stored through: scalar loads, issued a tile ahead behind the first run loads, so that no tile waits
    // for metadata and nothing at the top of a tile depends on another load's result but the run loads themselves
    // (COVER: a wave reads the record of ITS tile of the next group; the window path reads a tile's record when it is needed.)
    TileDesc nxt = TileDesc{};
    if constexpr (COVER) { if (blockIdx.x < n_steps && blockIdx.x * 4u + wvu < n_tiles) nxt = desc[blockIdx.x * 4u + wvu]; }   // (32-bit: a group's number is below 2^30)
    else if (blockIdx.x < n_tiles) nxt = desc[blockIdx.x];
    for (uint64_t it = blockIdx.x; it < n_steps; it += gridDim.x) {
      uint32_t todo = 1u;                                         // workgroup-uniform: bit k: tile it * GT + k takes the window path
      if constexpr (COVER) {
        // ---- the cover pass: an interior tile whose depths cannot wrap, asked for min_dep <= 1, needs no window when its runs cover it ----
        // TotalDepth is the sum of the candidates' lengths clipped to the tile, CoveredSite is all of the tile's cells when the sorted stream's runs leave no gap
        // (always, for min_dep = 0).  Wave k sweeps tile 4 * it + k by itself — no LDS window, no barrier, nothing shared with the other waves — lists a pile-up
        // tile and leaves its outcome in s_cov.  Behind ONE barrier the gate is played; a tile it leaves takes the window path below, all four waves together,
        // from its top, so the result never depends on the pass.
        const uint32_t tw = (uint32_t)it * 4u + wvu;              // this wave's tile
        const TileDesc mine = nxt;
        const uint32_t g_next = (uint32_t)it + gridDim.x;
        if (g_next < n_steps && g_next * 4u + wvu < n_tiles) nxt = desc[g_next * 4u + wvu];
        uint32_t outcome = COV_NONE, wsum = 0;                    // wave-uniform
        if (tw < n_tiles) {
            const uint32_t cand = (mine.shi - mine.slo) + (mine.ohi - mine.olo);
            const uint32_t p0 = (tw * ST) & 0xFFFFu;
            uint32_t ln = (uint32_t)lane;                          // made opaque here (register discipline)
            asm volatile("" : "+v"(ln));
            ln &= 63u;                                            // (its range known again: the loads' offsets fit 32 bits, so they need no address pairs)
            if (cand > 32000u) {                                  // the int-window kernel does this tile
                if (ln == 0u) heavy_list[atomicAdd(heavy_count, 1u)] = tw;
            } else {
                outcome = COV_WINDOW;
                if (cover_eligible(mine, cs, args, wrap_mask, gate.skip, wvu)) {
                    CoverResult r;
                    if constexpr (NARROW) r = cover_sweep_narrow(cs, mine, args, p0, ln, cov_fast);
                    else r = cover_sweep_wide(cs, mine, args, p0, ln);
                    outcome = r.outcome; wsum = r.wsum;
                }
            }
            if (ln == 0u) s_cov[cov_flip][wvu] = outcome;
        } else if (lane == 0) s_cov[cov_flip][wvu] = COV_NONE;
        __syncthreads();                                          // (the sets alternate: the next group's waves write the other four while a late wave still reads these)
        const GateOut go = cover_gate(s_cov[cov_flip], wvu, gate);
        cov_flip ^= 1u;
        todo = go.todo;
        if (go.write_mine && lane == 0) {
            uint32_t all = ST;
            asm volatile("" : "+v"(all));                         // (set here: register discipline)
            TilePart tp; tp.c0 = all; tp.c1 = 0u; tp.s0 = wsum; tp.s1 = 0ull; part[tw] = tp;
        }
      }
#pragma unroll 1
      for (uint32_t kt = 0; kt < GT; ++kt) {
        if (COVER && !((todo >> kt) & 1u)) continue;
        // COVER: what the window path derives from the thread's number is formed here again for every tile that takes it, not kept in registers
        // across the cover pass (72 VGPRs hold both only this way: the pass needs its three buffers)
        uint32_t tix = threadIdx.x;
        if constexpr (COVER) { asm volatile("" : "+v"(tix)); tix &= (uint32_t)WG - 1u; }
        const int lane = (int)(tix & 63u), wv = (int)(tix >> 6);
        const uint64_t t = it * GT + kt;
        const uint64_t a = t * ST;
        const TileDesc cur = COVER ? desc[t] : nxt;
        const uint64_t t_next = COVER ? ~0ull : t + gridDim.x;    // (COVER: nxt is not the window path's)
        const uint32_t ns = cur.shi - cur.slo, s_at = cur.slo;    // the tile's candidates in the sorted stream
        const uint32_t olo = cur.olo, no = cur.ohi - olo;         // ... and in the other stream
        const uint32_t cand = ns + no;
        const uint32_t clen = cur.clen;
        const uint32_t p0 = (uint32_t)a & 0xFFFFu;                // the low 16 bits of the tile's first flat cell, like the runs' begins in the lo plane
        const uint32_t pc = cur.pc;                               // the tile's first cell inside its contig
        if (!COVER && cand > 32000u) {                            // workgroup-uniform: the int-window kernel does this tile (no LDS touched: no barrier)
            if (tix == 0) heavy_list[atomicAdd(heavy_count, 1u)] = (uint32_t)t;
            if (t_next < n_tiles) nxt = desc[t_next];
            continue;
        }
        uint4 *w4 = reinterpret_cast<uint4 *>(win);
        int carry_s = 0;
        {
            // ONE sequence of chunks: those of the sorted stream's candidates, then those of the other stream's — which stream a chunk
            // belongs to is a scalar decision (base index, position, end), so the double-buffered loop runs through both without a restart
            constexpr uint32_t C = UN8 * WG;
            const uint32_t *__restrict__ const p = cs.lo;
            // JOIN: the sorted stream's full chunks, then its remainder and the other stream's runs as ONE sequence (a lane picks its array by
            // its index there) — four chunks for the typical tile's 2 730 + 300 candidates instead of four + one
            const uint32_t c1 = JOIN ? ns / C : (ns + C - 1) / C;
            const uint32_t rem = JOIN ? ns - c1 * C : 0u, tail = rem + no;
            const uint32_t nq = c1 + ((JOIN ? tail : no) + C - 1) / C;
            const uint32_t o_at = cs.o_base + olo;
            // slot k of a lane is run slot(k) of its chunk
            auto slot = [&](const int k) -> uint32_t { return (uint32_t)LW * (tix + (uint32_t)(k / LW) * WG) + (uint32_t)(k % LW); };
            auto load8 = [&](uint32_t (&dst)[UN8], const uint32_t q) {
                const bool second = q >= c1;
                if constexpr (JOIN) {
                    if (!second) {
                        const uint32_t *const pq = p + (s_at + q * C);
                        if constexpr (LW == 4) {
#pragma unroll
                            for (int k4 = 0; k4 < UN8 / 4; ++k4) {
                                const uint4 u = *reinterpret_cast<const uint4 *>(pq + slot(4 * k4));
                                dst[4 * k4] = u.x; dst[4 * k4 + 1] = u.y; dst[4 * k4 + 2] = u.z; dst[4 * k4 + 3] = u.w;
                            }
                        } else if constexpr (LW == 2) {
#pragma unroll
                            for (int k2 = 0; k2 < UN8 / 2; ++k2) {
                                const uint2 u = *reinterpret_cast<const uint2 *>(pq + slot(2 * k2));
                                dst[2 * k2] = u.x; dst[2 * k2 + 1] = u.y;
                            }
                        } else {
#pragma unroll
                            for (int k = 0; k < UN8; ++k) dst[k] = pq[slot(k)];
                        }
                    } else {
                        const uint32_t i = (q - c1) * C, s_rem = s_at + c1 * C, o_rem = o_at - rem, last = tail - 1u;
#pragma unroll
                        for (int k = 0; k < UN8; ++k) {
                            uint32_t j = i + slot(k); j = j < last ? j : last;
                            dst[k] = p[(j < rem ? s_rem : o_rem) + j];
                        }
                    }
                    return;
                }
                const uint32_t at = second ? o_at : s_at, i = (second ? q - c1 : q) * C, last = (second ? no : ns) - 1u;
#pragma unroll
                for (int k = 0; k < UN8; ++k) { const uint32_t j = i + tix + k * WG; dst[k] = p[at + (j < last ? j : last)]; }
            };
            auto ev8 = [&](const uint32_t r) {
                const uint32_t sb = (r - p0) & 0xFFFFu, se = sb + (r >> 16), se16 = se & 0xFFFFu;
                const unsigned long long m_c = __builtin_amdgcn_ballot_w64(se >= 0x10000u);
                if (sb < ST) atomicAdd(&win[sb & (HT - 1u)], 1u + (sb >> 12) * 0xFFFFu);
                if (se16 < ST) atomicSub(&win[se16 & (HT - 1u)], 1u + (se16 >> 12) * 0xFFFFu);
                carry_s += __builtin_popcountll(m_c);
            };
            auto work8 = [&](const uint32_t (&c)[UN8], const uint32_t q) {
                const bool second = q >= c1;
                const uint32_t left = JOIN ? (second ? tail - (q - c1) * C : C) : (second ? no : ns) - (second ? q - c1 : q) * C;
                if (left >= C) {
#pragma unroll
                    for (int k = 0; k < UN8; ++k) ev8(c[k]);
                } else {                                          // a stream's tail chunk: slots past the end become runs outside the tile
                    const int nu = LW * (int)((left + LW * WG - 1) / (LW * WG));   // uniform, 1 .. UN8
#pragma unroll
                    for (int k = 0; k < UN8; ++k) if (k < nu) ev8(slot(k) < left ? c[k] : (p0 + ST) & 0xFFFFu);
                }
            };
            auto clear_window = [&]() {                           // ... and the next tile's descriptor: behind the run loads, so that the wait in front of the barrier covers both
                for (uint32_t j = tix; j < HT / 4; j += WG) w4[j] = make_uint4(0u, 0u, 0u, 0u);
                if (tix == 0) s_carry = 0;
                if (t_next < n_tiles) nxt = desc[t_next];
                __syncthreads();
            };
            if (!nq) clear_window();                              // (workgroup-uniform: every thread meets one of the two barriers)
            else {
                uint32_t A[UN8], B[UN8];
                uint32_t q = 0;
                load8(A, q);                                      // the first chunk is on its way before the window is cleared: nothing it needs is in LDS
                clear_window();
#pragma unroll 1
                for (;;) {                                        // two buffers, no register copies: B is in flight while A is worked on
                    if (q + 1 < nq) load8(B, q + 1);
                    work8(A, q);
                    if (++q >= nq) break;
                    if (q + 1 < nq) load8(A, q + 1);
                    work8(B, q);
                    if (++q >= nq) break;
                }
            }
        }
        if (lane == 0 && carry_s != 0) atomicAdd(&s_carry, carry_s);
        __syncthreads();
        if constexpr (EXPORT) {
            export_packed_tile<ROWS>(win, a, t, ex, wtot);
            continue;
        }
        // ---- prefix sum of the packed window: both half-tiles at once ----
        int4 v[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint4 q = w4[wv * (ROWS * 64) + r * 64 + lane];
            v[r] = make_int4((int)q.x, (int)q.x + (int)q.y, 0, 0);
            v[r].z = v[r].y + (int)q.z; v[r].w = v[r].z + (int)q.w;
        }
        int ex[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) ex[r] = wave_incl_scan(v[r].w);
        int run = 0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int e = run + ex[r] - v[r].w;                   // exclusive prefix of this lane's group in the wave
            run += __builtin_amdgcn_readlane(ex[r], 63);
            ex[r] = e;
        }
        if (lane == 0) wtot[wv] = run;
        __syncthreads();
        int basep = 0;                                            // packed: words of the waves before this one
        for (int k = 0; k < wv; ++k) basep += wtot[k];
        const int totp = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        const int tl = (int)(short)(totp & 0xffff);               // begins - ends over the low half-tile
        const int carry_l = s_carry, carry_h = carry_l + tl;      // depth just before cell 0 / cell HT of the tile
        // ---- the tile's share of windows k0 and k0 + 1 ----
        const uint64_t local0 = pc;
        int c0 = 0, c1 = 0; unsigned long long s0 = 0, s1 = 0;
        bool uniform_counts = false;                              // c0 is a wave count (ballots), s0 a 32-bit lane sum
        if (local0 < clen) {
            const uint64_t k0 = local0 / w;
            const uint64_t nb64 = (k0 + 1) * (uint64_t)w - local0;   // tile-local start of window k0+1
            const uint32_t nb = nb64 > (uint64_t)ST ? ST : (uint32_t)nb64;
            const uint64_t left = (uint64_t)clen - local0;
            const uint32_t lim = left > (uint64_t)ST ? ST : (uint32_t)left;
            const uint64_t dmax = (uint64_t)(uint32_t)carry_l + cand;     // no depth in this tile exceeds carry + begins
            const bool inner = nb >= ST && lim >= ST;             // inside one window, inside the contig
            bool settled = false;                                 // wave-uniform
            if (inner && dmax <= 0xFFFFu && dmax <= wrap_mask) {
                // every depth of the tile fits 16 bits and cannot wrap: with both carries folded into the row's addend a packed word IS
                // two depths (the low half is >= 0, so nothing is borrowed from the high one).  Per word: a packed minimum and a sum of
                // both halves.  A wave whose least depth reaches the threshold has counted all its cells; any other takes the exact loops.
                typedef unsigned short us2 __attribute__((ext_vector_type(2)));
                const uint32_t both = ((uint32_t)carry_h << 16) + (uint32_t)carry_l;
                uint32_t mn = 0xFFFFFFFFu, acc = 0;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const uint32_t add = (uint32_t)(basep + ex[r]) + both;
                    const uint32_t pw[4] = {(uint32_t)v[r].x + add, (uint32_t)v[r].y + add, (uint32_t)v[r].z + add, (uint32_t)v[r].w + add};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        mn = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, mn), __builtin_bit_cast(us2, pw[q])));
                        acc = __builtin_amdgcn_sad_u16(pw[q], 0u, acc);
                    }
                }
                const uint32_t least = (mn & 0xFFFFu) < (mn >> 16) ? (mn & 0xFFFFu) : (mn >> 16);
                if (__builtin_amdgcn_ballot_w64(least < min_dep) == 0ull) {
                    c0 = (int)(ROWS * 8 * 64); s0 = acc; settled = true;
                }
            }
            if (settled) uniform_counts = true;
            else if (inner && dmax < (1u << 27)) {
                uint32_t s32 = 0; int cnt = 0;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int add = basep + ex[r];
                    const int pw[4] = {v[r].x + add, v[r].y + add, v[r].z + add, v[r].w + add};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int L = (int)(short)(pw[q] & 0xffff), H = (pw[q] - L) >> 16;
                        const uint32_t dl = (uint32_t)(L + carry_l) & wrap_mask, dh = (uint32_t)(H + carry_h) & wrap_mask;
                        const bool okl = dl >= min_dep, okh = dh >= min_dep;
                        cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(okl)) + __builtin_popcountll(__builtin_amdgcn_ballot_w64(okh));
                        s32 += (okl ? dl : 0u) + (okh ? dh : 0u);
                    }
                }
                c0 = cnt; s0 = s32; uniform_counts = true;
            } else {
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int add = basep + ex[r];
                    const uint32_t pos = (uint32_t)(wv * (ROWS * 256) + r * 256 + lane * 4);
                    const int pw[4] = {v[r].x + add, v[r].y + add, v[r].z + add, v[r].w + add};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int L = (int)(short)(pw[q] & 0xffff), H = (pw[q] - L) >> 16;
                        const uint32_t dl = (uint32_t)(L + carry_l) & wrap_mask, dh = (uint32_t)(H + carry_h) & wrap_mask;
                        const uint32_t pl = pos + q, ph = pl + HT;
                        if (pl < lim && dl >= min_dep) { if (pl < nb) { ++c0; s0 += dl; } else { ++c1; s1 += dl; } }
                        if (ph < lim && dh >= min_dep) { if (ph < nb) { ++c0; s0 += dh; } else { ++c1; s1 += dh; } }
                    }
                }
            }
        }
        if (uniform_counts) {                                     // workgroup-uniform
            const uint32_t s32 = (uint32_t)s0;
            const unsigned long long lo16 = (unsigned long long)(uint32_t)wave_total((int)(s32 & 0xffffu));
            const unsigned long long hi16 = (unsigned long long)(uint32_t)wave_total((int)(s32 >> 16));
            s0 = (hi16 << 16) + lo16;
        } else {
            c0 = wave_sum(c0); c1 = wave_sum(c1);
#pragma unroll
            for (int o = 32; o; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
        }
        if (lane == 0) { red_c[wv][0] = c0; red_c[wv][1] = c1; red_s[wv][0] = s0; red_s[wv][1] = s1; }
        __syncthreads();
        if (tix == 0) {
            TilePart tp;
            tp.c0 = (uint32_t)(red_c[0][0] + red_c[1][0] + red_c[2][0] + red_c[3][0]);
            tp.c1 = (uint32_t)(red_c[0][1] + red_c[1][1] + red_c[2][1] + red_c[3][1]);
            tp.s0 = red_s[0][0] + red_s[1][0] + red_s[2][0] + red_s[3][0];
            tp.s1 = red_s[0][1] + red_s[1][1] + red_s[2][1] + red_s[3][1];
            part[t] = tp;
        }
      }
    }
    if constexpr (COVER) {                                        // how many tiles the pass settled: one addition per workgroup, for the tests
        if (threadIdx.x == 0 && gate.settled) atomicAdd(heavy_count + PD_HEAVY_SETTLED, gate.settled);
        if constexpr (NARROW) {                                   // ... and how many chunks went the fast way: the four waves' counts, one addition
            __syncthreads();                                      // (wtot's last readers are done)
            if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = (int)cov_fast;
            __syncthreads();
            const uint32_t n_fast = (uint32_t)(wtot[0] + wtot[1] + wtot[2] + wtot[3]);
            if (threadIdx.x == 0 && n_fast) atomicAdd(heavy_count + PD_HEAVY_FAST, n_fast);
        }
    }
}

// Outcome of a direct pass: *fail = 1 unless every batch was complete and sorted and no run was
// longer than the look-back; re-arms the descriptors (the batches stay pending for the fallback).
__global__ void k_finish_direct(const PendSet ps, const uint32_t *n_long, uint32_t *fail)
{
    uint32_t bad = *n_long != 0, errs = 0;
    uint64_t handled = 0, has = 0, ends = 0, n = 0;
    for (int b = 0; b < ps.nb; ++b) {
        BatchDesc *desc = ps.b[b].desc;
        for (int k = 0; k < PD_CNT_SLOTS; ++k) {
            handled += desc->handled[k]; has += desc->has[k]; ends += desc->ends[k];
            desc->handled[k] = 0; desc->has[k] = 0; desc->ends[k] = 0;
        }
        n += ps.b[b].n;
        if (desc->err) bad = 1;
        errs |= desc->err;
        desc->ovf_count = 0; desc->err = 0; desc->t_first = 0; desc->n_active = 0;
    }
    if (handled != n || has != ends) bad = 1;
    *fail = bad;
    if (bad) {                                   // why (read by the host for its diagnostics): fail + 2 .. fail + 9
        const uint32_t err = errs;
        fail[2] = (uint32_t)handled; fail[3] = (uint32_t)(handled >> 32); fail[4] = (uint32_t)n; fail[5] = (uint32_t)(n >> 32);
        fail[6] = (uint32_t)has; fail[7] = (uint32_t)ends; fail[8] = err; fail[9] = *n_long;
    }
}

// ------------------------------------------------------------------------------------------
// launch wrappers (called from pd_windows.hip and pd_capi.hip; the row statistics of pd_rows.hip launch nothing of this file)
// ------------------------------------------------------------------------------------------
void launch_direct_tiles(hipStream_t st, const PendSet &ps, ContigTab tab, const uint32_t *tile_contig, uint32_t n_tiles,
                         uint32_t wrap_mask, uint32_t w, uint32_t min_dep, TilePart *part, const uint64_t *win_off,
                         uint32_t *cover, unsigned long long *sum, uint32_t *n_long, uint32_t *fail,
                         uint32_t *heavy_list, uint32_t *heavy_count, unsigned grid_tiles, int un)
{
    WinArgs wa; wa.w = w; wa.min_dep = min_dep; wa.inv_w = 1.0f / (float)w; wa.cover = cover; wa.sum = sum; wa.part = part;
    const DirectWide dw{w, min_dep, part};
    const DirectNarrow dn{wa, win_off};
#define PD_DIRECT(UN_, WPE_) hipLaunchKernelGGL((k_direct_tiles<UN_, WPE_, DirectWide>), dim3(grid_tiles), dim3(WG), 0, st, ps, \
                                                n_tiles, tab, tile_contig, wrap_mask, dw, n_long, heavy_list, heavy_count)
    if (w < (uint32_t)TILE)
        hipLaunchKernelGGL((k_direct_tiles<4, 4, DirectNarrow>), dim3(grid_tiles), dim3(WG), 0, st, ps, n_tiles, tab, tile_contig,
                           wrap_mask, dn, n_long, heavy_list, heavy_count);
    else if (un == 0 || un >= 3000) {        // second form (k_direct_wide3): 3000 + 100 x waves-per-SIMD target + loads in flight per thread
#define PD_DIRECT3(UN_, WPE_) hipLaunchKernelGGL((k_direct_wide3<UN_, WPE_, false>), dim3(grid_tiles), dim3(WG), 0, st, ps, n_tiles, tab, tile_contig, wrap_mask, dw, heavy_list, heavy_count, DirectExport{})
        // measured on the bench sample (ms; variants that were tried and are no longer compiled included): <2, 6> 3.08-3.13,
        // <4, 5> 3.10-3.28, <3, 5> 3.2, <2, 7> 3.3, <2, 5> 3.4, <4, 4> 3.6-3.8, <1, 8> 3.6, <2, 8> 4.1 (spills), <4, 6> 3.5
        // (spills); first form 3.52-3.69.  Grids of 16 K .. 262 K workgroups: within 2 %.
        switch (un) {
        case 3404: PD_DIRECT3(4, 4); break;
        case 3504: PD_DIRECT3(4, 5); break;
        default: PD_DIRECT3(2, 6); break;
        }
#undef PD_DIRECT3
    }
    else switch (un) {                       // tuning knob "direct_un": loads in flight per thread + 100 x waves-per-SIMD target
    default: PD_DIRECT(4, 5); break;         // 504 (or any other value below 3000): the first form, kept as the cross-check of the second
                                             // (measured on the bench sample, ms: <4, 5> 3.5-3.7; its other variants <8, 5> 3.3-3.6, <4, 4> 3.7, <8, 4> 3.7 are no longer compiled)
    }
#undef PD_DIRECT
    hipLaunchKernelGGL(k_direct_tiles_heavy, dim3(128), dim3(WG), 0, st, ps, n_tiles, tab, tile_contig, wrap_mask, wa, win_off,
                       n_long, (const uint32_t *)heavy_list, (const uint32_t *)heavy_count, DirectExport{});
    if (w < (uint32_t)TILE) launch_window_edges(st, part, TileMap{tile_contig, tab.off, tab.len, win_off}, n_tiles, w, cover, sum);   // (k_window_edges is pd_kernels.hip's)
    hipLaunchKernelGGL(k_finish_direct, dim3(1), dim3(1), 0, st, ps, n_long, fail);
}

// "direct_un" for a compact sample: 100 x waves-per-SIMD target + loads in flight per thread; + 1000: the joined tail (JOIN); 5000 + / 9000 +: JOIN with 8- / 16-byte
// loads (two / four runs per lane and load) in the sorted stream's full chunks.  One line per code: code, WPE, UN8, JOIN, LW.  What each measured: DESIGN.md, section 3.
#define PD_C8_CODES(X) \
    X(502, 5, 2, false, 1) \
    X(504, 5, 4, false, 1) \
    X(508, 5, 8, false, 1) \
    X(602, 6, 2, false, 1) \
    X(604, 6, 4, false, 1) \
    X(702, 7, 2, false, 1) \
    X(802, 8, 2, false, 1) \
    X(804, 8, 4, false, 1) \
    X(801, 8, 1, false, 1) \
    X(708, 7, 8, false, 1) \
    X(803, 8, 3, false, 1) \
    X(703, 7, 3, false, 1) \
    X(704, 7, 4, false, 1) \
    X(1803, 8, 3, true, 1) \
    X(1703, 7, 3, true, 1) \
    X(1704, 7, 4, true, 1) \
    X(1802, 8, 2, true, 1) \
    X(1708, 7, 8, true, 1) \
    X(5704, 7, 4, true, 2) \
    X(5702, 7, 2, true, 2) \
    X(5802, 8, 2, true, 2) \
    X(5706, 7, 6, true, 2) \
    X(5708, 7, 8, true, 2) \
    X(5608, 6, 8, true, 2) \
    X(9704, 7, 4, true, 4) \
    X(9708, 7, 8, true, 4) \
    X(9608, 6, 8, true, 4)

// The statistics form.  Any other code (0 among them) is the default <7, 4> with the joined tail: with the cover pass in front of the window path when L.cover,
// its narrow sweep when L.narrow as well and the sample has the nar plane.  Returns whether the narrow form was the one launched.
bool launch_direct_c8(const DirectC8Launch &L)
{
    const DirectWide dw{L.w, L.min_dep, L.part, L.cover_min, L.fast ? 1u : 0u};
#define PD_C8_GO(...) hipLaunchKernelGGL((k_direct_c8<__VA_ARGS__>), dim3(L.grid_tiles), dim3(WG), 0, L.st, L.cs, L.desc, L.n_tiles, L.wrap_mask, dw, L.heavy_list, L.heavy_count, DirectExport{})
#define PD_C8_CASE(CODE_, WPE_, UN8_, JOIN_, LW_) case CODE_: PD_C8_GO(WPE_, UN8_, false, JOIN_, LW_); return false;
    switch (L.un) { PD_C8_CODES(PD_C8_CASE) default: break; }
#undef PD_C8_CASE
    const bool narrow = L.cover && L.narrow && L.cs.nar;
    if (narrow) PD_C8_GO(7, 4, false, true, 1, true, true);
    else if (L.cover) PD_C8_GO(7, 4, false, true, 1, true);
    else PD_C8_GO(7, 4, false, true, 1);
#undef PD_C8_GO
    return narrow;
}

// k_c8_heavy's form, by measurement on the bench's 12 pile-up tiles of 32 025 - 48 063 candidates (profiles/r12_pileup_gather_ab.txt): 1024 threads with 8 loads each
constexpr int HEAVY_UN = 8, HEAVY_NT = 1024;

void launch_direct_c8_heavy(hipStream_t st, C8Sample cs, ContigTab tab, const uint32_t *tile_contig, uint32_t n_tiles, uint32_t wrap_mask, uint32_t w, uint32_t min_dep,
                            TilePart *part, const uint32_t *heavy_tiles, uint32_t n_heavy)
{
    if (!n_heavy) return;
    WinArgs wa; wa.w = w; wa.min_dep = min_dep; wa.inv_w = 1.0f / (float)w; wa.cover = nullptr; wa.sum = nullptr; wa.part = part;
    // a workgroup per listed tile (the sample's own count), so that no list is walked by a fixed few workgroups in turns
    const unsigned grid = n_heavy < 1024u ? n_heavy : 1024u;
    hipLaunchKernelGGL((k_c8_heavy<false, HEAVY_UN, HEAVY_NT>), dim3(grid), dim3(HEAVY_NT), 0, st, cs, n_tiles, tab, tile_contig, wrap_mask, wa, heavy_tiles,
                       (const uint32_t *)nullptr, n_heavy, DirectExport{});
}

void launch_direct_c8_export(const DirectC8Launch &L)
{
    const DirectExport de{(unsigned short *)L.img, L.exc, L.cap, L.count, L.sums};
    hipLaunchKernelGGL((k_direct_c8<7, 4, true, true>), dim3(L.grid_tiles), dim3(WG), 0, L.st, L.cs, L.desc, L.n_tiles, 0xFFFFFFFFu,
                       DirectWide{(uint32_t)TILE, 1u, nullptr}, L.heavy_list, L.heavy_count, de);
    WinArgs wa; wa.w = (uint32_t)TILE; wa.min_dep = 1; wa.inv_w = 0.f; wa.cover = nullptr; wa.sum = nullptr; wa.part = nullptr;
    // (launched for a sample without pile-up tiles too, one workgroup then: this call has no check of the list's length behind it)
    const unsigned grid = L.n_heavy < 1024u ? (L.n_heavy ? L.n_heavy : 1u) : 1024u;
    hipLaunchKernelGGL((k_c8_heavy<true, HEAVY_UN, HEAVY_NT>), dim3(grid), dim3(HEAVY_NT), 0, L.st, L.cs, L.n_tiles, L.tab, L.tile_contig, 0xFFFFFFFFu, wa,
                       (const uint32_t *)L.heavy_list, (const uint32_t *)L.heavy_count, 0u, de);
}

void launch_direct_export(hipStream_t st, const PendSet &ps, ContigTab tab, const uint32_t *tile_contig, uint32_t n_tiles,
                          void *img, pd_exc *exc, uint32_t cap, uint32_t *count, int *sums, uint32_t *n_long, uint32_t *fail,
                          uint32_t *heavy_list, uint32_t *heavy_count, unsigned grid_tiles)
{
    const DirectExport de{(unsigned short *)img, exc, cap, count, sums};
    // the second form of the direct kernel with its export branch (the first form's export instantiation — 128 VGPRs and
    // 160 bytes of spills — took 5.2 ms per sample)
    hipLaunchKernelGGL((k_direct_wide3<2, 5, true>), dim3(grid_tiles), dim3(WG), 0, st, ps, n_tiles, tab, tile_contig, 0xFFFFFFFFu,
                       DirectWide{(uint32_t)TILE, 1u, nullptr}, heavy_list, heavy_count, de);
    // tiles with more than 32 000 candidates: the int-window kernel exports them
    WinArgs wa; wa.w = (uint32_t)TILE; wa.min_dep = 1; wa.inv_w = 0.f; wa.cover = nullptr; wa.sum = nullptr; wa.part = nullptr;
    hipLaunchKernelGGL(k_direct_tiles_heavy, dim3(128), dim3(WG), 0, st, ps, n_tiles, tab, tile_contig, 0xFFFFFFFFu, wa,
                       (const uint64_t *)nullptr, n_long, (const uint32_t *)heavy_list, (const uint32_t *)heavy_count, de);
    hipLaunchKernelGGL(k_finish_direct, dim3(1), dim3(1), 0, st, ps, n_long, fail);
}

} // namespace pdk

#ifdef PD_WIDE3_TICKS
extern "C" int pd_x_wide3_ticks(unsigned long long *out16)
{
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(pdk::g_wide3_ticks), sizeof z) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(pdk::g_wide3_ticks), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
