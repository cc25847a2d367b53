// pd_kernels.hip — hand-written gfx950 kernels of the per-base depth engine, all but the direct depth pass (pd_direct.hip) and the levels, quantile and threshold kernels of the row statistics (pd_rows.hip;
// what the three files' kernels share is pd_dev.h).
//
// Everything here is HBM-bound integer work (no MFMA): a zero fill, the +1/-1 difference-array
// scatter (owner-tile LDS accumulation with plain int4 read-modify-write flush for sorted
// batches; device atomics for unsorted ones), the prefix-sum sweep (diff -> depth) with an
// optional fused fixed-window reduction, and a segmented interval reduction.
//
// Data layout in HBM (one allocation, int32 cells):
//   [ contig 0 slot | contig 1 slot | ... | tile sums ]
// Every contig slot is rounded up to PD_TILE cells, so a tile belongs to exactly one contig.
// Slot t holds the difference array d[p] (+1 at run begin, -1 at run end, runs clipped to
// [0, len]); a contig's slot sums to zero, so ONE flat prefix sum over all slots yields every
// contig's depth with no segment resets.  tile_sum[k] = sum of d over tile k is maintained by
// the scatter kernels; an exclusive scan of it gives each tile's carry-in, which makes the
// sweep a single embarrassingly parallel pass (no look-back, no inter-workgroup hand-off).
//
// Reference semantics restated (PD = /root/reference/src/PanDepth.cpp):
//   scatter        == `for (; StartRead<endTmp; StartRead++) depth[..][StartRead]++`  PD:449-452
//   scan (+wrap18) == the value a SiteInfo{unsigned Depth:18} / unsigned int cell holds PD:717, DataClass.h:85
//   reductions     == StatChrDepthLowMEM / StatChrDepthWin / mode-6 sweep              PD:329-348, 295-327, 4366-4389
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pd_kernels.h"
#include "pd_dev.h"
#include "pd_cover_rule.h"

namespace pdk {


// ------------------------------------------------------------------------------------------
// fill: 16 B/lane stores, grid-stride
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_fill(int4 *p, size_t n16)
{
    size_t i = blockIdx.x * (size_t)WG + threadIdx.x;
    const size_t st = (size_t)gridDim.x * WG;
    const int4 z = make_int4(0, 0, 0, 0);
    for (; i < n16; i += st) p[i] = z;
}

// pd_reset's four spans zeroed by ONE launch (four hipMemsetAsync calls were six fill kernels, 34 us of the traced bench step from the first one's
// start to the last one's end; this kernel: 3 us — profiles/r11_direct_call_ab.txt): 16-byte stores where the span begins on a 16-byte boundary,
// bytes for its tail (or for all of it)
__global__ __launch_bounds__(WG) void k_reset_spans(const ResetSpans rs)
{
    const size_t i0 = blockIdx.x * (size_t)WG + threadIdx.x;
    const size_t st = (size_t)gridDim.x * WG;
    const int4 z = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < ResetSpans::N; ++k) {
        unsigned char *p = static_cast<unsigned char *>(rs.p[k]);
        const size_t n = rs.bytes[k];
        const size_t n16 = (reinterpret_cast<uintptr_t>(p) & 15) ? 0 : n / 16;
        int4 *q = reinterpret_cast<int4 *>(p);
        for (size_t i = i0; i < n16; i += st) q[i] = z;
        for (size_t i = n16 * 16 + i0; i < n; i += st) p[i] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// scatter, unsorted fallback: two device atomics per run (+ tile-sum atomics only when the
// run crosses a tile boundary; inside one tile +1 and -1 cancel in the tile sum)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_scatter_atomic(const pd_iv *iv, size_t n, ContigTab tab,
                                                       int *diff, int *sums)
{
    size_t i = blockIdx.x * (size_t)WG + threadIdx.x;
    const size_t st = (size_t)gridDim.x * WG;
    for (; i < n; i += st) {
        const Ev e = expand(iv[i], tab);
        if (!e.has) continue;
        atomicAdd(&diff[e.gb], 1);
        atomicAdd(&diff[e.ge], -1);
        const uint64_t tb = e.gb / TILE, te = e.ge / TILE;
        if (tb != te) { atomicAdd(&sums[tb], 1); atomicAdd(&sums[te], -1); }
    }
}

// ------------------------------------------------------------------------------------------
// scatter, sorted batches.  Step 1: sparse index.  One thread per sample (every S-th run):
// because the batch is sorted by flat begin, sample values bracket where each tile's
// candidates start and stop.  For tile t = [a, a+TILE):
//   cand_lo[t] <= first run with gb >= a - LMAX   (look-back: short runs ending in the tile)
//   ub_a[t+1]  >= first run with gb >= a + TILE
// ------------------------------------------------------------------------------------------
template <int ST>
__global__ __launch_bounds__(WG) void k_index(const pd_iv *iv, uint32_t n, uint32_t S, ContigTab tab,
                                              uint32_t lmax, uint32_t dis, uint32_t *ub_a, uint32_t *cand_lo,
                                              uint32_t n_tiles, BatchDesc *desc)
{
    // `dis` = disorder bound D: for runs i < j of the batch, gb_j >= gb_i - D (0 = sorted).  Then
    //   every run at index >= p_k has gb >= s_k - D,   every run at index < p_k has gb <= s_k + D,
    // so all thresholds below just move by D; the samples themselves need not be monotone (any
    // sample pair that brackets a threshold gives a valid, possibly looser, bound).
    const uint32_t K = (n + S - 1) / S + 1;
    const uint32_t k = blockIdx.x * WG + threadIdx.x;
    if (k >= K) return;
    const uint64_t pk64 = (uint64_t)k * S;
    const uint32_t pk = pk64 < n ? (uint32_t)pk64 : n;
    const Ev last = expand(iv[n - 1], tab);
    const int64_t D = dis, T = ST;
    const int64_t sentinel = (int64_t)last.gb + 2 * D + lmax + 1;
    int64_t sk;
    if (pk < n) { const Ev e = expand(iv[pk], tab); if (!e.valid) atomicOr(&desc->err, 1u); sk = (int64_t)e.gb; }
    else sk = sentinel;
    int64_t t_last = (sentinel - D) / T; if (t_last >= (int64_t)n_tiles) t_last = (int64_t)n_tiles - 1;
    const Ev first = expand(iv[0], tab);
    const int64_t s0 = (int64_t)first.gb;
    const int64_t t_first = (s0 - D) > 0 ? (s0 - D) / T : 0;
    const int64_t sk_left = __shfl_up(sk, 1);               // every lane of the wave is still here
    if (k == 0) {
        desc->t_first = (uint32_t)t_first;
        if (t_first > t_last) { desc->n_active = 0; atomicOr(&desc->err, 2u); return; }   // not sorted
        desc->n_active = (uint32_t)(t_last - t_first + 1);
        int64_t t1 = (s0 - D) >= 0 ? (s0 - D) / T : -1; if (t1 > t_last + 1) t1 = t_last + 1;
        for (int64_t t = t_first; t <= t1; ++t) ub_a[t] = 0;
        int64_t t2 = (s0 + lmax + D) / T; if (t2 > t_last) t2 = t_last;
        for (int64_t t = t_first; t <= t2; ++t) cand_lo[t] = 0;
        ub_a[t_last + 1] = n;
        return;
    }
    const uint32_t pkm1 = (k - 1) * S;      // < n for every k >= 1
    int64_t sp;
    {
        // the previous sample is the left neighbour's value: one scattered 12-byte load per thread
        // instead of two (lane 0 of a wave and the thread right after the k == 0 exit load their own)
        const bool own = (threadIdx.x & 63) == 0;
        sp = own ? (int64_t)expand(iv[pkm1], tab).gb : sk_left;
    }
    {   // tiles with a_t + D in (sp, sk]: every run at index >= p_k starts at or after a_t
        int64_t lo = (sp - D) >= 0 ? (sp - D) / T + 1 : 0, hi = (sk - D) >= 0 ? (sk - D) / T : -1;
        if (lo < t_first) lo = t_first;
        if (hi > t_last + 1) hi = t_last + 1;
        for (int64_t t = lo; t <= hi; ++t) ub_a[t] = pk;
    }
    {   // tiles with a_t - lmax - D in (sp, sk]: every run at index < p_{k-1} ends before a_t
        int64_t lo = (sp + lmax + D) / T + 1, hi = (sk + lmax + D) / T;
        if (lo < t_first) lo = t_first;
        if (hi > t_last) hi = t_last;
        for (int64_t t = lo; t <= hi; ++t) cand_lo[t] = pkm1;
    }
}

// Step 2: owner tiles.  A persistent grid walks the tiles the pending batches touch (up to
// PD_MAXPEND sorted batches share ONE pass, e.g. a sample's first-run stream and its nearly sorted
// second-run stream); each workgroup zeroes an ST-cell LDS window, pulls every event that lands in
// ITS tile from each batch's candidate range (LDS atomics), then writes the window to HBM with
// plain 16-byte accesses: a half-tile that has not been written since the last reset is STORED
// (no read, no prior zero fill needed), otherwise read-modify-written with all-zero 16-byte
// groups skipped.  No global atomics on the hot path.  Ends of runs longer than LMAX go to the
// overflow list (applied by k_apply_overflow after this kernel).
template <int ST>
__global__ __launch_bounds__(WG) void k_scatter_tiles(const PendSet ps, uint32_t n_tiles, ContigTab tab,
                                                      const uint32_t *tile_contig, int *diff, int *sums,
                                                      uint8_t *hstate, uint64_t *ovf, uint32_t ovf_cap,
                                                      CheckWords *chk)
{
    __shared__ __attribute__((aligned(16))) int win[ST];
    __shared__ int s_sum;
    uint32_t tf[PD_MAXPEND], na[PD_MAXPEND];
    uint32_t n_beg[PD_MAXPEND], n_has[PD_MAXPEND], n_end[PD_MAXPEND];
    uint32_t t_lo = 0xFFFFFFFFu, t_hi = 0;
#pragma unroll
    for (int b = 0; b < PD_MAXPEND; ++b) {
        n_beg[b] = n_has[b] = n_end[b] = 0; tf[b] = 0; na[b] = 0;
        if (b < ps.nb) {
            tf[b] = ps.b[b].desc->t_first; na[b] = ps.b[b].desc->n_active;
            if (na[b]) { if (tf[b] < t_lo) t_lo = tf[b]; if (tf[b] + na[b] > t_hi) t_hi = tf[b] + na[b]; }
        }
    }
    if (t_hi > n_tiles) t_hi = n_tiles;
    const uint32_t lmax = ps.lmax;
    for (uint64_t t = (uint64_t)t_lo + blockIdx.x; t < t_hi; t += gridDim.x) {
        const uint64_t a = t * ST;
        int4 *w4 = reinterpret_cast<int4 *>(win);
        for (int j = threadIdx.x; j < ST / 4; j += WG) w4[j] = make_int4(0, 0, 0, 0);
        if (threadIdx.x == 0) s_sum = 0;
        // a scatter tile lies inside ONE contig slot, so only runs of that contig can land in it
        const int32_t ctg = (int32_t)tile_contig[a / TILE];
        const uint32_t clen = tab.len[ctg];
        const int64_t rel = (int64_t)(tab.off[ctg] - a);          // slot start relative to the tile (<= 0)
        const bool valid0 = hstate[a / PD_HALF] != 0;
        const bool valid1 = ST > PD_HALF ? hstate[a / PD_HALF + 1] != 0 : valid0;
        __syncthreads();
        int net = 0;
#pragma unroll
        for (int b = 0; b < PD_MAXPEND; ++b) {
            if (b >= ps.nb || t < tf[b] || t >= (uint64_t)tf[b] + na[b]) continue;
            // clamped: on a batch that was NOT sorted the index holds garbage, and the only
            // promise then is "reported, no out-of-bounds access"
            const uint32_t n = ps.b[b].n;
            uint32_t hi = ps.b[b].ub_a[t + 1]; if (hi > n) hi = n;
            uint32_t lo = ps.b[b].cand_lo[t]; if (lo > hi) lo = hi;
            const pd_iv *__restrict__ iv = ps.b[b].iv;
            // four candidates per thread in flight: the loop is bound by load latency, not by ALU
            constexpr int UN = 4;
            for (uint32_t i0 = lo + threadIdx.x; i0 < hi; i0 += UN * WG) {
                pd_iv vv[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const uint32_t i = i0 + u * WG;
                    vv[u] = iv[i < hi ? i : hi - 1];
                    if (i >= hi) vv[u].tid = -1;                  // never equals a contig id
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const pd_iv v = vv[u];
                    if (v.tid != ctg) continue;
                    uint32_t bb = v.beg < 0 ? 0u : (uint32_t)v.beg; if (bb > clen) bb = clen;
                    uint32_t x = v.end < 0 ? 0u : (uint32_t)v.end; if (x > clen) x = clen;
                    const bool has = bb < x;
                    const uint32_t len = has ? x - bb : 0u;
                    const uint64_t rb = (uint64_t)(rel + bb), re = (uint64_t)(rel + x);   // below-tile wraps high
                    if (rb < (uint64_t)ST) {
                        ++n_beg[b];
                        if (has) {
                            ++n_has[b];
                            atomicAdd(&win[rb], 1); ++net;
                            if (len > lmax) {
                                const uint32_t slot = atomicAdd(&chk->ovf_count, 1u);
                                if (slot < ovf_cap) { ovf[slot] = a + re; ++n_end[b]; } else atomicOr(&chk->err, 4u);
                            }
                        }
                    }
                    if (has && len <= lmax && re < (uint64_t)ST) { atomicAdd(&win[re], -1); --net; ++n_end[b]; }
                }
            }
        }
        net = wave_sum(net);
        if ((threadIdx.x & 63) == 0 && net != 0) atomicAdd(&s_sum, net);
        __syncthreads();
        int4 *o4 = reinterpret_cast<int4 *>(diff + a);
        constexpr int NG = ST / 4 / WG;                          // 16-byte groups per thread (4 or 8)
        int4 w[NG], o[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int j = threadIdx.x + g * WG;
            w[g] = w4[j];
            const bool valid = (ST > PD_HALF && j >= PD_HALF / 4) ? valid1 : valid0;
            // read-modify-write only what was written before AND changes now; issue all loads first
            if (valid && (w[g].x | w[g].y | w[g].z | w[g].w)) o[g] = o4[j]; else o[g] = make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int j = threadIdx.x + g * WG;
            const bool valid = (ST > PD_HALF && j >= PD_HALF / 4) ? valid1 : valid0;
            if (!valid || (w[g].x | w[g].y | w[g].z | w[g].w)) {
                o[g].x += w[g].x; o[g].y += w[g].y; o[g].z += w[g].z; o[g].w += w[g].w;
                o4[j] = o[g];                                    // first touch since reset: plain store of the window
            }
        }
        if (threadIdx.x == 0) {
            if (!valid0) hstate[a / PD_HALF] = 1;
            if (ST > PD_HALF && !valid1) hstate[a / PD_HALF + 1] = 1;
            if (s_sum != 0) {
                if (ST == TILE) sums[t] += s_sum;                // sole owner of this sum
                else atomicAdd(&sums[a / TILE], s_sum);          // two scatter tiles share one sum
            }
        }
        __syncthreads();
    }
    // every run must have found the owner of its begin, and every run with cells the owner of its
    // end (in a tile or on the overflow list); anything else means the batch broke its promise.
    // One atomic per workgroup and counter, spread over PD_CNT_SLOTS addresses.
    __shared__ unsigned s_cnt[PD_MAXPEND][3];
    if (threadIdx.x < PD_MAXPEND * 3) s_cnt[threadIdx.x / 3][threadIdx.x % 3] = 0;
    __syncthreads();
#pragma unroll
    for (int b = 0; b < PD_MAXPEND; ++b) {
        if (b >= ps.nb) continue;
        const int hb = wave_sum((int)n_beg[b]), hh = wave_sum((int)n_has[b]), he = wave_sum((int)n_end[b]);
        if ((threadIdx.x & 63) == 0) {
            if (hb) atomicAdd(&s_cnt[b][0], (unsigned)hb);
            if (hh) atomicAdd(&s_cnt[b][1], (unsigned)hh);
            if (he) atomicAdd(&s_cnt[b][2], (unsigned)he);
        }
    }
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
}

// ------------------------------------------------------------------------------------------
// compact samples (pd_runs_create / pd_push_runs, and what the GPU decoder leaves behind): see C8Sample in pd_kernels.h
// ------------------------------------------------------------------------------------------
// flat begin (clamped to the contig) and clamped length of a run; valid = its contig id is one
__device__ __forceinline__ uint64_t c8_flat(const pd_iv v, const ContigTab tab, uint32_t &len, bool &valid)
{
    valid = v.tid >= 0 && v.tid < tab.n;
    len = 0;
    if (!valid) return 0;
    const uint32_t clen = tab.len[v.tid];
    uint32_t b = v.beg < 0 ? 0u : (uint32_t)v.beg; if (b > clen) b = clen;
    uint32_t x = v.end < 0 ? 0u : (uint32_t)v.end; if (x > clen) x = clen;
    len = x > b ? x - b : 0u;
    return tab.off[v.tid] + b;             // (b <= clen < the slot's cells: always inside the contig's own slot, so below n_buckets << cshift)
}

// The sorted stream from 12-byte runs (pd_runs_create; the decoder's emit kernel, pd_bamwalk.h, does the same while it writes its runs):
// every run becomes 8 bytes — the low 32 bits of its flat begin, its clamped length, split over the two planes (C8Sample) —, its order is CHECKED against its predecessor
// (words[0]: a contig id out of range, or a run that begins before the one in front of it), runs longer than a bucket are counted
// (words[1]: such a sample is not used in this form), and the first run of every bucket leaves its index in b1[bucket] (pre-set to
// 0xFFFFFFFF; the buckets nobody begins in are filled by launch_c8_fill_starts).  The run's half-word goes to the narrow plane (C8Sample::nar) and the
// runs that half-word cannot hold (longer than 255 cells) are counted in words[3], one atomic per wave that has some.
__global__ __launch_bounds__(WG) void k_c8_from_sorted(const pd_iv *iv, uint32_t n, ContigTab tab, uint32_t bshift, uint32_t *lo, uint32_t *hi, uint16_t *nar, uint32_t *b1, uint32_t *words)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * WG + threadIdx.x;
    const uint32_t i = i64 < n ? (uint32_t)i64 : n - 1;
    const uint32_t cshift = 13u - bshift;                        // log2(cells per bucket)
    uint32_t len; bool valid;
    const uint64_t gb = c8_flat(iv[i], tab, len, valid);
    uint64_t prev = ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(gb >> 32), 1) << 32) | (uint32_t)__shfl_up((int)(uint32_t)gb, 1);
    bool pvalid = __shfl_up((int)valid, 1) != 0;
    if ((threadIdx.x & 63) == 0 && i > 0) { uint32_t pl; prev = c8_flat(iv[i - 1], tab, pl, pvalid); }
    const unsigned long long wide = __builtin_amdgcn_ballot_w64(i64 < n && pdcover::nar_is_wide(len));      // (before any lane leaves)
    if (wide != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&words[3], (uint32_t)__builtin_popcountll(wide));
    if (i64 >= n) return;
    if (!valid || (i > 0 && (!pvalid || gb < prev))) atomicOr(&words[0], 1u);
    if (len > (1u << cshift)) atomicAdd(&words[1], 1u);
    lo[i] = c8_lo((uint32_t)gb, len); hi[i] = c8_hi((uint32_t)gb, len);
    nar[i] = (uint16_t)pdcover::nar_pack((uint32_t)gb, len);
    if (valid && (i == 0 || !pvalid || (prev >> cshift) != (gb >> cshift))) atomicMin(&b1[gb >> cshift], i);
}

// The other streams (any order, but in practice the later runs of a file's reads in file order: nearly sorted).  Neighbouring lanes
// whose runs begin in the same bucket act ONCE: the first of them adds their number to the bucket's counter (a device atomic per
// run was 4.4 ms for the 1.1e8 later runs of the 1e9-record sample; per group of equal neighbours it is a tenth of that).
// group(key): the lane's group of equal neighbours as (first lane, size); every lane of the wave must call it
__device__ __forceinline__ void c8_group(const uint32_t key, int &head_lane, uint32_t &size)
{
    const int lane = threadIdx.x & 63;
    const uint32_t pk = (uint32_t)__shfl_up((int)key, 1);
    const unsigned long long heads = __ballot(lane == 0 || pk != key);
    const unsigned long long le = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    head_lane = 63 - __builtin_clzll(le);                         // (bit 0 is always set)
    // size of the group = distance from its first lane to the next group's first lane
    const unsigned long long above_h = head_lane == 63 ? 0ull : heads & ~((2ull << head_lane) - 1ull);
    size = (uint32_t)((above_h ? __builtin_ctzll(above_h) : 64) - head_lane);
}
__global__ __launch_bounds__(WG) void k_c8_hist(const pd_iv *iv, uint32_t n, ContigTab tab, uint32_t bshift, uint32_t *hist, uint32_t *words)
{
    const uint32_t cshift = 13u - bshift;
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * WG; base < n; base += (uint64_t)gridDim.x * WG) {      // (workgroup-uniform trip count)
        const uint64_t i = base + threadIdx.x;
        uint32_t key = 0xFFFFFFFFu;
        if (i < n) {
            uint32_t len; bool valid;
            const uint64_t gb = c8_flat(iv[i], tab, len, valid);
            if (!valid) atomicOr(&words[0], 1u);
            else { key = (uint32_t)(gb >> cshift); if (len > (1u << cshift)) atomicAdd(&words[1], 1u); }
        }
        int hl; uint32_t sz;
        c8_group(key, hl, sz);
        if (hl == lane && key != 0xFFFFFFFFu) atomicAdd(&hist[key], sz);
    }
}

// exclusive prefix sum of n 32-bit counts (three small kernels: sums of blocks of 1024, their scan, the blocks)
__global__ __launch_bounds__(WG) void k_scan_block_sums(const uint32_t *in, uint32_t n, uint32_t *bs)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = (uint64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (base + k < n) v += in[base + k];
    v = (uint32_t)wave_total((int)v);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) bs[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(1024) void k_scan_of_sums(uint32_t *bs, uint32_t nb)
{
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t run_s;
    if (threadIdx.x == 0) run_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? bs[i] : 0u;
        const uint32_t inc = (uint32_t)wave_incl_scan((int)v);
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t off = run_s;
        for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) off += wsum[k];
        if (i < nb) bs[i] = off + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) run_s = off + inc;
        __syncthreads();
    }
}
__global__ __launch_bounds__(WG) void k_scan_blocks(const uint32_t *in, uint32_t *out, uint32_t n, const uint32_t *bs)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = (uint64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    uint32_t x[4], v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = base + k < n ? in[base + k] : 0u; v += x[k]; }
    const uint32_t inc = (uint32_t)wave_incl_scan((int)v);
    if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t off = bs[blockIdx.x] + inc - v;
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) off += ws[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (base + k < n) out[base + k] = off; off += x[k]; }
}

// Bucket starts from the marks the first runs of the buckets left: a[k] = min(a[k], a[k + 1], ..., a[n - 1]) in place (a SUFFIX minimum;
// the caller has put the number of runs into a[n - 1]).  Same three-kernel shape as the prefix sum above, walked from the far end.
__device__ __forceinline__ uint32_t wave_suffix_min(uint32_t m)      // lane l: min over lanes l .. 63
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_down((int)m, d); if (lane + d < 64 && y < m) m = y; }
    return m;
}
__global__ __launch_bounds__(WG) void k_sfx_block_min(const uint32_t *a, uint32_t n, uint32_t *bm)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = (uint64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    uint32_t v = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (base + k < n && a[base + k] < v) v = a[base + k];
    v = wave_suffix_min(v);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t m = ws[0]; for (int k = 1; k < 4; ++k) if (ws[k] < m) m = ws[k]; bm[blockIdx.x] = m; }
}
// bm[j] := min(bm[j + 1 ..]) (what lies strictly behind block j), one workgroup
__global__ __launch_bounds__(1024) void k_sfx_of_mins(uint32_t *bm, uint32_t nb)
{
    __shared__ uint32_t wmin[16];
    __shared__ uint32_t run_s;
    if (threadIdx.x == 0) run_s = 0xFFFFFFFFu;
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t top = (nb + 1023u) / 1024u * 1024u; top > 0; top -= 1024) {
        const uint32_t i = top - 1024 + threadIdx.x;
        const uint32_t v = i < nb ? bm[i] : 0xFFFFFFFFu;
        const uint32_t inc = wave_suffix_min(v);                 // min over this wave's lanes lane .. 63
        if (lane == 0) wmin[wv] = inc;
        __syncthreads();
        uint32_t behind = run_s;                                  // later chunks
        for (int k = wv + 1; k < 16; ++k) if (wmin[k] < behind) behind = wmin[k];
        const uint32_t nxt = (uint32_t)__shfl_down((int)inc, 1);  // lanes lane + 1 .. 63 of this wave
        uint32_t ex = behind;
        if (lane < 63 && nxt < ex) ex = nxt;
        uint32_t all = behind; if (inc < all) all = inc;          // (thread 0: everything from this chunk on)
        __syncthreads();
        if (i < nb) bm[i] = ex;
        if (threadIdx.x == 0) run_s = all;
        __syncthreads();
    }
}
__global__ __launch_bounds__(WG) void k_sfx_blocks(uint32_t *a, uint32_t n, const uint32_t *bmx)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = (uint64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    uint32_t x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = base + k < n ? a[base + k] : 0xFFFFFFFFu;
#pragma unroll
    for (int k = 2; k >= 0; --k) if (x[k + 1] < x[k]) x[k] = x[k + 1];       // suffix minimum inside the thread's four
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t inc = wave_suffix_min(x[0]);
    if (lane == 0) ws[wv] = inc;
    __syncthreads();
    uint32_t behind = bmx[blockIdx.x];
    for (int k = wv + 1; k < 4; ++k) if (ws[k] < behind) behind = ws[k];
    const uint32_t nxt = (uint32_t)__shfl_down((int)inc, 1);
    if (lane < 63 && nxt < behind) behind = nxt;                   // what lies behind this thread's four
#pragma unroll
    for (int k = 0; k < 4; ++k) if (base + k < n) a[base + k] = x[k] < behind ? x[k] : behind;
}
__global__ void k_set_u32(uint32_t *p, uint32_t v) { *p = v; }

// the decoder's marks — per bucket the smallest (batch << 32 | index in the batch) of a run that begins there, all ones where none does —
// become indices into the sample's sorted stream: base[batch] + index (0xFFFFFFFF stays "nobody")
__global__ __launch_bounds__(WG) void k_c8_marks_to_index(const unsigned long long *marks, uint32_t n, const uint32_t *base, uint32_t *b1)
{
    const uint64_t k = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (k >= n) return;
    const unsigned long long m = marks[k];
    b1[k] = m == ~0ull ? 0xFFFFFFFFu : base[(uint32_t)(m >> 32)] + (uint32_t)m;
}

// the other streams' runs to their buckets: o1 = exclusive prefix sum of the histogram; the runs of a group of equal neighbours take
// consecutive places from ONE atomic on the bucket's cursor
__global__ __launch_bounds__(WG) void k_c8_place_other(const pd_iv *iv, uint32_t n, ContigTab tab, uint32_t bshift, const uint32_t *o1,
                                                       uint32_t *cursor, uint32_t *lo, uint32_t *hi)
{
    const uint32_t cshift = 13u - bshift;
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * WG; base < n; base += (uint64_t)gridDim.x * WG) {
        const uint64_t i = base + threadIdx.x;
        uint32_t key = 0xFFFFFFFFu, len = 0; uint64_t gb = 0;
        if (i < n) { bool valid; gb = c8_flat(iv[i], tab, len, valid); if (valid) key = (uint32_t)(gb >> cshift); }
        int hl; uint32_t sz;
        c8_group(key, hl, sz);
        uint32_t at = 0;
        if (hl == lane && key != 0xFFFFFFFFu) at = o1[key] + atomicAdd(&cursor[key], sz);
        at = (uint32_t)__shfl((int)at, hl);
        if (key != 0xFFFFFFFFu) { const uint32_t j = at + (uint32_t)(lane - hl); lo[j] = c8_lo((uint32_t)gb, len); hi[j] = c8_hi((uint32_t)gb, len); }
    }
}

// the reverse (a compact sample that has to take a path that reads 12-byte runs): bucket by bucket — a bucket's sorted-stream runs,
// then its other runs —, so the result is sorted up to one bucket's cells of disorder
__global__ __launch_bounds__(WG) void k_c8_expand(const C8Sample cs, const uint32_t *tile_contig, const uint64_t *contig_off, uint32_t n_tiles, pd_iv *out)
{
    const uint32_t cshift = 13u - cs.bshift, nbk = 1u << cs.bshift;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t k0 = t << cs.bshift;
        const int32_t ctg = (int32_t)tile_contig[t];
        const uint32_t a32 = (uint32_t)((uint64_t)t * TILE), c32 = (uint32_t)contig_off[ctg];
        for (uint32_t i = cs.b1[k0] + threadIdx.x; i < cs.b1[k0 + nbk]; i += WG) {
            const Run8 r = c8_join(cs.lo[i], cs.hi[i]);
            const uint32_t kb = k0 + ((r.b - a32) >> cshift), beg = r.b - c32;
            out[i + cs.o1[kb]] = pd_iv{ctg, (int32_t)beg, (int32_t)(beg + r.len)};
        }
        for (uint32_t j = cs.o1[k0] + threadIdx.x; j < cs.o1[k0 + nbk]; j += WG) {
            const Run8 r = c8_join(cs.lo[cs.o_base + j], cs.hi[cs.o_base + j]);
            const uint32_t kb = k0 + ((r.b - a32) >> cshift), beg = r.b - c32;
            out[j + cs.b1[kb + 1]] = pd_iv{ctg, (int32_t)beg, (int32_t)(beg + r.len)};
        }
    }
}

// A batch's runs on their way to their places (a few MB, twice per decode batch): the runtime's device-to-device copy is a blit kernel that
// took 0.15 ms per call among the decode kernels (13 % of the decode phase's kernel time, profiles/r05_decode_timeline.txt); this one moves
// 4-byte words with every lane on its own 16 bytes where source and destination allow it.
__device__ __forceinline__ void copy_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256, gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    // up to three words bring the destination to a 16-byte boundary (a plane of 4-byte runs starts anywhere); from there 16-byte stores, and
    // 16-byte loads where the source is on such a boundary too
    uint64_t head = ((0 - (uintptr_t)dst) >> 2) & 3; if (head > n) head = n;
    if (gid < head) dst[gid] = src[gid];
    dst += head; src += head; n -= head;
    const uint64_t n4 = n / 4;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    if (((uintptr_t)src & 15) == 0) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        for (uint64_t i = gid; i < n4; i += stride) d4[i] = s4[i];
    } else {
        for (uint64_t i = gid; i < n4; i += stride) d4[i] = make_uint4(src[4 * i], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]);
    }
    for (uint64_t i = n4 * 4 + gid; i < n; i += stride) dst[i] = src[i];
}
// The same copy for the LO words of a sorted stream: every word also leaves its half-word in nar (same index; C8Sample::nar) — from the register it
// is copied through, no second read — as one 8-byte store per four runs where the plane's place allows it; returns how many of this thread's words
// were runs the half-word cannot hold.  (The count sees the lo word's 16 bits of length only: a run of 65 536 cells or more keeps its upper bits in
// hi, but such a run is longer than a bucket, is counted in n_long by whoever emitted it, and the direct kernels — which read lengths from lo
// alone — never see that sample.)
__device__ __forceinline__ uint32_t copy_lo_words_nar(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t n, uint16_t *__restrict__ nar)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256, gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t wide = 0;
    auto half = [&](const uint32_t word) -> uint32_t { wide += pdcover::nar_is_wide(word >> 16) ? 1u : 0u; return pdcover::nar_of_lo(word); };
    uint64_t head = ((0 - (uintptr_t)dst) >> 2) & 3; if (head > n) head = n;
    if (gid < head) { const uint32_t v = src[gid]; dst[gid] = v; nar[gid] = (uint16_t)half(v); }
    dst += head; src += head; nar += head; n -= head;
    const uint64_t n4 = n / 4;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    const bool src16 = ((uintptr_t)src & 15) == 0, nar8 = ((uintptr_t)nar & 7) == 0;       // (kernel-uniform)
    for (uint64_t i = gid; i < n4; i += stride) {
        const uint4 v = src16 ? reinterpret_cast<const uint4 *>(src)[i] : make_uint4(src[4 * i], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]);
        d4[i] = v;
        const uint32_t h0 = half(v.x), h1 = half(v.y), h2 = half(v.z), h3 = half(v.w);
        if (nar8) reinterpret_cast<uint2 *>(nar)[i] = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
        else { nar[4 * i] = (uint16_t)h0; nar[4 * i + 1] = (uint16_t)h1; nar[4 * i + 2] = (uint16_t)h2; nar[4 * i + 3] = (uint16_t)h3; }
    }
    for (uint64_t i = n4 * 4 + gid; i < n; i += stride) { const uint32_t v = src[i]; dst[i] = v; nar[i] = (uint16_t)half(v); }
    return wide;
}
__global__ __launch_bounds__(256) void k_copy_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t n) { copy_words(dst, src, n); }
// the two planes of n compact runs (C8Sample) in one launch
__global__ __launch_bounds__(256) void k_copy_planes(uint32_t *__restrict__ dst_lo, uint32_t *__restrict__ dst_hi, const uint32_t *__restrict__ src_lo,
                                                     const uint32_t *__restrict__ src_hi, uint64_t n)
{
    copy_words(dst_lo, src_lo, n);
    copy_words(dst_hi, src_hi, n);
}
// ... of the SORTED stream on its way to the sample: the narrow plane is made from the lo words as they pass, and the runs longer than 255 cells
// are counted (*n_wide, one atomic per wave that met some)
__global__ __launch_bounds__(256) void k_copy_planes_nar(uint32_t *__restrict__ dst_lo, uint32_t *__restrict__ dst_hi, uint16_t *__restrict__ dst_nar,
                                                         const uint32_t *__restrict__ src_lo, const uint32_t *__restrict__ src_hi, uint64_t n, uint32_t *n_wide)
{
    const uint32_t wide = copy_lo_words_nar(dst_lo, src_lo, n, dst_nar);
    copy_words(dst_hi, src_hi, n);
    const unsigned long long some = __builtin_amdgcn_ballot_w64(wide != 0u);      // (every lane is here again)
    if (some != 0ull) {
        const uint32_t total = (uint32_t)wave_total((int)wide);
        if ((threadIdx.x & 63) == 0) atomicAdd(n_wide, total);
    }
}

// The per-tile descriptors of a finished compact sample (TileDesc in pd_kernels.h): one thread per tile reads the bucket starts around the
// tile in both streams and the tile's contig, so that k_direct_c8 finds them in one record instead of a chain of dependent loads.
__global__ __launch_bounds__(WG) void k_c8_tile_desc(const C8Sample cs, const ContigTab tab, const uint32_t *tile_contig, uint32_t n_tiles, TileDesc *desc, uint32_t *n_heavy,
                                                     uint32_t *heavy_tiles)
{
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= n_tiles) return;
    const uint32_t k0 = t << cs.bshift, nbk = 1u << cs.bshift;
    const uint32_t ctg = tile_contig[t];
    TileDesc d;
    d.pc = (uint32_t)((uint64_t)t * TILE - tab.off[ctg]);         // the tile's first cell inside its contig
    d.clen = tab.len[ctg];
    const uint32_t lo = d.pc ? k0 - 1 : k0;                       // a contig's first tile has nothing before it
    d.slo = cs.b1[lo]; d.shi = cs.b1[k0 + nbk];
    d.olo = cs.o1[lo]; d.ohi = cs.o1[k0 + nbk];
    d.spare0 = d.spare1 = 0;
    desc[t] = d;
    // a pile-up tile: k_direct_c8 will count the same candidates from this record and leave the tile to the int-window pass, whose list this is
    // (at most one entry per tile: the slot is below n_tiles, the list's room)
    if ((d.shi - d.slo) + (d.ohi - d.olo) > PD_C8_HEAVY_CAND) heavy_tiles[atomicAdd(n_heavy, 1u)] = t;
}

// a sorted stream of compact runs whose sample turned out not to be usable as one (the file's order does not hold after all): back to
// 12-byte runs; the contig of a flat begin by bisection over the slots (genomes below 2^32 cells only: the caller has made sure)
__global__ __launch_bounds__(WG) void k_r8_to_iv(const uint32_t *lo, const uint32_t *hi, uint64_t n, ContigTab tab, pd_iv *out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * WG) {
        const Run8 r = c8_join(lo[i], hi[i]);
        int a = 0, z = tab.n - 1;                               // last contig whose slot starts at or before r.b
        while (a < z) { const int mid = (a + z + 1) >> 1; if (tab.off[mid] <= (uint64_t)r.b) a = mid; else z = mid - 1; }
        const uint32_t beg = r.b - (uint32_t)tab.off[a];
        out[i] = pd_iv{a, (int32_t)beg, (int32_t)(beg + r.len)};
    }
}

// Zero-fills every half-tile that has not been written since the last reset (and marks it), so
// that the atomic kernels may add into any cell.  With only_if_overflow it returns at once unless
// the tile pass just put something on the overflow list.
__global__ __launch_bounds__(WG) void k_fill_invalid(int4 *buf, uint8_t *hstate, uint32_t n_half,
                                                     const CheckWords *chk, int only_if_overflow)
{
    if (chk->all_valid) return;
    if (only_if_overflow && chk->ovf_count == 0) return;
    const int4 z = make_int4(0, 0, 0, 0);
    for (uint32_t h = blockIdx.x; h < n_half; h += gridDim.x) {
        const bool written = hstate[h] != 0;
        __syncthreads();                 // every wave has read the flag before thread 0 may set it
        if (written) continue;                                   // uniform per workgroup
        int4 *p = buf + (size_t)h * (PD_HALF / 4);
        for (int j = threadIdx.x; j < PD_HALF / 4; j += WG) p[j] = z;
        if (threadIdx.x == 0) hstate[h] = 1;
    }
}

__global__ __launch_bounds__(WG) void k_apply_overflow(const uint64_t *ovf, CheckWords *chk, uint32_t ovf_cap,
                                                       int *diff, int *sums, int mark_valid)
{
    uint32_t n = chk->ovf_count; if (n > ovf_cap) n = ovf_cap;
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
        const uint64_t ge = ovf[i];
        atomicAdd(&diff[ge], -1);
        atomicAdd(&sums[ge / TILE], -1);
    }
    // the fill that preceded this kernel ran iff the list is not empty (or unconditionally)
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n > 0 || mark_valid)) chk->all_valid = 1;
}

__global__ void k_mark_all_valid(CheckWords *chk) { chk->all_valid = 1; }

// Folds one batch's outcome into the context-wide check words and re-arms the descriptor.
__global__ void k_finish_batch(const PendSet ps, CheckWords *chk)
{
    for (int b = 0; b < ps.nb; ++b) {
        BatchDesc *desc = ps.b[b].desc;
        uint64_t handled = 0, has = 0, ends = 0;
        for (int k = 0; k < PD_CNT_SLOTS; ++k) {
            handled += desc->handled[k]; has += desc->has[k]; ends += desc->ends[k];
            desc->handled[k] = 0; desc->has[k] = 0; desc->ends[k] = 0;
        }
        if (handled != (uint64_t)ps.b[b].n || has != ends) chk->unsorted_batches += 1;
        if (desc->err) chk->err |= desc->err;
        desc->ovf_count = 0; desc->err = 0; desc->t_first = 0; desc->n_active = 0;
    }
    chk->ovf_count = 0;
}

// ------------------------------------------------------------------------------------------
// tile carries: exclusive prefix sum of the tile sums (a few hundred thousand ints), one
// workgroup of 1024 threads, chunked.
// ------------------------------------------------------------------------------------------
// Two small kernels: (1) one workgroup per 1024 tile sums reduces them to a block sum; (2) every
// workgroup re-derives its block's offset from the <= few hundred block sums and scans its block.
__global__ __launch_bounds__(1024) void k_carry_block_sums(const int *sums, int *bsum, uint32_t n_tiles)
{
    __shared__ int wsum[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x;
    int v = i < n_tiles ? sums[i] : 0;
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int k = 0; k < 16; ++k) t += wsum[k]; bsum[blockIdx.x] = t; }
}

__global__ __launch_bounds__(1024) void k_tile_carry(const int *sums, const int *bsum, int *carry, uint32_t n_tiles)
{
    __shared__ int wsum[16];
    __shared__ int s_base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // offset of this block = sum of the block sums before it
    int part = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += 1024) part += bsum[k];
    part = wave_sum(part);
    if (lane == 0) wsum[wv] = part;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int k = 0; k < 16; ++k) t += wsum[k]; s_base = t; }
    __syncthreads();
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x;
    const int v = i < n_tiles ? sums[i] : 0;
    const int x = wave_incl_scan(v);
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int pre = s_base;
    for (int k = 0; k < wv; ++k) pre += wsum[k];
    if (i < n_tiles) carry[i] = pre + x - v;
}

// ------------------------------------------------------------------------------------------
// the sweep.  One workgroup per tile; 4 waves x 8 rows x (64 lanes x int4): every load/store is
// a full 1 KiB wave transaction.  Per row: in-lane scan of 4, wave scan of the 64 lane totals
// (all 8 rows' shuffle chains are independent -> ILP), running carry across rows, then the
// wave bases through LDS, plus the tile carry-in.
//   MODE_WRITE : depth written back in place (8 B/base)
//   MODE_WIN   : fused fixed-window reduction, nothing written back (4 B/base)
//   FROM_DEPTH : input already holds depth (reduction only)
// ------------------------------------------------------------------------------------------

// Load one tile (8 rows of int4 per wave) and, unless FROM_DEPTH, turn its difference array into wrapped depth in registers:
// the scan shared by k_sweep and k_sweep_hist.  `p4` points at this lane's first int4 of the tile, `t` is the tile's global
// index (hstate / carry), `wtot` four ints of LDS.  Contains one __syncthreads (not FROM_DEPTH): every thread must call it.
template <bool FROM_DEPTH>
__device__ __forceinline__ void sweep_tile_load_scan(int4 (&v)[TILE / (WG * 4)], const int4 *p4, uint64_t t, const int *carry,
                                                     uint32_t wrap_mask, const uint8_t *hstate, int *wtot, int lane, int wv)
{
    constexpr int ROWS = TILE / (WG * 4);                        // 8
    // a half-tile nobody has written since the reset holds stale bytes and counts as zeros; waves
    // 0-1 cover the first 4096 cells of the tile, waves 2-3 the second (wave-uniform branch)
    const bool live = FROM_DEPTH || hstate[t * (TILE / PD_HALF) + (wv >> 1)] != 0;
    if (live) {
        // every cell is read once (and, written back, written once): non-temporal, so that the lines do not wait in L2 for a reuse that never comes
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const v4i_nt x = __builtin_nontemporal_load(reinterpret_cast<const v4i_nt *>(p4 + r * 64));
            v[r] = make_int4(x.x, x.y, x.z, x.w);
        }
    } else {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) v[r] = make_int4(0, 0, 0, 0);
    }

    if (!FROM_DEPTH) {
        int tot[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            v[r].y += v[r].x; v[r].z += v[r].y; v[r].w += v[r].z;
            tot[r] = v[r].w;
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) tot[r] = wave_incl_scan(tot[r]);
        int run = 0;                                             // carry across this wave's rows
        int excl[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            excl[r] = run + tot[r] - v[r].w;
            run += __builtin_amdgcn_readlane(tot[r], 63);
        }
        if (lane == 0) wtot[wv] = run;
        __syncthreads();
        int base = carry[t];
        for (int k = 0; k < wv; ++k) base += wtot[k];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int b = base + excl[r];
            v[r].x = (int)((uint32_t)(v[r].x + b) & wrap_mask);
            v[r].y = (int)((uint32_t)(v[r].y + b) & wrap_mask);
            v[r].z = (int)((uint32_t)(v[r].z + b) & wrap_mask);
            v[r].w = (int)((uint32_t)(v[r].w + b) & wrap_mask);
        }
    }
}

template <bool WRITE, bool WIN, bool FROM_DEPTH>
__global__ __launch_bounds__(WG) void k_sweep(int *buf, const int *carry, uint32_t wrap_mask,
                                              const TileMap tmap, WinArgs wa, const uint8_t *hstate, uint32_t tile0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int wtot[4];
    constexpr int ROWS = TILE / (WG * 4);                        // 8
    // tile0: the sweep of a slice (a rank's share of the summed depth in the sharded list mode): `buf` holds tiles tile0, tile0 + 1, ...
    const uint64_t t = (uint64_t)blockIdx.x + tile0;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int4 *p4 = reinterpret_cast<int4 *>(buf + (uint64_t)blockIdx.x * TILE) + wv * (ROWS * 64) + lane;
    int4 v[ROWS];
    sweep_tile_load_scan<FROM_DEPTH>(v, p4, t, carry, wrap_mask, hstate, wtot, lane, wv);
    if (WRITE) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            v4i_nt x; x.x = v[r].x; x.y = v[r].y; x.z = v[r].z; x.w = v[r].w;
            __builtin_nontemporal_store(x, reinterpret_cast<v4i_nt *>(p4 + r * 64));
        }
    }
    if (WIN) {
        // contig-local position of this tile's first cell and the contig's length
        const uint32_t ctg = tmap.tile_contig[t];
        const uint64_t local0 = t * TILE - tmap.contig_off[ctg];
        const uint32_t clen = tmap.contig_len[ctg];
        const uint32_t w = wa.w;
        if (w >= (uint32_t)TILE) {
            // Large windows (the 10 Mb bins of whole-chromosome mode): a tile touches at most two
            // windows, k0 and k0+1.  Write the tile's two partial (cover, sum) pairs with plain
            // stores; k_window_gather adds them up per window.  No atomics: with ~1200 tiles per
            // window, same-address device atomics would serialise the whole sweep.
            __shared__ unsigned long long red_s[4][2];
            __shared__ int red_c[4][2];
            int c0 = 0, c1 = 0; unsigned long long s0 = 0, s1 = 0;
            if (local0 < clen) {
                const uint64_t k0 = local0 / w;
                const uint64_t nb = (k0 + 1) * (uint64_t)w - local0;     // tile-local start of window k0+1
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const uint32_t pos = (uint32_t)(wv * (ROWS * 256) + r * 256 + lane * 4);
                    const uint32_t d[4] = {(uint32_t)v[r].x, (uint32_t)v[r].y, (uint32_t)v[r].z, (uint32_t)v[r].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool ok = local0 + pos + q < clen && d[q] >= wa.min_dep;
                        if (ok) { if (pos + q < nb) { ++c0; s0 += d[q]; } else { ++c1; s1 += d[q]; } }
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
                wa.part[t] = tp;
            }
            return;
        }
        if (local0 >= clen) return;                              // pure padding tile (uniform)
        const uint64_t wbase = tmap.win_off[ctg];
        const uint64_t k0 = local0 / w;                          // first window touching the tile
        // general case: LDS accumulators for the windows overlapping this tile
        // one 64-bit accumulator per window: cover (<= 8192, 16 bits) in the top, depth sum
        // (<= 8192 * 2^32 = 2^45) in the low 48 bits -> a single ds_add_u64 per lane segment
        const uint32_t nacc = (uint32_t)((local0 + TILE - 1) / w - k0 + 1);
        unsigned long long *acc = reinterpret_cast<unsigned long long *>(smem);
        for (uint32_t j = threadIdx.x; j < nacc; j += WG) acc[j] = 0;
        __syncthreads();
        const uint32_t phase = (uint32_t)(local0 - k0 * w);      // offset of the tile inside window k0
        const uint32_t magic = w >= 2u ? narrow_magic(w) : 0u;
        const uint32_t left = (uint64_t)clen - local0 < (uint64_t)TILE ? (uint32_t)(clen - local0) : (uint32_t)TILE;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint32_t pos = (uint32_t)(wv * (ROWS * 256) + r * 256 + lane * 4);
            const uint32_t d[4] = {(uint32_t)v[r].x, (uint32_t)v[r].y, (uint32_t)v[r].z, (uint32_t)v[r].w};
            if (w >= 4u) { narrow_window_row(d, pos, phase, w, magic, wa.min_dep, left, acc, lane); continue; }
            // windows of 1-3 cells: several begin inside a lane's four cells; one atomic per window piece
            const uint32_t x = pos + phase;
            uint32_t q = (uint32_t)((float)x * wa.inv_w);
            if ((uint64_t)q * w > x) --q;
            if ((uint64_t)(q + 1) * w <= x) ++q;
            uint64_t nb = (uint64_t)(q + 1) * w - phase;         // tile-local cell where window q+1 starts
            uint32_t c = 0; unsigned long long s = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t pe = pos + e;
                if (pe == nb) {
                    if (c) atomicAdd(&acc[q], ((unsigned long long)c << 48) | s);
                    c = 0; s = 0; ++q; nb += w;
                }
                if (local0 + pe < clen && d[e] >= wa.min_dep) { ++c; s += d[e]; }
            }
            if (c) atomicAdd(&acc[q], ((unsigned long long)c << 48) | s);
        }
        __syncthreads();
        narrow_write_out(acc, nacc, k0, w, local0, clen, wbase, wa, wa.part + t);
    }
}

// w < TILE: the windows that lie across a tile boundary = the last share of the tile before it + the first share of the tile behind it
__global__ __launch_bounds__(WG) void k_window_edges(const TilePart *part, const TileMap tmap, uint32_t n_tiles, uint32_t w, uint32_t *cover,
                                                     unsigned long long *sum)
{
    const uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (t + 1 >= n_tiles) return;
    const uint32_t ctg = tmap.tile_contig[t];
    const uint64_t local0 = t * TILE - tmap.contig_off[ctg];
    const uint64_t clen = tmap.contig_len[ctg];
    if (local0 + TILE >= clen) return;                           // the contig's last tile (or padding): nothing goes on behind it
    const uint64_t k = (local0 + TILE - 1) / w;                  // the window of the tile's last cell
    if ((k + 1) * (uint64_t)w <= local0 + TILE) return;          // ends with the tile
    const TilePart a = part[t], b = part[t + 1];
    const uint32_t c = a.c1 + b.c0;
    if (!c) return;
    cover[tmap.win_off[ctg] + k] = c;
    sum[tmap.win_off[ctg] + k] = a.s1 + b.s0;
}

// w >= TILE: the partials of the tiles a window spans, added up with plain loads and stores.  WAVES = 1: a wave per window, four windows per
// workgroup (windows of up to a few hundred tiles: with w = 8192 there are as many windows as tiles); WAVES = 4: a workgroup per window and a
// cross-wave add (the 10 Mb bins' ~1 220 tiles: 792 waves left most of the device idle).  A lane keeps GU TilePart loads in flight: indices
// past the window's last tile are clamped to it and count nothing.  A tile's share of THIS window is its first pair when the tile begins at or
// behind the window's first cell k * w, its second pair when it begins before it — only the window's first tile can.
template <int WAVES>
__global__ __launch_bounds__(WG) void k_window_gather(const TilePart *__restrict__ part, const TileMap tmap, int32_t n_contigs,
                                                      uint32_t w, uint64_t n_windows, uint32_t *cover,
                                                      unsigned long long *sum, const GatherCall gc)
{
    static_assert(WAVES == 1 || WAVES == 4, "a wave or the workgroup per window");
    if (blockIdx.x == 0 && threadIdx.x == 0) {                   // (GatherCall in pd_kernels.h; the pointers are workgroup-uniform)
        if (gc.next_words) for (int i = 0; i < PD_STATUS_WORDS; ++i) gc.next_words[i] = 0u;
        if (gc.pin_words) for (int i = 0; i < PD_STATUS_READ; ++i) gc.pin_words[i] = gc.words[i];
    }
    constexpr int GU = 5;                                         // (256 lanes x 5 take a 10 Mb bin's 1 222 tiles in one trip, 64 x 5 any window of the wave form)
    constexpr uint32_t NL = WAVES * 64;                          // lanes per window
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t g = WAVES == 1 ? (uint64_t)blockIdx.x * 4 + wv : (uint64_t)blockIdx.x;
    if (g >= n_windows) return;                                  // (wave-uniform; WAVES = 4: workgroup-uniform)
    int lo = 0, hi = n_contigs;                                  // the last contig c with win_off[c] <= g: 64 probes a round (two dependent loads for 4 096 contigs, not twelve)
    while (hi - lo > 1) {
        const int step = (hi - lo + 63) >> 6, probe = lo + lane * step;
        const int le = __builtin_popcountll(__builtin_amdgcn_ballot_w64(probe < hi && tmap.win_off[probe] <= g));     // >= 1: lane 0 probes lo
        lo += (le - 1) * step;
        hi = hi < lo + step ? hi : lo + step;
    }
    const uint64_t k = g - tmap.win_off[lo];
    const uint64_t coff = tmap.contig_off[lo];
    const uint64_t clen = tmap.contig_len[lo];
    const uint64_t b = k * w;
    uint64_t e = b + w; if (e > clen) e = clen;
    const uint64_t t0 = (coff + b) / TILE, t1 = (coff + e - 1) / TILE;
    const uint64_t tb = (coff + b + TILE - 1) / TILE;             // the first tile that begins inside the window: t0 or t0 + 1
    uint32_t c = 0; unsigned long long s = 0;
    for (uint64_t base = t0 + (WAVES == 1 ? (uint32_t)lane : threadIdx.x); base <= t1; base += (uint64_t)NL * GU) {
        TilePart tp[GU];
#pragma unroll
        for (int u = 0; u < GU; ++u) { const uint64_t t = base + (uint64_t)u * NL; tp[u] = part[t <= t1 ? t : t1]; }
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const uint64_t t = base + (uint64_t)u * NL;
            const bool second = t < tb;
            const uint32_t ci = second ? tp[u].c1 : tp[u].c0;
            const unsigned long long si = second ? tp[u].s1 : tp[u].s0;
            if (t <= t1) { c += ci; s += si; }
        }
    }
    c = (uint32_t)wave_sum((int)c);
#pragma unroll
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if (WAVES == 1) {
        if (lane == 0) {
            cover[g] = c; sum[g] = s;
            if (gc.pin_cover) { gc.pin_cover[g] = c; gc.pin_sum[g] = s; }
        }
        return;
    }
    __shared__ uint32_t red_c[4];
    __shared__ unsigned long long red_s[4];
    if (lane == 0) { red_c[wv] = c; red_s[wv] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        c = red_c[0] + red_c[1] + red_c[2] + red_c[3]; s = red_s[0] + red_s[1] + red_s[2] + red_s[3];
        cover[g] = c; sum[g] = s;
        if (gc.pin_cover) { gc.pin_cover[g] = c; gc.pin_sum[g] = s; }
    }
}

// ------------------------------------------------------------------------------------------
// segmented interval reduction over the depth array: one wave per piece (a region, or a
// <= 16384-cell slice of a long region); partial results are added into the region's slot.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_reduce_pieces(const int *depth, const Piece *pieces, uint32_t n_pieces,
                                                      uint32_t min_dep, int *cover, unsigned long long *sum)
{
    const uint32_t pi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pi >= n_pieces) return;
    const int lane = threadIdx.x & 63;
    const Piece pc = pieces[pi];
    const uint32_t *d = reinterpret_cast<const uint32_t *>(depth) + pc.start;
    int c = 0; unsigned long long s = 0;
    for (uint32_t i = lane; i < pc.count; i += 64) {
        const uint32_t x = d[i];
        if (x >= min_dep) { ++c; s += x; }
    }
    c = wave_sum(c);
#pragma unroll
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0 && c) { atomicAdd(&cover[pc.region], c); atomicAdd(&sum[pc.region], s); }
}

// ------------------------------------------------------------------------------------------
// depth histograms (pd_scan_depth_histogram / pd_depth_histogram).  Counts go into LDS, one copy of
// the n_bins 32-bit counters per wave (COPIES = 4) or one for the workgroup (COPIES = 1); a
// workgroup covers a RUN of tiles (or pieces) and adds its non-zero bins into the contig's uint64
// row with 64-bit integer device atomics only when the contig changes and at the end (exact, the
// same bits every run).  Depth clusters: at 50x a row's 256 cells fall into a few dozen bins, so
// a lane folds equal neighbours of its four cells into one add (FOLD), and a row whose 256 cells
// share one bin (empty stretches, piles above the last bin) is one add by lane 0.
// ------------------------------------------------------------------------------------------
struct HistArgs { uint32_t n_bins, nbp; unsigned long long *hist; };   // nbp: counters per LDS copy (hist_lane4 and lds_drain: pd_dev.h)

// the workgroup's counters of one contig into its row of the histogram, zeroed behind (between two __syncthreads)
template <int COPIES>
__device__ __forceinline__ void hist_flush(uint32_t *hs, const HistArgs &ha, uint32_t ctg)
{
    unsigned long long *row = ha.hist + (uint64_t)ctg * ha.n_bins;
    for (uint32_t j = threadIdx.x; j < ha.n_bins; j += WG) {
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < COPIES; ++k) { s += hs[k * ha.nbp + j]; hs[k * ha.nbp + j] = 0; }
        if (s) atomicAdd(&row[j], (unsigned long long)s);
    }
}

// The fused histogram sweep: k_sweep's load + scan (sweep_tile_load_scan: hstate skip, carry, wrap mask), then every cell of
// [local0, clen) into the bins; no depth is written.  Workgroup g covers tiles [g * tpw, (g + 1) * tpw).  FROM_DEPTH: the
// buffer already holds depth (pd_depth_histogram over whole contigs).
template <bool FROM_DEPTH, int COPIES, bool FOLD>
__global__ __launch_bounds__(WG) void k_sweep_hist(const int *buf, const int *carry, uint32_t wrap_mask, const TileMap tmap,
                                                   const uint8_t *hstate, uint32_t n_tiles, uint32_t tpw, HistArgs ha)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int wtot[2][4];                                   // alternate per tile: a wave one tile ahead never writes what another still reads
    constexpr int ROWS = TILE / (WG * 4);
    uint32_t *hs = reinterpret_cast<uint32_t *>(smem);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *h = hs + (wv % COPIES) * ha.nbp;
    for (uint32_t j = threadIdx.x; j < COPIES * ha.nbp; j += WG) hs[j] = 0;
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * tpw;
    const uint64_t t1 = t0 + tpw < n_tiles ? t0 + tpw : n_tiles;
    if (t0 >= t1) return;
    const uint32_t nb1 = ha.n_bins - 1;
    uint32_t cur = tmap.tile_contig[t0];
    for (uint64_t t = t0; t < t1; ++t) {
        const uint32_t ctg = tmap.tile_contig[t];
        if (ctg != cur) { lds_drain(); __syncthreads(); hist_flush<COPIES>(hs, ha, cur); __syncthreads(); cur = ctg; }
        const uint64_t local0 = t * TILE - tmap.contig_off[ctg];
        const uint32_t clen = tmap.contig_len[ctg];
        if (local0 >= clen) continue;                            // pure padding tile (uniform)
        const int4 *p4 = reinterpret_cast<const int4 *>(buf + t * TILE) + wv * (ROWS * 64) + lane;
        int4 v[ROWS];
        sweep_tile_load_scan<FROM_DEPTH>(v, p4, t, carry, wrap_mask, hstate, wtot[(t - t0) & 1], lane, wv);
        const uint64_t rest = (uint64_t)clen - local0;
        const uint32_t left = rest < (uint64_t)TILE ? (uint32_t)rest : (uint32_t)TILE;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint32_t pos = (uint32_t)(wv * (ROWS * 256) + r * 256 + lane * 4);
            const uint32_t n = pos >= left ? 0u : (left - pos < 4u ? left - pos : 4u);
            const uint32_t b[4] = {min((uint32_t)v[r].x, nb1), min((uint32_t)v[r].y, nb1), min((uint32_t)v[r].z, nb1), min((uint32_t)v[r].w, nb1)};
            hist_lane4<FOLD>(h, b, n, lane);
        }
    }
    lds_drain();
    __syncthreads();
    hist_flush<COPIES>(hs, ha, cur);
}

// Regions over the materialised depth: bounded pieces (Piece.region = the contig id), sorted by contig; workgroup g covers
// pieces [g * ppw, (g + 1) * ppw), 1024 cells per step (four consecutive cells per lane).
template <int COPIES, bool FOLD>
__global__ __launch_bounds__(WG) void k_hist_pieces(const uint32_t *depth, const Piece *pieces, uint32_t n_pieces, uint32_t ppw, HistArgs ha)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *hs = reinterpret_cast<uint32_t *>(smem);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *h = hs + (wv % COPIES) * ha.nbp;
    for (uint32_t j = threadIdx.x; j < COPIES * ha.nbp; j += WG) hs[j] = 0;
    __syncthreads();
    const uint64_t p0 = (uint64_t)blockIdx.x * ppw;
    const uint64_t p1 = p0 + ppw < n_pieces ? p0 + ppw : n_pieces;
    if (p0 >= p1) return;
    const uint32_t nb1 = ha.n_bins - 1;
    uint32_t cur = pieces[p0].region;
    for (uint64_t i = p0; i < p1; ++i) {
        const Piece pc = pieces[i];
        if (pc.region != cur) { lds_drain(); __syncthreads(); hist_flush<COPIES>(hs, ha, cur); __syncthreads(); cur = pc.region; }
        const uint32_t *d = depth + pc.start;
        for (uint32_t base = 0; base < pc.count; base += WG * 4) {
            const uint32_t c0 = base + threadIdx.x * 4;
            const uint32_t n = c0 >= pc.count ? 0u : (pc.count - c0 < 4u ? pc.count - c0 : 4u);
            uint32_t b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = (uint32_t)q < n ? min(d[c0 + q], nb1) : 0u;
            hist_lane4<FOLD>(h, b, n, lane);
        }
    }
    lds_drain();
    __syncthreads();
    hist_flush<COPIES>(hs, ha, cur);
}

// ------------------------------------------------------------------------------------------
// int8 transport of the difference arrays for the multi-sample sum (xGMI is the bottleneck there:
// 4x fewer bytes on the links).  Cells with |d| <= thr travel as int8 (thr = 127 / world, so the
// sum over all ranks cannot overflow); the rare others (pile-ups) travel as (cell, value)
// exceptions and are zero in the image.  Bytes are stored BIASED (d + thr, an unsigned value in
// [0, 2 thr]): the sum over the ranks stays below 256 in every byte, so the collective can add the
// image as int32 words (four cells per element, no carry between bytes) at full int32 reduce
// speed; the importer subtracts n_ranks * thr.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_export_i8(const int *diff, const uint8_t *hstate, int4 *out, uint64_t n_cells,
                                                  int thr, pd_exc *exc, uint32_t cap, uint32_t *count)
{
    const uint64_t n16 = n_cells / 16;
    for (uint64_t i = blockIdx.x * (uint64_t)WG + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * WG) {
        const uint64_t c0 = i * 16;
        const unsigned zb = (unsigned)thr * 0x01010101u;          // four cells of value 0
        int4 o = make_int4((int)zb, (int)zb, (int)zb, (int)zb);
        if (hstate[c0 / PD_HALF]) {                              // never-written half-tiles are zeros
            const int4 *p = reinterpret_cast<const int4 *>(diff + c0);
            int v[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int4 q = p[k]; v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w; }
            unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                int x = v[k];
                if (x > thr || x < -thr) {
                    const uint32_t slot = atomicAdd(count, 1u);
                    if (slot < cap) { exc[slot].cell = c0 + k; exc[slot].value = x; exc[slot].pad = 0; }
                    x = 0;
                }
                w[k >> 2] |= (unsigned)((x + thr) & 0xff) << (8 * (k & 3));
            }
            o = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
        }
        out[i] = o;
    }
}

__global__ __launch_bounds__(WG) void k_import_i8(const int4 *in, int *diff, uint64_t n_cells, int bias)
{
    const uint64_t n16 = n_cells / 16;
    for (uint64_t i = blockIdx.x * (uint64_t)WG + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * WG) {
        const int4 q = in[i];
        const unsigned w[4] = {(unsigned)q.x, (unsigned)q.y, (unsigned)q.z, (unsigned)q.w};
        int4 *p = reinterpret_cast<int4 *>(diff + i * 16);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            p[k] = make_int4((int)(w[k] & 0xff) - bias, (int)((w[k] >> 8) & 0xff) - bias,
                             (int)((w[k] >> 16) & 0xff) - bias, (int)(w[k] >> 24) - bias);
    }
}

__global__ __launch_bounds__(WG) void k_apply_exceptions(const pd_exc *exc, uint64_t n, int *diff, uint64_t n_cells)
{
    for (uint64_t i = blockIdx.x * (uint64_t)WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * WG)
        if (exc[i].cell < n_cells) atomicAdd(&diff[exc[i].cell], exc[i].value);
}

// ------------------------------------------------------------------------------------------
// 4-bit transport for the SLICED sum: the images are exchanged pairwise (all-to-all) and added on
// the receiving GPU in int32, so a nibble (d + 8) per cell is enough whatever the number of ranks.
// ------------------------------------------------------------------------------------------
// one workgroup per tile and step; every load is a full 1 KiB wave transaction (lane-contiguous
// int4), every store 128 contiguous bytes (one ushort = 4 cells per lane)
__global__ __launch_bounds__(WG) void k_export_i4(const int *diff, const uint8_t *hstate, unsigned short *out,
                                                       uint32_t n_tiles, pd_exc *exc, uint32_t cap, uint32_t *count)
{
    constexpr int ROWS = TILE / (WG * 4);                        // 8
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t cw = (uint64_t)t * TILE + (uint64_t)wv * (ROWS * 256);       // first cell of this wave
        unsigned short *o = out + cw / 4 + lane;
        if (!hstate[(uint64_t)t * (TILE / PD_HALF) + (wv >> 1)]) {                   // wave-uniform
#pragma unroll
            for (int r = 0; r < ROWS; ++r) o[r * 64] = 0x8888;
            continue;
        }
        const int4 *p4 = reinterpret_cast<const int4 *>(diff + cw) + lane;
        int4 v[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) v[r] = p4[r * 64];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            int x[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
            unsigned w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (x[k] > 7 || x[k] < -8) {
                    const uint32_t slot = atomicAdd(count, 1u);
                    if (slot < cap) { exc[slot].cell = cw + r * 256 + lane * 4 + k; exc[slot].value = x[k]; exc[slot].pad = 0; }
                    x[k] = 0;
                }
                w |= (unsigned)((x[k] + 8) & 0xf) << (4 * k);
            }
            o[r * 64] = (unsigned short)w;
        }
    }
}

// dst += (nibble - 8) for the tiles [0, n_tiles) of a chunk: the single-process form of the sum
// (pd_accumulate_from).  Same row layout as k_export_i4: lane-contiguous int4 RMW of the cells, one
// ushort (4 cells) of the image per lane and row.
__global__ __launch_bounds__(WG) void k_add_i4(int *dst, const unsigned short *img, uint32_t n_tiles)
{
    constexpr int ROWS = TILE / (WG * 4);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t cw = (uint64_t)t * TILE + (uint64_t)wv * (ROWS * 256);
        const unsigned short *q = img + cw / 4 + lane;
        int4 *p4 = reinterpret_cast<int4 *>(dst + cw) + lane;
        unsigned short h[ROWS];
        int4 v[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) { h[r] = q[r * 64]; v[r] = p4[r * 64]; }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const unsigned w = h[r];
            v[r].x += (int)(w & 0xf) - 8; v[r].y += (int)((w >> 4) & 0xf) - 8;
            v[r].z += (int)((w >> 8) & 0xf) - 8; v[r].w += (int)(w >> 12) - 8;
            p4[r * 64] = v[r];
        }
    }
}

// marks the tiles of the slice [tile0, tile0 + n_tiles) that own an exception of any part (blockIdx.y)
__global__ __launch_bounds__(WG) void k_flag_exception_tiles(const pd_exc *exc, uint64_t exc_stride, const int32_t *counts,
                                                             uint64_t tile0, uint64_t n_tiles, uint8_t *flags)
{
    const uint32_t j = blockIdx.y;
    uint64_t n = counts[j] < 0 ? 0 : (uint64_t)counts[j];
    if (n > exc_stride) n = exc_stride;
    const pd_exc *e = exc + (uint64_t)j * exc_stride;
    for (uint64_t i = blockIdx.x * (uint64_t)WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * WG) {
        const uint64_t t = e[i].cell / TILE;
        if (t >= tile0 && t - tile0 < n_tiles) flags[t - tile0] = 1;
    }
}

// The receiving side of the sliced sum, fused: one workgroup per tile of the slice reads the tile's
// 4 KiB of every part (one 16-byte load per lane and part = the lane's 32 consecutive cells), adds
// them in registers, prefix-sums (32 cells in the lane, one wave scan of the lane totals, wave bases
// through LDS, tile carry), wraps, and reduces the tile's share of the (at most two) windows of
// w >= TILE cells it touches.  No int32 copy of the summed arrays ever exists.  Tiles that own
// exceptions (rare: pile-ups) patch them in through LDS.
struct I4Src {
    const uint8_t *parts; uint64_t stride; uint32_t n_parts;
    const uint8_t *flags;                     // per tile of the slice, or null
    const pd_exc *exc; uint64_t exc_stride; const int32_t *counts;
};

// PATCH = false: the tiles without exceptions (nearly all) — no 32 KB patch window in LDS, so eight workgroups fit a CU instead of
// five (the kernel waits for its one load per lane and part: residency is its throughput); PATCH = true: only the flagged tiles.
template <bool PATCH>
__global__ __launch_bounds__(WG) void k_sweep_i4(const I4Src src, const int *carry, uint32_t wrap_mask, const TileMap tmap,
                                                 uint32_t w, uint32_t min_dep, TilePart *part, uint32_t tile0, const uint32_t *list,
                                                 const uint32_t *n_list, int *depth_out)
{
    __shared__ int wtot[4];
    __shared__ int patch[PATCH ? TILE : 1];
    __shared__ unsigned long long red_s[4][2];
    __shared__ int red_c[4][2];
    // PATCH: a few workgroups walk the list of the tiles that own exceptions (k_list_flagged); else one workgroup per tile
    const uint32_t n_it = PATCH ? *n_list : blockIdx.x + 1;
    for (uint32_t it = blockIdx.x; it < n_it; it += gridDim.x) {
    const uint32_t i = PATCH ? list[it] : blockIdx.x;
    if (!PATCH && src.flags && src.flags[i] != 0) return;        // workgroup-uniform
    const uint64_t t = (uint64_t)i + tile0;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int a[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) a[k] = -8 * (int)src.n_parts;
    const uint8_t *p = src.parts + (uint64_t)i * (TILE / 2) + (uint64_t)tid * 16;
    // the parts are added as packed bytes (even / odd nibbles of each word widened to bytes: up to
    // 16 parts fit, 15 * 16 < 256) and only then spread into the 32 int accumulators
    for (uint32_t j0 = 0; j0 < src.n_parts; j0 += 16) {
        unsigned lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
        const uint32_t j1 = j0 + 16 < src.n_parts ? j0 + 16 : src.n_parts;
        for (uint32_t j = j0; j < j1; ++j) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p + (uint64_t)j * src.stride);
            const unsigned wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int m = 0; m < 4; ++m) { lo[m] += wd[m] & 0x0F0F0F0Fu; hi[m] += (wd[m] >> 4) & 0x0F0F0F0Fu; }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                a[8 * m + 2 * b] += (int)((lo[m] >> (8 * b)) & 0xff);
                a[8 * m + 2 * b + 1] += (int)((hi[m] >> (8 * b)) & 0xff);
            }
    }
    if constexpr (PATCH) {
        for (int k = tid; k < TILE; k += WG) patch[k] = 0;
        __syncthreads();
        for (uint32_t j = 0; j < src.n_parts; ++j) {
            uint64_t n = src.counts[j] < 0 ? 0 : (uint64_t)src.counts[j];
            if (n > src.exc_stride) n = src.exc_stride;
            const pd_exc *e = src.exc + (uint64_t)j * src.exc_stride;
            for (uint64_t x = tid; x < n; x += WG)
                if (e[x].cell / TILE == t) atomicAdd(&patch[e[x].cell % TILE], e[x].value);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 32; ++k) a[k] += patch[tid * 32 + k];
    }
    int run = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) { run += a[k]; a[k] = run; }
    const int incl = wave_incl_scan(run);
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    int base = carry[t] + incl - run;
    for (int k = 0; k < wv; ++k) base += wtot[k];

    if (depth_out) {                                              // (uniform) the slice's depth instead of statistics
#pragma unroll
        for (int k = 0; k < 32; ++k) depth_out[(uint64_t)i * TILE + (uint32_t)(tid * 32 + k)] = (int)((uint32_t)(a[k] + base) & wrap_mask);
        __syncthreads();
        continue;
    }
    const uint32_t ctg = tmap.tile_contig[t];
    const uint64_t local0 = t * TILE - tmap.contig_off[ctg];
    const uint32_t clen = tmap.contig_len[ctg];
    int c0 = 0, c1 = 0; unsigned long long s0 = 0, s1 = 0;
    if (local0 < clen) {
        const uint64_t k0 = local0 / w;
        const uint64_t nb = (k0 + 1) * (uint64_t)w - local0;     // tile-local start of window k0+1
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const uint32_t pos = (uint32_t)(tid * 32 + k);
            const uint32_t d = (uint32_t)(a[k] + base) & wrap_mask;
            if (local0 + pos < clen && d >= min_dep) { if (pos < nb) { ++c0; s0 += d; } else { ++c1; s1 += d; } }
        }
    }
    c0 = wave_sum(c0); c1 = wave_sum(c1);
#pragma unroll
    for (int o = 32; o; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
    if (lane == 0) { red_c[wv][0] = c0; red_c[wv][1] = c1; red_s[wv][0] = s0; red_s[wv][1] = s1; }
    __syncthreads();
    if (tid == 0) {
        TilePart tp;
        tp.c0 = (uint32_t)(red_c[0][0] + red_c[1][0] + red_c[2][0] + red_c[3][0]);
        tp.c1 = (uint32_t)(red_c[0][1] + red_c[1][1] + red_c[2][1] + red_c[3][1]);
        tp.s0 = red_s[0][0] + red_s[1][0] + red_s[2][0] + red_s[3][0];
        tp.s1 = red_s[0][1] + red_s[1][1] + red_s[2][1] + red_s[3][1];
        part[i] = tp;
    }
    __syncthreads();
    }
}

// the tiles of the slice whose flag is set, as a list
__global__ __launch_bounds__(WG) void k_list_flagged(const uint8_t *flags, uint32_t n_tiles, uint32_t *list, uint32_t *count)
{
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n_tiles; i += gridDim.x * WG)
        if (flags[i]) list[atomicAdd(count, 1u)] = i;
}

// The same sweep with ONE WAVE PER TILE (tiles without exceptions, at most 16 parts): a lane owns 4 x 32 consecutive cells (the
// 32 cells at lane * 32 of each of the tile's four 2048-cell quarters = one 16-byte load per quarter and part), the quarters are
// swept in order with the running depth carried in a register — no barriers, no LDS, and four loads per part in flight per lane,
// where the workgroup-per-tile form lived for one load's latency and three barriers per 4 KiB of image.
// DEPTH: no statistics — the summed, prefix-summed and wrapped cells of the slice are written out as int32 depth (depth_out: the slice's
// first cell), for the statistics that need the cells themselves (narrow windows, annotation intervals) on the rank that owns the slice.
template <bool DEPTH>
__device__ __forceinline__ void sweep_i4_tile_wave(const I4Src &src, const int *carry, uint32_t wrap_mask, const TileMap &tmap,
                                                   uint32_t w, uint32_t min_dep, TilePart *part, uint32_t tile0, uint32_t i, int *depth_out)
{
    const int lane = threadIdx.x & 63;
    if (src.flags && src.flags[i] != 0) return;                  // a tile with exceptions: k_sweep_i4<true>
    const uint64_t t = (uint64_t)i + tile0;
    const uint8_t *p = src.parts + (uint64_t)i * (TILE / 2) + (uint64_t)lane * 16;
    // the parts are added as packed bytes (even / odd nibbles of each word widened to bytes: 16 parts fit, 15 * 16 < 256)
    unsigned lo[4][4], hi[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int m = 0; m < 4; ++m) { lo[q][m] = 0; hi[q][m] = 0; }
    for (uint32_t j = 0; j < src.n_parts; ++j) {
        uint4 x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const uint4 *>(p + (uint64_t)j * src.stride + q * 1024);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned wd[4] = {x[q].x, x[q].y, x[q].z, x[q].w};
#pragma unroll
            for (int m = 0; m < 4; ++m) { lo[q][m] += wd[m] & 0x0F0F0F0Fu; hi[q][m] += (wd[m] >> 4) & 0x0F0F0F0Fu; }
        }
    }
    const uint32_t ctg = tmap.tile_contig[t];
    const uint64_t local0 = t * TILE - tmap.contig_off[ctg];
    const uint32_t clen = tmap.contig_len[ctg];
    int base = carry[t];                                          // depth just before the quarter's first cell
    int c0 = 0, c1 = 0; unsigned long long s0 = 0, s1 = 0;
    const bool any = local0 < clen;
    const uint64_t k0 = any ? local0 / w : 0;
    const uint64_t nb64 = (k0 + 1) * (uint64_t)w - local0;        // tile-local start of window k0 + 1
    const uint32_t nb = nb64 < (uint64_t)TILE ? (uint32_t)nb64 : (uint32_t)TILE;
    const uint32_t left = !any ? 0u : ((uint64_t)clen - local0 < (uint64_t)TILE ? (uint32_t)(clen - local0) : (uint32_t)TILE);   // cells of the contig in the tile
    const int bias = -8 * (int)src.n_parts;
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const uint32_t bN = 8u * src.n_parts;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t pos0 = (uint32_t)(q * 2048 + lane * 32);
        if constexpr (!DEPTH) {
            // The common quarter — every lane's 32 cells on one side of the window boundary and inside the contig, threshold <= 1, depths
            // below 2^16 (so neither the 18-bit wrap nor a 16-bit counter can bite) — never spreads the packed nibble sums into 32 ints:
            //   lane total and TotalDepth are dot products of the packed bytes (v_dot4_u32_u8: sum of v, and sum of (32 - c) v_c),
            //   CoveredSite counts the cells whose depth is not zero with packed 16-bit arithmetic, cells c and c + 16 side by side:
            //   prefix of v (v_pk_add), minus the value it has where the depth is zero (v_pk_sub), min 1 (v_pk_min), summed.
            // About 140 vector instructions per lane and quarter instead of 400.
            const uint32_t ones = 0x01010101u;
            const uint32_t t16 = __builtin_amdgcn_udot4(lo[q][0], ones, 0u, false) + __builtin_amdgcn_udot4(lo[q][1], ones, 0u, false) +
                                 __builtin_amdgcn_udot4(hi[q][0], ones, 0u, false) + __builtin_amdgcn_udot4(hi[q][1], ones, 0u, false);
            const uint32_t t32 = t16 + __builtin_amdgcn_udot4(lo[q][2], ones, 0u, false) + __builtin_amdgcn_udot4(lo[q][3], ones, 0u, false) +
                                 __builtin_amdgcn_udot4(hi[q][2], ones, 0u, false) + __builtin_amdgcn_udot4(hi[q][3], ones, 0u, false);
            const int run = (int)t32 - (int)(32u * bN);
            const int incl = wave_incl_scan(run);
            const int b0 = base + incl - run;
            const bool plain = pos0 + 32u <= left && (pos0 + 32u <= nb || pos0 >= nb);
            const bool small = (uint32_t)b0 < 60000u;             // (+ at most 32 x 7 x 16 inside the lane: below 2^16, and below any wrap)
            if (__builtin_expect(min_dep <= 1u && wrap_mask >= 0xFFFFu && __ballot(!plain || !small) == 0ull, 1)) {
                uint32_t w = 0;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint32_t wl = (32u - (8u * m)) | ((30u - 8u * m) << 8) | ((28u - 8u * m) << 16) | ((26u - 8u * m) << 24);
                    const uint32_t wh = (31u - (8u * m)) | ((29u - 8u * m) << 8) | ((27u - 8u * m) << 16) | ((25u - 8u * m) << 24);
                    w = __builtin_amdgcn_udot4(lo[q][m], wl, w, false);
                    w = __builtin_amdgcn_udot4(hi[q][m], wh, w, false);
                }
                const uint32_t sum32 = 32u * (uint32_t)b0 + w - bN * 528u;
                uint32_t cnt = 32u;
                if (min_dep) {
                    const uint32_t tl = (bN - (uint32_t)b0) & 0xffffu, th = (bN - ((uint32_t)b0 + t16 - 16u * bN)) & 0xffffu;
                    us2 tgt = __builtin_bit_cast(us2, tl | (th << 16)), r = __builtin_bit_cast(us2, 0u), acc = __builtin_bit_cast(us2, 0u);
                    const us2 step = __builtin_bit_cast(us2, bN | (bN << 16)), one2 = __builtin_bit_cast(us2, 0x00010001u);
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int m = k >> 3, b = (k & 7) >> 1;
                        const uint32_t sel = (uint32_t)b | (0x0cu << 8) | ((4u + (uint32_t)b) << 16) | (0x0cu << 24);
                        const uint32_t pair = (k & 1) ? __builtin_amdgcn_perm(hi[q][m + 2], hi[q][m], sel) : __builtin_amdgcn_perm(lo[q][m + 2], lo[q][m], sel);
                        r += __builtin_bit_cast(us2, pair);
                        acc += __builtin_elementwise_min((us2)(r - tgt), one2);
                        tgt += step;
                    }
                    const uint32_t a32 = __builtin_bit_cast(uint32_t, acc);
                    cnt = (a32 & 0xffffu) + (a32 >> 16);
                }
                const bool first = pos0 < nb;
                c0 += first ? (int)cnt : 0; s0 += first ? (unsigned long long)sum32 : 0ull;
                c1 += first ? 0 : (int)cnt; s1 += first ? 0ull : (unsigned long long)sum32;
                base += __builtin_amdgcn_readlane(incl, 63);
                continue;
            }
        }
        int a[32];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                a[8 * m + 2 * b] = bias + (int)((lo[q][m] >> (8 * b)) & 0xff);
                a[8 * m + 2 * b + 1] = bias + (int)((hi[q][m] >> (8 * b)) & 0xff);
            }
        int run = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) { run += a[k]; a[k] = run; }
        const int incl = wave_incl_scan(run);
        const int b0 = base + incl - run;
        if constexpr (DEPTH) {
            int4 *o = reinterpret_cast<int4 *>(depth_out + (uint64_t)i * TILE + pos0);
#pragma unroll
            for (int k = 0; k < 32; k += 4)
                o[k >> 2] = make_int4((int)((uint32_t)(a[k] + b0) & wrap_mask), (int)((uint32_t)(a[k + 1] + b0) & wrap_mask),
                                      (int)((uint32_t)(a[k + 2] + b0) & wrap_mask), (int)((uint32_t)(a[k + 3] + b0) & wrap_mask));
            base += __builtin_amdgcn_readlane(incl, 63);
            continue;
        }
        // a lane's 32 cells lie on one side of the window boundary and inside the contig, except in the one quarter of a tile that
        // holds the boundary or the contig's end: there every cell is tested (wave-uniform branch), elsewhere none is
        const bool plain = pos0 + 32u <= left && (pos0 + 32u <= nb || pos0 >= nb);
        if (__builtin_expect(__ballot(!plain) == 0ull, 1)) {
            uint32_t cnt = 0; unsigned long long sm = 0;
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const uint32_t d = (uint32_t)(a[k] + b0) & wrap_mask;
                const bool ok = d >= min_dep;
                cnt += ok ? 1u : 0u; sm += ok ? d : 0u;
            }
            const bool first = pos0 < nb;
            c0 += first ? (int)cnt : 0; s0 += first ? sm : 0ull;
            c1 += first ? 0 : (int)cnt; s1 += first ? 0ull : sm;
        } else {
#pragma unroll 4
            for (int k = 0; k < 32; ++k) {
                const uint32_t pos = pos0 + k;
                const uint32_t d = (uint32_t)(a[k] + b0) & wrap_mask;
                if (pos < left && d >= min_dep) { if (pos < nb) { ++c0; s0 += d; } else { ++c1; s1 += d; } }
            }
        }
        base += __builtin_amdgcn_readlane(incl, 63);
    }
    c0 = wave_sum(c0); c1 = wave_sum(c1);
#pragma unroll
    for (int o = 32; o; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
    if (DEPTH) return;
    if (lane == 0) { TilePart tp; tp.c0 = (uint32_t)c0; tp.c1 = (uint32_t)c1; tp.s0 = s0; tp.s1 = s1; part[i] = tp; }
}

// one wave per tile of the slice, or (only != null) the waves of a fixed grid over a list of tiles (the ones k_sweep_i4_fast left)
template <bool DEPTH>
__global__ __launch_bounds__(WG) void k_sweep_i4_wave(const I4Src src, const int *carry, uint32_t wrap_mask, const TileMap tmap,
                                                      uint32_t w, uint32_t min_dep, TilePart *part, uint32_t tile0, uint32_t tile_count, int *depth_out,
                                                      const uint32_t *only, const uint32_t *n_only)
{
    const uint32_t wave = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (!only) {
        if (wave < tile_count) sweep_i4_tile_wave<DEPTH>(src, carry, wrap_mask, tmap, w, min_dep, part, tile0, wave, depth_out);
        return;
    }
    const uint32_t n = *n_only;
    for (uint32_t k = wave; k < n; k += gridDim.x * (WG / 64)) sweep_i4_tile_wave<DEPTH>(src, carry, wrap_mask, tmap, w, min_dep, part, tile0, only[k], depth_out);
}

// The statistics sweep of the tiles that are nothing but common quarters — inside one window, inside the contig, no exceptions, threshold <= 1,
// depths below 2^16 — in a kernel of their own: the packed path of sweep_i4_tile_wave alone, taken quarter by quarter, needs a third of
// its registers, so eight waves share a SIMD instead of four.  A tile that turns out not to qualify
// (a window boundary or a contig's end inside it, a depth of 60 000 or more at some lane's first cell) goes to `slow`, the list
// k_sweep_i4_wave works through afterwards.
__global__ __launch_bounds__(WG, 8) void k_sweep_i4_fast(const I4Src src, const int *carry, const TileMap tmap, uint32_t w, uint32_t min_dep, TilePart *part,
                                                        uint32_t tile0, uint32_t tile_count, uint32_t *slow, uint32_t *n_slow)
{
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (i >= tile_count) return;
    if (src.flags && src.flags[i] != 0) return;                  // a tile with exceptions: k_sweep_i4<true>
    const uint64_t t = (uint64_t)i + tile0;
    const uint32_t ctg = tmap.tile_contig[t];
    const uint64_t local0 = t * TILE - tmap.contig_off[ctg];
    const uint32_t clen = tmap.contig_len[ctg];
    bool fast = local0 < clen && (uint64_t)clen - local0 >= (uint64_t)TILE;
    if (fast) { const uint64_t k0 = local0 / w; fast = (k0 + 1) * (uint64_t)w - local0 >= (uint64_t)TILE; }
    if (!fast) { if (lane == 0) slow[atomicAdd(n_slow, 1u)] = i; return; }
    const uint8_t *p = src.parts + (uint64_t)i * (TILE / 2) + (uint64_t)lane * 16;
    int base = carry[t];
    uint32_t c0 = 0; unsigned long long s0 = 0;
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const uint32_t bN = 8u * src.n_parts, ones = 0x01010101u, bN4 = bN * 0x01010101u;
    // quarter by quarter (the running depth makes them sequential anyway), one 16-byte load per part with the next one — the next part's,
    // or the next quarter's first — in flight: eight accumulators instead of thirty-two
    uint4 x = *reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned lo[4] = {0u, 0u, 0u, 0u}, hi[4] = {0u, 0u, 0u, 0u};
        for (uint32_t j = 0; j < src.n_parts; ++j) {
            const bool more = j + 1 < src.n_parts;
            uint4 nx = x;
            if (more) nx = *reinterpret_cast<const uint4 *>(p + (uint64_t)(j + 1) * src.stride + q * 1024);
            else if (q < 3) nx = *reinterpret_cast<const uint4 *>(p + (q + 1) * 1024);
            const unsigned wd[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int m = 0; m < 4; ++m) { lo[m] += wd[m] & 0x0F0F0F0Fu; hi[m] += (wd[m] >> 4) & 0x0F0F0F0Fu; }
            x = nx;
        }
        // (the arithmetic of sweep_i4_tile_wave's common quarter, see there)
        const uint32_t t32 = __builtin_amdgcn_udot4(lo[0], ones, 0u, false) + __builtin_amdgcn_udot4(lo[1], ones, 0u, false) +
                             __builtin_amdgcn_udot4(hi[0], ones, 0u, false) + __builtin_amdgcn_udot4(hi[1], ones, 0u, false) +
                             __builtin_amdgcn_udot4(lo[2], ones, 0u, false) + __builtin_amdgcn_udot4(lo[3], ones, 0u, false) +
                             __builtin_amdgcn_udot4(hi[2], ones, 0u, false) + __builtin_amdgcn_udot4(hi[3], ones, 0u, false);
        const int run = (int)t32 - (int)(32u * bN);
        const int incl = wave_incl_scan(run);
        const int b0 = base + incl - run;
        if (__ballot((uint32_t)b0 >= 60000u) != 0ull) { if (lane == 0) slow[atomicAdd(n_slow, 1u)] = i; return; }
        uint32_t wsum = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t wl = (32u - (8u * m)) | ((30u - 8u * m) << 8) | ((28u - 8u * m) << 16) | ((26u - 8u * m) << 24);
            const uint32_t wh = (31u - (8u * m)) | ((29u - 8u * m) << 8) | ((27u - 8u * m) << 16) | ((25u - 8u * m) << 24);
            wsum = __builtin_amdgcn_udot4(lo[m], wl, wsum, false);
            wsum = __builtin_amdgcn_udot4(hi[m], wh, wsum, false);
        }
        s0 += 32u * (uint32_t)b0 + wsum - bN * 528u;
        uint32_t cnt = 32u;
        if (min_dep) {
            // CoveredSite.  A depth is never negative, so a cell is uncovered only where the running depth has come DOWN to zero: if the depth
            // before the lane's first cell exceeds the sum of the NEGATIVE differences among its 32 cells, no cell of the lane can be zero
            // and all 32 count — eight v_sad_u8 (sum |v_c| = positives + negatives; their difference is `run`) instead of the 96
            // instructions of the packed prefix walk below, which only the wave-quarters with a lane near depth zero still take
            // (at 50x about one in 10^4; round 5's kernel walked every quarter: 0.27 of the HBM roofline, instruction-bound).
            uint32_t sad = 0;
#pragma unroll
            for (int m = 0; m < 4; ++m) { sad = __builtin_amdgcn_sad_u8(lo[m], bN4, sad); sad = __builtin_amdgcn_sad_u8(hi[m], bN4, sad); }
            const int neg = ((int)sad - run) >> 1;
            if (__builtin_expect(__ballot(b0 <= neg) != 0ull, 0)) {
                const uint32_t t16 = __builtin_amdgcn_udot4(lo[0], ones, 0u, false) + __builtin_amdgcn_udot4(lo[1], ones, 0u, false) +
                                     __builtin_amdgcn_udot4(hi[0], ones, 0u, false) + __builtin_amdgcn_udot4(hi[1], ones, 0u, false);
                const uint32_t tl = (bN - (uint32_t)b0) & 0xffffu, th = (bN - ((uint32_t)b0 + t16 - 16u * bN)) & 0xffffu;
                us2 tgt = __builtin_bit_cast(us2, tl | (th << 16)), r = __builtin_bit_cast(us2, 0u), acc = __builtin_bit_cast(us2, 0u);
                const us2 step = __builtin_bit_cast(us2, bN | (bN << 16)), one2 = __builtin_bit_cast(us2, 0x00010001u);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int m = k >> 3, b = (k & 7) >> 1;
                    const uint32_t sel = (uint32_t)b | (0x0cu << 8) | ((4u + (uint32_t)b) << 16) | (0x0cu << 24);
                    const uint32_t pair = (k & 1) ? __builtin_amdgcn_perm(hi[m + 2], hi[m], sel) : __builtin_amdgcn_perm(lo[m + 2], lo[m], sel);
                    r += __builtin_bit_cast(us2, pair);
                    acc += __builtin_elementwise_min((us2)(r - tgt), one2);
                    tgt += step;
                }
                const uint32_t a32 = __builtin_bit_cast(uint32_t, acc);
                cnt = (a32 & 0xffffu) + (a32 >> 16);
            }
        }
        c0 += cnt;
        base += __builtin_amdgcn_readlane(incl, 63);
    }
    c0 = (uint32_t)wave_sum((int)c0);
#pragma unroll
    for (int o = 32; o; o >>= 1) s0 += __shfl_xor(s0, o);
    if (lane == 0) { TilePart tp; tp.c0 = c0; tp.c1 = 0; tp.s0 = s0; tp.s1 = 0; part[i] = tp; }
}

__global__ __launch_bounds__(WG) void k_add_i32(int4 *dst, const int4 *src, size_t n16)
{
    size_t i = blockIdx.x * (size_t)WG + threadIdx.x;
    const size_t st = (size_t)gridDim.x * WG;
    for (; i < n16; i += st) {
        int4 a = dst[i]; const int4 b = src[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        dst[i] = a;
    }
}

void launch_add_i32(hipStream_t st, int *dst, const int *src, size_t n_words)
{
    const size_t n16 = n_words / 4;
    size_t g = (n16 + WG - 1) / WG; if (g > 8192) g = 8192; if (!g) return;
    hipLaunchKernelGGL(k_add_i32, dim3((unsigned)g), dim3(WG), 0, st, (int4 *)dst, (const int4 *)src, n16);
}

void launch_export_i8(hipStream_t st, const int *diff, const uint8_t *hstate, void *out, uint64_t n_cells, int thr,
                      pd_exc *exc, uint32_t cap, uint32_t *count)
{
    hipLaunchKernelGGL(k_export_i8, dim3(8192), dim3(WG), 0, st, diff, hstate, (int4 *)out, n_cells, thr, exc, cap, count);
}

void launch_import_i8(hipStream_t st, const void *in, int *diff, uint64_t n_cells, int bias, const pd_exc *exc,
                      uint64_t n_exc)
{
    hipLaunchKernelGGL(k_import_i8, dim3(8192), dim3(WG), 0, st, (const int4 *)in, diff, n_cells, bias);
    if (n_exc) hipLaunchKernelGGL(k_apply_exceptions, dim3(256), dim3(WG), 0, st, exc, n_exc, diff, n_cells);
}

void launch_export_i4(hipStream_t st, const int *diff, const uint8_t *hstate, void *out, uint64_t n_cells,
                      pd_exc *exc, uint32_t cap, uint32_t *count)
{
    hipLaunchKernelGGL(k_export_i4, dim3(16384), dim3(WG), 0, st, diff, hstate, (unsigned short *)out,
                       (uint32_t)(n_cells / TILE), exc, cap, count);
}

void launch_add_i4(hipStream_t st, int *dst, const void *img, uint32_t n_tiles, const pd_exc *exc, uint64_t n_exc,
                   uint64_t n_cells_total, int *dst_base)
{
    if (n_tiles) {
        unsigned g = n_tiles < 16384 ? n_tiles : 16384;
        hipLaunchKernelGGL(k_add_i4, dim3(g), dim3(WG), 0, st, dst, (const unsigned short *)img, n_tiles);
    }
    if (n_exc) hipLaunchKernelGGL(k_apply_exceptions, dim3(256), dim3(WG), 0, st, exc, n_exc, dst_base, n_cells_total);
}

// (A/B switch of the packed statistics kernel: pd_set_param "sweep_i4_fast")
static bool g_sweep_i4_fast = true;
void set_sweep_i4_fast(bool on) { g_sweep_i4_fast = on; }
static bool sweep_i4_fast_on() { return g_sweep_i4_fast; }

void launch_sweep_i4(hipStream_t st, const void *parts, uint32_t n_parts, uint64_t stride, uint32_t tile_first,
                     uint32_t tile_count, const pd_exc *exc, uint64_t exc_stride, const int32_t *exc_counts, uint8_t *flags, size_t flags_bytes,
                     const int *carry, uint32_t wrap_mask, TileMap tm, uint32_t w, uint32_t min_dep, TilePart *part, int *depth_out)
{
    if (!tile_count) return;
    const bool with_exc = exc && exc_counts && exc_stride && flags;
    // behind the flags (one byte per tile of the buffer): a counter and the list of the flagged tiles of this slice
    uint32_t *n_list = with_exc ? reinterpret_cast<uint32_t *>(flags + flags_bytes) : nullptr, *list = with_exc ? n_list + 4 : nullptr;
    if (with_exc) {
        (void)hipMemsetAsync(flags, 0, tile_count, st);
        (void)hipMemsetAsync(n_list, 0, 16, st);
        hipLaunchKernelGGL(k_flag_exception_tiles, dim3(64, n_parts), dim3(WG), 0, st, exc, exc_stride, exc_counts,
                           (uint64_t)tile_first, (uint64_t)tile_count, flags);
        hipLaunchKernelGGL(k_list_flagged, dim3(256), dim3(WG), 0, st, (const uint8_t *)flags, tile_count, list, n_list);
    }
    I4Src src{(const uint8_t *)parts, stride, n_parts, with_exc ? flags : nullptr, exc, exc_stride, exc_counts};
    if (n_parts <= 16) {
        const dim3 g((tile_count + WG / 64 - 1) / (WG / 64));
        const uint32_t *none = nullptr;
        // behind the flags and the list of the flagged tiles: a second counter and list, for the tiles the packed kernel leaves
        uint32_t *n_slow = flags ? reinterpret_cast<uint32_t *>(flags + flags_bytes) + 4 + ((tile_count + 3u) & ~3u) : nullptr, *slow = n_slow ? n_slow + 4 : nullptr;
        if (depth_out) hipLaunchKernelGGL(k_sweep_i4_wave<true>, g, dim3(WG), 0, st, src, carry, wrap_mask, tm, w, min_dep, part, tile_first, tile_count, depth_out, none, none);
        else if (n_slow && min_dep <= 1u && wrap_mask >= 0xFFFFu && sweep_i4_fast_on()) {
            (void)hipMemsetAsync(n_slow, 0, 16, st);
            hipLaunchKernelGGL(k_sweep_i4_fast, g, dim3(WG), 0, st, src, carry, tm, w, min_dep, part, tile_first, tile_count, slow, n_slow);
            hipLaunchKernelGGL(k_sweep_i4_wave<false>, dim3(g.x < 1024u ? g.x : 1024u), dim3(WG), 0, st, src, carry, wrap_mask, tm, w, min_dep, part, tile_first, tile_count,
                               depth_out, (const uint32_t *)slow, (const uint32_t *)n_slow);
        } else hipLaunchKernelGGL(k_sweep_i4_wave<false>, g, dim3(WG), 0, st, src, carry, wrap_mask, tm, w, min_dep, part, tile_first, tile_count, depth_out, none, none);
    } else if (depth_out) {                                      // (more than 16 parts: the workgroup form, every tile through the list-less PATCH-free kernel's depth branch)
        hipLaunchKernelGGL(k_sweep_i4<false>, dim3(tile_count), dim3(WG), 0, st, src, carry, wrap_mask, tm, w, min_dep, part, tile_first,
                           (const uint32_t *)nullptr, (const uint32_t *)nullptr, depth_out);
    } else
        hipLaunchKernelGGL(k_sweep_i4<false>, dim3(tile_count), dim3(WG), 0, st, src, carry, wrap_mask, tm, w, min_dep, part, tile_first,
                           (const uint32_t *)nullptr, (const uint32_t *)nullptr, (int *)nullptr);
    if (with_exc)
        hipLaunchKernelGGL(k_sweep_i4<true>, dim3(512), dim3(WG), 0, st, src, carry, wrap_mask, tm, w, min_dep, part, tile_first, (const uint32_t *)list,
                           (const uint32_t *)n_list, depth_out);
}

void launch_window_gather(hipStream_t st, const TilePart *part, TileMap tm, int32_t n_contigs, uint32_t w,
                          uint64_t n_windows, uint32_t *cover, unsigned long long *sum, const GatherCall &gc)
{
    if (!n_windows) return;
    // a workgroup per window once a window's tiles give each of its 256 lanes one (w >= 256 tiles), a wave per window below that
    if (w / (uint32_t)TILE >= (uint32_t)WG)
        hipLaunchKernelGGL(k_window_gather<4>, dim3((unsigned)n_windows), dim3(WG), 0, st, part, tm, n_contigs, w, n_windows, cover, sum, gc);
    else
        hipLaunchKernelGGL(k_window_gather<1>, dim3((unsigned)((n_windows + 3) / 4)), dim3(WG), 0, st, part, tm, n_contigs, w, n_windows, cover, sum, gc);
}

// ------------------------------------------------------------------------------------------
// launch wrappers (called from pd_capi.hip, pd_windows.hip and pd_rows.hip)
// ------------------------------------------------------------------------------------------
void launch_fill(hipStream_t st, void *p, size_t bytes)
{
    const size_t n16 = bytes / 16;
    size_t g = (n16 + WG - 1) / WG; if (g > 4096) g = 4096; if (g == 0) g = 1;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)g), dim3(WG), 0, st, (int4 *)p, n16);
}

void launch_reset_spans(hipStream_t st, const ResetSpans &rs)
{
    size_t most = 0;
    for (int k = 0; k < ResetSpans::N; ++k) if (rs.bytes[k] > most) most = rs.bytes[k];
    size_t g = (most / 16 + WG - 1) / WG; if (g > 2048) g = 2048; if (g == 0) g = 1;
    hipLaunchKernelGGL(k_reset_spans, dim3((unsigned)g), dim3(WG), 0, st, rs);
}

void launch_scatter_atomic(hipStream_t st, const pd_iv *iv, size_t n, ContigTab tab, int *diff, int *sums)
{
    size_t g = (n + WG - 1) / WG; if (g > 8192) g = 8192; if (g == 0) return;
    hipLaunchKernelGGL(k_scatter_atomic, dim3((unsigned)g), dim3(WG), 0, st, iv, n, tab, diff, sums);
}

void launch_scatter_index(hipStream_t st, const pd_iv *iv, uint32_t n, ContigTab tab, uint32_t lmax,
                          uint32_t disorder, uint32_t sample, uint32_t *ub_a, uint32_t *cand_lo,
                          uint32_t n_stiles, int stile, BatchDesc *desc)
{
    const uint32_t K = (n + sample - 1) / sample + 1;
    const dim3 g((K + WG - 1) / WG), b(WG);
    if (stile == 4096)
        hipLaunchKernelGGL(k_index<4096>, g, b, 0, st, iv, n, sample, tab, lmax, disorder, ub_a, cand_lo, n_stiles, desc);
    else
        hipLaunchKernelGGL(k_index<8192>, g, b, 0, st, iv, n, sample, tab, lmax, disorder, ub_a, cand_lo, n_stiles, desc);
}

void launch_scatter_tiles(hipStream_t st, const PendSet &ps, ContigTab tab, const uint32_t *tile_contig,
                          uint32_t n_stiles, int stile, int *diff, int *sums, uint8_t *hstate,
                          uint64_t *ovf, uint32_t ovf_cap, CheckWords *chk, unsigned grid_tiles)
{
    if (stile == 4096)
        hipLaunchKernelGGL(k_scatter_tiles<4096>, dim3(grid_tiles), dim3(WG), 0, st, ps, n_stiles, tab, tile_contig,
                           diff, sums, hstate, ovf, ovf_cap, chk);
    else
        hipLaunchKernelGGL(k_scatter_tiles<8192>, dim3(grid_tiles), dim3(WG), 0, st, ps, n_stiles, tab, tile_contig,
                           diff, sums, hstate, ovf, ovf_cap, chk);
}

static unsigned grid_1k(uint64_t n) { return (unsigned)((n + 1023) / 1024 ? (n + 1023) / 1024 : 1); }

void launch_c8_from_sorted(hipStream_t st, const pd_iv *iv, uint32_t n, ContigTab tab, uint32_t bshift, uint32_t *lo, uint32_t *hi, uint16_t *nar, uint32_t *b1, uint32_t *words)
{
    if (!n) return;
    hipLaunchKernelGGL(k_c8_from_sorted, dim3((unsigned)(((uint64_t)n + WG - 1) / WG)), dim3(WG), 0, st, iv, n, tab, bshift, lo, hi, nar, b1, words);
}

void launch_c8_hist(hipStream_t st, const pd_iv *iv, uint32_t n, ContigTab tab, uint32_t bshift, uint32_t *hist, uint32_t *words)
{
    if (!n) return;
    const uint64_t g = ((uint64_t)n + WG - 1) / WG;
    hipLaunchKernelGGL(k_c8_hist, dim3((unsigned)(g > 65536 ? 65536 : g)), dim3(WG), 0, st, iv, n, tab, bshift, hist, words);
}

void launch_excl_scan_u32(hipStream_t st, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *block_sums)
{
    const unsigned nb = grid_1k(n);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(WG), 0, st, in, n, block_sums);
    hipLaunchKernelGGL(k_scan_of_sums, dim3(1), dim3(1024), 0, st, block_sums, nb);
    hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(WG), 0, st, in, out, n, (const uint32_t *)block_sums);
}

// b1[0 .. n_buckets]: the marks of the buckets' first runs (0xFFFFFFFF where nobody begins) -> the index of the first run at or behind
// every bucket; b1[n_buckets] = n_runs.  tmp: n_buckets / 1024 + 2 words.
void launch_c8_fill_starts(hipStream_t st, uint32_t *b1, uint32_t n_buckets, uint32_t n_runs, uint32_t *tmp)
{
    const uint32_t n = n_buckets + 1;
    const unsigned nb = grid_1k(n);
    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, b1 + n_buckets, n_runs);
    hipLaunchKernelGGL(k_sfx_block_min, dim3(nb), dim3(WG), 0, st, (const uint32_t *)b1, n, tmp);
    hipLaunchKernelGGL(k_sfx_of_mins, dim3(1), dim3(1024), 0, st, tmp, nb);
    hipLaunchKernelGGL(k_sfx_blocks, dim3(nb), dim3(WG), 0, st, b1, n, (const uint32_t *)tmp);
}

void launch_c8_marks_to_index(hipStream_t st, const unsigned long long *marks, uint32_t n_buckets, const uint32_t *base, uint32_t *b1)
{
    if (!n_buckets) return;
    hipLaunchKernelGGL(k_c8_marks_to_index, dim3((unsigned)(((uint64_t)n_buckets + WG - 1) / WG)), dim3(WG), 0, st, marks, n_buckets, base, b1);
}

void launch_c8_place_other(hipStream_t st, const pd_iv *iv, uint32_t n, ContigTab tab, uint32_t bshift, const uint32_t *o1, uint32_t *cursor, uint32_t *lo, uint32_t *hi)
{
    if (!n) return;
    const uint64_t g = ((uint64_t)n + WG - 1) / WG;
    hipLaunchKernelGGL(k_c8_place_other, dim3((unsigned)(g > 65536 ? 65536 : g)), dim3(WG), 0, st, iv, n, tab, bshift, o1, cursor, lo, hi);
}

void launch_c8_expand(hipStream_t st, C8Sample cs, const uint32_t *tile_contig, const uint64_t *contig_off, uint32_t n_tiles, pd_iv *out)
{
    hipLaunchKernelGGL(k_c8_expand, dim3(n_tiles < 16384u ? (n_tiles ? n_tiles : 1u) : 16384u), dim3(WG), 0, st, cs, tile_contig, contig_off, n_tiles, out);
}

void launch_copy_words(hipStream_t st, void *dst, const void *src, uint64_t n_words)
{
    if (!n_words) return;
    const uint64_t g = (n_words / 4 + 255) / 256 + 1;
    hipLaunchKernelGGL(k_copy_words, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, st, (uint32_t *)dst, (const uint32_t *)src, n_words);
}

void launch_copy_planes(hipStream_t st, uint32_t *dst_lo, uint32_t *dst_hi, const uint32_t *src_lo, const uint32_t *src_hi, uint64_t n, uint16_t *dst_nar, uint32_t *n_wide)
{
    if (!n) return;
    const uint64_t g = (n / 4 + 255) / 256 + 1;
    if (dst_nar) hipLaunchKernelGGL(k_copy_planes_nar, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, st, dst_lo, dst_hi, dst_nar, src_lo, src_hi, n, n_wide);
    else hipLaunchKernelGGL(k_copy_planes, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, st, dst_lo, dst_hi, src_lo, src_hi, n);
}

void launch_c8_tile_desc(hipStream_t st, C8Sample cs, ContigTab tab, const uint32_t *tile_contig, uint32_t n_tiles, TileDesc *desc, uint32_t *n_heavy, uint32_t *heavy_tiles)
{
    if (n_tiles) hipLaunchKernelGGL(k_c8_tile_desc, dim3((n_tiles + WG - 1) / WG), dim3(WG), 0, st, cs, tab, tile_contig, n_tiles, desc, n_heavy, heavy_tiles);
}

void launch_r8_to_iv(hipStream_t st, const uint32_t *lo, const uint32_t *hi, uint64_t n, ContigTab tab, pd_iv *out)
{
    if (!n) return;
    const uint64_t g = (n + WG - 1) / WG;
    hipLaunchKernelGGL(k_r8_to_iv, dim3((unsigned)(g > 65536 ? 65536 : g)), dim3(WG), 0, st, lo, hi, n, tab, out);
}

void launch_fill_invalid(hipStream_t st, int *diff, uint8_t *hstate, uint32_t n_half, CheckWords *chk,
                         bool only_if_overflow, unsigned grid)
{
    hipLaunchKernelGGL(k_fill_invalid, dim3(grid), dim3(WG), 0, st, (int4 *)diff, hstate, n_half, chk,
                       only_if_overflow ? 1 : 0);
    if (!only_if_overflow) hipLaunchKernelGGL(k_mark_all_valid, dim3(1), dim3(1), 0, st, chk);
}

void launch_mark_all_valid(hipStream_t st, CheckWords *chk)
{
    hipLaunchKernelGGL(k_mark_all_valid, dim3(1), dim3(1), 0, st, chk);
}

void launch_scatter_finish(hipStream_t st, const PendSet &ps, int *diff, int *sums, const uint64_t *ovf,
                           uint32_t ovf_cap, CheckWords *chk)
{
    hipLaunchKernelGGL(k_apply_overflow, dim3(256), dim3(WG), 0, st, ovf, chk, ovf_cap, diff, sums, 0);
    hipLaunchKernelGGL(k_finish_batch, dim3(1), dim3(1), 0, st, ps, chk);
}

void launch_tile_carry(hipStream_t st, const int *sums, int *bsum, int *carry, uint32_t n_tiles)
{
    const unsigned nb = (n_tiles + 1023) / 1024;
    hipLaunchKernelGGL(k_carry_block_sums, dim3(nb), dim3(1024), 0, st, sums, bsum, n_tiles);
    hipLaunchKernelGGL(k_tile_carry, dim3(nb), dim3(1024), 0, st, sums, bsum, carry, n_tiles);
}

void launch_scan_write(hipStream_t st, int *buf, const int *carry, uint32_t n_tiles, uint32_t wrap_mask,
                       const uint8_t *hstate)
{
    TileMap tm{}; WinArgs wa{};
    hipLaunchKernelGGL((k_sweep<true, false, false>), dim3(n_tiles), dim3(WG), 0, st, buf, carry, wrap_mask, tm, wa, hstate, 0u);
}

static size_t win_lds_bytes(uint32_t w)
{
    if (w >= (uint32_t)TILE) return 16;                // large windows use per-tile partials, no LDS accumulators
    const size_t nacc = (size_t)TILE / w + 2;
    return nacc * 8 + 16;
}

int launch_sweep_windows(hipStream_t st, int *buf, const int *carry, uint32_t n_tiles, uint32_t wrap_mask,
                         TileMap tm, uint32_t w, uint32_t min_dep, uint32_t *cover, unsigned long long *sum,
                         TilePart *part, uint64_t n_windows, int32_t n_contigs, bool from_depth,
                         const uint8_t *hstate)
{
    WinArgs wa; wa.w = w; wa.min_dep = min_dep; wa.inv_w = 1.0f / (float)w; wa.cover = cover; wa.sum = sum;
    wa.part = part;
    const size_t lds = win_lds_bytes(w);
    hipError_t e = hipSuccess;
    if (from_depth) {
        if (lds > 48 * 1024) e = hipFuncSetAttribute((const void *)k_sweep<false, true, true>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((k_sweep<false, true, true>), dim3(n_tiles), dim3(WG), lds, st, buf, carry, wrap_mask, tm, wa, hstate, 0u);
    } else {
        if (lds > 48 * 1024) e = hipFuncSetAttribute((const void *)k_sweep<false, true, false>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((k_sweep<false, true, false>), dim3(n_tiles), dim3(WG), lds, st, buf, carry, wrap_mask, tm, wa, hstate, 0u);
    }
    if (w >= (uint32_t)TILE) launch_window_gather(st, part, tm, n_contigs, w, n_windows, cover, sum);
    if (w < (uint32_t)TILE && n_tiles > 1)
        hipLaunchKernelGGL(k_window_edges, dim3((n_tiles + WG - 1) / WG), dim3(WG), 0, st, (const TilePart *)part, tm, n_tiles, w, cover, sum);
    return 0;
}

// Narrow windows over a SLICE of the summed depth (tiles [tile_first, tile_first + tile_count) of the genome, `depth_slice` holding exactly
// those): windows inside the slice's tiles into the (whole-genome) window arrays, the shares of the windows across tile edges into
// part[tile] (whole-genome indexing); the caller merges ranks and runs launch_window_edges once everything is together.
int launch_sweep_windows_slice(hipStream_t st, int *depth_slice, uint32_t tile_first, uint32_t tile_count, TileMap tm, uint32_t w, uint32_t min_dep,
                               uint32_t *cover, unsigned long long *sum, TilePart *part)
{
    if (!tile_count) return 0;
    WinArgs wa; wa.w = w; wa.min_dep = min_dep; wa.inv_w = 1.0f / (float)w; wa.cover = cover; wa.sum = sum; wa.part = part;
    const size_t lds = win_lds_bytes(w);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_sweep<false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((k_sweep<false, true, true>), dim3(tile_count), dim3(WG), lds, st, depth_slice, (const int *)nullptr, 0xFFFFFFFFu, tm, wa,
                       (const uint8_t *)nullptr, tile_first);
    return 0;
}

void launch_window_edges(hipStream_t st, const TilePart *part, TileMap tm, uint32_t n_tiles, uint32_t w, uint32_t *cover, unsigned long long *sum)
{
    if (n_tiles > 1) hipLaunchKernelGGL(k_window_edges, dim3((n_tiles + WG - 1) / WG), dim3(WG), 0, st, part, tm, n_tiles, w, cover, sum);
}

void launch_reduce_pieces(hipStream_t st, const int *depth, const Piece *pieces, uint32_t n_pieces,
                          uint32_t min_dep, int *cover, unsigned long long *sum)
{
    if (!n_pieces) return;
    hipLaunchKernelGGL(k_reduce_pieces, dim3((n_pieces + 3) / 4), dim3(WG), 0, st, depth, pieces, n_pieces,
                       min_dep, cover, sum);
}

// LDS of the histogram kernels: `copies` copies of n_bins counters (padded to 16 B)
static size_t hist_lds_bytes(uint32_t n_bins, int copies, uint32_t *nbp)
{
    *nbp = (n_bins + 3u) & ~3u;
    return (size_t)copies * *nbp * 4;
}

// variant: bit 0 = one LDS copy for the workgroup (else one per wave), bit 1 = no folding of equal neighbours
int launch_sweep_hist(hipStream_t st, const int *buf, const int *carry, uint32_t n_tiles, uint32_t wrap_mask, TileMap tm,
                      const uint8_t *hstate, bool from_depth, uint32_t n_bins, unsigned long long *hist, unsigned grid, int variant)
{
    if (!n_tiles) return 0;
    if (grid < 1) grid = 1;
    const uint32_t tpw = (uint32_t)((n_tiles + grid - 1) / grid);
    grid = (n_tiles + tpw - 1) / tpw;
    HistArgs ha; ha.n_bins = n_bins; ha.hist = hist;
    const int copies = (variant & 1) ? 1 : 4;
    const size_t lds = hist_lds_bytes(n_bins, copies, &ha.nbp);
#define PD_HIST_GO(FD, C, F)                                                                                           \
    do {                                                                                                               \
        if (int e = hist_lds_reserve(k_sweep_hist<FD, C, F>, lds)) return e;                                           \
        hipLaunchKernelGGL((k_sweep_hist<FD, C, F>), dim3(grid), dim3(WG), lds, st, buf, carry, wrap_mask, tm, hstate, \
                           n_tiles, tpw, ha);                                                                          \
    } while (0)
    switch ((from_depth ? 4 : 0) | (variant & 3)) {
    case 0: PD_HIST_GO(false, 4, true); break;
    case 1: PD_HIST_GO(false, 1, true); break;
    case 2: PD_HIST_GO(false, 4, false); break;
    case 3: PD_HIST_GO(false, 1, false); break;
    case 4: PD_HIST_GO(true, 4, true); break;
    case 5: PD_HIST_GO(true, 1, true); break;
    case 6: PD_HIST_GO(true, 4, false); break;
    default: PD_HIST_GO(true, 1, false); break;
    }
#undef PD_HIST_GO
    return 0;
}

int launch_hist_pieces(hipStream_t st, const int *depth, const Piece *pieces, uint32_t n_pieces, uint32_t n_bins,
                       unsigned long long *hist, unsigned grid, int variant)
{
    if (!n_pieces) return 0;
    if (grid < 1) grid = 1;
    const uint32_t ppw = (n_pieces + grid - 1) / grid;
    grid = (n_pieces + ppw - 1) / ppw;
    HistArgs ha; ha.n_bins = n_bins; ha.hist = hist;
    const int copies = (variant & 1) ? 1 : 4;
    const size_t lds = hist_lds_bytes(n_bins, copies, &ha.nbp);
    const uint32_t *d = reinterpret_cast<const uint32_t *>(depth);
#define PD_HIST_GO(C, F)                                                                                               \
    do {                                                                                                               \
        if (int e = hist_lds_reserve(k_hist_pieces<C, F>, lds)) return e;                                              \
        hipLaunchKernelGGL((k_hist_pieces<C, F>), dim3(grid), dim3(WG), lds, st, d, pieces, n_pieces, ppw, ha);        \
    } while (0)
    switch (variant & 3) {
    case 0: PD_HIST_GO(4, true); break;
    case 1: PD_HIST_GO(1, true); break;
    case 2: PD_HIST_GO(4, false); break;
    default: PD_HIST_GO(1, false); break;
    }
#undef PD_HIST_GO
    return 0;
}

} // namespace pdk
