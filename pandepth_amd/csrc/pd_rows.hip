// pd_rows.hip — the row statistics of the resident depth and nothing else: the depth histograms (pd_scan_depth_histogram, pd_depth_histogram), the
// interval sums (pd_reduce_intervals), the levels (pd_depth_levels), the quantiles (pd_window_quantiles, pd_depth_quantiles) and the thresholds
// (pd_window_thresholds, pd_depth_thresholds).  The levels, quantile and threshold kernels and their launchers are this file's; the histogram and
// interval kernels (k_sweep_hist, k_hist_pieces, k_reduce_pieces) stay in pd_kernels.hip with the sweeps they share code with.  What a call decides from
// numbers — clipping, pieces, batch ends, launch shapes, group shifts — is pd_rows_rule.h's, checked on the CPU; this file queues the work.
#include "pd_ctx.h"
#include "pd_dev.h"
#include "pd_rows_rule.h"

namespace pdk {

// The rows of the quantiles and thresholds over the depth left by pd_scan.  Row r of a batch is the segments segs[seg_off[r] .. seg_off[r + 1])
// (Piece.start = flat cell, Piece.count; region unused) or, with segs == nullptr, window row0 + r of pd_window_layout(w), found on the device.
// `list` (may be null: rows 0 .. n - 1) names the rows a launch takes.  q[r * P.n + j] = the nearest-rank P.p[j] quantile, 0xFFFFFFFF for a row
// without cells (launch_quant_block with ghist: the row's 4096 bins were counted by launch_hist_pieces into ghist[slot * 4096 ..), slot = the launch's row number).
struct QRows {
    const Piece *segs; const uint64_t *seg_off;
    const uint64_t *win_off, *contig_off; const uint32_t *contig_len;
    uint64_t row0; uint32_t w; int32_t n_contigs;
};
struct QPct { uint32_t n; uint32_t p[16]; };
// out[r * T.n + j] = the cells of row r that are >= T.t[j]; T.t[T.n ..) is 2^32-1; out is uint64 for segment rows, uint32 for windows
struct ThrSet { uint32_t n; uint32_t t[16]; };

// ------------------------------------------------------------------------------------------
// depth levels (pd_depth_levels): the materialised depth of one contig range as runs of equal depth, or of equal depth class —
// an ORDERED stream compaction.  Cell i opens a run when it is the range's first or class(d[i]) != class(d[i-1]).
//   k_levels<EDGES, false> : every wave counts the runs that open in its 2048 cells
//   k_levels_scan          : exclusive scan of the waves' counts (one workgroup), total behind the last
//   k_levels<EDGES, true>  : every wave with runs writes its (start, class) pairs at its offset, in cell order
// A wave owns 8 rows of 64 int4 (lane = four consecutive cells, non-temporal loads); waves are independent — the unit of the
// count / offset arrays is the wave, so neither pass needs a workgroup-wide exchange, and the emit pass does not even load the
// cells of a wave in which no run opens (quantised output: most of them).  The left neighbour of a lane's first cell comes from
// the lane below (__shfl_up), of a row's first cell from the row before (readlane), of the wave's first cell from one extra
// load.  `src` points at an int4-aligned cell at most three cells in front of the range; the range is [lo, hi) relative to it,
// and nothing outside it is read (cell lo always opens a run, so it needs no neighbour).
// class(): the identity (EDGES = false), else the index of the last edge <= d (0xFFFFFFFF below the first): a 256-entry LDS
// table for low depths, and — for a row in which ANY lane holds a deeper cell, a wave-uniform choice — a branch-free six-step
// search of the edges in LDS (edge[0] apart, edge[1 .. 63] padded with 0xFFFFFFFF).
// ------------------------------------------------------------------------------------------
namespace {
constexpr int LV_ROWS = 8;
constexpr uint32_t LV_WAVE = LV_ROWS * 256;          // cells per wave
constexpr uint32_t LV_LUT = 256;                     // depths classified by table
static_assert(LV_LUT == WG, "one table entry per thread");
}

__device__ __forceinline__ uint32_t level_search(uint32_t d, const uint32_t *edge, uint32_t n_edges)
{
    uint32_t pos = 0;                                            // edges among edge[1 .. 63] that are <= d
#pragma unroll
    for (uint32_t s = 32; s; s >>= 1) pos += edge[pos + s] <= d ? s : 0u;
    pos = min(pos, n_edges - 1u);                                // (d = 0xFFFFFFFF meets the padding)
    return d < edge[0] ? 0xFFFFFFFFu : pos;
}

template <bool EDGES, bool WRITE>
__global__ __launch_bounds__(WG) void k_levels(const uint32_t *src, uint32_t first_cell, uint32_t lo, uint32_t hi, const uint32_t *edges,
                                               uint32_t n_edges, uint32_t *wave_cnt, const uint32_t *wave_off, uint2 *out, uint32_t cap)
{
    __shared__ uint32_t s_edge[64];
    __shared__ uint32_t s_lut[LV_LUT];
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (EDGES) {
        if (threadIdx.x < 64) s_edge[threadIdx.x] = threadIdx.x < n_edges ? edges[threadIdx.x] : 0xFFFFFFFFu;
        __syncthreads();
        s_lut[threadIdx.x] = level_search(threadIdx.x, s_edge, n_edges);
        __syncthreads();
    }
    const uint32_t w0 = g * LV_WAVE;                             // (wave-uniform from here on: no barrier below)
    uint32_t run = 0;
    if (WRITE) {
        run = wave_off[g];
        if (wave_off[g + 1] == run) return;                      // no run opens here (or the wave lies behind the range)
    } else if (w0 >= hi) {
        if (lane == 0) wave_cnt[g] = 0;
        return;
    }
    uint32_t c[LV_ROWS][4];
#pragma unroll
    for (int r = 0; r < LV_ROWS; ++r) {
        const uint32_t rel = w0 + r * 256 + lane * 4;
        if (rel >= lo && rel + 4 <= hi) {
            const v4i_nt x = __builtin_nontemporal_load(reinterpret_cast<const v4i_nt *>(src + rel));
            c[r][0] = (uint32_t)x.x; c[r][1] = (uint32_t)x.y; c[r][2] = (uint32_t)x.z; c[r][3] = (uint32_t)x.w;
        } else {                                                 // the range's unaligned head and tail, and what lies outside
#pragma unroll
            for (int k = 0; k < 4; ++k) c[r][k] = (rel + k >= lo && rel + k < hi) ? src[rel + k] : 0u;
        }
    }
    uint32_t left_row = w0 > lo ? src[w0 - 1] : 0u;              // (w0 - 1 is inside [lo, hi) then)
    if (EDGES) left_row = level_search(left_row, s_edge, n_edges);
    uint32_t total = 0;
#pragma unroll
    for (int r = 0; r < LV_ROWS; ++r) {
        if (EDGES) {
            const uint32_t m = max(max(c[r][0], c[r][1]), max(c[r][2], c[r][3]));
            if (__ballot(m >= LV_LUT) == 0ull) {
#pragma unroll
                for (int k = 0; k < 4; ++k) c[r][k] = s_lut[c[r][k]];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) c[r][k] = level_search(c[r][k], s_edge, n_edges);
            }
        }
        const uint32_t rel = w0 + r * 256 + lane * 4;
        uint32_t left = (uint32_t)__shfl_up((int)c[r][3], 1);
        if (lane == 0) left = left_row;
        left_row = (uint32_t)__builtin_amdgcn_readlane((int)c[r][3], 63);
        bool f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t x = rel + k;
            f[k] = x >= lo && x < hi && (x == lo || c[r][k] != (k ? c[r][k - 1] : left));
        }
        if (!WRITE) {
#pragma unroll
            for (int k = 0; k < 4; ++k) total += (uint32_t)__popcll(__ballot(f[k]));
        } else {
            const uint32_t cnt = (uint32_t)f[0] + (uint32_t)f[1] + (uint32_t)f[2] + (uint32_t)f[3];
            if (__ballot(cnt != 0u) == 0ull) continue;
            const uint32_t incl = (uint32_t)wave_incl_scan((int)cnt);
            uint32_t o = run + incl - cnt;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (f[k]) { if (o < cap) out[o] = make_uint2(first_cell + rel + k, c[r][k]); ++o; }
            run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
    }
    if (!WRITE && lane == 0) wave_cnt[g] = total;
}

// exclusive scan of the waves' run counts: one workgroup, 16 consecutive entries per thread and round; off[n] = the total
__global__ __launch_bounds__(WG) void k_levels_scan(const uint32_t *cnt, uint32_t n, uint32_t *off)
{
    constexpr int PER = 16;
    __shared__ uint32_t wsum[WG / 64];
    __shared__ uint32_t carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n; b0 += WG * PER) {
        const uint32_t i0 = b0 + threadIdx.x * PER;
        uint32_t v[PER], mine = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { v[k] = i0 + k < n ? cnt[i0 + k] : 0u; mine += v[k]; }
        const uint32_t incl = (uint32_t)wave_incl_scan((int)mine);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t base = carry + incl - mine;
        for (int k = 0; k < wv; ++k) base += wsum[k];
#pragma unroll
        for (int k = 0; k < PER; ++k) { if (i0 + k < n) off[i0 + k] = base; base += v[k]; }
        __syncthreads();
        if (threadIdx.x == WG - 1) carry = base;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n] = carry;
}

// first_cell = the contig-local index of src[0], lo < 4.  write = false: the waves' run counts and their exclusive scan (wave_off[levels_waves(hi)] =
// the total); write = true: out[j] = (start, class) for j < cap.  wave_cnt: levels_waves(hi) words, wave_off: one more; edges: n_edges ascending device words.
static uint32_t levels_waves(uint64_t span) { return (uint32_t)((span + LV_WAVE - 1) / LV_WAVE + 3) / 4 * 4; }

static void launch_levels(hipStream_t st, const uint32_t *src, uint32_t first_cell, uint32_t lo, uint32_t hi, const uint32_t *edges, uint32_t n_edges,
                          uint32_t *wave_cnt, uint32_t *wave_off, uint2 *out, uint32_t cap, bool write)
{
    const uint32_t nw = levels_waves(hi), nb = nw / 4;
    if (!write) {
        if (n_edges) hipLaunchKernelGGL((k_levels<true, false>), dim3(nb), dim3(WG), 0, st, src, first_cell, lo, hi, edges, n_edges, wave_cnt, wave_off, out, cap);
        else hipLaunchKernelGGL((k_levels<false, false>), dim3(nb), dim3(WG), 0, st, src, first_cell, lo, hi, edges, n_edges, wave_cnt, wave_off, out, cap);
        hipLaunchKernelGGL(k_levels_scan, dim3(1), dim3(WG), 0, st, wave_cnt, nw, wave_off);
    } else {
        if (n_edges) hipLaunchKernelGGL((k_levels<true, true>), dim3(nb), dim3(WG), 0, st, src, first_cell, lo, hi, edges, n_edges, wave_cnt, wave_off, out, cap);
        else hipLaunchKernelGGL((k_levels<false, true>), dim3(nb), dim3(WG), 0, st, src, first_cell, lo, hi, edges, n_edges, wave_cnt, wave_off, out, cap);
    }
}

// ------------------------------------------------------------------------------------------
// depth quantiles (pd_depth_quantiles / pd_window_quantiles): exact nearest-rank order statistics of the cells of many rows.
// A row is a multiset of segments of the materialised depth (QRows: a segment list, or the windows of pd_window_layout(w) found
// on the device).  Three launch shapes, chosen per row by its cell count on the host:
//   k_quant_narrow        a GROUP of 8 .. 64 lanes per row: the cells go to LDS once, every rank is found by a bitwise radix
//                         descent from the highest bit set in the row (ballot + popcount per 64 cells and bit); exact for any uint32
//   k_quant_block<.., 0>  a workgroup per row: LDS histogram of min(v, 4095), block prefix, every rank picked from it
//   k_hist_pieces + k_quant_block<.., 1>   rows cut into pieces over many workgroups, added into the row's uint64 histogram in
//                         memory (the -dist kernel, one row of 4096 bins per quantile row), then a workgroup per row picks
// A rank that falls into the last bin (v >= 4095) is refined by the workgroup that found it (q_deep): three more passes over the
// row's cells, histograms of bits 31..20, 19..8 and 7..0 of the cells that are >= 4095 and share the bits fixed so far.
// ------------------------------------------------------------------------------------------
struct QSel { unsigned long long below[16], total, dbelow; uint32_t bin[16], dbin; };

// window g of pd_window_layout: the last contig whose first window is <= g, and the window's cells in it
__device__ __forceinline__ int q_win_contig(const QRows &R, uint64_t g)
{
    int lo = 0, hi = R.n_contigs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (R.win_off[mid] <= g) lo = mid; else hi = mid - 1; }
    return lo;
}
__device__ __forceinline__ void q_win_cells(const QRows &R, uint64_t g, int t, uint64_t *ws, uint32_t *wc)
{
    const uint64_t b = (g - R.win_off[t]) * R.w, clen = R.contig_len[t];
    *ws = R.contig_off[t] + b;
    *wc = b >= clen ? 0u : (uint32_t)(clen - b < (uint64_t)R.w ? clen - b : (uint64_t)R.w);
}

// the cells of row r: segments [s0, s0 + ns) of R.segs, or (window mode) the one stretch (ws, wc)
__device__ __forceinline__ void q_row_begin(const QRows &R, uint64_t r, uint64_t *s0, uint32_t *ns, uint64_t *ws, uint32_t *wc)
{
    if (R.segs) { *s0 = R.seg_off[r]; *ns = (uint32_t)(R.seg_off[r + 1] - *s0); *ws = 0; *wc = 0; return; }
    const uint64_t g = R.row0 + r;
    *s0 = 0; *ns = 1;
    q_win_cells(R, g, q_win_contig(R, g), ws, wc);
}
__device__ __forceinline__ void q_seg(const QRows &R, uint64_t s0, uint32_t i, uint64_t ws, uint32_t wc, uint64_t *start, uint32_t *count)
{
    if (R.segs) { const Piece pc = R.segs[s0 + i]; *start = pc.start; *count = pc.count; }
    else { *start = ws; *count = wc; }
}
__device__ __forceinline__ unsigned long long q_rank(uint32_t p, unsigned long long cells)
{
    const unsigned long long r = ((unsigned long long)p * cells + 99ull) / 100ull;
    return r ? r : 1ull;
}

__global__ __launch_bounds__(WG) void k_quant_narrow(const uint32_t *depth, const QRows R, const uint32_t *list, uint32_t n, uint32_t cap,
                                                     uint32_t gshift, const QPct P, uint32_t *q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t G = 1u << gshift, gl = threadIdx.x & (G - 1), grp = threadIdx.x >> gshift;
    const uint64_t slot = (uint64_t)blockIdx.x * (WG >> gshift) + grp;
    if (slot >= n) return;                                       // (whole groups leave; nothing below synchronises the workgroup)
    const uint64_t r = list ? list[slot] : slot;
    uint32_t *v = reinterpret_cast<uint32_t *>(smem) + (size_t)grp * cap;
    uint64_t s0, ws; uint32_t ns, wc;
    q_row_begin(R, r, &s0, &ns, &ws, &wc);
    uint32_t C = 0, any = 0;
    for (uint32_t i = 0; i < ns; ++i) {
        uint64_t start; uint32_t count;
        q_seg(R, s0, i, ws, wc, &start, &count);
        const uint32_t *d = depth + start;
        for (uint32_t k = gl; k < count && C + k < cap; k += G) { const uint32_t x = d[k]; v[C + k] = x; any |= x; }
        C += count;
    }
    if (C > cap) C = cap;                                        // (the host sends no such row here)
    __threadfence_block();                                       // the group's lanes read each other's cells: same wave, LDS writes drained
    for (uint32_t o = G >> 1; o; o >>= 1) any |= (uint32_t)__shfl_xor((int)any, (int)o);
    uint32_t *out = q + r * P.n;
    if (C == 0) { if (gl < P.n) out[gl] = 0xFFFFFFFFu; return; }
    const int hb = any ? 31 - __clz((int)any) : -1;
    const uint32_t gbase = (threadIdx.x & 63u) & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
    for (uint32_t j = 0; j < P.n; ++j) {
        uint32_t rank = (uint32_t)q_rank(P.p[j], C), prefix = 0;
        for (int bit = hb; bit >= 0; --bit) {
            uint32_t cnt = 0;                                    // cells that share the bits fixed so far and have this one clear
            for (uint32_t k0 = 0; k0 < C; k0 += G) {
                const uint32_t k = k0 + gl;
                const bool z = k < C && ((v[k] ^ prefix) >> bit) == 0;
                cnt += (uint32_t)__popcll((__ballot(z) >> gbase) & gmask);
            }
            if (rank > cnt) { rank -= cnt; prefix |= 1u << bit; }
        }
        if (gl == 0) out[j] = prefix;
    }
}

__device__ __forceinline__ unsigned long long q_block_scan(unsigned long long mine, unsigned long long *sc, unsigned long long *total)
{
    sc[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < WG; o <<= 1) {
        const unsigned long long a = (int)threadIdx.x >= o ? sc[threadIdx.x - o] : 0ull;
        __syncthreads();
        sc[threadIdx.x] += a;
        __syncthreads();
    }
    const unsigned long long incl = sc[threadIdx.x];
    *total = sc[WG - 1];
    __syncthreads();
    return incl;
}

// the thread whose `per` bins hold the r-th smallest writes the bin and the number of cells below it
template <typename T>
__device__ __forceinline__ void q_pick(const T *h, uint32_t per, unsigned long long excl, unsigned long long mine, unsigned long long r,
                                       uint32_t *bin, unsigned long long *below)
{
    if (r <= excl || r > excl + mine) return;
    unsigned long long acc = excl;
    for (uint32_t k = 0; k < per; ++k) {
        const unsigned long long x = h[threadIdx.x * per + k];
        if (r <= acc + x) { *bin = threadIdx.x * per + k; *below = acc; return; }
        acc += x;
    }
}

// the r-th smallest of the row's cells that are >= 4095 (whole workgroup; h: 4096 LDS counters)
template <typename T>
__device__ uint32_t q_deep(const uint32_t *depth, const QRows &R, uint64_t s0, uint32_t ns, uint64_t ws, uint32_t wc, unsigned long long r,
                           T *h, unsigned long long *sc, QSel *sel)
{
    uint32_t prefix = 0;
    for (int pass = 0; pass < 3; ++pass) {
        const uint32_t shift = pass == 0 ? 20u : pass == 1 ? 8u : 0u, nb = pass == 2 ? 256u : 4096u, fixed = pass == 1 ? 20u : 8u;
        for (uint32_t j = threadIdx.x; j < 4096; j += WG) h[j] = 0;
        __syncthreads();
        for (uint32_t i = 0; i < ns; ++i) {
            uint64_t start; uint32_t count;
            q_seg(R, s0, i, ws, wc, &start, &count);
            const uint32_t *d = depth + start;
            for (uint32_t k = threadIdx.x; k < count; k += WG) {
                const uint32_t x = d[k];
                if (x >= 4095u && (pass == 0 || (x >> fixed) == (prefix >> fixed))) atomicAdd(&h[(x >> shift) & (nb - 1)], (T)1);
            }
        }
        lds_drain();
        __syncthreads();
        const uint32_t per = nb / WG;
        unsigned long long mine = 0, total;
        for (uint32_t k = 0; k < per; ++k) mine += h[threadIdx.x * per + k];
        const unsigned long long incl = q_block_scan(mine, sc, &total);
        q_pick(h, per, incl - mine, mine, r, &sel->dbin, &sel->dbelow);
        __syncthreads();
        prefix |= sel->dbin << shift;
        r -= sel->dbelow;
        __syncthreads();
    }
    return prefix;
}

// A workgroup per row.  FROM_HIST: the row's 4096 uint64 bins are in memory already (ghist + slot * 4096); else they are counted here.
template <typename T, bool FROM_HIST>
__global__ __launch_bounds__(WG) void k_quant_block(const uint32_t *depth, const QRows R, const uint32_t *list, const QPct P, uint32_t *q,
                                                    const unsigned long long *ghist)
{
    __shared__ T h[4096];
    __shared__ unsigned long long sc[WG];
    __shared__ QSel sel;
    const int lane = threadIdx.x & 63;
    const uint64_t r = list ? list[blockIdx.x] : blockIdx.x;
    uint64_t s0, ws; uint32_t ns, wc;
    q_row_begin(R, r, &s0, &ns, &ws, &wc);
    const T *src = h;
    if constexpr (FROM_HIST) src = reinterpret_cast<const T *>(ghist) + (size_t)blockIdx.x * 4096;
    else {
        for (uint32_t j = threadIdx.x; j < 4096; j += WG) h[j] = 0;
        __syncthreads();
        for (uint32_t i = 0; i < ns; ++i) {
            uint64_t start; uint32_t count;
            q_seg(R, s0, i, ws, wc, &start, &count);
            const uint32_t *d = depth + start;
            for (uint32_t base = 0; base < count; base += WG * 4) {
                const uint32_t c0 = base + threadIdx.x * 4;
                const uint32_t n = c0 >= count ? 0u : (count - c0 < 4u ? count - c0 : 4u);
                uint32_t b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = (uint32_t)k < n ? min(d[c0 + k], 4095u) : 0u;
                hist_lane4<true>(reinterpret_cast<uint32_t *>(h), b, n, lane);
            }
        }
        lds_drain();
        __syncthreads();
    }
    unsigned long long mine = 0, total;
    for (uint32_t k = 0; k < 16; ++k) mine += src[threadIdx.x * 16 + k];
    const unsigned long long incl = q_block_scan(mine, sc, &total);
    uint32_t *out = q + r * P.n;
    if (total == 0) { if (threadIdx.x < P.n) out[threadIdx.x] = 0xFFFFFFFFu; return; }
    for (uint32_t j = 0; j < P.n; ++j) q_pick(src, 16, incl - mine, mine, q_rank(P.p[j], total), &sel.bin[j], &sel.below[j]);
    __syncthreads();
    unsigned long long last_r = 0; uint32_t last_v = 0;
    for (uint32_t j = 0; j < P.n; ++j) {
        uint32_t val = sel.bin[j];
        if (val == 4095u) {                                      // cells >= 4095: refine (uniform over the workgroup; q_deep leaves bin[] / below[] alone)
            const unsigned long long rd = q_rank(P.p[j], total) - sel.below[j];
            if (rd != last_r) { last_v = q_deep<T>(depth, R, s0, ns, ws, wc, rd, h, sc, &sel); last_r = rd; }
            val = last_v;
        }
        if (threadIdx.x == 0) out[j] = val;
    }
}

static int launch_quant_narrow(hipStream_t st, const int *depth, const QRows &R, const uint32_t *list, uint32_t n, uint32_t cap, uint32_t gshift,
                               const QPct &P, uint32_t *q)
{
    if (!n) return 0;
    if (cap < 1) cap = 1;
    const uint32_t gpb = (uint32_t)WG >> gshift;
    const size_t lds = (size_t)gpb * cap * 4;
    if (int e = hist_lds_reserve(k_quant_narrow, lds)) return e;
    hipLaunchKernelGGL(k_quant_narrow, dim3((n + gpb - 1) / gpb), dim3(WG), lds, st, reinterpret_cast<const uint32_t *>(depth), R, list, n, cap, gshift, P, q);
    return 0;
}

static void launch_quant_block(hipStream_t st, const int *depth, const QRows &R, const uint32_t *list, uint32_t n, const QPct &P, uint32_t *q,
                               const unsigned long long *ghist)
{
    if (!n) return;
    const uint32_t *d = reinterpret_cast<const uint32_t *>(depth);
    if (ghist) hipLaunchKernelGGL((k_quant_block<unsigned long long, true>), dim3(n), dim3(WG), 0, st, d, R, list, P, q, ghist);
    else hipLaunchKernelGGL((k_quant_block<uint32_t, false>), dim3(n), dim3(WG), 0, st, d, R, list, P, q, ghist);
}

// ------------------------------------------------------------------------------------------
// depth thresholds (pd_depth_thresholds / pd_window_thresholds): for every row (QRows, as the quantiles have them) the number of
// cells >= T.t[j], j < T.n.  A cell is read once; a lane keeps NT counters in registers (NT = 1, 4 or 16, the thresholds padded
// with 2^32-1 and the padding's counters never written), the thresholds sit in scalar registers.  A stretch of cells is read by
// thr_span: scalar head to the first 16-byte boundary, 16-byte loads (four in flight per lane), scalar tail.  Two launch shapes:
//   k_thr_narrow   a GROUP of 8 .. 64 lanes per row, many rows per wave, `rpg` consecutive rows per group one after the other (a
//                  window's contig is found by bisection for the group's first row and by stepping for the rest); the group's
//                  counters are summed with __shfl_xor and the row has one writer (no atomics, the result need not be zeroed)
//   k_thr_pieces   rows cut into pieces of at most 16384 cells (Piece.region = the row's slot); a WAVE per piece, every wave of
//                  `grid` workgroups takes a run of consecutive pieces; at the end of a row's pieces the wave's counters are summed
//                  with __shfl_xor and added to the zeroed result row with T.n atomics
// ------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ void thr_count(uint32_t v, const ThrSet &T, uint32_t (&cnt)[NT])
{
#pragma unroll
    for (int j = 0; j < NT; ++j) cnt[j] += v >= T.t[j] ? 1u : 0u;
}
template <int NT>
__device__ __forceinline__ void thr_count4(const uint4 x, const ThrSet &T, uint32_t (&cnt)[NT])
{
    thr_count<NT>(x.x, T, cnt); thr_count<NT>(x.y, T, cnt); thr_count<NT>(x.z, T, cnt); thr_count<NT>(x.w, T, cnt);
}

// cells d[0 .. count) by lanes gl = 0 .. G - 1 (G >= 4); d is a cell of the depth array, whose base is 16-byte aligned
template <int NT>
__device__ __forceinline__ void thr_span(const uint32_t *d, uint32_t count, uint32_t gl, uint32_t G, const ThrSet &T, uint32_t (&cnt)[NT])
{
    uint32_t head = (4u - (uint32_t)((reinterpret_cast<uintptr_t>(d) >> 2) & 3u)) & 3u;     // cells before the first 16-byte boundary
    if (head > count) head = count;
    const uint32_t n4 = (count - head) >> 2, tail0 = head + (n4 << 2);
    if (gl < head) thr_count<NT>(d[gl], T, cnt);
    const uint4 *d4 = reinterpret_cast<const uint4 *>(d + head);
    for (uint32_t k0 = 0; k0 < n4; k0 += 4 * G) {               // the same trips for every lane of the group; a lane past the end reads d4[0] and skips the count
        const uint32_t k = k0 + gl;
        const bool ok0 = k < n4, ok1 = k + G < n4, ok2 = k + 2 * G < n4, ok3 = k + 3 * G < n4;
        const uint4 x0 = d4[ok0 ? k : 0u], x1 = d4[ok1 ? k + G : 0u], x2 = d4[ok2 ? k + 2 * G : 0u], x3 = d4[ok3 ? k + 3 * G : 0u];
        if (ok0) thr_count4<NT>(x0, T, cnt);
        if (ok1) thr_count4<NT>(x1, T, cnt);
        if (ok2) thr_count4<NT>(x2, T, cnt);
        if (ok3) thr_count4<NT>(x3, T, cnt);
    }
    if (tail0 + gl < count) thr_count<NT>(d[tail0 + gl], T, cnt);                           // (fewer than 4 cells)
}

template <int NT, typename OutT>
__global__ __launch_bounds__(WG) void k_thr_narrow(const uint32_t *depth, const QRows R, const uint32_t *list, uint32_t n, uint32_t gshift,
                                                   uint32_t rpg, const ThrSet T, OutT *out)
{
    const uint32_t G = 1u << gshift, gl = threadIdx.x & (G - 1);
    const uint64_t slot0 = ((uint64_t)blockIdx.x * (WG >> gshift) + (threadIdx.x >> gshift)) * rpg;
    int t = -1;                                                  // window mode: the contig of the row before
    for (uint32_t i = 0; i < rpg; ++i) {
        const uint64_t slot = slot0 + i;
        if (slot >= n) break;                                    // (whole groups leave; nothing below synchronises the workgroup)
        const uint64_t r = list ? list[slot] : slot;
        uint32_t cnt[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) cnt[j] = 0;
        if (R.segs) {
            const uint64_t s0 = R.seg_off[r], s1 = R.seg_off[r + 1];
            for (uint64_t s = s0; s < s1; ++s) { const Piece pc = R.segs[s]; thr_span<NT>(depth + pc.start, pc.count, gl, G, T, cnt); }
        } else {
            const uint64_t g = R.row0 + r;
            if (t < 0) t = q_win_contig(R, g);
            else while (R.win_off[t + 1] <= g) ++t;              // (g is below win_off[n_contigs]: t stays a contig)
            uint64_t ws; uint32_t wc;
            q_win_cells(R, g, t, &ws, &wc);
            thr_span<NT>(depth + ws, wc, gl, G, T, cnt);
        }
        OutT *o = out + r * T.n;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            int x = (int)cnt[j];                                 // (constant distances: the first steps are DPP moves)
            if (G > 32) x += __shfl_xor(x, 32);
            if (G > 16) x += __shfl_xor(x, 16);
            if (G > 8) x += __shfl_xor(x, 8);
            x += __shfl_xor(x, 4); x += __shfl_xor(x, 2); x += __shfl_xor(x, 1);
            if ((uint32_t)j < T.n && gl == (uint32_t)j % G) o[j] = (OutT)x;
        }
    }
}

template <int NT, typename OutT>
__device__ __forceinline__ void thr_add_row(uint32_t (&cnt)[NT], uint32_t lane, const ThrSet &T, OutT *o)
{
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const uint32_t x = (uint32_t)wave_sum((int)cnt[j]);
        if ((uint32_t)j < T.n && lane == (uint32_t)j && x) atomicAdd(&o[j], (OutT)x);
        cnt[j] = 0;
    }
}

// wave k of the grid takes pieces [k * ppw, (k + 1) * ppw): consecutive pieces of one row are added to it once
template <int NT, typename OutT>
__global__ __launch_bounds__(WG) void k_thr_pieces(const uint32_t *depth, const Piece *pieces, uint32_t n_pieces, uint32_t ppw, const ThrSet T, OutT *out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p0 = ((uint64_t)blockIdx.x * (WG / 64) + (threadIdx.x >> 6)) * ppw;
    if (p0 >= n_pieces) return;
    const uint32_t p1 = (uint32_t)(p0 + ppw < n_pieces ? p0 + ppw : n_pieces);
    uint32_t cnt[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) cnt[j] = 0;
    uint32_t cur = pieces[p0].region;
    for (uint32_t pi = (uint32_t)p0; pi < p1; ++pi) {
        const Piece pc = pieces[pi];
        if (pc.region != cur) { thr_add_row<NT>(cnt, lane, T, out + (size_t)cur * T.n); cur = pc.region; }
        thr_span<NT>(depth + pc.start, pc.count, lane, 64u, T, cnt);
    }
    thr_add_row<NT>(cnt, lane, T, out + (size_t)cur * T.n);
}

template <typename OutT>
static void thr_narrow_any(hipStream_t st, const int *depth, const QRows &R, const uint32_t *list, uint32_t n, uint32_t gshift, uint32_t rpg, const ThrSet &T, OutT *out)
{
    if (!n) return;
    if (rpg < 1) rpg = 1;
    const uint32_t rpb = ((uint32_t)WG >> gshift) * rpg;         // rows per workgroup
    const dim3 grid((n + rpb - 1) / rpb);
    const uint32_t *d = reinterpret_cast<const uint32_t *>(depth);
    if (T.n == 1) hipLaunchKernelGGL((k_thr_narrow<1, OutT>), grid, dim3(WG), 0, st, d, R, list, n, gshift, rpg, T, out);
    else if (T.n <= 4) hipLaunchKernelGGL((k_thr_narrow<4, OutT>), grid, dim3(WG), 0, st, d, R, list, n, gshift, rpg, T, out);
    else hipLaunchKernelGGL((k_thr_narrow<16, OutT>), grid, dim3(WG), 0, st, d, R, list, n, gshift, rpg, T, out);
}
template <typename OutT>
static void thr_pieces_any(hipStream_t st, const int *depth, const Piece *pieces, uint32_t n_pieces, const ThrSet &T, OutT *out, unsigned grid)
{
    if (!n_pieces) return;
    if (grid < 1) grid = 1;
    const uint32_t waves = grid * (WG / 64), ppw = (n_pieces + waves - 1) / waves;           // pieces per wave
    const dim3 g((n_pieces + ppw * (WG / 64) - 1) / (ppw * (WG / 64)));
    const uint32_t *d = reinterpret_cast<const uint32_t *>(depth);
    if (T.n == 1) hipLaunchKernelGGL((k_thr_pieces<1, OutT>), g, dim3(WG), 0, st, d, pieces, n_pieces, ppw, T, out);
    else if (T.n <= 4) hipLaunchKernelGGL((k_thr_pieces<4, OutT>), g, dim3(WG), 0, st, d, pieces, n_pieces, ppw, T, out);
    else hipLaunchKernelGGL((k_thr_pieces<16, OutT>), g, dim3(WG), 0, st, d, pieces, n_pieces, ppw, T, out);
}

// (overloads, not calls of the templates: the order in which the kernel templates are first instantiated — here, uint32 before uint64, narrow before pieces — changes register numbering)
static void launch_thr_narrow(hipStream_t st, const int *depth, const QRows &R, const uint32_t *list, uint32_t n, uint32_t gshift, uint32_t rpg, const ThrSet &T, uint32_t *out)
{ thr_narrow_any(st, depth, R, list, n, gshift, rpg, T, out); }
static void launch_thr_narrow(hipStream_t st, const int *depth, const QRows &R, const uint32_t *list, uint32_t n, uint32_t gshift, uint32_t rpg, const ThrSet &T, unsigned long long *out)
{ thr_narrow_any(st, depth, R, list, n, gshift, rpg, T, out); }
static void launch_thr_pieces(hipStream_t st, const int *depth, const Piece *pieces, uint32_t n_pieces, const ThrSet &T, uint32_t *out, unsigned grid)
{ thr_pieces_any(st, depth, pieces, n_pieces, T, out, grid); }
static void launch_thr_pieces(hipStream_t st, const int *depth, const Piece *pieces, uint32_t n_pieces, const ThrSet &T, unsigned long long *out, unsigned grid)
{ thr_pieces_any(st, depth, pieces, n_pieces, T, out, grid); }

} // namespace pdk

// ---- the host side: what the entry points below share ----
namespace {
using namespace pdrows;

// c->scratch handed out front to back.  A call states its regions once, as a plan of take()s (it rounds the sizes itself); carve() runs the plan to size the
// buffer, with `tail` spare bytes behind the last region, and once more to set the pointers.
struct Carver {
    uintptr_t base = 0; size_t used = 0;
    template <class T> void take(T *&p, size_t bytes) { p = reinterpret_cast<T *>(base + used); used += bytes; }
};
template <class Plan> int carve(pd_ctx *c, size_t tail, Plan &&plan)
{
    Carver size; plan(size);
    if (int rc = ensure_scratch(c, size.used + tail)) return rc;
    Carver place; place.base = (uintptr_t)c->scratch; plan(place);
    return PD_OK;
}

inline Span seg_cells(const pd_ctx *c, const pd_region &r)      // a segment's cells, clipped to its contig: Span.start is the flat cell
{
    const Span s = seg_clip(r.first, r.second, c->len[(size_t)r.tid]);
    return Span{c->off[(size_t)r.tid] + s.start, s.count};
}
inline void cut_into(std::vector<Piece> &v, uint64_t start, uint64_t count, uint32_t slot)
{
    cut_pieces(start, count, slot, PIECE_CELLS, [&](uint64_t s, uint32_t n, uint32_t sl) { v.push_back(Piece{s, n, sl}); return 0; });
}

// The one piece feed of the quantiles and thresholds: the pieces on the host, their place in the scratch, and the flush — up they go, the stream is
// waited for (the host vector is refilled), Call::pieces(pieces, n) adds them into the statistic's rows (Piece.region = the row's slot there).
template <class Call> struct PieceFeed {
    pd_ctx *c; Piece *d_pc = nullptr; Feed<Piece> feed{FLUSH_PIECES};
    explicit PieceFeed(pd_ctx *ctx) : c(ctx) {}
    int flush(std::vector<Piece> &held)
    {
        HIPOK(c, hipMemcpyAsync(d_pc, held.data(), held.size() * sizeof(Piece), hipMemcpyHostToDevice, c->stream));
        HIPOK(c, hipStreamSynchronize(c->stream));
        if (int rc = static_cast<Call *>(this)->pieces(d_pc, (uint32_t)held.size())) return rc;
        HIPOK(c, hipGetLastError());
        return PD_OK;
    }
    int add(uint64_t start, uint64_t count, uint32_t slot) { return feed.add(start, count, slot, [this](std::vector<Piece> &h) { return flush(h); }); }
    int finish() { return feed.finish([this](std::vector<Piece> &h) { return flush(h); }); }
};

// The batch at hand: the rows one round of launches takes, and where their results go (rows [row0, row0 + n_rows) of the call).  windows_serve: the windows of the layout
// `wo`, all of one shape, no lists.  rows_serve: their clipped segments, the segment offsets and the rows of every launch shape by their number in the batch, on the host and in the scratch.
struct RowBatch {
    QRows R{}; size_t row0 = 0, n_rows = 0;
    uint32_t n[3] = {0, 0, 0}; uint32_t *d_list[3] = {nullptr, nullptr, nullptr};    // the rows of shape 0 .. 2, and which they are (null: rows 0 .. n - 1)
    uint32_t cap = 0, gshift = 6, rpg = 1;                       // narrow launches: the largest row of shape 0, the group's lanes, the rows a group takes
    const uint64_t *wo = nullptr; int32_t t = 0;                 // windows: the layout, the contig of the window walked last
    Piece *d_seg = nullptr; uint64_t *d_off = nullptr;
    std::vector<Piece> hseg; std::vector<uint64_t> hoff; std::vector<uint32_t> list[3];
    void take(Carver &S, size_t rows, size_t segs)
    {
        S.take(d_seg, al256(std::min<size_t>(SEG_BATCH, segs) * sizeof(Piece)));
        S.take(d_off, al256((std::min(ROW_BATCH, rows) + 1) * 8));
        for (auto &d : d_list) S.take(d, al256(std::min(ROW_BATCH, rows) * 4));
    }
    // rows k0 .. k1 - 1 of shape 2, upwards: f(k, the row's number in the batch, first flat cell, cells) per cell span, 0 to go on (millions of windows a call: the loop's state is in locals)
    template <class F> int wide_spans(const pd_ctx *c, uint32_t k0, uint32_t k1, F &&f)
    {
        const uint32_t *len = c->len.data(); const uint64_t *off = c->off.data(), *wl = wo, g0 = R.row0; const uint32_t w = R.w; int32_t tt = t;
        for (uint32_t k = k0; wl && k < k1; ++k) { const Span s = win_span(wl, len, w, g0 + k, &tt); if (int rc = f(k, k, off[tt] + s.start, s.count)) return rc; }
        for (uint32_t k = k0; !wl && k < k1; ++k)
            for (uint64_t r = list[2][k], j = hoff[r]; j < hoff[r + 1]; ++j)
                if (int rc = f(k, (uint32_t)r, hseg[j].start, (uint64_t)hseg[j].count)) return rc;
        t = tt;
        return 0;
    }
};

// windows [0, nw) of width w in batches of BR, every one of launch shape `shape`; serve() launches over the batch in B and brings its results back
template <class Serve>
int windows_serve(pd_ctx *c, uint32_t w, const std::vector<uint64_t> &wo, const uint64_t *d_wo, uint64_t nw, uint64_t BR, int shape, RowBatch &B, Serve serve)
{
    B.wo = wo.data();
    for (uint64_t row0 = 0; row0 < nw; row0 += BR) {
        B.row0 = row0; B.n_rows = (size_t)std::min<uint64_t>(BR, nw - row0);
        B.n[shape] = (uint32_t)B.n_rows;
        B.R = QRows{nullptr, nullptr, d_wo, c->d_off, c->d_len, row0, w, c->n_contigs};
        if (int rc = serve()) return rc;
    }
    return PD_OK;
}
inline uint32_t win_weff(const pd_ctx *c, uint32_t w) { return std::min(w, c->len.empty() ? 0u : *std::max_element(c->len.begin(), c->len.end())); }   // the widest window there is

// What pd_depth_quantiles and pd_depth_thresholds share: the checks of a row list, the rows' cells, and the batches in which they go up.
int rows_check(pd_ctx *c, const char *fn, const pd_region *segs, size_t n_segs, const uint64_t *row_off, size_t n_rows)
{
    const std::string f(fn);
    if (row_off[0] != 0 || row_off[n_rows] != n_segs) return fail(c, PD_EINVAL, f + ": row_off must run from 0 to n_segs");
    for (size_t i = 0; i < n_rows; ++i) {
        if (row_off[i + 1] < row_off[i] || row_off[i + 1] > n_segs) return fail(c, PD_EINVAL, f + ": row_off must not decrease");
        if (row_off[i + 1] - row_off[i] > SEG_BATCH) return fail(c, PD_EINVAL, f + ": at most 2^21 segments per row");
    }
    for (size_t i = 0; i < n_segs; ++i)
        if (segs[i].tid < 0 || segs[i].tid >= c->n_contigs) return fail(c, PD_EINVAL, f + ": contig id out of range");
    return PD_OK;
}

// cells[i] = the cells of row i; the rows of shape 2 and the pieces they will be cut into
void rows_measure(const pd_ctx *c, const pd_region *segs, const uint64_t *row_off, size_t n_rows, uint32_t wave_max, uint32_t split, uint64_t *cells, size_t *n_wide, uint64_t *wide_pieces)
{
    *n_wide = 0; *wide_pieces = 0;
    for (size_t i = 0; i < n_rows; ++i) {
        uint64_t C = 0, np = 0;
        for (uint64_t k = row_off[i]; k < row_off[i + 1]; ++k) { const uint64_t cn = seg_cells(c, segs[k]).count; C += cn; np += piece_count(cn); }
        cells[i] = C;
        if (row_shape(C, wave_max, split) == 2) { ++*n_wide; *wide_pieces += np; }
    }
}

template <class Serve>
int rows_serve(pd_ctx *c, const pd_region *segs, const uint64_t *row_off, size_t n_rows, const uint64_t *cells, uint32_t wave_max, uint32_t split, RowBatch &B, Serve serve)
{
    for (size_t r0 = 0; r0 < n_rows;) {
        const size_t r1 = batch_end(row_off, n_rows, r0, ROW_BATCH, SEG_BATCH);
        B.row0 = r0; B.n_rows = r1 - r0; B.cap = 0;
        B.hseg.clear(); B.hoff.clear(); for (auto &l : B.list) l.clear();
        for (size_t i = r0; i < r1; ++i) {
            B.hoff.push_back(B.hseg.size());
            for (uint64_t k = row_off[i]; k < row_off[i + 1]; ++k) {
                const Span sp = seg_cells(c, segs[k]);
                B.hseg.push_back(Piece{sp.start, (uint32_t)sp.count, 0});
            }
            const int rg = row_shape(cells[i], wave_max, split);
            if (rg == 0) B.cap = std::max(B.cap, (uint32_t)cells[i]);
            B.list[rg].push_back((uint32_t)(i - r0));
        }
        B.hoff.push_back(B.hseg.size());
        if (!B.hseg.empty()) HIPOK(c, hipMemcpyAsync(B.d_seg, B.hseg.data(), B.hseg.size() * sizeof(Piece), hipMemcpyHostToDevice, c->stream));
        HIPOK(c, hipMemcpyAsync(B.d_off, B.hoff.data(), B.hoff.size() * 8, hipMemcpyHostToDevice, c->stream));
        for (int k = 0; k < 3; ++k) {
            B.n[k] = (uint32_t)B.list[k].size();
            if (B.n[k]) HIPOK(c, hipMemcpyAsync(B.d_list[k], B.list[k].data(), B.list[k].size() * 4, hipMemcpyHostToDevice, c->stream));
        }
        HIPOK(c, hipStreamSynchronize(c->stream));          // the host arrays are refilled by the next batch
        B.R = QRows{B.d_seg, B.d_off, nullptr, c->d_off, c->d_len, 0, 0, c->n_contigs};
        if (int rc = serve()) return rc;
        r0 = r1;
    }
    return PD_OK;
}

// ---- depth histograms ----  The rows go to a zeroed uint64 array at the front of the scratch buffer, the kernels add into it, the host gets it
// back.  Grid: eight workgroups per CU, each a run of tiles / pieces (one flush of its non-zero bins per contig).
int hist_finish(pd_ctx *c, uint64_t *d_hist, size_t b_hist, uint64_t *hist)
{
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipMemcpyAsync(hist, d_hist, b_hist, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    return PD_OK;
}
// whole contigs: the histogram sweep (int4 rows) over the depth, or (from_depth false) over the difference arrays behind the tile carries
int hist_sweep(pd_ctx *c, const char *name, bool from_depth, uint32_t mask, uint32_t n_bins, uint64_t *hist)
{
    const size_t b_hist = (size_t)c->n_contigs * n_bins * 8;
    if (int rc = ensure_scratch(c, b_hist + 64)) return rc;
    uint64_t *d_hist = (uint64_t *)c->scratch;
    HIPOK(c, hipMemsetAsync(d_hist, 0, b_hist, c->stream));
    if (!from_depth) { ProfScope ps(c, "tile_carry"); launch_tile_carry(c->stream, c->sums, c->bsum, c->carry, (uint32_t)c->n_tiles); }
    {
        ProfScope ps(c, name);
        TileMap tm{c->d_tile_contig, c->d_off, c->d_len, nullptr};
        if (launch_sweep_hist(c->stream, c->buf, from_depth ? nullptr : c->carry, (uint32_t)c->n_tiles, mask, tm, from_depth ? nullptr : c->hstate, from_depth, n_bins,
                              (unsigned long long *)d_hist, (unsigned)c->n_cu * 8, c->hist_variant))
            return fail(c, PD_EHIP, "histogram sweep: cannot reserve LDS");
    }
    return hist_finish(c, d_hist, b_hist, hist);
}

// ---- depth quantiles ----
// Rows go to the device in batches whose scratch does not grow with the row count: at most 2^20 rows (2^22 windows) and 2^21
// segments a batch, 1024 histogram rows and 2^21 pieces a wide launch.  A row takes the narrow kernel up to "quantile_wave_max"
// cells, the workgroup kernel up to "quantile_split_cells", and is cut into pieces over many workgroups above that.
int quant_pct(pd_ctx *c, const uint32_t *pct, uint32_t n_pct, const char *fn, QPct *P)
{
    if (!pct || n_pct < 1 || n_pct > 16) return fail(c, PD_EINVAL, std::string(fn) + ": 1 to 16 percentages");
    P->n = n_pct;
    for (uint32_t j = 0; j < 16; ++j) P->p[j] = 0;
    for (uint32_t j = 0; j < n_pct; ++j) {
        if (pct[j] > 100 || (j && pct[j] <= pct[j - 1])) return fail(c, PD_EINVAL, std::string(fn) + ": percentages must be 0..100, strictly ascending");
        P->p[j] = pct[j];
    }
    return PD_OK;
}

// the quantile shapes over a batch: d_q = the batch's results, d_hist = the histograms of one wide launch (Piece.region = the row's number in it)
struct QuantCall : PieceFeed<QuantCall> {
    QPct P; uint32_t *q; uint32_t *d_q = nullptr; unsigned long long *d_hist = nullptr;
    QuantCall(pd_ctx *ctx, uint32_t *out) : PieceFeed(ctx), q(out) {}
    int pieces(const Piece *p, uint32_t n)
    {
        ProfScope ps(c, "quantile_pieces");
        if (launch_hist_pieces(c->stream, c->buf, p, n, 4096, d_hist, (unsigned)c->n_cu * 8, c->hist_variant))
            return fail(c, PD_EHIP, "quantile histograms: cannot reserve LDS");
        return PD_OK;
    }
    int serve(RowBatch &B)
    {
        if (B.n[0]) {
            ProfScope ps(c, "quantile_narrow");
            if (launch_quant_narrow(c->stream, c->buf, B.R, B.d_list[0], B.n[0], B.cap, B.gshift, P, d_q)) return fail(c, PD_EHIP, "quantile kernel: cannot reserve LDS");
        }
        if (B.n[1]) {
            ProfScope ps(c, "quantile_block");
            launch_quant_block(c->stream, c->buf, B.R, B.d_list[1], B.n[1], P, d_q, nullptr);
        }
        for (uint32_t w0 = 0; w0 < B.n[2]; w0 += WIDE_ROWS) {
            const uint32_t nwr = std::min(WIDE_ROWS, B.n[2] - w0);
            HIPOK(c, hipMemsetAsync(d_hist, 0, (size_t)nwr * 4096 * 8, c->stream));
            if (int rc = B.wide_spans(c, w0, w0 + nwr, [&](uint32_t k, uint32_t, uint64_t st, uint64_t cn) { return add(st, cn, k - w0); })) return rc;
            if (int rc = finish()) return rc;
            ProfScope ps(c, "quantile_pick");
            launch_quant_block(c->stream, c->buf, B.R, B.d_list[2] ? B.d_list[2] + w0 : nullptr, nwr, P, d_q, d_hist);
        }
        HIPOK(c, hipGetLastError());
        HIPOK(c, hipMemcpyAsync(q + B.row0 * P.n, d_q, B.n_rows * P.n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPOK(c, hipStreamSynchronize(c->stream));
        return PD_OK;
    }
};

// ---- depth thresholds ----
// The quantiles' rows and batches with two launch shapes: a row of up to "threshold_wave_max" cells is counted by a group of
// lanes, a longer one is cut into pieces that add into the batch's zeroed result rows.
int thr_set(pd_ctx *c, const uint32_t *thr, uint32_t n_thr, const char *fn, ThrSet *T)
{
    if (!thr || n_thr < 1 || n_thr > 16) return fail(c, PD_EINVAL, std::string(fn) + ": 1 to 16 thresholds");
    T->n = n_thr;
    for (uint32_t j = 0; j < 16; ++j) T->t[j] = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < n_thr; ++j) {
        if (j && thr[j] <= thr[j - 1]) return fail(c, PD_EINVAL, std::string(fn) + ": thresholds must be strictly ascending");
        T->t[j] = thr[j];
    }
    return PD_OK;
}

// the threshold shapes over a batch: d_cnt = the batch's results (Piece.region = the row's number in the batch), OutT wide as the caller's counts
template <typename OutT> struct ThrCall : PieceFeed<ThrCall<OutT>> {
    using Base = PieceFeed<ThrCall<OutT>>; using Base::c;
    ThrSet T; void *counts; OutT *d_cnt = nullptr;
    ThrCall(pd_ctx *ctx, void *out) : Base(ctx), counts(out) {}
    int pieces(const Piece *p, uint32_t n)
    {
        ProfScope ps(c, "threshold_pieces");
        launch_thr_pieces(c->stream, c->buf, p, n, T, d_cnt, (unsigned)c->n_cu * 8);
        return PD_OK;
    }
    int serve(RowBatch &B)
    {
        const size_t bytes = B.n_rows * T.n * sizeof(OutT);
        if (B.n[2]) HIPOK(c, hipMemsetAsync(d_cnt, 0, bytes, c->stream));       // (the narrow rows are written, not added to)
        if (B.n[0]) {
            ProfScope ps(c, "threshold_narrow");
            launch_thr_narrow(c->stream, c->buf, B.R, B.d_list[0], B.n[0], B.gshift, B.rpg, T, d_cnt);
        }
        if (int rc = B.wide_spans(c, 0, B.n[2], [&](uint32_t, uint32_t row, uint64_t st, uint64_t cn) { return this->add(st, cn, row); })) return rc;
        if (int rc = this->finish()) return rc;
        HIPOK(c, hipGetLastError());
        HIPOK(c, hipMemcpyAsync((unsigned char *)counts + B.row0 * T.n * sizeof(OutT), d_cnt, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPOK(c, hipStreamSynchronize(c->stream));
        return PD_OK;
    }
};
} // namespace

extern "C" {

int pd_scan_depth_histogram(pd_ctx *c, uint32_t n_bins, unsigned wrap_bits, uint64_t *hist)
{
    if (!c || !hist || n_bins < 2 || n_bins > 4097 || wrap_bits > 32) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 0, "pd_scan_depth_histogram")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    if (int rc = flush_pending(c)) return rc;                    // a deferred sample is materialised (later calls see it as before)
    if (int rc = check_words(c)) return rc;
    return hist_sweep(c, "scan_depth_histogram", false, pdwin::wrap_mask(wrap_bits), n_bins, hist);
}

int pd_depth_histogram(pd_ctx *c, const pd_region *regs, size_t n, uint32_t n_bins, uint64_t *hist)
{
    if (!c || !hist || (n && !regs) || n_bins < 2 || n_bins > 4097) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_depth_histogram")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    if (!regs || n == 0) return hist_sweep(c, "depth_histogram", true, 0xFFFFFFFFu, n_bins, hist);
    const size_t b_hist = (size_t)c->n_contigs * n_bins * 8;
    // regions: checked, clipped to [0, len), cut into pieces (Piece.region = the contig)
    std::vector<Piece> pieces;
    pieces.reserve(n + n / 8);
    int32_t prev_tid = -1; int64_t prev_first = 0, prev_end = 0;
    for (size_t i = 0; i < n; ++i) {
        const pd_region &r = regs[i];
        if (r.tid < 0 || r.tid >= c->n_contigs) return fail(c, PD_EINVAL, "pd_depth_histogram: contig id out of range");
        const int64_t b0 = (int64_t)r.first - 1, e0 = r.second;
        if (r.tid < prev_tid || (r.tid == prev_tid && r.first < prev_first))
            return fail(c, PD_EINVAL, "pd_depth_histogram: regions not sorted by (tid, first)");
        if (r.tid != prev_tid) prev_end = INT64_MIN;
        if (e0 > b0) {
            if (b0 < prev_end) return fail(c, PD_EINVAL, "pd_depth_histogram: regions overlap");
            prev_end = e0;
        }
        prev_tid = r.tid; prev_first = r.first;
        const Span sp = seg_cells(c, r);
        cut_into(pieces, sp.start, sp.count, (uint32_t)r.tid);
    }
    if (pieces.size() > 0xFFFFFFF0ull) return fail(c, PD_EINVAL, "pd_depth_histogram: too many regions");
    const size_t b_p = pieces.size() * sizeof(Piece);
    uint64_t *d_hist; Piece *d_p;
    if (int rc = carve(c, 64, [&](Carver &S) { S.take(d_hist, (b_hist + 15) / 16 * 16); S.take(d_p, b_p); })) return rc;
    HIPOK(c, hipMemsetAsync(d_hist, 0, b_hist, c->stream));
    if (!pieces.empty()) HIPOK(c, hipMemcpyAsync(d_p, pieces.data(), b_p, hipMemcpyHostToDevice, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));          // pieces is a local
    {
        ProfScope ps(c, "depth_histogram_regions");
        if (launch_hist_pieces(c->stream, c->buf, d_p, (uint32_t)pieces.size(), n_bins, (unsigned long long *)d_hist,
                               (unsigned)c->n_cu * 8, c->hist_variant))
            return fail(c, PD_EHIP, "histogram of regions: cannot reserve LDS");
    }
    return hist_finish(c, d_hist, b_hist, hist);
}

int pd_reduce_intervals(pd_ctx *c, const pd_region *regs, size_t n, uint32_t min_dep, int32_t *cover, uint64_t *sum)
{
    if (!c || (n && (!regs || !cover || !sum))) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_reduce_intervals")) return rs;
    if (n == 0) return PD_OK;
    if (n > 0xFFFFFFF0ull) return fail(c, PD_EINVAL, "too many regions");
    HIPOK(c, hipSetDevice(c->device));
    std::vector<Piece> pieces;
    pieces.reserve(n + n / 8);
    for (size_t i = 0; i < n; ++i) {
        const pd_region &r = regs[i];
        if (r.tid < 0 || r.tid >= c->n_contigs) return fail(c, PD_EINVAL, "pd_reduce_intervals: contig id out of range");
        // cells [first-1, second), clipped to the slot (the reference reads its padding; it is zero here)
        const Span sp = seg_clip(r.first, r.second, c->off[r.tid + 1] - c->off[r.tid]);
        cut_into(pieces, c->off[r.tid] + sp.start, sp.count, (uint32_t)i);
    }
    const size_t b_p = pieces.size() * sizeof(Piece), b_sum = n * 8, b_cov = n * 4;
    unsigned long long *d_sum; Piece *d_p; int *d_cov;
    if (int rc = carve(c, 64, [&](Carver &S) { S.take(d_sum, b_sum); S.take(d_p, b_p); S.take(d_cov, b_cov); })) return rc;
    if (!pieces.empty()) HIPOK(c, hipMemcpyAsync(d_p, pieces.data(), b_p, hipMemcpyHostToDevice, c->stream));
    HIPOK(c, hipMemsetAsync(d_sum, 0, b_sum, c->stream));
    HIPOK(c, hipMemsetAsync(d_cov, 0, b_cov, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));          // pieces is a local
    {
        ProfScope ps(c, "reduce_intervals");
        launch_reduce_pieces(c->stream, c->buf, d_p, (uint32_t)pieces.size(), min_dep, d_cov, d_sum);
    }
    HIPOK(c, hipGetLastError());
    HIPOK(c, hipMemcpyAsync(sum, d_sum, b_sum, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipMemcpyAsync(cover, d_cov, b_cov, hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    return PD_OK;
}

// ---- depth levels ----
// Scratch: the edges, the waves' run counts, their offsets, then the pairs.  The pairs' size is known only after the count, so the
// count runs first with the head alone; when the buffer then has to grow (it is freed for that), the count is simply run again.
int pd_depth_levels(pd_ctx *c, int32_t tid, uint32_t beg, size_t n, const uint32_t *edges, uint32_t n_edges, pd_level *out, size_t cap, size_t *n_levels)
{
    if (!c || !n_levels || (!out && cap) || (!edges && n_edges)) return PD_EINVAL;
    *n_levels = 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_depth_levels")) return rs;
    if (tid < 0 || tid >= c->n_contigs) return fail(c, PD_EINVAL, "pd_depth_levels: contig id out of range");
    if ((uint64_t)beg + n > (uint64_t)c->len[tid]) return fail(c, PD_EINVAL, "pd_depth_levels: range past the contig's end");
    if (n > ((size_t)1 << 27)) return fail(c, PD_EINVAL, "pd_depth_levels: at most 2^27 cells per call");
    if (n_edges > 64) return fail(c, PD_EINVAL, "pd_depth_levels: at most 64 edges");
    for (uint32_t k = 1; k < n_edges; ++k)
        if (edges[k] <= edges[k - 1]) return fail(c, PD_EINVAL, "pd_depth_levels: edges not strictly ascending");
    if (n == 0) return PD_OK;
    HIPOK(c, hipSetDevice(c->device));
    const uint32_t a0 = beg & ~3u, lo = beg - a0, hi = lo + (uint32_t)n;        // int4-aligned start; the range relative to it
    const uint32_t nw = levels_waves(hi);
    const uint32_t *src = (const uint32_t *)(c->buf + c->off[tid] + a0);
    const uint32_t kcap = (uint32_t)(cap < n ? cap : n);         // (a range of n cells has at most n runs)
    uint32_t total = 0;
    uint32_t *d_edge = nullptr, *d_cnt = nullptr, *d_off = nullptr; uint2 *d_out = nullptr;
    for (int round = 0; ; ++round) {
        size_t b_head = 0;
        if (int rc = carve(c, 64, [&](Carver &S) {
                S.take(d_edge, 256); S.take(d_cnt, (size_t)nw * 4); S.take(d_off, ((size_t)nw * 4 + 4 + 15) / 16 * 16); b_head = S.used;
                S.take(d_out, round == 0 ? 0 : (size_t)std::min(total, kcap) * 8);
            })) return rc;
        if (n_edges) HIPOK(c, hipMemcpyAsync(d_edge, edges, (size_t)n_edges * 4, hipMemcpyHostToDevice, c->stream));
        {
            ProfScope ps(c, "depth_levels");
            launch_levels(c->stream, src, a0, lo, hi, d_edge, n_edges, d_cnt, d_off, nullptr, 0, false);
        }
        HIPOK(c, hipGetLastError());
        HIPOK(c, hipMemcpyAsync(&total, d_off + nw, 4, hipMemcpyDeviceToHost, c->stream));
        HIPOK(c, hipStreamSynchronize(c->stream));
        if (b_head + (size_t)std::min(total, kcap) * 8 + 64 <= c->scratch_bytes) break;
        if (round) return fail(c, PD_EHIP, "pd_depth_levels: scratch did not grow");
    }
    *n_levels = total;
    const uint32_t n_out = std::min(total, kcap);
    if (n_out) {
        {
            ProfScope ps(c, "depth_levels");
            launch_levels(c->stream, src, a0, lo, hi, d_edge, n_edges, d_cnt, d_off, d_out, n_out, true);
        }
        HIPOK(c, hipGetLastError());
        HIPOK(c, hipMemcpyAsync(out, d_out, (size_t)n_out * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(c, hipStreamSynchronize(c->stream));
    }
    if ((size_t)total > cap) return fail(c, PD_ERANGE, "pd_depth_levels: more runs than the output holds");
    return PD_OK;
}

int pd_window_quantiles(pd_ctx *c, uint32_t w, const uint32_t *pct, uint32_t n_pct, uint32_t *q)
{
    if (!c || !q || w == 0) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_window_quantiles")) return rs;
    QuantCall Q(c, q);
    if (int rc = quant_pct(c, pct, n_pct, "pd_window_quantiles", &Q.P)) return rc;
    std::vector<uint64_t> wo;
    const uint64_t nw = win_table(c, w, &wo).nw;
    if (nw == 0) return PD_OK;
    HIPOK(c, hipSetDevice(c->device));
    const uint32_t weff = win_weff(c, w);
    const int shape = row_shape(weff, c->q_wave_max, c->q_split);
    const uint64_t BR = shape == 2 ? WIDE_ROWS : win_batch_rows(n_pct), nbmax = std::min(BR, nw);
    uint64_t *d_wo;
    if (int rc = carve(c, 256, [&](Carver &S) {
            S.take(d_wo, al256(wo.size() * 8)); S.take(Q.d_q, al256((size_t)nbmax * n_pct * 4));
            S.take(Q.d_hist, shape == 2 ? al256((size_t)nbmax * 4096 * 8) : 0); S.take(Q.d_pc, shape == 2 ? FLUSH_PIECES * sizeof(Piece) : 0);
        })) return rc;
    HIPOK(c, hipMemcpyAsync(d_wo, wo.data(), wo.size() * 8, hipMemcpyHostToDevice, c->stream));
    RowBatch B; B.cap = weff; B.gshift = quant_gshift(weff);
    return windows_serve(c, w, wo, d_wo, nw, BR, shape, B, [&] { return Q.serve(B); });
}

int pd_depth_quantiles(pd_ctx *c, const pd_region *segs, size_t n_segs, const uint64_t *row_off, size_t n_rows,
                       const uint32_t *pct, uint32_t n_pct, uint64_t *cells, uint32_t *q)
{
    if (!c || (n_segs && !segs) || !row_off || (n_rows && !q)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_depth_quantiles")) return rs;
    QuantCall Q(c, q);
    if (int rc = quant_pct(c, pct, n_pct, "pd_depth_quantiles", &Q.P)) return rc;
    if (int rc = rows_check(c, "pd_depth_quantiles", segs, n_segs, row_off, n_rows)) return rc;
    if (n_rows == 0) return PD_OK;
    HIPOK(c, hipSetDevice(c->device));
    std::vector<uint64_t> own_cells;
    if (!cells) { own_cells.resize(n_rows); cells = own_cells.data(); }
    size_t n_wide; uint64_t wide_pieces;
    rows_measure(c, segs, row_off, n_rows, c->q_wave_max, c->q_split, cells, &n_wide, &wide_pieces);
    RowBatch B;
    if (int rc = carve(c, 256, [&](Carver &S) {
            B.take(S, n_rows, n_segs);
            S.take(Q.d_q, al256(std::min(ROW_BATCH, n_rows) * n_pct * 4)); S.take(Q.d_hist, al256(std::min<size_t>(WIDE_ROWS, n_wide) * 4096 * 8));
            S.take(Q.d_pc, al256((size_t)std::min<uint64_t>(FLUSH_PIECES, wide_pieces) * sizeof(Piece)));
        })) return rc;
    return rows_serve(c, segs, row_off, n_rows, cells, c->q_wave_max, c->q_split, B, [&] { return Q.serve(B); });
}

int pd_window_thresholds(pd_ctx *c, uint32_t w, const uint32_t *thr, uint32_t n_thr, uint32_t *counts)
{
    if (!c || !counts || w == 0) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_window_thresholds")) return rs;
    ThrCall<uint32_t> Q(c, counts);
    if (int rc = thr_set(c, thr, n_thr, "pd_window_thresholds", &Q.T)) return rc;
    std::vector<uint64_t> wo;
    const uint64_t nw = win_table(c, w, &wo).nw;
    if (nw == 0) return PD_OK;
    HIPOK(c, hipSetDevice(c->device));
    const uint32_t weff = win_weff(c, w);
    const int shape = row_shape(weff, c->t_wave_max, c->t_wave_max);
    const uint64_t BR = win_batch_rows(n_thr), nbmax = std::min(BR, nw);
    uint64_t *d_wo;
    if (int rc = carve(c, 256, [&](Carver &S) {
            S.take(d_wo, al256(wo.size() * 8)); S.take(Q.d_cnt, al256((size_t)nbmax * n_thr * 4)); S.take(Q.d_pc, shape == 2 ? FLUSH_PIECES * sizeof(Piece) : 0);
        })) return rc;
    HIPOK(c, hipMemcpyAsync(d_wo, wo.data(), wo.size() * 8, hipMemcpyHostToDevice, c->stream));
    RowBatch B; B.gshift = thr_gshift(weff); B.rpg = thr_rpg(weff);
    return windows_serve(c, w, wo, d_wo, nw, BR, shape, B, [&] { return Q.serve(B); });
}

int pd_depth_thresholds(pd_ctx *c, const pd_region *segs, size_t n_segs, const uint64_t *row_off, size_t n_rows,
                        const uint32_t *thr, uint32_t n_thr, uint64_t *cells, uint64_t *counts)
{
    if (!c || (n_segs && !segs) || !row_off || (n_rows && !counts)) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_depth_thresholds")) return rs;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counts are copied as they are");
    ThrCall<unsigned long long> Q(c, counts);
    if (int rc = thr_set(c, thr, n_thr, "pd_depth_thresholds", &Q.T)) return rc;
    if (int rc = rows_check(c, "pd_depth_thresholds", segs, n_segs, row_off, n_rows)) return rc;
    if (n_rows == 0) return PD_OK;
    HIPOK(c, hipSetDevice(c->device));
    std::vector<uint64_t> own_cells;
    if (!cells) { own_cells.resize(n_rows); cells = own_cells.data(); }
    size_t n_wide; uint64_t wide_pieces;
    rows_measure(c, segs, row_off, n_rows, c->t_wave_max, c->t_wave_max, cells, &n_wide, &wide_pieces);
    RowBatch B;
    if (int rc = carve(c, 256, [&](Carver &S) {
            B.take(S, n_rows, n_segs);
            S.take(Q.d_cnt, al256(std::min(ROW_BATCH, n_rows) * n_thr * 8)); S.take(Q.d_pc, al256((size_t)std::min<uint64_t>(FLUSH_PIECES, wide_pieces) * sizeof(Piece)));
        })) return rc;
    return rows_serve(c, segs, row_off, n_rows, cells, c->t_wave_max, c->t_wave_max, B, [&] { B.gshift = thr_gshift(B.cap); return Q.serve(B); });
}

} // extern "C"
