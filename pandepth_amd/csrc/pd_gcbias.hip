// pd_gcbias.hip — pd_depth_gc_bias (the -gcbias file): depth by GC content of fixed windows.  The depth is resident after pd_scan; the
// bases come up from the host in PIECES of whole windows, a page-locked staging buffer and a device buffer per turn (two turns), so that
// the copy of piece k + 1 runs under the kernel of piece k.  One pass: every depth cell (4 B) and every base byte is read once.
//
// A piece is [16 B pad | the bases of its windows, segment after segment | pad to 16 B | 16 B pad | GcSeg x n_seg] and goes up in ONE copy.
// A segment is a stretch of whole windows of one contig or region: where its cells lie in the depth array (a 64-bit cell offset), where its
// bases lie in the piece, and the number of its first window in the piece; a window finds its segment by bisection.  Cells a record does not
// reach (a short record, a contig without one) are staged as byte 0, which no rule calls a base: "invalid" is a property of the byte alone.
//
// k_gc_bias, two launch shapes (the results are sums of integers and do not depend on the shape, the piece size or the order of arrival):
//   narrow   a GROUP of 1 .. 64 lanes per window (about sixteen cells a lane), many windows per wave, reduced with __shfl_xor
//   block    a WORKGROUP per window, in strides of 256 lanes: the waves reduce with __shfl_xor and meet in LDS
// Depth is read as thr_span reads it (scalar head to the first 16-byte boundary, 16-byte loads, four in flight per lane, scalar tail).  Bases
// are read in the ALIGNED 16-byte chunks that cover the window (the pads keep the first and the last chunk inside the buffer) and classified
// on packed bytes: after `| 0x20` a byte is 'c' / 'g' / 'a' / 't' exactly where the XOR with that letter is a zero byte (RefSeqs::gc's zero-byte
// test); bytes of a chunk outside the window are masked.  Per window: the GC count, an any-invalid flag, a 64-bit depth sum.  The window's
// bin, (200 g + W) / 2W, is counted in LDS — 101 x (windows, 64-bit sum) and the skipped windows per workgroup — and a workgroup flushes once,
// one 64-bit atomicAdd per non-empty bin and quantity: no global atomic per window, whatever the genome's GC looks like.
#include "pd_ctx.h"

namespace {

constexpr int GC_WG = 256;
constexpr uint32_t GC_BINS = 101;
constexpr uint32_t GC_SEG_CAP = 65536;                           // segments per piece (1 MiB of GcSeg)
constexpr uint32_t GC_W_MAX = 1u << 20;

struct GcSeg { uint64_t cell; uint32_t boff; uint32_t win0; };  // first depth cell; first base byte in the piece; first window in the piece
struct GcPiece { const uint32_t *depth; const uint8_t *bases; const GcSeg *segs; uint32_t n_seg, n_win, w; };

// 0x80 in every byte of v that is zero
__device__ __forceinline__ uint32_t gc_zero80(uint32_t v) { return ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v | 0x7f7f7f7fu); }

// four bases; keep: 0x80 in the bytes that belong to the window
__device__ __forceinline__ void gc_word(uint32_t x, uint32_t keep, uint32_t &gc, uint32_t &bad)
{
    const uint32_t y = x | 0x20202020u;
    const uint32_t g = gc_zero80(y ^ 0x63636363u) | gc_zero80(y ^ 0x67676767u);
    const uint32_t v = g | gc_zero80(y ^ 0x61616161u) | gc_zero80(y ^ 0x74747474u);
    gc += (uint32_t)__popc(g & keep);
    bad |= ~v & keep;
}

// the bytes of the word at p that lie in [s, e)
__device__ __forceinline__ uint32_t gc_keep(uint32_t p, uint32_t s, uint32_t e)
{
    const uint32_t lo = s > p ? (s - p < 4u ? s - p : 4u) : 0u, hi = e > p ? (e - p < 4u ? e - p : 4u) : 0u;
    return hi > lo ? (0x80808080u >> (8u * (4u - hi))) & (0x80808080u << (8u * lo)) : 0u;
}

// the aligned chunk at byte p of the piece, of the window's bytes [s, e)
__device__ __forceinline__ void gc_chunk(const uint4 x, uint32_t p, uint32_t s, uint32_t e, uint32_t &gc, uint32_t &bad)
{
    if (p >= s && p + 16u <= e) {
        gc_word(x.x, 0x80808080u, gc, bad); gc_word(x.y, 0x80808080u, gc, bad); gc_word(x.z, 0x80808080u, gc, bad); gc_word(x.w, 0x80808080u, gc, bad);
    } else {
        gc_word(x.x, gc_keep(p, s, e), gc, bad); gc_word(x.y, gc_keep(p + 4u, s, e), gc, bad);
        gc_word(x.z, gc_keep(p + 8u, s, e), gc, bad); gc_word(x.w, gc_keep(p + 12u, s, e), gc, bad);
    }
}

__device__ __forceinline__ uint64_t gc_sum4(const uint4 x) { return ((uint64_t)x.x + x.y) + ((uint64_t)x.z + x.w); }

// window of W cells: depth d[0 .. W) (d a cell of the depth array, whose base is 16-byte aligned), bases B[s .. s + W) (B 16-byte aligned, s >= 16),
// by lanes gl = 0 .. G - 1
__device__ __forceinline__ void gc_span(const uint32_t *d, const uint8_t *B, uint32_t s, uint32_t W, uint32_t gl, uint32_t G, uint64_t &sum, uint32_t &gc, uint32_t &bad)
{
    uint32_t head = (4u - (uint32_t)((reinterpret_cast<uintptr_t>(d) >> 2) & 3u)) & 3u;     // cells before the first 16-byte boundary
    if (head > W) head = W;
    const uint32_t n4 = (W - head) >> 2, tail0 = head + (n4 << 2);
    for (uint32_t i = gl; i < head; i += G) sum += d[i];
    const uint4 *d4 = reinterpret_cast<const uint4 *>(d + head);
    for (uint32_t k0 = 0; k0 < n4; k0 += 4 * G) {               // the same trips for every lane of the group; a lane past the end reads d4[0] and adds nothing
        const uint32_t k = k0 + gl;
        const bool ok0 = k < n4, ok1 = k + G < n4, ok2 = k + 2 * G < n4, ok3 = k + 3 * G < n4;
        const uint4 x0 = d4[ok0 ? k : 0u], x1 = d4[ok1 ? k + G : 0u], x2 = d4[ok2 ? k + 2 * G : 0u], x3 = d4[ok3 ? k + 3 * G : 0u];
        if (ok0) sum += gc_sum4(x0);
        if (ok1) sum += gc_sum4(x1);
        if (ok2) sum += gc_sum4(x2);
        if (ok3) sum += gc_sum4(x3);
    }
    for (uint32_t i = tail0 + gl; i < W; i += G) sum += d[i];    // (fewer than 4 cells)
    const uint32_t e = s + W, c0 = s >> 4, nc = ((e + 15u) >> 4) - c0;
    const uint4 *B4 = reinterpret_cast<const uint4 *>(B) + c0;
    for (uint32_t k0 = 0; k0 < nc; k0 += 4 * G) {
        const uint32_t k = k0 + gl;
        const bool ok0 = k < nc, ok1 = k + G < nc, ok2 = k + 2 * G < nc, ok3 = k + 3 * G < nc;
        const uint4 x0 = B4[ok0 ? k : 0u], x1 = B4[ok1 ? k + G : 0u], x2 = B4[ok2 ? k + 2 * G : 0u], x3 = B4[ok3 ? k + 3 * G : 0u];
        if (ok0) gc_chunk(x0, (c0 + k) << 4, s, e, gc, bad);
        if (ok1) gc_chunk(x1, (c0 + k + G) << 4, s, e, gc, bad);
        if (ok2) gc_chunk(x2, (c0 + k + 2 * G) << 4, s, e, gc, bad);
        if (ok3) gc_chunk(x3, (c0 + k + 3 * G) << 4, s, e, gc, bad);
    }
}

// out: windows[101] | sums[101] | skipped, added to
template <bool BLOCK>
__global__ __launch_bounds__(GC_WG) void k_gc_bias(const GcPiece P, uint32_t gshift, unsigned long long *out)
{
    __shared__ unsigned long long s_sum[GC_BINS];
    __shared__ uint32_t s_cnt[GC_BINS];
    __shared__ unsigned long long r_sum;                         // BLOCK: where the waves of a window meet
    __shared__ uint32_t s_skip, r_gc, r_bad;
    for (uint32_t b = threadIdx.x; b < GC_BINS; b += GC_WG) { s_sum[b] = 0; s_cnt[b] = 0; }
    if (threadIdx.x == 0) { s_skip = 0; r_sum = 0; r_gc = 0; r_bad = 0; }
    __syncthreads();
    const uint32_t G = BLOCK ? (uint32_t)GC_WG : 1u << gshift, gl = BLOCK ? threadIdx.x : threadIdx.x & (G - 1u);
    const uint32_t gpb = BLOCK ? 1u : (uint32_t)GC_WG >> gshift;                 // groups per workgroup
    const uint64_t stride = (uint64_t)gridDim.x * gpb;
    for (uint64_t wi = (uint64_t)blockIdx.x * gpb + (BLOCK ? 0u : threadIdx.x >> gshift); wi < P.n_win; wi += stride) {   // (BLOCK: the same trips for the whole workgroup)
        uint32_t lo = 0, hi = P.n_seg;                           // the last segment that starts at or before window wi
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (P.segs[mid].win0 <= wi) lo = mid; else hi = mid; }
        const GcSeg sg = P.segs[lo];
        const uint64_t j = (wi - sg.win0) * P.w;
        uint64_t sum = 0; uint32_t gc = 0, bad = 0;
        gc_span(P.depth + sg.cell + j, P.bases, sg.boff + (uint32_t)j, P.w, gl, G, sum, gc, bad);
        for (uint32_t m = (BLOCK ? 64u : G) >> 1; m; m >>= 1) {
            sum += (uint64_t)__shfl_xor((unsigned long long)sum, (int)m); gc += (uint32_t)__shfl_xor((int)gc, (int)m); bad |= (uint32_t)__shfl_xor((int)bad, (int)m);
        }
        if (BLOCK) {
            if ((threadIdx.x & 63u) == 0) { atomicAdd(&r_sum, (unsigned long long)sum); atomicAdd(&r_gc, gc); atomicOr(&r_bad, bad); }
            __syncthreads();
            if (threadIdx.x == 0) { sum = r_sum; gc = r_gc; bad = r_bad; r_sum = 0; r_gc = 0; r_bad = 0; }
        }
        if (gl == 0) {
            if (bad) atomicAdd(&s_skip, 1u);
            else {
                const uint32_t b = (200u * gc + P.w) / (2u * P.w);
                atomicAdd(&s_cnt[b], 1u);
                atomicAdd(&s_sum[b], (unsigned long long)sum);
            }
        }
        if (BLOCK) __syncthreads();
    }
    __syncthreads();
    if (threadIdx.x < GC_BINS) {
        const uint32_t n = s_cnt[threadIdx.x];
        const unsigned long long t = s_sum[threadIdx.x];
        if (n) atomicAdd(&out[threadIdx.x], (unsigned long long)n);
        if (t) atomicAdd(&out[GC_BINS + threadIdx.x], t);
    } else if (threadIdx.x == GC_BINS && s_skip) atomicAdd(&out[2 * GC_BINS], (unsigned long long)s_skip);
}

// what the call owns beside the context's scratch: two page-locked staging buffers, the stream of the copies, an event per turn and kind
struct GcCall {
    pd_ctx *c;
    uint8_t *host[2] = {nullptr, nullptr};
    hipStream_t copy = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
    explicit GcCall(pd_ctx *ctx) : c(ctx) {}
    ~GcCall()
    {
        if (copy) (void)hipStreamSynchronize(copy);
        (void)hipStreamSynchronize(c->stream);
        for (int k = 0; k < 2; ++k) {
            if (host[k]) (void)hipHostFree(host[k]);
            if (copied[k]) (void)hipEventDestroy(copied[k]);
            if (done[k]) (void)hipEventDestroy(done[k]);
        }
        if (copy) (void)hipStreamDestroy(copy);
    }
};

struct GcSpan { int32_t tid; uint64_t b, e; };                  // cells [b, e) of a contig, tiled from b

} // namespace

extern "C" int pd_depth_gc_bias(pd_ctx *c, const pd_region *regs, size_t n, uint32_t w, const char *const *bases, const uint32_t *n_bases,
                                uint64_t *windows, uint64_t *sum, uint64_t *skipped)
{
    if (!c || !windows || !sum || !skipped || (n && !regs) || (bases && !n_bases) || w == 0 || w > GC_W_MAX) return PD_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rs = need_state(c, 1, "pd_depth_gc_bias")) return rs;
    HIPOK(c, hipSetDevice(c->device));
    std::vector<GcSpan> spans;
    if (!regs || n == 0) {
        for (int32_t t = 0; t < c->n_contigs; ++t) spans.push_back(GcSpan{t, 0, c->len[(size_t)t]});
    } else {                                                     // pd_depth_histogram's rule: sorted by (tid, first), disjoint, clipped to the contig
        int32_t prev_tid = -1; int64_t prev_first = 0, prev_end = 0;
        for (size_t i = 0; i < n; ++i) {
            const pd_region &r = regs[i];
            if (r.tid < 0 || r.tid >= c->n_contigs) return fail(c, PD_EINVAL, "pd_depth_gc_bias: contig id out of range");
            const int64_t b0 = (int64_t)r.first - 1, e0 = r.second;
            if (r.tid < prev_tid || (r.tid == prev_tid && r.first < prev_first)) return fail(c, PD_EINVAL, "pd_depth_gc_bias: regions not sorted by (tid, first)");
            if (r.tid != prev_tid) prev_end = INT64_MIN;
            if (e0 > b0) {
                if (b0 < prev_end) return fail(c, PD_EINVAL, "pd_depth_gc_bias: regions overlap");
                prev_end = e0;
            }
            prev_tid = r.tid; prev_first = r.first;
            const int64_t b = b0 < 0 ? 0 : b0, e = e0 > (int64_t)c->len[(size_t)r.tid] ? (int64_t)c->len[(size_t)r.tid] : e0;
            if (b < e) spans.push_back(GcSpan{r.tid, (uint64_t)b, (uint64_t)e});
        }
    }
    // a piece: at most `wpp` windows and GC_SEG_CAP segments
    uint64_t all_win = 0;
    for (const GcSpan &sp : spans) all_win += (sp.e - sp.b) / w;
    if (!all_win) {                                              // no window anywhere: nothing to stage, nothing to launch
        memset(windows, 0, GC_BINS * 8); memset(sum, 0, GC_BINS * 8); *skipped = 0;
        return PD_OK;
    }
    const uint64_t wpp = std::min<uint64_t>(std::max<uint64_t>(1, c->gc_piece_cells / w), all_win), cap_cells = wpp * w;   // (a small call stages small buffers)
    const size_t seg_cap = std::min<size_t>(GC_SEG_CAP, spans.size());                  // (a piece holds at most one segment of a span)
    const size_t b_out = 2048, b_buf = (size_t)((16 + cap_cells + 15) / 16 * 16) + 16 + seg_cap * sizeof(GcSeg);
    if (int rc = ensure_scratch(c, b_out + 2 * b_buf)) return rc;
    unsigned long long *d_out = (unsigned long long *)c->scratch;
    uint8_t *dev[2] = {(uint8_t *)c->scratch + b_out, (uint8_t *)c->scratch + b_out + b_buf};
    GcCall call(c);
    for (int k = 0; k < 2; ++k) {
        if (hipHostMalloc((void **)&call.host[k], b_buf, hipHostMallocDefault) != hipSuccess) { call.host[k] = nullptr; return fail(c, PD_ENOMEM, "pd_depth_gc_bias: page-locked staging allocation failed"); }
        memset(call.host[k], 0, 16);
        HIPOK(c, hipEventCreateWithFlags(&call.copied[k], hipEventDisableTiming));
        HIPOK(c, hipEventCreateWithFlags(&call.done[k], hipEventDisableTiming));
    }
    HIPOK(c, hipStreamCreateWithFlags(&call.copy, hipStreamNonBlocking));
    HIPOK(c, hipMemsetAsync(d_out, 0, b_out, c->stream));
    HIPOK(c, hipEventRecord(call.done[0], c->stream));           // the scratch is the copy stream's from here on
    HIPOK(c, hipStreamWaitEvent(call.copy, call.done[0], 0));

    uint64_t turn = 0, cells = 0, n_win = 0;                     // the piece being filled: its turn, the cells and windows it holds
    std::vector<GcSeg> segs;
    auto submit = [&]() -> int {
        const int k = (int)(turn & 1);
        const size_t soff = (size_t)((16 + cells + 15) / 16 * 16) + 16, bytes = soff + segs.size() * sizeof(GcSeg);
        memcpy(call.host[k] + soff, segs.data(), segs.size() * sizeof(GcSeg));
        if (turn >= 2) HIPOK(c, hipStreamWaitEvent(call.copy, call.done[k], 0));          // the kernel that read this device buffer last
        HIPOK(c, hipMemcpyAsync(dev[k], call.host[k], bytes, hipMemcpyHostToDevice, call.copy));
        HIPOK(c, hipEventRecord(call.copied[k], call.copy));
        HIPOK(c, hipStreamWaitEvent(c->stream, call.copied[k], 0));
        const GcPiece P{(const uint32_t *)c->buf, dev[k], (const GcSeg *)(dev[k] + soff), (uint32_t)segs.size(), (uint32_t)n_win, w};
        const unsigned cap = (unsigned)c->n_cu * 8;
        {
            ProfScope ps(c, "gc_bias");
            if (w > c->gc_wave_max) {
                hipLaunchKernelGGL((k_gc_bias<true>), dim3((unsigned)std::min<uint64_t>(n_win, cap)), dim3(GC_WG), 0, c->stream, P, 0u, d_out);
            } else {
                uint32_t gshift = 0;
                while (gshift < 6 && (16u << gshift) < w) ++gshift;                      // about sixteen cells a lane
                const uint64_t gpb = (uint64_t)GC_WG >> gshift;
                hipLaunchKernelGGL((k_gc_bias<false>), dim3((unsigned)std::min<uint64_t>((n_win + gpb - 1) / gpb, cap)), dim3(GC_WG), 0, c->stream, P, gshift, d_out);
            }
        }
        HIPOK(c, hipGetLastError());
        HIPOK(c, hipEventRecord(call.done[k], c->stream));
        ++turn; cells = 0; n_win = 0; segs.clear();
        return PD_OK;
    };
    for (const GcSpan &sp : spans) {
        uint64_t pos = sp.b, left = (sp.e - sp.b) / w;           // windows still to place; a trailing stretch shorter than w belongs to none
        const char *src = bases ? bases[sp.tid] : nullptr;
        const uint64_t have = src ? n_bases[sp.tid] : 0;
        while (left) {
            if (n_win == wpp || segs.size() == seg_cap) { if (int rc = submit()) return rc; }
            const int k = (int)(turn & 1);
            if (n_win == 0 && turn >= 2) HIPOK(c, hipEventSynchronize(call.copied[k]));   // the one wait of a buffer turn: the staging buffer's last copy has left it
            const uint64_t take = std::min<uint64_t>(left, wpp - n_win), nc = take * w;
            uint8_t *dst = call.host[k] + 16 + cells;
            const uint64_t got = pos < have ? std::min<uint64_t>(have - pos, nc) : 0;
            if (got) memcpy(dst, src + pos, (size_t)got);
            if (got < nc) memset(dst + got, 0, (size_t)(nc - got));
            segs.push_back(GcSeg{c->off[(size_t)sp.tid] + pos, (uint32_t)(16 + cells), (uint32_t)n_win});
            cells += nc; n_win += take; pos += nc; left -= take;
        }
    }
    if (n_win) { if (int rc = submit()) return rc; }
    uint64_t res[2 * GC_BINS + 1];
    HIPOK(c, hipMemcpyAsync(res, d_out, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    HIPOK(c, hipStreamSynchronize(c->stream));
    memcpy(windows, res, GC_BINS * 8);
    memcpy(sum, res + GC_BINS, GC_BINS * 8);
    *skipped = res[2 * GC_BINS];
    return PD_OK;
}
