// pd_rowcounts.h — the records of a batch counted per ROW of the main table (`-rowreads`, PD_DECODE_ROW_COUNTS): one more pass over the
// record chain that pd_bamwalk.h's pass 1 has confirmed, of pd_recstats.h's shape with a bin lookup in it.  It reads refID, pos, mapq and
// flag of every record (20 of its 36 fixed bytes) and no CIGAR.
//
// A record STARTS AT cell (refID, pos) when 0 <= refID < n_ref and 0 <= pos < contig_len[refID]; every other record (unplaced, pos == -1,
// pos >= len — the header test of the walk lets pos == len through) starts nowhere and is in no bin.  A record is counted in the one bin
// its start lies in, so the bins of a contig add up to the contig.
//
// Bins are ELEMENTARY INTERVALS of the contigs, one mechanism for the three table families (Bins):
//   * window form (w > 0): bin = off[tid] + pos / w, off = pd_window_layout(w); no table is read;
//   * edge form (w == 0): off[t] .. off[t + 1] index contig t's strictly ascending edges; contig t with k edges has k + 1 bins, and a
//     start at (t, pos) goes to bin off[t] + t + j, j = the number of t's edges <= pos.  No edges: one bin per contig.
// A bin is RC_WORDS u64 words: records, passed (flag & X == 0), mapq0 (passed, mapq == 0), kept (passed, mapq >= Q), forward (kept,
// flag & 0x10 == 0), mapq_sum (of the kept).  X / Q: the session's flag mask and mapq bound; `kept` is the FILTER's verdict, as in
// pd_recstats.h — contig_on, short contigs, spans, -frag and -del play no part.
//
// One wave per segment: lane l starts at LaneOut::start of its stretch and goes from record to record by block size, behind the three
// bounds checks of walk_lane, to the end of its stretch.  The lane keeps the six counters of its OPEN bin in registers together with the
// bin's [lo, hi) on its contig — its run-length: with -w 1000 on 50x short reads a lane's ~20 records lie in one or two bins — and adds
// them to global memory (64-bit atomics, non-zero words only) when a record starts outside.  The edge search: the lane's first record
// takes a binary search over its contig's edges; a later record that lies at or behind `hi` on the same contig gallops forward from the
// open bin (1, 2, 4 ... edges, then a binary search inside the last step), and one whose pos went backwards or whose contig changed takes
// the full search again.  At the end the lanes that stand on the same bin as the first lane that holds one are reduced with wave scans
// and added once, then the same again for the lanes that are left (a sorted file: most of a wave stands on one or two bins); whoever
// still holds counters adds them singly.  None of this bears on the result: every path ends in integer atomic adds, in any record order.
//
// The same source compiles for gfx950 and for the host (tests/harness/rowcounts_check.cpp).
#ifndef PD_ROWCOUNTS_H_
#define PD_ROWCOUNTS_H_
#include "pd_bamwalk.h"                  // PW_FN, the wave classes, Cfg / Seg / LaneOut, rd32 / rd16, SUB, NONE

namespace pdrc {

enum { RC_RECORDS = 0, RC_PASSED = 1, RC_MAPQ0 = 2, RC_KEPT = 3, RC_FORWARD = 4, RC_MAPQ_SUM = 5, RC_WORDS = PD_ROWCOUNT_WORDS };
static_assert(RC_MAPQ_SUM + 1 == RC_WORDS, "a bin is six words");

struct Bins {                             // wave-uniform: the session's bin table (pd_decode_row_bins)
    uint32_t w;                           // > 0: window form
    const uint64_t *off;                  // n_ref + 1: the contigs' first windows (window form) or their places in `edges` (edge form)
    const uint32_t *edges;                // edge form: off[n_ref] edges (unread when there are none)
    uint64_t n_bins;
};

#if defined(__HIP_DEVICE_COMPILE__)
PW_FN void add_u64(unsigned long long *p, unsigned long long v) { atomicAdd(p, v); }
#else
PW_FN void add_u64(unsigned long long *p, unsigned long long v) { *p += v; }
#endif

// six counters into one bin (a bin outside the table — there is none by the table's construction — is dropped, never written)
PW_FN void add_bin(const Bins &B, unsigned long long *counts, uint64_t bin, const uint32_t *k)
{
    if (bin >= B.n_bins) return;
    unsigned long long *p = counts + bin * (uint64_t)RC_WORDS;
#pragma unroll
    for (int j = 0; j < RC_WORDS; ++j) if (k[j]) add_u64(p + j, k[j]);
}

// the number of e[0 .. n)'s values <= pos, searched in [a, n) (every value before a is <= pos)
PW_FN uint32_t edges_le(const uint32_t *e, uint32_t a, uint32_t n, uint32_t pos)
{
    uint32_t lo = a, hi = n;
    while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (e[m] <= pos) lo = m + 1; else hi = m; }
    return lo;
}

// One wave, one segment whose chain is confirmed.
template <class W>
PW_FN void rows_segment(const pdb2::Cfg &cfg, const pdb2::Seg &sg, const pdb2::LaneOut *lanes, const Bins &B, unsigned long long *counts)
{
    using namespace pdb2;
    typedef typename W::template Var<uint32_t> U;
    const uint8_t *const buf = cfg.buf;
    const uint64_t avail = sg.avail;
    U o_bin, o_k[RC_WORDS];                                       // what every lane still holds at its end (bin 0xFFFFFFFF: nothing; n_bins <= 2^28)
    W::each([&](int l) {
        uint32_t k[RC_WORDS] = {0, 0, 0, 0, 0, 0};
        uint32_t bin = 0xFFFFFFFFu, ctid = 0xFFFFFFFFu, lo = 0, hi = 0, cj = 0;      // the open bin, its contig, its cells [lo, hi), its place among the contig's edges
        const uint64_t a = sg.begin + (uint64_t)l * SUB;
        const uint64_t b = a + SUB < sg.end ? a + SUB : sg.end;
        const uint64_t s = lanes[l].start;
        if (a < sg.end && s != NONE && s < b) {
            uint64_t p = s;
            for (uint32_t guard = 0; p < b && guard < SUB / 36 + 2; ++guard) {
                // (walk_lane's checks before it opens a record; none of them fails in a counted unit)
                if (p + 36 > avail) break;
                const uint8_t *r = buf + p;
                const uint32_t bs = rd32(r);
                if (bs < 32 || bs > (1u << 29)) break;
                if (p + 4 + (uint64_t)bs > avail) break;
                const int32_t tid = (int32_t)rd32(r + 4), ipos = (int32_t)rd32(r + 8);
                p += 4 + (uint64_t)bs;
                if (tid < 0 || tid >= cfg.n_ref || ipos < 0 || (uint32_t)ipos >= cfg.contig_len[tid]) continue;      // starts nowhere
                const uint32_t pos = (uint32_t)ipos, mapq = r[13], flag = rd16(r + 18);
                if ((uint32_t)tid != ctid || pos < lo || pos >= hi) {
                    if (bin != 0xFFFFFFFFu) add_bin(B, counts, bin, k);
#pragma unroll
                    for (int j = 0; j < RC_WORDS; ++j) k[j] = 0;
                    const uint64_t base = B.off[tid];
                    if (B.w) {
                        const uint32_t j = pos / B.w;
                        const uint64_t e = (uint64_t)j * B.w + B.w;
                        lo = j * B.w; hi = e > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)e;
                        bin = (uint32_t)(base + j);
                    } else {
                        const uint32_t n = (uint32_t)(B.off[tid + 1] - base);
                        const uint32_t *e = n ? B.edges + base : nullptr;                     // (a contig without edges reads none)
                        uint32_t j;
                        if ((uint32_t)tid == ctid && pos >= hi) {
                            // forward on the same contig: e[cj] = hi <= pos.  Gallop: the first step that overshoots bounds the search
                            uint32_t from = cj + 1, step = 1, to = n;
                            while (from + step - 1 < n) {
                                if (e[from + step - 1] > pos) { to = from + step - 1; break; }
                                from += step; step <<= 1;
                            }
                            j = edges_le(e, from, to, pos);
                        } else j = edges_le(e, 0, n, pos);
                        cj = j;
                        lo = j ? e[j - 1] : 0u; hi = j < n ? e[j] : 0xFFFFFFFFu;
                        bin = (uint32_t)(base + (uint32_t)tid + j);
                    }
                    ctid = (uint32_t)tid;
                }
                ++k[RC_RECORDS];
                if (!(flag & cfg.flag_mask)) {
                    ++k[RC_PASSED];
                    if (mapq == 0) ++k[RC_MAPQ0];
                    if ((int32_t)mapq >= cfg.min_mapq) { ++k[RC_KEPT]; k[RC_MAPQ_SUM] += mapq; if (!(flag & 0x10)) ++k[RC_FORWARD]; }
                }
            }
        }
        o_bin[l] = bin;
        for (int j = 0; j < RC_WORDS; ++j) o_k[j][l] = k[j];
    });
    // the bins the lanes still hold: twice, those of the first such lane's bin are reduced and added once; then the others go singly
    // (a lane holds at most SUB / 36 + 2 records of mapq <= 255: a wave's sum stays far below 2^32)
    for (int round = 0; round < 2; ++round) {
        const uint64_t has = W::ballot_ne(o_bin, 0xFFFFFFFFu);
        if (!has) return;
        const uint32_t b0 = W::bcast(o_bin, ctz64(has));
        uint32_t tot[RC_WORDS];
        for (int j = 0; j < RC_WORDS; ++j) {
            U x;
            W::each([&](int l) { x[l] = o_bin[l] == b0 ? o_k[j][l] : 0u; });
            (void)W::excl_scan(x, &tot[j]);
        }
        W::each([&](int l) {
            if (o_bin[l] == b0) o_bin[l] = 0xFFFFFFFFu;
            if (l == 0) add_bin(B, counts, b0, tot);
        });
    }
    W::each([&](int l) {
        if (o_bin[l] == 0xFFFFFFFFu) return;
        uint32_t k[RC_WORDS];
        for (int j = 0; j < RC_WORDS; ++j) k[j] = o_k[j][l];
        add_bin(B, counts, o_bin[l], k);
    });
}

} // namespace pdrc
#endif
