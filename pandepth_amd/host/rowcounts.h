// rowcounts.h — `-rowreads`: how many records START in every row of the main table, and how well they mapped.  The run's bin table
// (RowBins, built once from the table's rows: extras.cpp) and one accumulator over its bins, laid out as the engine's
// (include/pandepth_amd.h: pd_decode_row_bins / pd_decode_row_counts — PD_ROWCOUNT_WORDS words per bin), fed either a record at a time by
// the host readers (add, before any filter `continue`) or a session at a time by the device (add_device); the threaded readers add to
// their context's array through RowCountsShare, without a copy of it.
// A record starts at cell (refID, pos) when 0 <= refID < n_ref and 0 <= pos < the contig's length; every other record starts nowhere and
// is in no bin.  Bins are elementary intervals of the contigs: with w > 0 bin off[t] + pos / w (off: pd_window_layout(w)); with w == 0
// contig t's edges are edges[off[t] .. off[t + 1]), strictly ascending, and a start goes to bin off[t] + t + (the number of t's edges <= pos).
// The six words of a bin: records, passed (flag & -x == 0), mapq0 (passed, mapq == 0), kept (passed, mapq >= -q: ReadFilter::pass, the
// filter's verdict), forward (kept, flag & 0x10 == 0), the sum of the kept ones' mapq.
#ifndef PD_ROWCOUNTS_HOST_H_
#define PD_ROWCOUNTS_HOST_H_
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "bam.h"
#include "../../include/pandepth_amd.h"

namespace pdh {

struct RowBins {
    uint32_t w = 0;                          // > 0: the window form
    std::vector<uint64_t> off;               // n_ref + 1
    std::vector<uint32_t> edges;
    std::vector<uint32_t> lens;              // the contigs' lengths
    uint64_t n_bins = 0;
    // the bin of a start (the caller has tested 0 <= pos < lens[tid])
    uint64_t bin_of(int32_t tid, uint32_t pos) const
    {
        if (w) return off[(size_t)tid] + pos / w;
        const uint32_t *b = edges.data() + off[(size_t)tid], *e = edges.data() + off[(size_t)tid + 1];
        return off[(size_t)tid] + (uint64_t)tid + (uint64_t)(std::upper_bound(b, e, pos) - b);
    }
};

struct RowCounts {
    enum { RECORDS = 0, PASSED = 1, MAPQ0 = 2, KEPT = 3, FORWARD = 4, MAPQ_SUM = 5, WORDS = PD_ROWCOUNT_WORDS };
    bool on = false;
    uint32_t flag_mask = 0; int min_mapq = 0;
    const RowBins *tab = nullptr;            // the run's (it outlives every accumulator)
    std::vector<uint64_t> cnt;               // n_bins * WORDS

    void init(uint32_t x, int q, const RowBins *t)
    {
        on = true; flag_mask = x; min_mapq = q; tab = t;
        cnt.assign((size_t)t->n_bins * WORDS, 0);
    }
    void init_like(const RowCounts &o) { if (o.on) init(o.flag_mask, o.min_mapq, o.tab); }
    // the bin a record starts in (false: it starts nowhere)
    inline bool place(const AlnRec &r, uint64_t *bin) const
    {
        if (r.tid < 0 || (size_t)r.tid >= tab->lens.size() || r.pos < 0 || (uint32_t)r.pos >= tab->lens[(size_t)r.tid]) return false;
        *bin = tab->bin_of(r.tid, (uint32_t)r.pos);
        return true;
    }
    // one record into the six words of its bin
    inline void tally(uint64_t *k, const AlnRec &r) const
    {
        ++k[RECORDS];
        if (r.flag & flag_mask) return;
        ++k[PASSED];
        if (r.mapq == 0) ++k[MAPQ0];
        if ((int)r.mapq < min_mapq) return;
        ++k[KEPT]; k[MAPQ_SUM] += r.mapq;
        if (!(r.flag & 0x10)) ++k[FORWARD];
    }
    inline void add(const AlnRec &r) { uint64_t b; if (place(r, &b)) tally(cnt.data() + b * WORDS, r); }
    void add_device(const uint64_t *c) { for (size_t i = 0; i < cnt.size(); ++i) cnt[i] += c[i]; }
    void merge(const RowCounts &o) { if (o.on) add_device(o.cnt.data()); }
};

// A threaded reader's view of its context's accumulator: no copy of the bins (with a small -w on a large genome they are hundreds of MB).  The thread
// keeps the six counters of its OPEN bin — its run-length, as a lane of k_row_counts does — and adds them to the shared array with relaxed
// atomics when a record starts in another bin and when the thread is through.  Integer adds: the order plays no part.
struct RowCountsShare {
    RowCounts *rc;                           // null: the option is off
    uint64_t bin = ~0ull, k[RowCounts::WORDS] = {0, 0, 0, 0, 0, 0};
    explicit RowCountsShare(RowCounts *shared) : rc(shared && shared->on ? shared : nullptr) {}
    RowCountsShare(const RowCountsShare &) = delete;
    RowCountsShare &operator=(const RowCountsShare &) = delete;
    ~RowCountsShare() { flush(); }
    void flush()
    {
        if (bin == ~0ull) return;
        uint64_t *p = rc->cnt.data() + bin * RowCounts::WORDS;
        for (int j = 0; j < RowCounts::WORDS; ++j) if (k[j]) { __atomic_fetch_add(p + j, k[j], __ATOMIC_RELAXED); k[j] = 0; }
        bin = ~0ull;
    }
    inline void add(const AlnRec &r)
    {
        uint64_t b;
        if (!rc->place(r, &b)) return;
        if (b != bin) { flush(); bin = b; }
        rc->tally(k, r);
    }
    RowCountsShare *ptr() { return rc ? this : nullptr; }
};

} // namespace pdh
#endif
