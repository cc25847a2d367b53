// recstats.h — `-readstats N`: what the RECORDS of the inputs were, beside the depth they made.  One accumulator, laid out as the engine's
// (include/pandepth_amd.h: pd_decode_record_stats — PD_RECSTAT_FIXED + N + 1 sums, 3 words per contig), fed either a record at a time by
// the host readers (add, before any filter `continue`) or a session at a time by the device (add_device); the threaded readers keep one
// per thread and merge.  The classes of a record, in this order, disjoint:
//   unplaced  refID < 0 || refID >= n_ref      dropped_flag  flag & -x      dropped_mapq  mapq < -q      kept  everything else
// `kept` is ReadFilter::pass, the filter's verdict — not whether the record added depth: contigs without targets, contigs shorter than two
// bases and the -g / -b span test play no part.  An insert pair is a kept record with flag & 0x3 == 0x3, flag & 0x908 == 0,
// next_refID == refID and tlen > 0 (-frag's carrying read with no bound); its bin is min(tlen, N).
#ifndef PD_RECSTATS_HOST_H_
#define PD_RECSTATS_HOST_H_
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "bam.h"
#include "../../include/pandepth_amd.h"

namespace pdh {

struct RecStats {
    enum { RECORDS = 0, UNPLACED = 1, DROPPED_FLAG = 2, DROPPED_MAPQ = 3, KEPT = 4, PAIRS = 5, TLEN = 6, FLAG = 7, MAPQ = 19, FIXED = PD_RECSTAT_FIXED };
    bool on = false;
    uint32_t flag_mask = 0, n_bins = 0; int min_mapq = 0; int32_t n_ref = 0;
    std::vector<uint64_t> sums, per;

    void init(uint32_t x, int q, uint32_t n, int32_t contigs)
    {
        on = true; flag_mask = x; min_mapq = q; n_bins = n; n_ref = contigs;
        sums.assign((size_t)FIXED + n + 1, 0); per.assign(3 * (size_t)contigs, 0);
    }
    void init_like(const RecStats &o) { if (o.on) init(o.flag_mask, o.min_mapq, o.n_bins, o.n_ref); }
    inline void add(const AlnRec &r)
    {
        ++sums[RECORDS];
        for (int k = 0; k < 12; ++k) sums[FLAG + k] += (r.flag >> k) & 1u;
        if (r.tid < 0 || r.tid >= n_ref) { ++sums[UNPLACED]; return; }
        ++per[3 * (size_t)r.tid];
        if (r.flag & flag_mask) { ++sums[DROPPED_FLAG]; return; }
        ++sums[MAPQ + r.mapq];
        if ((int)r.mapq < min_mapq) { ++sums[DROPPED_MAPQ]; return; }
        ++sums[KEPT]; ++per[3 * (size_t)r.tid + 1]; per[3 * (size_t)r.tid + 2] += r.mapq;
        if ((r.flag & 0x3) == 0x3 && !(r.flag & 0x908) && r.mtid == r.tid && r.tlen > 0) {
            ++sums[PAIRS]; sums[TLEN] += (uint32_t)r.tlen;
            ++sums[FIXED + ((uint32_t)r.tlen < n_bins ? (uint32_t)r.tlen : n_bins)];
        }
    }
    void add_device(const uint64_t *s, const uint64_t *p)
    {
        for (size_t i = 0; i < sums.size(); ++i) sums[i] += s[i];
        for (size_t i = 0; i < per.size(); ++i) per[i] += p[i];
    }
    void merge(const RecStats &o) { if (o.on) add_device(o.sums.data(), o.per.data()); }

    // <prefix>.reads.stat.gz: tab-separated, every data line behind a two-letter section tag, every section behind one '#' line naming its columns
    std::string text(const std::vector<std::string> &names, const std::vector<uint32_t> &lens) const
    {
        auto u = [](uint64_t v) { return std::to_string(v); };
        auto f2 = [](uint64_t a, uint64_t b) { char t[64]; snprintf(t, sizeof t, "%.2f", (double)a / (double)b); return std::string(t); };
        const uint64_t pairs = sums[PAIRS];
        std::string s = "# SN\tkey\tvalue\n";
        static const char *const cls[5] = {"records", "unplaced", "dropped_flag", "dropped_mapq", "kept"};
        for (int k = 0; k < 5; ++k) s += std::string("SN\t") + cls[k] + "\t" + u(sums[k]) + "\n";
        s += "SN\tflag_mask\t" + u(flag_mask) + "\nSN\tmin_mapq\t" + std::to_string(min_mapq) + "\nSN\tinsert_bins\t" + u(n_bins) + "\nSN\tinsert_pairs\t" + u(pairs) + "\n";
        if (pairs) {
            // the nearest-rank lower median, read from the histogram
            const uint64_t rank = (pairs + 1) / 2;
            uint64_t cum = 0; uint32_t med = n_bins;
            for (uint32_t b = 1; b <= n_bins; ++b) { cum += sums[FIXED + b]; if (cum >= rank) { med = b; break; } }
            s += "SN\tinsert_mean\t" + f2(sums[TLEN], pairs) + "\nSN\tinsert_median\t" + (med == n_bins ? ">=" + u(n_bins) : u(med)) + "\n";
        } else s += "SN\tinsert_mean\tNA\nSN\tinsert_median\tNA\n";
        s += "# FL\tbit\tcount\n";
        for (int k = 0; k < 12; ++k) { char t[16]; snprintf(t, sizeof t, "0x%x", 1u << k); s += std::string("FL\t") + t + "\t" + u(sums[FLAG + k]) + "\n"; }
        s += "# CT\tcontig\tLength\tRecords\tKept\tMeanMapQ\n";
        for (size_t t = 0; t < names.size() && 3 * t + 2 < per.size(); ++t)
            s += "CT\t" + names[t] + "\t" + u(lens[t]) + "\t" + u(per[3 * t]) + "\t" + u(per[3 * t + 1]) + "\t" + (per[3 * t + 1] ? f2(per[3 * t + 2], per[3 * t + 1]) : std::string("NA")) + "\n";
        s += "CT\t*\t0\t" + u(sums[UNPLACED]) + "\t0\tNA\n";
        s += "# MQ\tmapq\tcount\n";
        for (uint32_t q = 0; q < 256; ++q) if (sums[MAPQ + q]) s += "MQ\t" + u(q) + "\t" + u(sums[MAPQ + q]) + "\n";
        s += "# IS\tsize\tcount\n";
        for (uint32_t b = 1; b < n_bins; ++b) if (sums[FIXED + b]) s += "IS\t" + u(b) + "\t" + u(sums[FIXED + b]) + "\n";
        if (sums[FIXED + n_bins]) s += "IS\t>=" + u(n_bins) + "\t" + u(sums[FIXED + n_bins]) + "\n";
        return s;
    }
};

} // namespace pdh
#endif
