// alnstats.h — `-alnstats W`: the CIGAR operations and read lengths of the inputs' records, beside the depth they made.  One accumulator, laid
// out as the engine's (include/pandepth_amd.h: pd_decode_aln_stats — PD_ALNSTAT_WORDS sums, the rule is written there), fed either a record at
// a time by the host readers (add, before any filter `continue`) or a session at a time by the device (add_device); the threaded readers keep
// one per thread and merge.  The CIGAR of a record is the one the reader hands out (host/bam.cpp: the record's own, or the CG tag's by
// htslib's rule).  An aligned record has 0 <= refID < n_ref, flag & -x == 0, mapq >= -q (ReadFilter::pass, the filter's verdict — contigs
// without targets, short contigs and the -g / -b span test play no part), flag & 4 == 0 and at least one operation; a primary one also has
// flag & 0x900 == 0.  q = M I S = X, h = H, L = q + h, a = M I = X, r = M D N = X; clipped: an S or H of length > 0.
#ifndef PD_ALNSTATS_HOST_H_
#define PD_ALNSTATS_HOST_H_
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "bam.h"
#include "../../include/pandepth_amd.h"

namespace pdh {

struct AlnStats {
    enum { RECORDS = PD_ALNSTAT_RECORDS, ALIGNED = PD_ALNSTAT_ALIGNED, PRIMARY = PD_ALNSTAT_PRIMARY, CLIPPED = PD_ALNSTAT_CLIPPED, READ_MAX = PD_ALNSTAT_READ_MAX,
           READ_BASES = PD_ALNSTAT_READ_BASES, ALIGNED_BASES = PD_ALNSTAT_ALIGNED_BASES, REF_BASES = PD_ALNSTAT_REF_BASES, OPS = PD_ALNSTAT_OPS, INS = PD_ALNSTAT_INS,
           DEL = PD_ALNSTAT_DEL, AF = PD_ALNSTAT_AF, RL = PD_ALNSTAT_RL, AL = PD_ALNSTAT_AL, WORDS = PD_ALNSTAT_WORDS, LEN_BINS = PD_ALNSTAT_LEN_BINS,
           INDEL_BINS = PD_ALNSTAT_INDEL_BINS };
    bool on = false;
    uint32_t flag_mask = 0, width = 0; int min_mapq = 0; int32_t n_ref = 0;
    std::vector<uint64_t> sums;

    void init(uint32_t x, int q, uint32_t w, int32_t contigs)
    {
        on = true; flag_mask = x; min_mapq = q; width = w; n_ref = contigs;
        sums.assign((size_t)WORDS, 0);
    }
    void init_like(const AlnStats &o) { if (o.on) init(o.flag_mask, o.min_mapq, o.width, o.n_ref); }
    void bin_len(size_t base, uint64_t v)
    {
        uint64_t b = v / width;
        if (b > (uint64_t)LEN_BINS - 1) b = (uint64_t)LEN_BINS - 1;
        ++sums[base + 2 * b]; sums[base + 2 * b + 1] += v;
    }
    inline void add(const AlnRec &r)
    {
        ++sums[RECORDS];
        if (r.tid < 0 || r.tid >= n_ref || (r.flag & flag_mask) || (int)r.mapq < min_mapq || (r.flag & 4) || r.n_cigar < 1) return;
        uint64_t b[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < r.n_cigar; ++i) {
            const uint32_t code = r.cigar[i] & 0xfu, len = r.cigar[i] >> 4, cls = code <= 8 ? code : 9u;
            ++sums[OPS + 2 * cls]; sums[OPS + 2 * cls + 1] += len; b[cls] += len;
            if (cls == 1 || cls == 2) ++sums[(cls == 1 ? INS : DEL) + (len < (uint32_t)INDEL_BINS ? len : (uint32_t)INDEL_BINS)];
        }
        const uint64_t a = b[0] + b[1] + b[7] + b[8], L = a + b[4] + b[5];
        ++sums[ALIGNED];
        if (b[4] | b[5]) ++sums[CLIPPED];
        sums[ALIGNED_BASES] += a; sums[REF_BASES] += b[0] + b[2] + b[3] + b[7] + b[8];
        bin_len(AL, a);
        if (r.flag & 0x900) return;
        ++sums[PRIMARY]; sums[READ_BASES] += L;
        if (L > sums[READ_MAX]) sums[READ_MAX] = L;
        bin_len(RL, L);
        if (L) ++sums[AF + (size_t)(100 * a / L)];
    }
    void add_device(const uint64_t *s)
    {
        for (size_t i = 0; i < sums.size(); ++i) { if (i == READ_MAX) { if (s[i] > sums[i]) sums[i] = s[i]; } else sums[i] += s[i]; }
    }
    void merge(const AlnStats &o) { if (o.on) add_device(o.sums.data()); }

    // <prefix>.aln.stat.gz: tab-separated, every data line behind a two-letter section tag, every section behind one '#' line naming its columns
    std::string text() const
    {
        auto u = [](uint64_t v) { return std::to_string(v); };
        auto f2 = [](uint64_t a, uint64_t b) { char t[64]; snprintf(t, sizeof t, "%.2f", (double)a / (double)b); return std::string(t); };
        const uint64_t primary = sums[PRIMARY], aligned = sums[ALIGNED], read_bases = sums[READ_BASES];
        std::string s = "# SN\tkey\tvalue\n";
        static const char *const cls[4] = {"records", "aligned", "primary", "clipped"};
        for (int k = 0; k < 4; ++k) s += std::string("SN\t") + cls[k] + "\t" + u(sums[k]) + "\n";
        s += "SN\tflag_mask\t" + u(flag_mask) + "\nSN\tmin_mapq\t" + std::to_string(min_mapq) + "\nSN\tbin_width\t" + u(width) + "\nSN\tlen_bins\t" + u(LEN_BINS) + "\n";
        s += "SN\tread_bases\t" + u(read_bases) + "\n";
        s += "SN\tread_mean\t" + (primary ? f2(read_bases, primary) : std::string("NA")) + "\n";
        s += "SN\tread_max\t" + (primary ? u(sums[READ_MAX]) : std::string("NA")) + "\n";
        std::string n50 = "NA";
        if (read_bases) {
            // down from the last bin: the first bin at which the bins' bases reach half of all is the N50 bin; its lower edge is printed
            const uint64_t half = (read_bases + 1) / 2;
            uint64_t cum = 0;
            for (int b = LEN_BINS - 1; b >= 0; --b) {
                cum += sums[RL + 2 * (size_t)b + 1];
                if (cum >= half) { n50 = (b == LEN_BINS - 1 ? ">=" : "") + u((uint64_t)b * width); break; }
            }
        }
        s += "SN\tread_n50\t" + n50 + "\n";
        s += "SN\taligned_bases\t" + u(sums[ALIGNED_BASES]) + "\n";
        s += "SN\taligned_mean\t" + (aligned ? f2(sums[ALIGNED_BASES], aligned) : std::string("NA")) + "\n";
        s += "SN\tref_bases\t" + u(sums[REF_BASES]) + "\n";
        s += "# OP\top\tops\tbases\n";
        static const char *const ops[10] = {"M", "I", "D", "N", "S", "H", "P", "=", "X", "other"};
        for (int k = 0; k < 10; ++k) s += std::string("OP\t") + ops[k] + "\t" + u(sums[OPS + 2 * k]) + "\t" + u(sums[OPS + 2 * k + 1]) + "\n";
        s += "# ID\tlength\tinsertions\tdeletions\n";
        for (uint32_t b = 0; b <= (uint32_t)INDEL_BINS; ++b)
            if (sums[INS + b] | sums[DEL + b]) s += "ID\t" + (b == (uint32_t)INDEL_BINS ? ">=" + u(b) : u(b)) + "\t" + u(sums[INS + b]) + "\t" + u(sums[DEL + b]) + "\n";
        for (int which = 0; which < 2; ++which) {
            const size_t base = which ? AL : RL;
            const std::string tag = which ? "AL" : "RL";
            s += "# " + tag + "\tfrom\tto\trecords\tbases\n";
            for (uint32_t b = 0; b < (uint32_t)LEN_BINS; ++b) {
                if (!sums[base + 2 * b]) continue;
                const uint64_t from = (uint64_t)b * width;
                s += tag + "\t" + u(from) + "\t" + (b == (uint32_t)LEN_BINS - 1 ? std::string("inf") : u(from + width - 1)) + "\t" + u(sums[base + 2 * b]) + "\t" + u(sums[base + 2 * b + 1]) + "\n";
            }
        }
        s += "# AF\tpercent\trecords\n";
        for (uint32_t p = 0; p <= 100; ++p) if (sums[AF + p]) s += "AF\t" + u(p) + "\t" + u(sums[AF + p]) + "\n";
        return s;
    }
};

} // namespace pdh
#endif
