// pd_recstats.h — statistics of the RECORDS of a batch (`-readstats`, PD_DECODE_RECORD_STATS): one more pass over the record chain that
// pd_bamwalk.h's pass 1 has confirmed.  Where the walk passes describe depth, this pass describes what the depth is made from: how many
// records there were, how many each filter dropped, how many every contig got, the MAPQ distribution `-q` chooses in and the insert sizes
// `-fragmax` is set from.  It reads the 36 fixed bytes of every record (refID, pos, mapq, flag, next_refID, tlen) and no CIGAR.
//
// One wave per segment, as in the walk: lane l starts at LaneOut::start of its stretch and goes from record to record by block size until
// the stretch ends — exactly the records walk_lane counted in n_rec for that lane, opened behind the same three bounds checks.  A counted
// unit has no record that stops the chain (WF_MORE / WF_BAD); should one turn up, the lane stops there and reads nothing behind it.
//
// The classes of a record, in this order, disjoint (n_ref: contigs of the header, X: the flag mask, Q: the mapq bound):
//   unplaced  refID < 0 || refID >= n_ref        dropped_flag  flag & X        dropped_mapq  mapq < Q        kept  everything else
// `kept` is the FILTER's verdict, not the walk's keep: contigs without targets, contigs of fewer than two bases and the -g / -b span test
// play no part.  An INSERT PAIR is a kept record with flag & 0x3 == 0x3, flag & 0x908 == 0, next_refID == refID and tlen > 0 (-frag's
// carrying read with no bound); its bin is min(tlen, N), N = the session's "decode_isize_bins".
//
// The sums (all u64, integers: the result does not depend on the order of the atomics), index = RS_*:
//   [RS_RECORDS .. RS_KEPT] the classes and their total, RS_PAIRS / RS_TLEN the insert pairs and the sum of their tlen, RS_FLAG + k the
//   records with flag bit 1 << k (k < 12, all records), RS_MAPQ + q the placed records that pass the flag mask with mapq q,
//   RS_FIXED + b the insert pairs of bin b (0 .. N; bin 0 stays 0, bin N is ">= N"); and per contig t, per_contig[3 t ..]: records with
//   that refID, kept ones, the sum of the kept ones' mapq.
// Accumulation: a lane counts in registers; the wave reduces the counters and adds them to the workgroup's LDS copy of the sums' first
// RS_FIXED + RS_LDS_BINS words, where the lanes' MAPQ and insert bins go with LDS atomics as the records are read; insert bins at or above
// RS_LDS_BINS, the sum of tlen and the contig triples (run-length in the lane: a sorted file changes contig a handful of times; the
// lanes that end on the wave's commonest contig are reduced first) go to global memory.  flush_hist then adds the non-zero LDS words.
//
// The same source compiles for gfx950 and for the host (tests/harness/recstats_check.cpp).
#ifndef PD_RECSTATS_H_
#define PD_RECSTATS_H_
#include "pd_bamwalk.h"                  // PW_FN, the wave classes, Cfg / Seg / LaneOut, rd32 / rd16, SUB, NONE

namespace pdrs {

enum { RS_RECORDS = 0, RS_UNPLACED = 1, RS_DROPPED_FLAG = 2, RS_DROPPED_MAPQ = 3, RS_KEPT = 4, RS_PAIRS = 5, RS_TLEN = 6, RS_FLAG = 7, RS_MAPQ = 19,
       RS_FIXED = PD_RECSTAT_FIXED,
       RS_LDS_BINS = 2048,               // insert bins the workgroup keeps in LDS (read pairs of a short-read library lie far below it)
       RS_LDS_WORDS = RS_FIXED + RS_LDS_BINS,
       RS_SKIP = 1 };                    // Seg::pad2: the segment belongs to a unit that is handed back — nothing of it is counted
static_assert(RS_MAPQ + 256 == RS_FIXED, "the fixed sums end with the 256 MAPQ bins");

#if defined(__HIP_DEVICE_COMPILE__)
PW_FN void add_u64(unsigned long long *p, unsigned long long v) { atomicAdd(p, v); }
PW_FN void add_u32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
#else
PW_FN void add_u64(unsigned long long *p, unsigned long long v) { *p += v; }
PW_FN void add_u32(uint32_t *p, uint32_t v) { *p += v; }
#endif

// words of the LDS copy a session with n_bins insert bins uses
PW_FN uint32_t lds_words(uint32_t n_bins) { return (uint32_t)RS_FIXED + (n_bins + 1u < (uint32_t)RS_LDS_BINS ? n_bins + 1u : (uint32_t)RS_LDS_BINS); }

// one contig triple to global memory
PW_FN void add_contig(unsigned long long *per_contig, uint32_t tid, uint32_t n_rec, uint32_t n_kept, uint32_t mq)
{
    if (n_rec) add_u64(per_contig + 3ull * tid, n_rec);
    if (n_kept) add_u64(per_contig + 3ull * tid + 1, n_kept);
    if (mq) add_u64(per_contig + 3ull * tid + 2, mq);
}

// One wave, one segment whose chain is confirmed.  hist: the workgroup's copy of sums[0 .. lds_words(n_bins)), zeroed before, flushed behind.
template <class W>
PW_FN void stats_segment(const pdb2::Cfg &cfg, const pdb2::Seg &sg, const pdb2::LaneOut *lanes, uint32_t n_bins, unsigned long long *sums,
                         unsigned long long *per_contig, uint32_t *hist)
{
    using namespace pdb2;
    typedef typename W::template Var<uint32_t> U;
    const uint8_t *const buf = cfg.buf;
    const uint64_t avail = sg.avail;
    U cnt[RS_PAIRS + 1], fb[12], tl_lo, tl_hi, ct_tid, ct_rec, ct_kept, ct_mq;
    W::each([&](int l) {
        uint32_t k[RS_PAIRS + 1] = {0, 0, 0, 0, 0, 0}, f[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint64_t tlen_sum = 0;
        uint32_t cur = 0xFFFFFFFFu, c_rec = 0, c_kept = 0, c_mq = 0;             // the lane's open contig triple
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
                const int32_t tid = (int32_t)rd32(r + 4);
                const uint32_t mapq = r[13], flag = rd16(r + 18);
                ++k[RS_RECORDS];
#pragma unroll
                for (int j = 0; j < 12; ++j) f[j] += (flag >> j) & 1u;
                if (tid < 0 || tid >= cfg.n_ref) ++k[RS_UNPLACED];
                else {
                    if ((uint32_t)tid != cur) {
                        if (cur != 0xFFFFFFFFu) add_contig(per_contig, cur, c_rec, c_kept, c_mq);
                        cur = (uint32_t)tid; c_rec = c_kept = c_mq = 0;
                    }
                    ++c_rec;
                    if (flag & cfg.flag_mask) ++k[RS_DROPPED_FLAG];
                    else {
                        add_u32(hist + RS_MAPQ + mapq, 1u);
                        if ((int32_t)mapq < cfg.min_mapq) ++k[RS_DROPPED_MAPQ];
                        else {
                            ++k[RS_KEPT]; ++c_kept; c_mq += mapq;
                            const int32_t mtid = (int32_t)rd32(r + 24), tlen = (int32_t)rd32(r + 32);
                            if ((flag & 0x3) == 0x3 && !(flag & 0x908) && mtid == tid && tlen > 0) {
                                ++k[RS_PAIRS]; tlen_sum += (uint32_t)tlen;
                                const uint32_t bin = (uint32_t)tlen < n_bins ? (uint32_t)tlen : n_bins;
                                if (bin < (uint32_t)RS_LDS_BINS) add_u32(hist + RS_FIXED + bin, 1u);
                                else add_u64(sums + RS_FIXED + bin, 1ull);
                            }
                        }
                    }
                }
                p += 4 + (uint64_t)bs;
            }
        }
        for (int j = 0; j <= RS_PAIRS; ++j) cnt[j][l] = k[j];
        for (int j = 0; j < 12; ++j) fb[j][l] = f[j];
        tl_lo[l] = (uint32_t)(tlen_sum & 0xFFFFFu); tl_hi[l] = (uint32_t)(tlen_sum >> 20);      // (a lane's sum stays below 2^38: two halves a 32-bit scan holds)
        ct_tid[l] = cur; ct_rec[l] = c_rec; ct_kept[l] = c_kept; ct_mq[l] = c_mq;
    });
    // the counters: wave totals, one LDS add per counter
    uint32_t tot[RS_PAIRS + 1], ftot[12], lo = 0, hi = 0;
    for (int j = 0; j <= RS_PAIRS; ++j) (void)W::excl_scan(cnt[j], &tot[j]);
    for (int j = 0; j < 12; ++j) (void)W::excl_scan(fb[j], &ftot[j]);
    (void)W::excl_scan(tl_lo, &lo);
    (void)W::excl_scan(tl_hi, &hi);
    // the contig triples the lanes still hold: those of the first such lane's contig are reduced, the others go singly
    const uint64_t has = W::ballot_ne(ct_tid, 0xFFFFFFFFu);
    uint32_t t0 = 0xFFFFFFFFu, r_rec = 0, r_kept = 0, r_mq = 0;
    if (has) {
        t0 = W::bcast(ct_tid, ctz64(has));
        U x, y, z;
        W::each([&](int l) {
            const bool same = ct_tid[l] == t0;
            x[l] = same ? ct_rec[l] : 0u; y[l] = same ? ct_kept[l] : 0u; z[l] = same ? ct_mq[l] : 0u;
            if (!same && ct_tid[l] != 0xFFFFFFFFu) add_contig(per_contig, ct_tid[l], ct_rec[l], ct_kept[l], ct_mq[l]);
        });
        (void)W::excl_scan(x, &r_rec); (void)W::excl_scan(y, &r_kept); (void)W::excl_scan(z, &r_mq);
    }
    W::each([&](int l) {
        if (l != 0) return;
        for (int j = 0; j <= RS_PAIRS; ++j) if (tot[j]) add_u32(hist + j, tot[j]);
        for (int j = 0; j < 12; ++j) if (ftot[j]) add_u32(hist + RS_FLAG + j, ftot[j]);
        const uint64_t tl = (uint64_t)lo + ((uint64_t)hi << 20);
        if (tl) add_u64(sums + RS_TLEN, tl);
        if (has) add_contig(per_contig, t0, r_rec, r_kept, r_mq);
    });
}

// the workgroup's LDS copy into the sums: thread t of n takes every n-th word (the caller has waited for the workgroup's waves)
PW_FN void flush_hist(const uint32_t *hist, uint32_t n_words, unsigned long long *sums, uint32_t t, uint32_t n)
{
    for (uint32_t i = t; i < n_words; i += n) { const uint32_t v = hist[i]; if (v) add_u64(sums + i, v); }
}

} // namespace pdrs
#endif
