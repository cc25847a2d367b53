// pd_alnstats.h — the CIGAR operations and read lengths of the records of a batch (`-alnstats W`, PD_DECODE_ALN_STATS): one more pass over the
// record chain that pd_bamwalk.h's pass 1 has confirmed, and the first record pass that opens a CIGAR.  pd_recstats.h and pd_rowcounts.h stop
// at the 36 fixed bytes of a record; this pass says what a long-read user asks of `samtools stats` (RL, ID, "bases mapped (cigar)") or NanoStat
// in a second read of the file: how long the reads are, how much of each aligned and how much was clipped, and what insertions and deletions
// the alignments carry.
//
// THE RULE (include/pandepth_amd.h: pd_decode_aln_stats; host/alnstats.h and tests/alnstats_model.py say the same).  The CIGAR of a record is its
// own operations, or htslib's CG-tag rule where it applies (cg_tag_cigar of pd_bamwalk.h: a first operation <l_seq>S, refID >= 0, pos >= 0, the
// first CG tag of type B,I / B,i with at least n_cigar_op entries inside the record).  An operation is a 32-bit word, code c = word & 0xf,
// len = word >> 4; its class is c for c <= 8 (M I D N S H P = X) and 9, `other`, for 9 .. 15.  An ALIGNED record has 0 <= refID < n_ref,
// flag & X == 0, mapq >= Q (pd_recstats.h's `kept`), flag & 4 == 0 and at least one operation; a PRIMARY record is an aligned one with
// flag & 0x900 == 0.  Per aligned record, in 64-bit arithmetic: q = sum of len over M I S = X, h = over H, L = q + h, a = over M I = X,
// r = over M D N = X; it is clipped when an S or H has len > 0, which is S's sum + h > 0.  The sums (all u64, index PD_ALNSTAT_*): records,
// aligned, primary, clipped; read_max (max of L over primary), read_bases (sum of L over primary), aligned_bases (sum of a), ref_bases (sum of
// r); ten (operations, bases) pairs; INS[0 .. 256] / DEL[0 .. 256] by min(len, 256); AF[0 .. 100] = floor(100 a / L) of primary records with
// L > 0; RL[b] (records, sum of L) of primary records with min(L / W, 8191) == b; AL[b] the same over all aligned records by a.
//
// THE WALK.  One wave per segment, as in the walk: lane l starts at LaneOut::start of its stretch and goes from record to record by block size
// — the records walk_lane counted for that lane, behind its three bounds checks and a fourth, open_record's 32 + l_name + 4 n_cigar <= bs,
// because this pass reads CIGAR bytes: a record that fails one ends the lane (the fourth: counted as a record, nothing else).  The tag search
// runs for aligned records only.  A record of fewer than COOP_MIN operations is walked by its lane; a longer one is left to the wave as
// run_lanes leaves a Pending: 64 operations per step, lane i takes operation 64 s + i — a 70 000-operation CIGAR is 1 094 steps of the wave,
// not 70 000 of one lane while 63 idle.
//
// WHAT A LANE KEEPS.  Its ten (operations, bases) pairs stay in registers across the whole segment, own records and cooperative strides alike,
// and are reduced ONCE when the segment is through; aligned_bases and ref_bases are sums of those pairs (M I = X, M D N = X) and need no
// accumulator of their own.  What a RECORD needs — a, S's sum and h; q = a + S, L = q + h — is the difference of the lane's class sums across
// the record; for a cooperative record the lanes' differences are reduced (wave_sum64) and the owning lane bins the record.
//
// 64-BIT SUMS THROUGH 32-BIT SCANS.  wave_sum64 adds 64 u64 values as four 16-bit pieces: a piece is below 2^16, so a scan's total is below
// 2^22 and never wraps, and the pieces' totals shifted back add up to the sum modulo 2^64 — exact whenever the true sum is below 2^64, with no
// bound on a single value.  The true sums: a record has fewer than 2^29 operations of less than 2^28 bases, so its sums are below 2^57; the
// operations a segment's wave reads lie in disjoint 4-byte words of the batch's inflated bytes, so a segment's class sums are below
// (avail / 4) * 2^28 — below 2^64 while a batch inflates to less than 2^38 bytes, 256 GiB (a batch is a few hundred MiB).  The hostile
// lengths of the tests, 200 operations of 2^28 - 1 bases in one record, make 2^35.6.  Differences of class sums are taken modulo 2^64 and are
// exact for the same reason.  A piece whose values are all zero skips its scan.
//
// ACCUMULATION.  The workgroup keeps a copy of the fixed words, INS / DEL, AF and the first AS_LDS_BINS bins of RL and AL in LDS as 64-bit words
// (a bin's base sum passes 2^32 with one hostile record, and ds_add_u64 costs what ds_add_u32 does): 21.5 KiB, seven workgroups a CU.  512 bins
// hold every short read at W = 1 — the input where all records hit the same two bins and global atomics would queue on one address; long
// reads spread over the bins and are few, so bins above go straight to global memory.  read_max is a global atomic maximum per segment.
// flush_hist adds the non-zero LDS words with 64-bit global atomics.
//
// The same source compiles for gfx950 and for the host (tests/harness/alnstats_check.cpp).
#ifndef PD_ALNSTATS_H_
#define PD_ALNSTATS_H_
#include "pd_bamwalk.h"                  // PW_FN, the wave classes, Cfg / Seg / LaneOut, rd32 / rd16, cg_tag_cigar, COOP_MIN, SUB, NONE

namespace pdas {

enum { AS_FIXED = PD_ALNSTAT_RL,         // the words before RL: all of them have their LDS copy
       AS_LDS_BINS = 512,                // bins of RL and of AL the workgroup keeps in LDS
       AS_LDS_RL = AS_FIXED, AS_LDS_AL = AS_FIXED + 2 * AS_LDS_BINS,
       AS_LDS_WORDS = AS_FIXED + 4 * AS_LDS_BINS,
       AS_SKIP = 1 };                    // Seg::pad2: the segment belongs to a unit that is handed back (= pdrs::RS_SKIP)
enum { C_M = 0, C_I = 1, C_D = 2, C_N = 3, C_S = 4, C_H = 5, C_P = 6, C_EQ = 7, C_X = 8, C_OTHER = 9, N_CLASS = 10 };

#if defined(__HIP_DEVICE_COMPILE__)
PW_FN void add_u64(unsigned long long *p, unsigned long long v) { atomicAdd(p, v); }
PW_FN void max_u64(unsigned long long *p, unsigned long long v) { atomicMax(p, v); }
#else
PW_FN void add_u64(unsigned long long *p, unsigned long long v) { *p += v; }
PW_FN void max_u64(unsigned long long *p, unsigned long long v) { if (v > *p) *p = v; }
#endif

// what a lane holds across its segment
struct LaneAcc { uint32_t n[N_CLASS]; uint64_t b[N_CLASS]; uint32_t rec, aln, pri, clip; uint64_t read_bases, read_max; };
struct Pend { uint64_t cig_off, next_p; uint32_t n_cig, flag; };

// the sum of the lanes' values modulo 2^64 (the header comment: exact for every sum this pass forms)
template <class W>
PW_FN uint64_t wave_sum64(const typename W::template Var<uint64_t> &x)
{
    typename W::template Var<uint32_t> part;
    uint64_t tot = 0;
    for (int s = 0; s < 64; s += 16) {
        W::each([&](int l) { part[l] = (uint32_t)(x[l] >> s) & 0xFFFFu; });
        if (!W::ballot_ne(part, 0u)) continue;
        uint32_t t = 0;
        (void)W::excl_scan(part, &t);
        tot += (uint64_t)t << s;
    }
    return tot;
}

// one operation of an aligned record: its class pair, and its indel bin (an LDS atomic)
PW_FN void add_op(LaneAcc &A, uint32_t word, unsigned long long *hist)
{
    const uint32_t code = word & 0xfu, len = word >> 4, cls = code <= 8u ? code : (uint32_t)C_OTHER;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)N_CLASS; ++k) { const bool is = cls == k; A.n[k] += is ? 1u : 0u; A.b[k] += is ? (uint64_t)len : 0ull; }
    if (cls == (uint32_t)C_I || cls == (uint32_t)C_D)
        add_u64(hist + (cls == (uint32_t)C_I ? PD_ALNSTAT_INS : PD_ALNSTAT_DEL) + (len < (uint32_t)PD_ALNSTAT_INDEL_BINS ? len : (uint32_t)PD_ALNSTAT_INDEL_BINS), 1ull);
}

PW_FN uint64_t sum_a(const LaneAcc &A) { return A.b[C_M] + A.b[C_I] + A.b[C_EQ] + A.b[C_X]; }

// a record by a length: the pair (records, sum) of bin min(v / width, 8191) — low bins in LDS, the others in global memory
PW_FN void bin_len(unsigned long long *hist, unsigned long long *sums, uint32_t lds_base, uint32_t base, uint64_t v, uint32_t width)
{
    uint64_t b = v / width;
    if (b > (uint64_t)PD_ALNSTAT_LEN_BINS - 1) b = (uint64_t)PD_ALNSTAT_LEN_BINS - 1;
    unsigned long long *const at = b < (uint64_t)AS_LDS_BINS ? hist + lds_base + 2 * b : sums + base + 2 * b;
    add_u64(at, 1ull);
    if (v) add_u64(at + 1, v);
}

// one aligned record whose sums are known: a, S's sum, h
PW_FN void bin_record(LaneAcc &A, uint32_t flag, uint64_t a, uint64_t s, uint64_t h, uint32_t width, unsigned long long *sums, unsigned long long *hist)
{
    const uint64_t L = a + s + h;
    ++A.aln;
    if (s | h) ++A.clip;
    bin_len(hist, sums, AS_LDS_AL, PD_ALNSTAT_AL, a, width);
    if (flag & 0x900u) return;
    ++A.pri; A.read_bases += L;
    if (L > A.read_max) A.read_max = L;
    bin_len(hist, sums, AS_LDS_RL, PD_ALNSTAT_RL, L, width);
    if (L) add_u64(hist + PD_ALNSTAT_AF + (uint32_t)(100ull * a / L), 1ull);             // (a <= L < 2^57: 100 a does not wrap)
}

// Records starting in [p, b), from where the lane stands.  Returns true when it has stopped AT an aligned record whose CIGAR the wave is to walk
// (`pd` says which; the record is counted in A.rec, nothing else of it yet) and false when the lane is through.
PW_FN bool walk_lane(const pdb2::Cfg &c, uint64_t &p, uint64_t b, uint32_t &guard, LaneAcc &A, Pend &pd, uint32_t width, unsigned long long *sums, unsigned long long *hist)
{
    using namespace pdb2;
    for (; p < b && guard < SUB / 36 + 2; ++guard) {
        // (walk_lane's checks before it opens a record; none of them fails in a counted unit)
        if (p + 36 > c.avail) break;
        const uint8_t *r = c.buf + p;
        const uint32_t bs = rd32(r);
        if (bs < 32 || bs > (1u << 29)) break;
        if (p + 4 + (uint64_t)bs > c.avail) break;
        ++A.rec;
        const uint32_t l_name = r[12], mapq = r[13], flag = rd16(r + 18);
        uint32_t n_cig = rd16(r + 16);
        if ((uint64_t)32 + l_name + 4ull * n_cig > bs) break;                             // (open_record's: the CIGAR would leave the record)
        const int32_t tid = (int32_t)rd32(r + 4);
        if (tid >= 0 && tid < c.n_ref && !(flag & c.flag_mask) && (int32_t)mapq >= c.min_mapq && !(flag & 4u) && n_cig >= 1) {
            const uint8_t *cig = r + 36 + l_name;
            const uint32_t l_seq = rd32(r + 20);
            if ((int32_t)rd32(r + 8) >= 0 && (rd32(cig) & 0xf) == 4 && (rd32(cig) >> 4) == l_seq) cg_tag_cigar(c.buf, p, bs, l_name, l_seq, cig, n_cig);
            if (n_cig >= (uint32_t)COOP_MIN) {
                pd.cig_off = (uint64_t)(cig - c.buf); pd.next_p = p + 4 + (uint64_t)bs; pd.n_cig = n_cig; pd.flag = flag;
                ++guard;
                return true;
            }
            const uint64_t a0 = sum_a(A), s0 = A.b[C_S], h0 = A.b[C_H];
            for (uint32_t i = 0; i < n_cig; ++i) add_op(A, rd32(cig + 4 * i), hist);
            bin_record(A, flag, sum_a(A) - a0, A.b[C_S] - s0, A.b[C_H] - h0, width, sums, hist);
        }
        p += 4 + (uint64_t)bs;
    }
    return false;
}

// One wave, one segment whose chain is confirmed.  hist: the workgroup's LDS copy (AS_LDS_WORDS words), zeroed before, flushed behind.
template <class W>
PW_FN void stats_segment(const pdb2::Cfg &cfg, const pdb2::Seg &sg, const pdb2::LaneOut *lanes, uint32_t width, unsigned long long *sums, unsigned long long *hist)
{
    using namespace pdb2;
    typedef typename W::template Var<uint32_t> U;
    typedef typename W::template Var<uint64_t> U64;
    Cfg c = cfg; c.avail = sg.avail;
    typename W::template Var<LaneAcc> acc;
    U active, guard, pending, pn, pflag;
    U64 p, bb, pcig, pnext;
    W::each([&](int l) {
        LaneAcc &A = acc[l];
#pragma unroll
        for (int k = 0; k < N_CLASS; ++k) { A.n[k] = 0; A.b[k] = 0; }
        A.rec = A.aln = A.pri = A.clip = 0; A.read_bases = A.read_max = 0;
        const uint64_t a = sg.begin + (uint64_t)l * SUB;
        const uint64_t b = a + SUB < sg.end ? a + SUB : sg.end;
        const uint64_t s = lanes[l].start;
        active[l] = a < sg.end && s != NONE && s < b ? 1u : 0u;
        p[l] = s; bb[l] = b; guard[l] = 0; pending[l] = 0; pn[l] = 0; pflag[l] = 0; pcig[l] = 0; pnext[l] = 0;
    });
    for (;;) {
        W::each([&](int l) {
            if (!active[l]) return;
            Pend pd; pd.cig_off = 0; pd.next_p = 0; pd.n_cig = 0; pd.flag = 0;
            uint64_t pp = p[l]; uint32_t g = guard[l];
            const bool stop = walk_lane(c, pp, bb[l], g, acc[l], pd, width, sums, hist);
            p[l] = pp; guard[l] = g;
            pending[l] = stop ? 1u : 0u;
            if (stop) { pcig[l] = pd.cig_off; pnext[l] = pd.next_p; pn[l] = pd.n_cig; pflag[l] = pd.flag; }
            else active[l] = 0;
        });
        uint64_t pm = W::ballot_ne(pending, 0u);
        if (!pm) break;
        while (pm) {
            // the record lane j stands at, by the whole wave: lane i takes operations i, 64 + i, ... into its own class pairs
            const int j = ctz64(pm);
            pm &= pm - 1;
            const uint64_t cig_off = W::bcast64(pcig, j);
            const uint32_t n = W::bcast(pn, j);
            U64 da, ds, dh;
            W::each([&](int l) { da[l] = sum_a(acc[l]); ds[l] = acc[l].b[C_S]; dh[l] = acc[l].b[C_H]; });
            for (uint32_t k0 = 0; k0 < n; k0 += 64)
                W::each([&](int l) { const uint32_t i = k0 + (uint32_t)l; if (i < n) add_op(acc[l], rd32(c.buf + cig_off + 4ull * i), hist); });
            W::each([&](int l) { da[l] = sum_a(acc[l]) - da[l]; ds[l] = acc[l].b[C_S] - ds[l]; dh[l] = acc[l].b[C_H] - dh[l]; });
            const uint64_t a = wave_sum64<W>(da), s = wave_sum64<W>(ds), h = wave_sum64<W>(dh);
            W::each([&](int l) {
                if (l != j) return;
                bin_record(acc[l], pflag[l], a, s, h, width, sums, hist);
                p[l] = pnext[l]; pending[l] = 0;
            });
        }
    }
    // the segment's totals: one reduction per counter and per class that occurred, one LDS add each
    U64 v;
    U any;
    uint64_t fixed[8], ops[2 * N_CLASS];
    const auto total = [&](auto get) { W::each([&](int l) { v[l] = get(acc[l]); }); return wave_sum64<W>(v); };
    fixed[PD_ALNSTAT_RECORDS] = total([](const LaneAcc &A) { return (uint64_t)A.rec; });
    fixed[PD_ALNSTAT_ALIGNED] = total([](const LaneAcc &A) { return (uint64_t)A.aln; });
    fixed[PD_ALNSTAT_PRIMARY] = total([](const LaneAcc &A) { return (uint64_t)A.pri; });
    fixed[PD_ALNSTAT_CLIPPED] = total([](const LaneAcc &A) { return (uint64_t)A.clip; });
    fixed[PD_ALNSTAT_READ_BASES] = total([](const LaneAcc &A) { return A.read_bases; });
    W::each([&](int l) { v[l] = acc[l].read_max; });
    fixed[PD_ALNSTAT_READ_MAX] = W::reduce_max64(v);
#pragma unroll
    for (int k = 0; k < N_CLASS; ++k) {
        W::each([&](int l) { any[l] = acc[l].n[k]; });
        ops[2 * k] = ops[2 * k + 1] = 0;
        if (!W::ballot_ne(any, 0u)) continue;
        W::each([&](int l) { v[l] = acc[l].n[k]; });
        ops[2 * k] = wave_sum64<W>(v);
        W::each([&](int l) { v[l] = acc[l].b[k]; });
        ops[2 * k + 1] = wave_sum64<W>(v);
    }
    fixed[PD_ALNSTAT_ALIGNED_BASES] = ops[2 * C_M + 1] + ops[2 * C_I + 1] + ops[2 * C_EQ + 1] + ops[2 * C_X + 1];
    fixed[PD_ALNSTAT_REF_BASES] = ops[2 * C_M + 1] + ops[2 * C_D + 1] + ops[2 * C_N + 1] + ops[2 * C_EQ + 1] + ops[2 * C_X + 1];
    W::each([&](int l) {
        if (l != 0) return;
        for (int k = 0; k < 8; ++k) if (k != PD_ALNSTAT_READ_MAX && fixed[k]) add_u64(hist + k, fixed[k]);
        if (fixed[PD_ALNSTAT_READ_MAX]) max_u64(sums + PD_ALNSTAT_READ_MAX, fixed[PD_ALNSTAT_READ_MAX]);
        for (int k = 0; k < 2 * N_CLASS; ++k) if (ops[k]) add_u64(hist + PD_ALNSTAT_OPS + k, ops[k]);
    });
}

// the workgroup's LDS copy into the sums: thread t of n takes every n-th word (the caller has waited for the workgroup's waves)
PW_FN void flush_hist(const unsigned long long *hist, unsigned long long *sums, uint32_t t, uint32_t n)
{
    for (uint32_t i = t; i < (uint32_t)AS_LDS_WORDS; i += n) {
        const unsigned long long x = hist[i];
        if (!x) continue;
        const uint32_t g = i < (uint32_t)AS_LDS_RL ? i : i < (uint32_t)AS_LDS_AL ? (uint32_t)PD_ALNSTAT_RL + (i - (uint32_t)AS_LDS_RL) : (uint32_t)PD_ALNSTAT_AL + (i - (uint32_t)AS_LDS_AL);
        add_u64(sums + g, x);
    }
}

} // namespace pdas
#endif
