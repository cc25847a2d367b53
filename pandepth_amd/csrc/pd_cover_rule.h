// pd_cover_rule.h — when is a tile of the direct depth pass COVERED by its candidates, decided from the runs alone (no per-cell depth)?
//
// k_direct_c8's cover pass (pd_direct.hip) and tests/harness/cover_rule_check.cpp (against a per-cell union, on the CPU) share this code.
//
// The candidates of a tile are lo words r = (b & 0xFFFF) | (len << 16) (pd_kernels.h) and p0 is the low 16 bits of the tile's first flat
// cell.  In the kernel's own 16-bit arithmetic sb = (r - p0) & 0xFFFF is < tile for the tile's own runs and lies in [2^16 - bucket, 2^16)
// for the runs of the bucket before it, which stand for NEGATIVE begins: begin = (int16)sb, end = begin + (r >> 16), both tile-relative.
//
// The rule: sweep the runs in the order they are stored, reach = 0; a run with begin > reach is a GAP, any other run makes
// reach = max(reach, end).  With no gap and reach >= tile at the end, every cell of [0, tile) lies in some run — by induction [0, reach) is
// covered after every run, whatever the order of the runs, so a stream that is not sorted after all can only make the rule decline.  On a
// stream sorted by begin the rule is exact.  A run without cells is swept like any other: its end equals its begin, so it never
// extends the reach past a cell that is not covered, and where it begins beyond the reach the next run with cells begins there too.
//
// The kernel sweeps a tile's sorted candidates as ONE segment (a wave per tile), so for it the rule is exact.
// A sweep may also be cut into SEGMENTS of consecutive runs (the CPU check does, 1 - 4 of them).  A segment judges its gaps by its own running maximum,
// which starts at its first begin; combine() then asks of every segment, in order, that its first begin is within the reach of those before
// it.  That declines some covered tiles (a run reached only by an earlier segment's maximum), never the reverse.
// The sum of the lengths clipped to the tile (the tile's TotalDepth when nothing wraps) and the number of runs that begin before the tile
// and reach its first cell (the window path's carry-in) need no order at all.  The cover pass itself needs no carry — a settled tile's depths
// are never formed — and does not compute one (it passes 0); seg_add keeps it so that the CPU check can hold the 16-bit carry test against the cells.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PD_COVER_HD __host__ __device__
#else
#define PD_COVER_HD
#endif

namespace pdcover {

constexpr int NONE = -32768;                    // below every begin and end of a candidate (a look-back begin is >= -8192)

struct Seg {                                    // the summary of consecutive runs of one stream
    int first;                                  // the first run's begin (NONE: no run)
    int maxend;                                 // the largest end (NONE: no run)
    int gap;                                    // != 0: a run began in the tile, beyond the running maximum of the runs before it in this segment
    uint32_t sum;                               // lengths clipped to [0, tile)
    uint32_t carry;                             // runs with begin < 0 <= end
};
struct Tile { bool covered; uint32_t sum, carry; };

PD_COVER_HD inline Seg seg_none() { return Seg{NONE, NONE, 0, 0u, 0u}; }
PD_COVER_HD inline int run_begin(uint32_t r, uint32_t p0) { return (int)(int16_t)(uint16_t)(r - p0); }
PD_COVER_HD inline int run_end(uint32_t r, int begin) { return begin + (int)(r >> 16); }
// |[b, e) ∩ [0, tile)|, for b < tile and b <= e
PD_COVER_HD inline uint32_t run_clipped(int b, int e, int tile)
{
    const int hi = e < 0 ? 0 : (e > tile ? tile : e), lo = b < 0 ? 0 : b;
    return (uint32_t)(hi - lo);
}
// a run that changes no summary it is swept into (the kernel puts it in the places of a partial chunk that hold no run of the lane's own)
PD_COVER_HD inline uint32_t run_neutral(uint32_t p0) { return (p0 + 0x8000u) & 0xFFFFu; }

PD_COVER_HD inline void seg_add(Seg &s, uint32_t r, uint32_t p0, int tile)
{
    const int b = run_begin(r, p0), e = run_end(r, b);
    if (b == NONE) return;                      // run_neutral
    if (s.first == NONE) { s.first = b; s.maxend = b; }
    if (b > s.maxend && b > 0) s.gap = 1;       // (nothing before cell 0 has to be covered)
    if (e > s.maxend) s.maxend = e;
    s.sum += run_clipped(b, e, tile);
    s.carry += (b < 0 && e >= 0) ? 1u : 0u;     // == ((r - p0) & 0xFFFF) + (r >> 16) >= 2^16 for a run no longer than a bucket
}

PD_COVER_HD inline Seg seg_sweep(const uint32_t *lo, uint32_t n, uint32_t p0, int tile)
{
    Seg s = seg_none();
    for (uint32_t i = 0; i < n; ++i) seg_add(s, lo[i], p0, tile);
    return s;
}

// The tile's answer from the summaries of the sorted stream's segments, in order, and of the other stream's, in any order.  The other
// stream gives its sums only: what it covers is ignored, so a gap that only one of its runs closes declines the tile.
PD_COVER_HD inline Tile combine(const Seg *sorted, int n_sorted, const Seg *other, int n_other, int tile)
{
    Tile t{true, 0u, 0u};
    int reach = 0;
    for (int k = 0; k < n_sorted; ++k) {
        const Seg &s = sorted[k];
        t.sum += s.sum; t.carry += s.carry;
        if (s.first == NONE) continue;
        if (s.gap || s.first > reach) t.covered = false;
        if (s.maxend > reach) reach = s.maxend;
    }
    if (reach < tile) t.covered = false;
    for (int k = 0; k < n_other; ++k) { t.sum += other[k].sum; t.carry += other[k].carry; }
    return t;
}

// ---- the NARROW plane of the sorted stream: two bytes per run (C8Sample::nar) ----
// nar[i] = (begin & 0xFF) | (min(len, 255) << 8), begin and len as in the lo word.  The narrow form of the cover pass sweeps a tile's sorted candidates
// from these half-words alone: it knows the first candidate's begin (one lo word) and REBUILDS every other one by adding the differences of
// consecutive low bytes, each taken modulo 256.  Lengths are exact for a sample without a sorted run longer than 255 cells (the producers count
// those: pd_runs::n_wide_sorted, and only a sample with none is swept this way).
// The stream is sorted, so every true difference is >= 0 and a rebuilt difference is the true one minus a multiple of 256: never larger.  Hence
//   * every rebuilt begin is <= its true begin, and equal while no difference has reached 256;
//   * the rebuilt begin of the LAST candidate equals its true begin (a second lo word) if and only if no difference reached 256: the END CHECK.
// A too-small begin can by itself only close a true gap, never open one (behind the first hidden difference every begin and end is shifted down by the
// same amount, those in front are exact), so a gap the narrow sweep meets is a true gap and needs no check; a tile is settled only when the sweep
// met no gap AND the end check passed, and then every begin, end and clipped length it used was the true one.  A difference of exactly 256
// rebuilds as 0: the case the check exists for.  The span of a tile's candidates is below a tile plus a bucket, so the comparison is exact in ints.
PD_COVER_HD inline uint32_t nar_pack(uint32_t begin, uint32_t len) { return (begin & 0xFFu) | ((len < 255u ? len : 255u) << 8); }
PD_COVER_HD inline uint32_t nar_of_lo(uint32_t lo_word) { return nar_pack(lo_word & 0xFFFFu, lo_word >> 16); }
PD_COVER_HD inline bool nar_is_wide(uint32_t len) { return len > 255u; }          // a run the half-word cannot hold
// the rebuild step: how far the run of half-word h begins behind its predecessor, whose half-word (or low byte) is prev
PD_COVER_HD inline int nar_step(uint32_t h, uint32_t prev) { return (int)((h - prev) & 255u); }
PD_COVER_HD inline int nar_len(uint32_t h) { return (int)((h >> 8) & 255u); }
// what stands in a place of a partial chunk that holds no run of the lane's own: the predecessor's low byte with length 0 (a step of 0, an empty run)
PD_COVER_HD inline uint32_t nar_neutral(uint32_t prev) { return prev & 255u; }
// the end check: rebuilt_last is the rebuilt tile-relative begin of the tile's last sorted candidate, lo_last that candidate's lo word
PD_COVER_HD inline bool nar_end_ok(int rebuilt_last, uint32_t lo_last, uint32_t p0) { return rebuilt_last == run_begin(lo_last, p0); }

// One sweep of n sorted candidates from their half-words, as the kernel's narrow form does it (ONE segment); lo_first and lo_last are the lo
// words of the first and the last of them.  begins (may be null) receives the rebuilt begins.  *end_ok: the end check.
PD_COVER_HD inline Seg seg_sweep_nar(const uint16_t *nar, uint32_t n, uint32_t lo_first, uint32_t lo_last, uint32_t p0, int tile, bool *end_ok, int *begins)
{
    Seg s = seg_none();
    *end_ok = true;
    if (!n) return s;
    int b = run_begin(lo_first, p0);
    uint32_t prev = lo_first;
    for (uint32_t i = 0; i < n; ++i) {
        b += nar_step(nar[i], prev); prev = nar[i];
        const int e = b + nar_len(nar[i]);
        if (begins) begins[i] = b;
        if (s.first == NONE) { s.first = b; s.maxend = b; }
        if (b > s.maxend && b > 0) s.gap = 1;
        if (e > s.maxend) s.maxend = e;
        s.sum += run_clipped(b, e, tile);
        s.carry += (b < 0 && e >= 0) ? 1u : 0u;
    }
    *end_ok = nar_end_ok(b, lo_last, p0);
    return s;
}

// ---- the FAST CHUNK of the narrow sweep: a full chunk (512 runs, eight consecutive runs per lane, 64 lanes) settled without a begin per run ----
// A lane holds its eight half-words as four words x[0 .. 3] (run 2j in the low half of x[j]).  Everything below is relative to the lane's
// PREDECESSOR, the run in front of the lane's first (the lane before's last; lane 0: the last run of the chunk before, or the tile's first candidate):
//   rb[k]  the rebuilt begin of the lane's run k minus the predecessor's — the prefix sum of the low-byte differences, each modulo 256;
//   T      = rb[7], the lane's last begin;   Mrel = max_k(rb[k] + len[k]), the lane's largest end;   lens = the sum of the eight lengths.
// With `base` the rebuilt begin of the run before the chunk, lane l's last begin is lane_last = base + T_0 + .. + T_l and its largest end is
// lane_last - T_l + Mrel_l: two wave scans give every lane P = max(reach, largest end of the lanes before it) and the chunk its largest end, top.
// The chunk is ACCEPTED when base >= 0, every lane has lane_last <= P, and top <= tile.  Then the rule (seg_sweep_nar) leaves exactly: no new gap,
// reach = max(reach, top), sum += the lengths, because
//   * every begin of a lane is <= its last (the steps are >= 0) <= P <= the running maximum the rule would compare it with: no run is a gap;
//   * the rebuilt begins never decrease, so base >= 0 puts every begin at or behind cell 0: nothing is clipped in front;
//   * top <= tile: no end is clipped behind.  The clipped sum is the sum of the length bytes.
// A chunk that is not accepted says nothing (a gap inside a lane may be closed by a long run of an earlier lane): it goes through the rule itself.
struct NarLane { int T, Mrel; uint32_t lens; };

// the two steps of a word: x holds two runs' half-words, y their predecessors' (y = (x << 16) | (the word before >> 16)); the low byte of each half of
// the result is that run's step (nar_step), the high bytes mean nothing.  (A packed 16-bit subtraction: v_pk_sub_u16.)
PD_COVER_HD inline uint32_t nar_pair_steps(uint32_t x, uint32_t y)
{
    typedef unsigned short u16x2 __attribute__((vector_size(4)));
    u16x2 a, b;
    __builtin_memcpy(&a, &x, 4); __builtin_memcpy(&b, &y, 4);
    a -= b;
    uint32_t d;
    __builtin_memcpy(&d, &a, 4);
    return d;
}
// the predecessors' word of x, `before` being the word in front of it (for a lane's first word: the lane before's last; the predecessor alone: << 16)
PD_COVER_HD inline uint32_t nar_pred_word(uint32_t x, uint32_t before) { return (x << 16) | (before >> 16); }
// x . (0, 1, 0, 1) over bytes: the two lengths of a word, added to acc (v_dot4_u32_u8 with the selector NAR_LEN_SEL)
constexpr uint32_t NAR_LEN_SEL = 0x01000100u;
PD_COVER_HD inline uint32_t nar_add_lens(uint32_t x, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(x, NAR_LEN_SEL, acc, false);
#else
    for (int k = 0; k < 4; ++k) acc += ((x >> (8 * k)) & 255u) * ((NAR_LEN_SEL >> (8 * k)) & 255u);
    return acc;
#endif
}
// the lane's summary from its four words and `before`, whose HIGH half is the predecessor's half-word
PD_COVER_HD inline NarLane nar_lane_summary(const uint32_t (&x)[4], uint32_t before)
{
    NarLane s{0, NONE, 0u};
    int rb = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t d = nar_pair_steps(x[j], nar_pred_word(x[j], j ? x[j - 1] : before));
        rb += (int)(d & 255u);
        const int e0 = rb + (int)((x[j] >> 8) & 255u);
        rb += (int)((d >> 16) & 255u);
        const int e1 = rb + (int)(x[j] >> 24);
        const int m = e0 > e1 ? e0 : e1;
        s.Mrel = s.Mrel > m ? s.Mrel : m;
        s.lens = nar_add_lens(x[j], s.lens);
    }
    s.T = rb;
    return s;
}
// may a chunk of cnt runs behind a run that begins at base be tried at all? (wave-uniform, known before any work)
PD_COVER_HD inline bool chunk_fast_entry(uint32_t cnt, int base) { return cnt == 512u && base >= 0; }
// one lane's part of the test: before = the largest end of the lanes before it (NONE for lane 0)
PD_COVER_HD inline bool chunk_fast_lane_ok(int lane_last, int before, int reach) { return !(lane_last > (before > reach ? before : reach)); }
// the acceptance test: every lane's part held, and the chunk's largest end lies in the tile
PD_COVER_HD inline bool chunk_fast_ok(bool every_lane_ok, int top, int tile) { return every_lane_ok && top <= tile; }

// The sweep's state between chunks, and the fast chunk on it, lane after lane (the kernel's wave does the two scans with DPP): true and the state
// moved when the chunk was accepted, false and NOTHING changed otherwise.  nar: the chunk's 512 half-words; pb: the half-word of the run before it.
struct NarState { int base, reach; uint32_t pb, sum; int gap; };
PD_COVER_HD inline bool chunk_fast(const uint16_t *nar, NarState &st, int tile)
{
    if (!chunk_fast_entry(512u, st.base)) return false;
    uint32_t before = st.pb << 16, lens = 0u;
    int lane_last = st.base, incl = NONE;
    bool every = true;
    for (int l = 0; l < 64; ++l) {
        uint32_t x[4];
        for (int j = 0; j < 4; ++j) x[j] = (uint32_t)nar[8 * l + 2 * j] | ((uint32_t)nar[8 * l + 2 * j + 1] << 16);
        const NarLane s = nar_lane_summary(x, before);
        lane_last += s.T;
        every = every && chunk_fast_lane_ok(lane_last, incl, st.reach);
        const int m = lane_last - s.T + s.Mrel;
        incl = incl > m ? incl : m;
        lens += s.lens;
        before = x[3];
    }
    if (!chunk_fast_ok(every, incl, tile)) return false;
    st.reach = st.reach > incl ? st.reach : incl;
    st.base = lane_last; st.pb = before >> 16; st.sum += lens;
    return true;
}

// ---- the sweeps' software pipeline: three register buffers of N words in turn, no copies (the kernel's sweeps; tests/harness/sweep3_check.cpp on the CPU) ----
// PRECONDITION: nq >= 1 (both callers ask `if (nq)`; for nq = 0 nothing would be worked on, and the kernel's loads clamp a chunk's number to nq - 1).
// load(x, q) fills x with chunk q and also serves q >= nq (the kernel: all lanes to one place); work(x, q) is called for the chunks 0 .. min(nq - 1, the chunk
// behind which stop() first says true), in order, each with the buffer load(., q) filled; primed() runs behind the first two loads' issue.
// Two chunks stay in flight behind the one worked on: the wait in front of work(., q) must count the loads of chunks q + 1 and q + 2 and nothing else.
// The loop has ONE exit, at its bottom, and every load of a rotation is issued whatever the rotation meets.  A software-pipelined loop with an exit behind every
// chunk gets all its exits routed through the latch block by this compiler, and the pass that places the waits, which is not path-sensitive, then takes the state
// of "left behind the first chunk" (the load into C the newest one pending) for the back edge's: it drains EVERY load (vmcnt(0)) in front of the load at the
// loop's top, every third chunk (profiles/r20_sweep_inflight_isa.txt).  With one exit every wait counts what it should.
// The loop runs WHOLE rotations only (q + 3 <= nq), so it loads no chunk beyond nq + 1, and the last one or two chunks, by then in A and B, are worked on
// behind it without a load: a one-exit loop that runs to the last chunk issues up to two loads more behind it, and the wait that ends the sweep then pays
// a whole round trip per tile — measured slower than the loop with three exits (0.693 -> 0.705 ms a step; profiles/r20_sweep_inflight_ab.txt, section 2).  A stop() inside a rotation skips the
// rotation's remaining work, not its loads.
// The sweep ends with nothing in flight, so that the next sweep's waits count its own loads only.
PD_COVER_HD inline void sweep_drain()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0)
#endif
}
template <int N, class Load, class Work, class Stop, class Primed>
PD_COVER_HD inline __attribute__((always_inline)) void sweep3(const Load &load, const Work &work, const uint32_t nq, const Stop &stop, const Primed &primed)
{
    uint32_t A[N], B[N], C[N];
    uint32_t q = 0;
    bool go = true;
    load(A, 0u);
    load(B, 1u);
    primed();
    if (nq >= 3u) {
#pragma unroll 1
        for (;;) {
            load(C, q + 2u);
            work(A, q);
            go = !stop();
            load(A, q + 3u);
            if (go) { work(B, q + 1u); go = !stop(); }
            load(B, q + 4u);
            if (go) { work(C, q + 2u); go = !stop(); }
            q += 3u;
            if (!go || q + 3u > nq) break;
        }
    }
    if (go && q < nq) {
        work(A, q);
        if (q + 1u < nq && !stop()) work(B, q + 1u);
    }
    sweep_drain();
}

} // namespace pdcover
