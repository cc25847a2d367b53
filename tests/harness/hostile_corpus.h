// tests/harness/hostile_corpus.h — TEST INFRASTRUCTURE: families of CONSTRUCTED raw DEFLATE streams (deflate_builder.h) —
// well-formed streams built to expand as far as the format allows, to overflow a counter, a table or a scratch area, or to be
// wrong in exactly one field — and the judge that runs the product's decoders over them inside fenced memory:
//   pdw::inflate_block<HostWave>, pdw::inflate_member<HostWave> (pd_inflate_wave.h) and pdi::inflate_block with its fast
//   tables apart from ("LDS") and inside ("global") its table struct (pd_inflate_core.h), each against zlib's raw inflate
//   with the same out_len:
//     result 0           =>  zlib ends the stream with exactly out_len bytes, and the bytes are equal;
//     zlib does that     =>  result 0 (PD_W_HOST only from the wave decoder and only in a family tagged "may decline");
//     otherwise          =>  a negative code (or PD_W_HOST);
//   and never an access outside the buffers: the output (out_len bytes + 16 of slack that may be read, never written — what
//   pd_x_bgzf_inflate allocates), the input (in_len + the 8-byte BGZF trailer for the wave decoder, in_len for the other), the
//   token scratch (pdw::TOK_SCRATCH entries) and the table structs each lie in an arena between two inaccessible regions of
//   256 MiB, flush against the one behind them or the one in front of them (the two wave entry points take turns, so do the
//   two pdi modes, so every case meets both); the rest of each arena holds 0xEE and is checked after every run.  A stray access
//   at any distance a 32-bit offset of these decoders can reach stops the run in the SIGSEGV handler, which names the case.
// Case counts and seeds are fixed here.  The whole corpus built with -fsanitize=address,undefined -O1 took 89 s on one core of the development
// machine (69 of them the one member of 70 001 empty blocks); tests/test_inflate_hostile.py allows 900.
#ifndef HOSTILE_CORPUS_H_
#define HOSTILE_CORPUS_H_
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include <zlib.h>
#include <map>
#include <random>
#include <string>
#include <vector>
#include "deflate_builder.h"

namespace hostile {

enum { FAM_MAXEXP, FAM_WRAP, FAM_TOKENS, FAM_HEADER, FAM_BODY, FAM_TINY, FAM_SUBTABLE, FAM_MUTATE, N_FAM };
struct Family { const char *name; bool may_decline, body_level; uint32_t seed; int attempts; };
// may_decline: the wave decoder hands incomplete codes (other than the one-code distance set) and sub-table overflow to the host decoder
// (PD_W_HOST).  Only header-abuse holds a stream that zlib inflates and this decoder declines — exactly one, which the test asserts: the
// literal/length code of a single one-bit code (the end of the block).
// attempts: how many cases the generator draws from its seed (a draw above the 128 KiB input limit is dropped: maximal-expansion makes 99
// of 100); 0: a hand-made list.  The report prints the real counts.
static const Family FAMILIES[N_FAM] = {
    {"maximal-expansion", false, true, 101, 100},
    {"wrap-targets", false, true, 102, 72},
    {"token-scratch", false, true, 103, 28},
    {"header-abuse", true, false, 0, 0},
    {"body-abuse", false, true, 105, 0},             // (the seed: its garbage bytes)
    {"many-tiny-blocks", false, true, 106, 24},      // (+ 1 hand-made)
    {"long-codes", false, true, 107, 60},
    {"structured-mutation", false, true, 108, 300},
};

struct Case { std::string name; int family; std::vector<uint8_t> in; uint32_t out_len; bool wrong_crc; };

// ---- marks from inside the wave decoder (PW_MARK) ----------------------------------------------------------------------
struct Marks { uint64_t body, merges, merges_over_n, merges_over_m; uint32_t sub_ll, sub_d, sub_over; };
static Marks g_marks;
static inline void mark(uint32_t code, uint32_t val)
{
    if (code == 22) g_marks.body++;                                           // tables built, decode_body is next
    else if (code == 31) { g_marks.merges++; if (val > 0x1ffffu) g_marks.merges_over_n++; }   // a re-decode merged; val = the pass's bytes
    else if (code == 32) { if (val > 0x7fffu) g_marks.merges_over_m++; }                      // ... val = the pass's matches
    else if (code == 33) { if (val > g_marks.sub_ll) g_marks.sub_ll = val; if (val > (uint32_t)pdw::LL_SUBCAP) g_marks.sub_over++; }   // sub-table entries a literal/length code needs
    else if (code == 34) { if (val > g_marks.sub_d) g_marks.sub_d = val; if (val > (uint32_t)pdw::D_SUBCAP) g_marks.sub_over++; }      // ... a distance code
}

// ---- fenced arenas -------------------------------------------------------------------------------------------------------
static const size_t GUARD = 256u << 20;
struct Arena {
    const char *what; uint8_t *map, *body; size_t cap;                        // body[0, cap) is accessible, GUARD bytes on either side are not
    uint8_t *p; size_t n;                                                     // the buffer of the current run
    void init(const char *w, size_t bytes)
    {
        const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
        what = w; cap = (bytes + pg - 1) / pg * pg; if (!cap) cap = pg;
        map = (uint8_t *)mmap(nullptr, GUARD + cap + GUARD, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (map == MAP_FAILED || mprotect(map + GUARD, cap, PROT_READ | PROT_WRITE)) { perror("mmap"); exit(2); }
        body = map + GUARD; p = body; n = 0;
    }
    uint8_t *place(size_t bytes, bool at_end)                                // the buffer ends at the rear fence, or begins at the front one
    {
        const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
        const size_t used = (bytes + pg - 1) / pg * pg ? (bytes + pg - 1) / pg * pg : pg;      // (only the pages the buffer needs stay accessible)
        mprotect(body, cap, PROT_NONE); mprotect(at_end ? body + cap - used : body, used, PROT_READ | PROT_WRITE);
        uint8_t *lo = at_end ? body + cap - used : body;
        memset(lo, 0xEE, used);
        n = bytes; p = at_end ? body + cap - bytes : body;
        lim_lo = lo; lim_hi = lo + used;
        return p;
    }
    uint8_t *lim_lo, *lim_hi;
    bool untouched_outside(size_t keep_from = 0) const                       // nothing written around the buffer (or, keep_from < n: from that byte of it on)
    {
        for (const uint8_t *q = lim_lo; q < p; ++q) if (*q != 0xEE) return false;
        for (const uint8_t *q = p + keep_from; q < lim_hi; ++q) if (q >= p + n || keep_from < n) { if (*q != 0xEE) return false; }
        return true;
    }
};
static Arena a_out, a_in, a_tok, a_T, a_fast, a_slow;
static const char *volatile g_case = "(none)";
static const char *volatile g_decoder = "";
static char g_msg[512];
static void on_segv(int, siginfo_t *si, void *)
{
    const uint8_t *at = (const uint8_t *)si->si_addr;
    const char *where = "no arena";
    long off = 0;
    size_t len = 0;
    const Arena *all[] = {&a_out, &a_in, &a_tok, &a_T, &a_fast, &a_slow};
    for (const Arena *a : all) if (at >= a->map && at < a->map + GUARD + a->cap + GUARD) { where = a->what; off = (long)(at - a->p); len = a->n; }
    const int k = snprintf(g_msg, sizeof g_msg, "FENCE: case \"%s\", %s: access outside a buffer: %s, byte %ld of a buffer of %zu\n", g_case, g_decoder, where, off, len);
    if (k > 0) { ssize_t r = write(2, g_msg, (size_t)k); (void)r; }
    _exit(3);
}
static void init_fences()
{
    a_out.init("output", 65536 + 16); a_in.init("input", (1u << 17) + 4096 + 8); a_tok.init("token scratch", sizeof(pdw::Token) * pdw::TOK_SCRATCH);
    a_T.init("wave tables", sizeof(pdw::Tables)); a_fast.init("pdi fast tables", sizeof(pdi::Fast)); a_slow.init("pdi tables", sizeof(pdi::Tables));
    static uint8_t alt[1 << 16];
    stack_t ss; ss.ss_sp = alt; ss.ss_size = sizeof alt; ss.ss_flags = 0; sigaltstack(&ss, nullptr);
    struct sigaction sa; memset(&sa, 0, sizeof sa); sa.sa_sigaction = on_segv; sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
    sigaction(SIGSEGV, &sa, nullptr); sigaction(SIGBUS, &sa, nullptr);
}

// ---- the reference ------------------------------------------------------------------------------------------------------
static bool zlib_accepts(const std::vector<uint8_t> &in, uint32_t out_len, std::vector<uint8_t> &ref)
{
    ref.assign((size_t)out_len + 1, 0);
    z_stream zs; memset(&zs, 0, sizeof zs); inflateInit2(&zs, -15);
    zs.next_in = (Bytef *)in.data(); zs.avail_in = (uInt)in.size(); zs.next_out = ref.data(); zs.avail_out = out_len;
    const int zr = inflate(&zs, Z_FINISH);
    const bool ok = zr == Z_STREAM_END && zs.avail_out == 0;
    inflateEnd(&zs);
    return ok;
}

// ---- the families ---------------------------------------------------------------------------------------------------------
typedef std::mt19937 Rng;
static uint32_t pick(Rng &r, uint32_t n) { return n ? (uint32_t)(r() % n) : 0u; }

// a block in front, so that the block under test starts `o` bytes into the output and at a bit position the lanes do not guess
static uint32_t prefix(dfb::Stream &s, Rng &r, int kind, uint32_t want)
{
    std::vector<uint8_t> d(want);
    for (auto &x : d) x = (uint8_t)('A' + pick(r, 20));
    if (kind == 1) { s.stored(false, d.data(), d.size()); return want; }
    if (kind == 2) { s.begin_fixed(false); for (uint8_t x : d) s.lit(x); s.eob(); return want; }     // 3 + 8 want + 7 bits
    if (kind == 3) { s.begin_fixed(false); for (uint8_t x : d) s.lit(0x90 | (x & 15)); s.eob(); return want; }   // 9-bit literals: 3 + 9 want + 7 bits
    return 0;
}

static void gen_maxexp(std::vector<Case> &out)
{
    const Family &F = FAMILIES[FAM_MAXEXP];
    Rng r(F.seed);
    static const uint32_t NM[] = {0, 1, 2, 253, 254, 255, 300, 508, 509, 510, 1000, 5000, 20000, 21845, 21846, 60000, 120000, 250000, 500000};
    static const uint32_t PAD[] = {0, 0, 512, 515, 4099, 12345, 65536, 65510, 131072};        // member sizes: S = 64, odd widths, 8192, 16384
    for (int i = 0; i < F.attempts; ++i) {
        dfb::Dyn d; d.ll[285] = 1; d.ll['a'] = 2; d.ll[256] = 2; d.dist[0] = 1; d.finish();
        dfb::Stream s;
        const int pk = (int)pick(r, 4);
        const uint32_t pl = pk ? (i % 5 == 0 ? 32768u : i % 7 == 0 ? 60000u : pick(r, 9)) : 0u;
        uint32_t o = prefix(s, r, pk, pl);
        uint32_t n = NM[pick(r, sizeof NM / sizeof *NM)];
        uint32_t pad = PAD[pick(r, sizeof PAD / sizeof *PAD)];
        if (i % 3) { if (n > 21846) n = NM[pick(r, 14)]; if (pad > 65536) pad = 4099; }       // (the big ones are a third of the family: they take the time)
        s.begin_dynamic(true, d);
        s.lit('a');
        for (uint32_t k = 0; k < n; ++k) s.match(258, 1);
        s.eob();
        const uint64_t truth = (uint64_t)o + 1 + 258ull * n;
        uint32_t ol;
        switch (pick(r, 5)) {
        case 0: ol = (uint32_t)(truth <= 65536 ? truth : 65536); break;
        case 1: ol = (uint32_t)(truth <= 65536 ? truth - 1 : truth % 65536); break;
        case 2: ol = (uint32_t)(truth < 65536 ? truth + 1 : 65535); break;
        case 3: ol = 65536; break;
        default: ol = (uint32_t)((truth & 0x1ffff) <= 65536 ? (truth & 0x1ffff) : 1000); break;   // what a count kept in 17 bits would say
        }
        if (s.w.bytes.size() > (1u << 17)) continue;
        char nm[160]; snprintf(nm, sizeof nm, "maxexp #%d: prefix kind %d of %u bytes, %u matches of 258, true output %llu, out_len %u, member %zu bytes", i, pk, pl, n,
                               (unsigned long long)truth, ol, s.w.bytes.size() > pad ? s.w.bytes.size() : (size_t)pad);
        out.push_back(Case{nm, FAM_MAXEXP, s.take(pad), ol, false});
    }
}

// Lanes whose TRUE byte count is 2^17 + a little, in a stream whose passes from a wrong start fall back onto the true symbol
// boundaries (an odd-length code does that: 'b' has three bits, everything else one or two) and so merge at the first checkpoint;
// out_len = the sum of the lanes' counts modulo 2^17 — the total a decoder that keeps 17 bits per lane believes in.
static void gen_wrap(std::vector<Case> &out)
{
    const Family &F = FAMILIES[FAM_WRAP];
    Rng r(F.seed);
    static const uint32_t LEN[] = {16384, 16384, 20001, 32768, 65510, 131072};
    for (int i = 0; i < F.attempts; ++i) {
        const bool three = i % 6 == 5;                                         // 3-byte matches: as many MATCHES per lane as the bits allow (S / 2 <= 8192 < 2^15)
        dfb::Dyn d; d.ll[three ? 257 : 285] = 1; d.ll['a'] = 2; d.ll['b'] = 3; d.ll[256] = 3; d.dist[0] = 1; d.dist[1] = 1; d.finish();
        dfb::Stream s;
        const int pk = (int)pick(r, 3);
        const uint32_t o0 = prefix(s, r, pk, pk ? pick(r, 40) : 0);
        s.begin_dynamic(true, d);
        const uint32_t in_len = three ? 131072u : LEN[pick(r, 6)];
        const uint64_t base = s.bit_count(), in_bits = 8ull * in_len;
        uint64_t S = (in_bits - base + 63) / 64; if (S < 64) S = 64;
        const uint32_t n_big = 1 + pick(r, 3), first_big = 1 + pick(r, 3);
        std::vector<uint64_t> lane_n(64, 0);
        uint32_t lane = 0;
        auto at_lane = [&]() { while (lane < 63 && s.bit_count() >= base + (lane + 1) * S) ++lane; return lane; };
        auto lit = [&](int c) { lane_n[at_lane()] += 1; s.lit(c); };
        auto match = [&](uint32_t len) { lane_n[at_lane()] += len; s.match(len, 1); };
        lit('a'); lit('a');
        const uint32_t last = first_big + n_big - 1;
        for (uint32_t l = 0; l <= last; ++l) {
            const uint64_t end = base + (l + 1) * S;
            // the head of every subsequence: literals of two and three bits at random, a sixteenth of its width: passes that differ by a bit meet in here
            while (s.bit_count() < end - S + S / 16) lit(pick(r, 3) ? 'a' : 'b');
            if (l >= first_big) {
                const uint32_t m = three ? (uint32_t)(S / 2) : 508 + pick(r, 3) + (i % 4 == 0 ? pick(r, 600) : 0);
                for (uint32_t k = 0; k < m && s.bit_count() + 8 < end; ++k) match(three ? 3 : 258);
            }
            const uint32_t tail = l == last ? pick(r, 64) : 0xffffffffu;
            for (uint32_t k = 0; k < tail && s.bit_count() + 6 < end; ++k) lit(pick(r, 8) ? 'a' : 'b');
        }
        s.eob();
        uint64_t truth = o0, kept = o0;
        for (uint64_t n : lane_n) { truth += n; kept += n & 0x1ffff; }
        uint32_t ol = (uint32_t)(kept <= 65536 ? kept : kept & 0xffff);
        if (i % 9 == 8) ol = ol > 3 ? ol - 3 : 1;
        if (i % 9 == 7 && ol < 65000) ol += 100;
        if (s.w.bytes.size() > in_len) continue;
        char nm[200]; snprintf(nm, sizeof nm, "wrap #%d: member %u bytes (S = %llu), lanes %u..%u hold %s, true output %llu, sum of the lanes' counts mod 2^17 %llu, out_len %u",
                               i, in_len, (unsigned long long)S, first_big, last, three ? "S/2 matches of 3" : "2^17 + a few bytes", (unsigned long long)truth, (unsigned long long)kept, ol);
        out.push_back(Case{nm, FAM_WRAP, s.take(in_len), ol, false});
    }
}

static void gen_tokens(std::vector<Case> &out)
{
    const Family &F = FAMILIES[FAM_TOKENS];
    Rng r(F.seed);
    static const uint32_t NM[] = {1000, 21844, 21845, 21846, 21847, 21909, 21910, 30000, 40000, 100000, 400000};
    for (int i = 0; i < F.attempts; ++i) {
        dfb::Dyn d; d.ll[257] = 1; d.ll['t'] = 2; d.ll[256] = 2; d.dist[0] = 1; d.finish();
        dfb::Stream s;
        const int pk = (int)pick(r, 3);
        const uint32_t o = prefix(s, r, pk, pk ? pick(r, 7) : 0);
        const uint32_t n = NM[i % 11];
        s.begin_dynamic(true, d);
        s.lit('t');
        for (uint32_t k = 0; k < n; ++k) s.match(3, 1);
        s.eob();
        const uint64_t truth = (uint64_t)o + 1 + 3ull * n;
        const uint32_t ol = i % 3 == 0 || truth > 65536 ? (truth <= 65536 && i % 3 == 0 ? (uint32_t)truth : i % 2 ? 65536u : 3001u) : (uint32_t)truth - (i % 3 == 1 ? 0 : 1);
        char nm[160]; snprintf(nm, sizeof nm, "tokens #%d: %u matches of 3 after %u bytes, true output %llu, out_len %u", i, n, o, (unsigned long long)truth, ol);
        out.push_back(Case{nm, FAM_TOKENS, s.take(i % 4 == 3 ? 131072 : 0), ol, false});
    }
}

// a valid description: codes, body, output size
struct BodySym { int kind; uint32_t a, b; };                                 // 0 literal a; 1 match (length a, distance b); 2 end of block
struct Desc { dfb::Dyn d; std::vector<BodySym> body; uint32_t out_len; };
// code lengths of a COMPLETE prefix code with n leaves of at most max_len bits: leaves are split at random, deep ones first when `deep`
static std::vector<uint8_t> random_lengths(Rng &r, int n, int max_len, bool deep)
{
    std::vector<uint8_t> L = {1, 1};
    while ((int)L.size() < n) {
        size_t k = pick(r, (uint32_t)L.size());
        if (deep) { const size_t k2 = pick(r, (uint32_t)L.size()), k3 = pick(r, (uint32_t)L.size()); if (L[k2] > L[k] && L[k2] < max_len) k = k2; if (L[k3] > L[k] && L[k3] < max_len) k = k3; }
        if (L[k] >= max_len) { bool any = false; for (size_t j = 0; j < L.size(); ++j) if (L[j] < max_len) { k = j; any = true; break; } if (!any) break; }
        L[k]++; L.push_back(L[k]);
    }
    return L;
}
static Desc random_desc(Rng &r, int n_ll, int n_d, bool deep, uint32_t target)
{
    Desc D;
    std::vector<int> syms;                                                    // which symbols get codes: 256, some literals, some lengths
    syms.push_back(256);
    const int n_len = n_ll > 40 ? 6 + (int)pick(r, 23) : 2;
    std::vector<int> pool;
    for (int s = 257; s <= 285; ++s) pool.push_back(s);
    for (int k = 0; k < n_len && !pool.empty(); ++k) { const size_t j = pick(r, (uint32_t)pool.size()); syms.push_back(pool[j]); pool.erase(pool.begin() + j); }
    pool.clear();
    for (int s = 0; s < 256; ++s) pool.push_back(s);
    while ((int)syms.size() < n_ll && !pool.empty()) { const size_t j = pick(r, (uint32_t)pool.size()); syms.push_back(pool[j]); pool.erase(pool.begin() + j); }
    std::vector<uint8_t> L = random_lengths(r, (int)syms.size(), 15, deep);
    for (size_t k = 0; k < syms.size() && k < L.size(); ++k) D.d.ll[syms[pick(r, 2) ? k : syms.size() - 1 - k]] = 0;
    for (size_t k = 0; k < syms.size() && k < L.size(); ++k) D.d.ll[syms[k]] = L[k];
    std::vector<int> ds;
    pool.clear();
    for (int s = 0; s < 30; ++s) pool.push_back(s);
    for (int k = 0; k < n_d; ++k) { const size_t j = pick(r, (uint32_t)pool.size()); ds.push_back(pool[j]); pool.erase(pool.begin() + j); }
    if (n_d == 1) D.d.dist[ds[0]] = 1;
    else { std::vector<uint8_t> LD = random_lengths(r, n_d, 15, deep); for (int k = 0; k < n_d; ++k) D.d.dist[ds[k]] = LD[k]; }
    D.d.use_repeats = pick(r, 4) != 0;
    D.d.finish();
    std::vector<int> lits, lens;
    for (int s : syms) { if (s < 256) lits.push_back(s); else if (s > 256) lens.push_back(s); }
    uint32_t o = 0;
    while (o < target) {
        if (!lits.empty() && (o == 0 || lens.empty() || pick(r, 3) == 0)) { D.body.push_back({0, (uint32_t)lits[pick(r, (uint32_t)lits.size())], 0}); ++o; continue; }
        if (lens.empty() || o == 0) break;
        const int ls = lens[pick(r, (uint32_t)lens.size())] - 257, dsym = ds[pick(r, (uint32_t)ds.size())];
        const uint32_t len = dfb::LEN_BASE[ls] + pick(r, 1u << dfb::LEN_EXTRA[ls]);
        uint32_t dist = dfb::DIST_BASE[dsym] + pick(r, 1u << dfb::DIST_EXTRA[dsym]);
        if (dist > o) { if (dfb::DIST_BASE[dsym] > o) { if (lits.empty()) break; D.body.push_back({0, (uint32_t)lits[0], 0}); ++o; continue; } dist = dfb::DIST_BASE[dsym]; }
        if (o + len > 65536) break;
        D.body.push_back({1, len, dist}); o += len;
    }
    D.body.push_back({2, 0, 0});
    D.out_len = o;
    return D;
}
static void write_desc(dfb::Stream &s, const Desc &D, bool final)
{
    s.begin_dynamic(final, D.d);
    for (const BodySym &b : D.body) { if (b.kind == 0) s.lit((int)b.a); else if (b.kind == 1) s.match(b.a, b.b); else s.eob(); }
}

static void gen_long_codes(std::vector<Case> &out)
{
    const Family &F = FAMILIES[FAM_SUBTABLE];
    Rng r(F.seed);
    for (int i = 0; i < F.attempts; ++i) {
        // up to all 286 / 30 symbols, lengths up to 15 bits, many of the deepest: the sub-table areas fill to and past LL_SUBCAP / D_SUBCAP
        const Desc D = random_desc(r, i % 5 == 0 ? 286 : 150 + (int)pick(r, 137), i % 4 == 0 ? 30 : 2 + (int)pick(r, 29), i % 3 != 2, 200 + pick(r, i % 10 == 0 ? 60000 : 3000));
        dfb::Stream s;
        const int pk = (int)pick(r, 3);
        const uint32_t o = prefix(s, r, pk, pk ? pick(r, 5) : 0);
        write_desc(s, D, true);
        char nm[160]; snprintf(nm, sizeof nm, "long codes #%d: %d + %d symbols, %zu body symbols, out_len %u", i, D.d.hlit, D.d.hdist, D.body.size(), o + D.out_len);
        out.push_back(Case{nm, FAM_SUBTABLE, s.take(), o + D.out_len, false});
    }
}

static void gen_header(std::vector<Case> &out)
{
    auto add = [&](const char *nm, dfb::Stream &s, uint32_t ol) { out.push_back(Case{std::string("header: ") + nm, FAM_HEADER, s.take(), ol, false}); };
    auto simple = [&](const char *nm, dfb::Dyn d, uint32_t n_lit, int lit_sym, bool use_match = false) {
        dfb::Stream s; s.begin_dynamic(true, d);
        for (uint32_t k = 0; k < n_lit; ++k) s.lit(lit_sym);
        if (use_match) s.match(3, 1);
        s.eob();
        add(nm, s, n_lit + (use_match ? 3 : 0));
    };
    { dfb::Dyn d; d.ll['x'] = 1; d.ll['y'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.finish(); simple("over-subscribed literal/length code (three 1-bit codes)", d, 4, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 2; d.ll[256] = 2; d.dist[0] = 1; d.finish(); simple("incomplete literal/length code (two 2-bit codes)", d, 4, 'x'); }
    { dfb::Dyn d; d.ll[256] = 1; d.dist[0] = 1; d.finish(); simple("literal/length code of one 1-bit code: the end of the block (zlib accepts)", d, 0, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.finish(); simple("no distance codes at all, literals only (legal)", d, 9, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2; d.finish(); simple("no distance codes, and a match", d, 4, 'x', true); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2; d.dist[0] = 1; d.dist[1] = 1; d.dist[2] = 1; d.finish(); simple("over-subscribed distance code", d, 4, 'x', true); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2; d.dist[0] = 2; d.dist[1] = 2; d.finish(); simple("incomplete distance code of two 2-bit codes", d, 4, 'x', true); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2; d.dist[0] = 2; d.finish(); simple("one distance code of two bits", d, 4, 'x', true); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2; d.dist[5] = 1; d.finish(); simple("one distance code of one bit, symbol 5, unused", d, 4, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2; d.dist[0] = 1; d.finish();
      dfb::Stream s; s.begin_dynamic(true, d); s.lit('x'); s.ll_sym(257); s.raw(1, 1); s.eob(); add("the missing code of a one-code distance set is used", s, 4); }
    for (int hl : {286, 287, 288}) { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[hl - 1] = 2; d.dist[0] = 1; d.finish();
      char nm[64]; snprintf(nm, sizeof nm, "HLIT says %d symbols", hl); simple(nm, d, 5, 'x'); }
    for (int hd : {30, 31, 32}) { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2; d.dist[0] = 1; d.dist[hd - 1] = 1; d.finish();
      char nm[64]; snprintf(nm, sizeof nm, "HDIST says %d symbols", hd); simple(nm, d, 5, 'x', true); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.finish(); d.cl_syms.insert(d.cl_syms.begin(), {16, 0}); d.make_clc();
      simple("repeat code 16 is the first length", d, 3, 'x'); }
    { dfb::Dyn d; for (int s = 250; s <= 256; ++s) d.ll[s] = 3; d.ll[0] = 3; d.dist[0] = 3; d.dist[1] = 3; d.dist[2] = 3; d.dist[3] = 3; d.dist[4] = 2; d.dist[5] = 2; d.count_symbols();
      // lengths 250 .. 256 and distances 0 .. 3 are ONE run of 3s written as 3, 16(6), 16(4): the repeat runs across the boundary (legal)
      d.hlit = 257; d.encode_lengths(); d.make_clc(); simple("a repeat runs from the literal/length lengths into the distance lengths", d, 6, 250); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.finish(); d.cl_syms.push_back({18, 100}); d.make_clc(); simple("a zero run past HLIT + HDIST", d, 3, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.finish(); d.cl_syms.back() = {1, 0}; d.cl_syms.push_back({16, 3}); d.make_clc(); simple("a 16 repeat past HLIT + HDIST", d, 3, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll['y'] = 1; d.dist[0] = 1; d.finish(); simple("no end-of-block code", d, 5, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.finish(); for (int s = 0; s < 19; ++s) d.clc[s] = 0; d.clc[0] = d.clc[1] = 2; simple("incomplete code-length code", d, 3, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.finish(); for (int s = 0; s < 19; ++s) d.clc[s] = 1; simple("over-subscribed code-length code", d, 3, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.finish(); for (int s = 0; s < 19; ++s) d.clc[s] = 0; simple("code-length code without codes", d, 3, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.finish(); d.hclen = 4; simple("HCLEN 4 cuts the code-length code short", d, 3, 'x'); }
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 1; d.dist[0] = 1; d.use_repeats = false; d.finish(); simple("every length written literally", d, 7, 'x'); }
    for (int cut = 1; cut <= 12; ++cut) {                                     // the input ends inside the header
        dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2; d.dist[0] = 1; d.finish();
        dfb::Stream s; s.begin_dynamic(true, d); s.lit('x'); s.eob();
        std::vector<uint8_t> b = s.take(); if ((size_t)cut >= b.size()) break; b.resize(b.size() - (size_t)cut);
        char nm[64]; snprintf(nm, sizeof nm, "header: the input ends %d bytes early", cut); out.push_back(Case{nm, FAM_HEADER, b, 1, false});
    }
    // All 30 distance symbols with a deep tail: 1 .. 6 and 8 bits, then 9 .. 15 bits in three chains.  Codes are canonical, so the long ones sit side by
    // side behind the last root prefixes (sub-tables of 2, 4 and 128 entries here).  That order is also why the sub-table areas cannot overflow for a
    // COMPLETE code: lengths never decrease along the code space, so a prefix's longest code is no longer than the next prefix's shortest — only the
    // last prefix can hold a deep sub-tree unless a whole prefix is filled with codes of one length (2^b symbols for 2^b entries); with 30 symbols
    // behind an 8-bit root that stays far below D_SUBCAP = 256, and for 286 symbols behind a 9-bit root zlib's `enough` gives 852 - 512 = 340 =
    // LL_SUBCAP.  The report prints the largest areas the corpus needed and how often one was exceeded (only incomplete or over-subscribed
    // headers get that far, and those are refused before).
    { dfb::Dyn d; d.ll['x'] = 1; d.ll[256] = 2; d.ll[257] = 2;
      static const uint8_t DL[30] = {1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 15, 9, 10, 11, 12, 13, 14, 15, 15, 9, 10, 11, 12, 13, 14, 14};
      for (int k = 0; k < 30; ++k) d.dist[k] = DL[k];
      d.finish();
      dfb::Stream s; s.begin_dynamic(true, d); for (int k = 0; k < 40; ++k) s.lit('x'); s.match(3, 1); s.match(3, 2); s.match(3, 4); s.match(3, 40); s.eob();
      add("all 30 distance symbols, lengths 1 .. 15 with a deep tail", s, 52); }
    // 15-bit codes on a chain: lengths 1 .. 14 once and two of 15 in the literal/length code; all 30 distance symbols with the deepest shape
    { dfb::Dyn d; for (int l = 1; l <= 14; ++l) d.ll[l == 1 ? 256 : 40 + l] = (uint8_t)l; d.ll[100] = 15; d.ll[101] = 15; d.ll[257] = 0;
      for (int l = 1; l <= 14; ++l) d.dist[l - 1] = (uint8_t)l; d.dist[14] = 15; d.dist[15] = 15; d.finish();
      dfb::Stream s; s.begin_dynamic(true, d); for (int k = 0; k < 40; ++k) s.lit(k % 2 ? 100 : 101); s.lit(54); s.eob(); add("a chain of lengths 1 .. 15", s, 41); }
}

static void gen_body(std::vector<Case> &out)
{
    Rng r(FAMILIES[FAM_BODY].seed);
    auto add = [&](const std::string &nm, std::vector<uint8_t> b, uint32_t ol, bool bad_crc = false) { out.push_back(Case{"body: " + nm, FAM_BODY, b, ol, bad_crc}); };
    for (int sym : {286, 287}) { dfb::Stream s; s.begin_fixed(true); s.lit('q'); s.ll_sym(sym); s.d_sym(0); s.eob(); add("length symbol " + std::to_string(sym), s.take(), 4); }
    for (int sym : {30, 31}) { dfb::Stream s; s.begin_fixed(true); s.lit('q'); s.ll_sym(257); s.d_sym(sym); s.raw(0, 13); s.eob(); add("distance symbol " + std::to_string(sym), s.take(), 4); }
    for (uint32_t o : {0u, 1u, 2u, 32768u, 40000u}) for (int over : {0, 1}) {
        dfb::Stream s; std::vector<uint8_t> d(o, 'z');
        if (o > 2) s.stored(false, d.data(), o);
        s.begin_fixed(true);
        if (o <= 2) for (uint32_t k = 0; k < o; ++k) s.lit('z');
        const uint32_t dist = o + (uint32_t)over > 32768 ? 32768 : o + (uint32_t)over;
        if (dist) s.match(5, dist); else { s.ll_sym(259); s.d_sym(0); }
        s.eob();
        add("distance " + std::to_string(dist) + " with " + std::to_string(o) + " bytes written", s.take(), o + 5);
    }
    {   // the input ends: inside a symbol, inside extra bits, inside a stored block's LEN / NLEN and its bytes — every cut of a small stream
        dfb::Stream s; const uint8_t st[5] = {1, 2, 3, 4, 5};
        s.begin_fixed(false); for (int k = 0; k < 6; ++k) s.lit(0x90 + k); s.match(200, 3); s.match(67, 6); s.eob();
        s.stored(false, st, 5);
        s.begin_fixed(true); s.match(258, 270); s.lit('e'); s.eob();
        const std::vector<uint8_t> whole = s.take();
        const uint32_t ol = 6 + 200 + 67 + 5 + 258 + 1;
        for (size_t n = 0; n <= whole.size(); ++n) add("the input ends after " + std::to_string(n) + " of " + std::to_string(whole.size()) + " bytes", std::vector<uint8_t>(whole.begin(), whole.begin() + n), ol);
        add("the whole stream, wrong CRC-32 in the trailer", whole, ol, true);
        for (int k = 0; k < 6; ++k) { std::vector<uint8_t> g = whole; for (int j = 0; j < 1 + k * 40; ++j) g.push_back((uint8_t)r()); add("a final block followed by " + std::to_string(1 + k * 40) + " bytes of garbage", g, ol); }
        for (uint32_t o2 : {ol - 1, ol + 1, 0u, 65536u}) add("the stream of " + std::to_string(ol) + " bytes with out_len " + std::to_string(o2), whole, o2);
    }
    { const uint8_t st[4] = {9, 8, 7, 6}; dfb::Stream s; s.stored_raw(true, 4, 4, st, 4); add("NLEN is not the complement", s.take(), 4); }
    { const uint8_t st[4] = {9, 8, 7, 6}; dfb::Stream s; s.stored_raw(true, 4, 0xfffb ^ 1, st, 4); add("NLEN off by one bit", s.take(), 4); }
    for (uint32_t len : {5u, 300u, 65535u}) { std::vector<uint8_t> d(len, 'k'); dfb::Stream s; s.begin_fixed(false); s.lit('j'); s.eob(); s.stored(true, d.data(), len);
      add("a stored block of " + std::to_string(len) + " bytes, longer than the rest of the output", s.take(), len > 300 ? 65536 - 200 : len - 1); }
    { std::vector<uint8_t> d(65535, 'k'); dfb::Stream s; s.stored(false, d.data(), d.size()); s.stored(true, d.data(), 1); add("two stored blocks fill 65536 bytes", s.take(), 65536); }
    { std::vector<uint8_t> d(65535, 'k'); dfb::Stream s; s.stored(false, d.data(), d.size()); s.stored(true, d.data(), 1); add("two stored blocks fill 65536 bytes, wrong CRC-32", s.take(), 65536, true); }
    { dfb::Stream s; s.begin_fixed(true); s.lit('p'); for (int k = 0; k < 254; ++k) s.match(258, 1); s.match(3, 1); s.eob(); add("fixed block: exactly 65536 bytes, wrong CRC-32", s.take(), 65536, true); }
    { dfb::Stream s; s.begin_fixed(true); s.lit('c'); s.eob(); add("one literal, wrong CRC-32", s.take(), 1, true); }
    { dfb::Stream s; s.begin_fixed(true); s.eob(); add("an empty member, wrong CRC-32", s.take(), 0, true); }
    { std::vector<uint8_t> d(300, 'k'); dfb::Stream s; s.stored_raw(true, 300, 300 ^ 0xffff, d.data(), 100); add("a stored block announces more bytes than the input holds", s.take(), 300); }
    { dfb::Stream s; s.begin_fixed(false); s.lit('n'); s.eob(); s.begin_fixed(false); s.lit('o'); s.eob(); add("BFINAL never set", s.take(), 2); }
    { dfb::Stream s; s.begin_fixed(false); s.lit('n'); s.eob(); add("BFINAL never set, zero bytes follow", s.take(600), 1); }
    { dfb::Stream s; s.header(true, 3); s.raw(0x5a5a, 16); add("BTYPE 3", s.take(), 0); }
    { dfb::Stream s; s.begin_fixed(false); s.lit('n'); s.eob(); s.header(true, 3); s.raw(0x5a5a, 16); add("BTYPE 3 after a good block", s.take(), 1); }
    { dfb::Stream s; s.begin_fixed(true); for (int k = 0; k < 300; ++k) s.lit('p'); add("a fixed block without its end", s.take(), 300); }
    { dfb::Stream s; s.begin_fixed(true); s.lit('p'); for (int k = 0; k < 300; ++k) s.match(258, 1); s.eob(); add("fixed block: 300 matches of 258, out_len 65536", s.take(), 65536); }
    { dfb::Stream s; s.begin_fixed(true); s.lit('p'); for (int k = 0; k < 254; ++k) s.match(258, 1); s.match(3, 1); s.eob(); add("fixed block: exactly 65536 bytes", s.take(), 65536); }
    { std::vector<uint8_t> none; add("no input at all", none, 0); add("no input at all, out_len 10", none, 10); }
}

static void gen_tiny(std::vector<Case> &out)
{
    const Family &F = FAMILIES[FAM_TINY];
    Rng r(F.seed);
    static const uint32_t NB[] = {1, 100, 300, 1000, 3000, 10000};
    for (int i = 0; i < F.attempts; ++i) {
        dfb::Stream s;
        const uint32_t nb = NB[i % 6];
        const int mode = i % 3;                                               // empty fixed blocks, empty stored blocks, both at random
        uint32_t o = 0;
        if (i % 2) { s.begin_fixed(false); s.lit('u'); s.eob(); ++o; }
        for (uint32_t k = 0; k < nb && s.w.bytes.size() < (1u << 17) - 64; ++k) {
            if (mode == 0 || (mode == 2 && pick(r, 2))) { s.begin_fixed(false); s.eob(); } else s.stored(false, nullptr, 0);
        }
        const bool more = i % 4 < 2;
        s.begin_fixed(true); if (more) { s.lit('v'); ++o; } s.eob();
        const uint32_t ol = i % 5 == 4 ? o - (more ? 1 : 0) : o;               // (out_len without the last literal: a decoder that stops counting blocks would accept)
        char nm[160]; snprintf(nm, sizeof nm, "tiny #%d: %u empty %s blocks, %zu bytes, out_len %u (true %u)", i, nb, mode == 0 ? "fixed" : mode == 1 ? "stored" : "fixed and stored", s.w.bytes.size(), ol, o);
        out.push_back(Case{nm, FAM_TINY, s.take(), ol, false});
    }
    // more blocks than a decoder's block counter may allow (ten bits each: only a member above 64 KiB holds them), a literal behind them; a decoder that
    // stops counting there and reports what it has would accept the stream with out_len 1
    // (ONE such case: the wave decoder spreads what is left of the member over its lanes for every block, so its cost is blocks x member bits —
    // bounded, but this case alone is most of the corpus's time)
    {
        dfb::Stream s; s.begin_fixed(false); s.lit('u'); s.eob();
        for (uint32_t k = 0; k < 70001; ++k) { s.begin_fixed(false); s.eob(); }
        s.begin_fixed(true); s.lit('v'); s.eob();
        out.push_back(Case{"tiny: 70001 empty fixed blocks between two literals, out_len 1", FAM_TINY, s.take(), 1, false});
    }
}

static void gen_mutate(std::vector<Case> &out)
{
    const Family &F = FAMILIES[FAM_MUTATE];
    Rng r(F.seed);
    for (int i = 0; i < F.attempts; ++i) {
        Desc D = random_desc(r, i % 7 == 0 ? 4 + (int)pick(r, 6) : 20 + (int)pick(r, 260), 1 + (int)pick(r, 30), pick(r, 2) != 0, 50 + pick(r, i % 25 == 0 ? 40000 : 1500));
        const int what = i % 8;
        bool recount = true, relen = true;
        std::string did;
        auto used_ll = [&]() { std::vector<int> u; for (int s = 0; s < 288; ++s) if (D.d.ll[s]) u.push_back(s); return u; };
        auto used_d = [&]() { std::vector<int> u; for (int s = 0; s < 32; ++s) if (D.d.dist[s]) u.push_back(s); return u; };
        if (what == 0) { const auto u = used_ll(); const int s = u[pick(r, (uint32_t)u.size())]; const int dl = pick(r, 2) ? 1 : -1; D.d.ll[s] = (uint8_t)(D.d.ll[s] + dl > 15 ? 15 : D.d.ll[s] + dl); did = "literal/length symbol " + std::to_string(s) + (dl > 0 ? " one bit longer" : " one bit shorter"); }
        else if (what == 1) { const auto u = used_d(); const int s = u[pick(r, (uint32_t)u.size())]; const int dl = pick(r, 2) ? 1 : -1; D.d.dist[s] = (uint8_t)(D.d.dist[s] + dl > 15 ? 15 : D.d.dist[s] + dl); did = "distance symbol " + std::to_string(s) + (dl > 0 ? " one bit longer" : " one bit shorter"); }
        else if (what == 2) { const auto u = used_ll(); const int s = u[pick(r, (uint32_t)u.size())], t = u[pick(r, (uint32_t)u.size())]; std::swap(D.d.ll[s], D.d.ll[t]); did = "lengths of symbols " + std::to_string(s) + " and " + std::to_string(t) + " swapped"; }
        else if (what == 3) { D.d.count_symbols(); const int dl = (int)pick(r, 7) - 3; D.d.hlit += dl; if (D.d.hlit < 257) D.d.hlit = 257; if (D.d.hlit > 288) D.d.hlit = 288; recount = false; did = "HLIT changed by " + std::to_string(dl); }
        else if (what == 4) { D.body.pop_back(); did = "end of block dropped"; }
        else if (what == 5) { if (D.body.size() > 3) { const size_t a = pick(r, (uint32_t)D.body.size() - 1), b = pick(r, (uint32_t)D.body.size() - 1); std::swap(D.body[a], D.body[b]); } did = "two body symbols swapped"; }
        else if (what == 6) { for (auto &b : D.body) if (b.kind == 1 && pick(r, 4) == 0) { const int ds = dfb::distance_symbol(b.b); b.b = dfb::DIST_BASE[ds] + (1u << dfb::DIST_EXTRA[ds]) - 1; break; } did = "a distance raised to the top of its symbol"; }
        else { did = "nothing (the valid stream)"; }
        if (recount) D.d.count_symbols();
        if (relen) { D.d.encode_lengths(); D.d.make_clc(); }
        dfb::Stream s;
        const int pk = (int)pick(r, 3);
        const uint32_t o = prefix(s, r, pk, pk ? pick(r, 6) : 0);
        write_desc(s, D, true);
        if (s.w.bytes.size() > (1u << 17)) continue;
        out.push_back(Case{"mutation #" + std::to_string(i) + ": " + did + " (" + std::to_string(D.d.hlit) + " + " + std::to_string(D.d.hdist) + " symbols, out_len " + std::to_string(o + D.out_len) + ")",
                           FAM_MUTATE, s.take(), o + D.out_len, false});
    }
}

static std::vector<Case> family_cases(int fam)
{
    std::vector<Case> c;
    switch (fam) {
    case FAM_MAXEXP: gen_maxexp(c); break;
    case FAM_WRAP: gen_wrap(c); break;
    case FAM_TOKENS: gen_tokens(c); break;
    case FAM_HEADER: gen_header(c); break;
    case FAM_BODY: gen_body(c); break;
    case FAM_TINY: gen_tiny(c); break;
    case FAM_SUBTABLE: gen_long_codes(c); break;
    case FAM_MUTATE: gen_mutate(c); break;
    }
    return c;
}

// ---- the judge --------------------------------------------------------------------------------------------------------------
struct Tally { uint32_t sub_ll = 0, sub_d = 0; long sub_over = 0; long cases = 0, reached_body = 0, zlib_ok = 0, declined = 0, violations = 0, merges = 0, merges_over_n = 0, merges_over_m = 0; std::map<int, long> rc_wave, rc_member, rc_pdi; };

static int violation(const Case &c, const char *dec, const char *what, int rc)
{
    fprintf(stderr, "VIOLATION: case \"%s\", %s: %s (result %d)\n", c.name.c_str(), dec, what, rc);
    return 1;
}
// the verdict of one run against zlib's: 0 or the number of rules broken
static int verdict(const Case &c, const char *dec, int rc, bool zok, bool may_decline, const uint8_t *mine, const std::vector<uint8_t> &ref, bool crc_wrong)
{
    int bad = 0;
    if (rc == 0) {
        if (!zok) bad += violation(c, dec, "accepted a stream that zlib does not end with exactly out_len bytes", rc);
        else if (crc_wrong) bad += violation(c, dec, "a wrong CRC-32 went unnoticed", rc);
        else if (c.out_len && memcmp(mine, ref.data(), c.out_len) != 0) bad += violation(c, dec, "output differs from zlib's", rc);
    } else if (rc == pdw::PD_W_HOST) {
        if (zok && !may_decline) bad += violation(c, dec, "declined a stream zlib inflates, in a family that may not", rc);
    } else if (rc > 0) bad += violation(c, dec, "a result that is no code", rc);
    else if (zok && !(crc_wrong && rc == -20)) bad += violation(c, dec, "rejected a stream zlib inflates", rc);
    return bad;
}

static uint32_t g_crc, g_isize;
static int run_case(const Case &c, size_t index, Tally &t)
{
    const Family &F = FAMILIES[c.family];
    std::vector<uint8_t> ref;
    const bool zok = zlib_accepts(c.in, c.out_len, ref);
    const uint32_t in_len = (uint32_t)c.in.size();
    uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), ref.data(), c.out_len);   // (of whatever zlib wrote where it does not accept: nothing is compared with it then)
    if (c.wrong_crc) crc ^= 0x00100000u;
    g_crc = crc; g_isize = c.out_len;
    int bad = 0;
    g_case = c.name.c_str();
    t.cases++; t.zlib_ok += zok;
    for (int d = 0; d < 4; ++d) {
        // wave block / wave member / pdi "LDS" / pdi "global"; the placement alternates so that every case meets both fences in both decoders
        const bool at_end = ((index + (size_t)d) & 1) == 0;
        const bool wave = d < 2;
        static const char *const names[4] = {"pdw::inflate_block<HostWave>", "pdw::inflate_member<HostWave>", "pdi::inflate_block (fast tables apart)", "pdi::inflate_block (one table struct)"};
        g_decoder = names[d];
        const size_t in_n = (size_t)in_len + (wave ? 8 : 0), out_n = (size_t)c.out_len + (wave ? 16 : 0);
        uint8_t *in = a_in.place(in_n, at_end), *o = a_out.place(out_n, at_end);
        if (in_len) memcpy(in, c.in.data(), in_len);
        if (wave) { memcpy(in + in_len, &crc, 4); memcpy(in + in_len + 4, &c.out_len, 4); }
        int rc;
        bool tables_ok = true;
        if (wave) {
            pdw::Token *tok = (pdw::Token *)a_tok.place(sizeof(pdw::Token) * pdw::TOK_SCRATCH, at_end);
            pdw::Tables *T = (pdw::Tables *)a_T.place(sizeof(pdw::Tables), at_end);
            Marks before = g_marks;
            if (d == 0) { g_marks.sub_ll = g_marks.sub_d = 0; before = g_marks; }
            rc = d == 0 ? pdw::inflate_block<pdw::HostWave>(in, in_len, o, c.out_len, *T, tok, nullptr) : pdw::inflate_member<pdw::HostWave>(in, in_len, o, c.out_len, *T, tok, nullptr);
            if (d == 0) {
                t.reached_body += g_marks.body > before.body; t.rc_wave[rc]++; t.declined += zok && rc == pdw::PD_W_HOST;
                if (g_marks.sub_ll > t.sub_ll) t.sub_ll = g_marks.sub_ll;
                if (g_marks.sub_d > t.sub_d) t.sub_d = g_marks.sub_d;
                t.sub_over += (long)(g_marks.sub_over - before.sub_over);
                t.merges += (long)(g_marks.merges - before.merges); t.merges_over_n += (long)(g_marks.merges_over_n - before.merges_over_n); t.merges_over_m += (long)(g_marks.merges_over_m - before.merges_over_m);
            } else t.rc_member[rc]++;
            tables_ok = a_tok.untouched_outside(a_tok.n) && a_T.untouched_outside(a_T.n);
        } else {
            pdi::Tables *T = (pdi::Tables *)a_slow.place(sizeof(pdi::Tables), at_end);
            pdi::Fast *fast = (pdi::Fast *)a_fast.place(sizeof(pdi::Fast), at_end);
            rc = pdi::inflate_block(in, in_len, o, c.out_len, d == 2 ? *fast : T->fast, T->slow);
            if (d == 2) t.rc_pdi[rc]++;
            tables_ok = a_slow.untouched_outside(a_slow.n) && a_fast.untouched_outside(d == 2 ? a_fast.n : 0);
        }
        bad += verdict(c, names[d], rc, zok, wave && F.may_decline, o, ref, d == 1 && c.wrong_crc);
        // the 0xEE bytes: the 16 bytes of slack behind the wave decoders' output and everything else around the buffers
        if (!a_out.untouched_outside(c.out_len)) bad += violation(c, names[d], "wrote outside out[0, out_len)", rc);
        if ((in_len && memcmp(in, c.in.data(), in_len) != 0) || !a_in.untouched_outside(a_in.n)) bad += violation(c, names[d], "wrote to its input", rc);
        if (!tables_ok) bad += violation(c, names[d], "wrote outside its tables or its token scratch", rc);
    }
    g_case = "(none)";
    t.violations += bad;
    return bad;
}

} // namespace hostile
#endif
