// tests/harness/deflate_builder.h — TEST INFRASTRUCTURE: assembles raw DEFLATE streams (RFC 1951) bit by bit from a
// description, so that a test can hand a decoder WELL-FORMED streams built to be expensive, to overflow something, or to be
// wrong in exactly one chosen field.  Written from the RFC; it shares no code with the decoders under test
// (pd_inflate_wave.h, pd_inflate_core.h) and does not go through zlib's deflate.
//   Stream s;
//   s.stored(false, bytes, n);                       // a stored block (s.stored_raw: LEN / NLEN chosen freely)
//   s.begin_fixed(false); s.lit('a'); s.match(258, 1); s.eob();
//   Dyn d; d.ll[285] = 1; d.ll['a'] = 2; d.ll[256] = 2; d.dist[0] = 1; d.finish();
//   s.begin_dynamic(true, d); s.lit('a'); s.match(258, 1); s.eob();
//   s.raw(v, n) writes n plain bits; s.ll_sym / s.d_sym write a symbol of the block's codes with no questions asked.
#ifndef DEFLATE_BUILDER_H_
#define DEFLATE_BUILDER_H_
#include <stdint.h>
#include <utility>
#include <vector>

namespace dfb {

struct BitWriter {                            // RFC 1951 §3.1.1: bits are packed from the least significant bit of each byte
    std::vector<uint8_t> bytes;
    uint64_t nbits = 0;
    void bit(uint32_t b) { if ((nbits & 7) == 0) bytes.push_back(0); bytes.back() |= (uint8_t)((b & 1u) << (nbits & 7)); ++nbits; }
    void bits(uint32_t v, int n) { for (int i = 0; i < n; ++i) bit(v >> i); }                 // a value: least significant bit first
    void huff(uint32_t code, int len) { for (int i = len - 1; i >= 0; --i) bit(code >> i); }  // a Huffman code: most significant bit first
    void align() { while (nbits & 7) bit(0); }
};

// Canonical code values from code lengths (§3.2.2).  Over-subscribed sets get codes too (truncated to their length): such a
// header is written to be rejected, its body only has to be some bits.
inline std::vector<uint32_t> canonical(const std::vector<uint8_t> &len)
{
    uint32_t count[16] = {0}, next[16] = {0};
    for (uint8_t l : len) count[l]++;
    count[0] = 0;
    uint32_t code = 0;
    for (int b = 1; b <= 15; ++b) { code = (code + count[b - 1]) << 1; next[b] = code; }
    std::vector<uint32_t> out(len.size(), 0);
    for (size_t s = 0; s < len.size(); ++s) if (len[s]) out[s] = next[len[s]]++ & ((1u << len[s]) - 1u);
    return out;
}

static const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

inline int length_symbol(uint32_t len) { int s = 28; while (s > 0 && LEN_BASE[s] > len) --s; if (len == 258) s = 28; else if (s == 28) s = 27; return s; }   // 0 .. 28 (+ 257)
inline int distance_symbol(uint32_t dist) { int s = 29; while (s > 0 && DIST_BASE[s] > dist) --s; return s; }

// The header of a dynamic block.  Fill ll[] / dist[] (code lengths per symbol, 0 = unused) and call finish(); every field
// finish() derives can be overwritten afterwards (that is what the header-abuse and mutation cases do).
struct Dyn {
    std::vector<uint8_t> ll = std::vector<uint8_t>(288, 0), dist = std::vector<uint8_t>(32, 0);
    int hlit = 0, hdist = 0, hclen = 0;                       // numbers of symbols (257 .. 288, 1 .. 32) and of code-length-code lengths (4 .. 19)
    bool use_repeats = true;                                  // code lengths through 16 / 17 / 18 where they apply, or every one literally
    uint8_t clc[19] = {0};                                    // the code-length code's own lengths, by symbol
    std::vector<std::pair<uint8_t, uint8_t>> cl_syms;         // the code lengths as written: (symbol 0 .. 18, value of its extra bits)

    void count_symbols() { hlit = 257; for (int s = 257; s < 288; ++s) if (ll[s]) hlit = s + 1; hdist = 1; for (int s = 1; s < 32; ++s) if (dist[s]) hdist = s + 1; }
    // the hlit + hdist lengths as ONE sequence (§3.2.7: repeats may run from the literal/length lengths into the distance lengths)
    void encode_lengths()
    {
        std::vector<uint8_t> all(ll.begin(), ll.begin() + hlit);
        all.insert(all.end(), dist.begin(), dist.begin() + hdist);
        cl_syms.clear();
        for (size_t i = 0; i < all.size();) {
            size_t run = 1;
            while (i + run < all.size() && all[i + run] == all[i]) ++run;
            if (use_repeats && all[i] == 0 && run >= 3) { const size_t r = run > 138 ? 138 : run; if (r >= 11) cl_syms.push_back({18, (uint8_t)(r - 11)}); else cl_syms.push_back({17, (uint8_t)(r - 3)}); i += r; }
            else if (use_repeats && run >= 4) { cl_syms.push_back({all[i], 0}); size_t left = run - 1; i += 1; while (left >= 3) { const size_t r = left > 6 ? 6 : left; cl_syms.push_back({16, (uint8_t)(r - 3)}); left -= r; i += r; } }
            else { cl_syms.push_back({all[i], 0}); ++i; }
        }
    }
    // a complete code-length code over the symbols cl_syms uses (zlib takes no incomplete one), all 19 lengths written
    void make_clc()
    {
        bool used[19] = {false};
        for (auto &p : cl_syms) used[p.first] = true;
        int k = 0;
        for (int s = 0; s < 19; ++s) k += used[s];
        for (int s = 0; k < 2 && s < 19; ++s) if (!used[s]) { used[s] = true; ++k; }
        int L = 1;
        while ((1 << L) < k) ++L;
        int n_short = (1 << L) - k;                           // that many symbols get L - 1 bits, the others L
        for (int s = 0; s < 19; ++s) { clc[s] = 0; if (used[s]) { clc[s] = (uint8_t)(n_short > 0 ? L - 1 : L); --n_short; } }
        hclen = 19;
    }
    void finish() { count_symbols(); encode_lengths(); make_clc(); }
};

struct Stream {
    BitWriter w;
    std::vector<uint8_t> ll_len, d_len;                       // the codes of the block being written
    std::vector<uint32_t> ll_code, d_code;

    void header(bool final, int type) { w.bits(final ? 1 : 0, 1); w.bits((uint32_t)type, 2); }
    void stored_raw(bool final, uint32_t len, uint32_t nlen, const uint8_t *data, size_t n_data)
    {
        header(final, 0); w.align(); w.bits(len, 16); w.bits(nlen, 16);
        for (size_t i = 0; i < n_data; ++i) w.bits(data[i], 8);
    }
    void stored(bool final, const uint8_t *data, size_t n) { stored_raw(final, (uint32_t)n, (uint32_t)n ^ 0xffffu, data, n); }
    void begin_fixed(bool final)
    {
        header(final, 1);
        ll_len.assign(288, 8);
        for (int s = 144; s < 256; ++s) ll_len[s] = 9;
        for (int s = 256; s < 280; ++s) ll_len[s] = 7;
        d_len.assign(32, 5);
        ll_code = canonical(ll_len); d_code = canonical(d_len);
    }
    void begin_dynamic(bool final, const Dyn &d)
    {
        header(final, 2);
        w.bits((uint32_t)(d.hlit - 257), 5); w.bits((uint32_t)(d.hdist - 1), 5); w.bits((uint32_t)(d.hclen - 4), 4);
        for (int i = 0; i < d.hclen; ++i) w.bits(d.clc[CL_ORDER[i]], 3);
        const std::vector<uint8_t> cl(d.clc, d.clc + 19);
        const std::vector<uint32_t> cc = canonical(cl);
        for (auto &p : d.cl_syms) {
            w.huff(cc[p.first], cl[p.first]);
            if (p.first == 16) w.bits(p.second, 2); else if (p.first == 17) w.bits(p.second, 3); else if (p.first == 18) w.bits(p.second, 7);
        }
        ll_len = d.ll; d_len = d.dist;
        ll_code = canonical(ll_len); d_code = canonical(d_len);
    }
    void raw(uint32_t v, int n) { w.bits(v, n); }
    void ll_sym(int s) { w.huff(ll_code[s], ll_len[s]); }
    void d_sym(int s) { w.huff(d_code[s], d_len[s]); }
    void lit(int b) { ll_sym(b); }
    void eob() { ll_sym(256); }
    void match(uint32_t len, uint32_t dist)
    {
        const int ls = length_symbol(len), ds = distance_symbol(dist);
        ll_sym(257 + ls); w.bits(len - LEN_BASE[ls], LEN_EXTRA[ls]);
        d_sym(ds); w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds]);
    }
    uint64_t bit_count() const { return w.nbits; }
    std::vector<uint8_t> take(size_t pad_to = 0, uint8_t fill = 0) { std::vector<uint8_t> b = w.bytes; if (b.size() < pad_to) b.resize(pad_to, fill); return b; }
};

} // namespace dfb
#endif
