// tests/harness/wave_ops_gpu_check.hip — TEST INFRASTRUCTURE: every wave primitive of pdw::DevWave (pd_inflate_wave.h: DPP row shifts
// and broadcasts, readlane, mbcnt, Hillis-Steele scans) and of pdz::DevWaveZ (pd_lz77_devwave.h) on the GPU against the host forms the
// CPU tests run the same algorithms with (pdw::HostWave, pdz::HostWave: 64 lanes in a loop), lane by lane and bit for bit.
// One kernel, one wave, launched once per case; every lane stores what it holds after every primitive, so a value that should be
// the same in all lanes is compared in all of them.  Not compared: each / sync / fence / opaque / uniform_u8 / loads_landed (no value
// of their own) and DevWaveZ::lead (the host form has one thread and answers true).
//   wave_ops_gpu_check   -> "N cases, 0 differ", or the first primitive, case and lane that differ (exit 1)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../pandepth_amd/csrc/pd_inflate_wave.h"
#include "../../pandepth_amd/csrc/pd_lz77.h"
#include "../../pandepth_amd/csrc/pd_lz77_devwave.h"

struct Case {
    uint32_t a[64];        // the 32-bit vector
    uint32_t b[64];        // shfl: where every lane reads from; min_where: the lanes to skip (non-zero)
    uint64_t q[64];        // the 64-bit vector
    uint32_t h[64];        // seg_excl_scan_max64: 1 + the lane where the lane's segment begins (0: before lane 0)
    uint64_t mask;         // prefix_count
    uint32_t v, fill;      // ballot_eq / ballot_ne / uni; shift_up1
};

enum {
    S_BALLOT_EQ, S_BALLOT_NE, S_PREFIX_COUNT, S_EXCL_SCAN, S_EXCL_SCAN_TOTAL, S_SHIFT_UP1, S_INCL_SCAN_MAX, S_SHFL, S_MIN_WHERE, S_UNI,
    S_EXCL_SCAN_MAX64, S_SEG_EXCL_SCAN_MAX64, S_REDUCE_OR, S_REDUCE_XOR, S_REDUCE_MAX, S_REDUCE_MAX64, S_REDUCE_MIN64,
    S_Z_BALLOT_EQ, S_Z_BALLOT_NE, S_Z_REDUCE_MAX, S_Z_UNI,
    S_BCAST,                         // 64 slots each from here on: one per source lane
    S_BCAST_U = S_BCAST + 64, S_BCAST64 = S_BCAST_U + 64, S_Z_BCAST = S_BCAST64 + 64, N_SLOT = S_Z_BCAST + 64
};
static const char *const SLOT_NAME[] = {
    "DevWave::ballot_eq", "DevWave::ballot_ne", "DevWave::prefix_count", "DevWave::excl_scan", "DevWave::excl_scan (total)", "DevWave::shift_up1",
    "DevWave::incl_scan_max", "DevWave::shfl", "DevWave::min_where", "DevWave::uni", "DevWave::excl_scan_max64", "DevWave::seg_excl_scan_max64",
    "DevWave::reduce_or", "DevWave::reduce_xor", "DevWave::reduce_max", "DevWave::reduce_max64", "DevWave::reduce_min64",
    "DevWaveZ::ballot_eq", "DevWaveZ::ballot_ne", "DevWaveZ::reduce_max", "DevWaveZ::uni"};
static std::string slot_name(int s)
{
    if (s < S_BCAST) return SLOT_NAME[s];
    const char *n = s < S_BCAST_U ? "DevWave::bcast" : s < S_BCAST64 ? "DevWave::bcast_u" : s < S_Z_BCAST ? "DevWave::bcast64" : "DevWaveZ::bcast";
    return std::string(n) + " from lane " + std::to_string((s - S_BCAST) & 63);
}

__global__ __launch_bounds__(64) void k_wave_ops(const Case *in, uint64_t *out /* [N_SLOT][64] */)
{
    typedef pdw::DevWave W;
    typedef pdz::DevWaveZ Z;
    const int l = (int)(threadIdx.x & 63);
    W::Var<uint32_t> a, b, h; W::Var<uint64_t> q;
    a.v = in->a[l]; b.v = in->b[l]; h.v = in->h[l]; q.v = in->q[l];
    Z::Var<uint32_t> za; za.v = in->a[l];
    const uint64_t mask = in->mask; const uint32_t v = in->v, fill = in->fill;
    auto put = [&](int slot, uint64_t x) { out[slot * 64 + l] = x; };
    put(S_BALLOT_EQ, W::ballot_eq(a, v));
    put(S_BALLOT_NE, W::ballot_ne(a, v));
    put(S_PREFIX_COUNT, W::prefix_count(mask, l));
    uint32_t total = 0;
    put(S_EXCL_SCAN, W::excl_scan(a, &total).v);
    put(S_EXCL_SCAN_TOTAL, total);
    put(S_SHIFT_UP1, W::shift_up1(a, fill).v);
    put(S_INCL_SCAN_MAX, W::incl_scan_max(a).v);
    put(S_SHFL, W::shfl(a, b).v);
    put(S_MIN_WHERE, W::min_where(a, b));
    put(S_UNI, W::uni(v));
    put(S_EXCL_SCAN_MAX64, W::excl_scan_max64(q).v);
    put(S_SEG_EXCL_SCAN_MAX64, W::seg_excl_scan_max64(q, h).v);
    put(S_REDUCE_OR, W::reduce_or(a));
    put(S_REDUCE_XOR, W::reduce_xor(a));
    put(S_REDUCE_MAX, W::reduce_max(a));
    put(S_REDUCE_MAX64, W::reduce_max64(q));
    put(S_REDUCE_MIN64, W::reduce_min64(q));
    put(S_Z_BALLOT_EQ, Z::ballot_eq(za, v));
    put(S_Z_BALLOT_NE, Z::ballot_ne(za, v));
    put(S_Z_REDUCE_MAX, Z::reduce_max(za));
    put(S_Z_UNI, Z::uni(v));
    for (int s = 0; s < 64; ++s) {                  // (s is the same in every lane, as the primitives require)
        put(S_BCAST + s, W::bcast(a, s));
        put(S_BCAST_U + s, W::bcast_u(a, (uint32_t)s));
        put(S_BCAST64 + s, W::bcast64(q, s));
        put(S_Z_BCAST + s, Z::bcast(za, s));
    }
}

// the same with the host forms
static void host_ops(const Case &c, uint64_t *out)
{
    typedef pdw::HostWave W;
    typedef pdz::HostWave Z;
    W::Var<uint32_t> a, b, h; W::Var<uint64_t> q; Z::Var<uint32_t> za;
    for (int l = 0; l < 64; ++l) { a[l] = c.a[l]; b[l] = c.b[l]; h[l] = c.h[l]; q[l] = c.q[l]; za[l] = c.a[l]; }
    uint32_t total = 0;
    const W::Var<uint32_t> es = W::excl_scan(a, &total), su = W::shift_up1(a, c.fill), im = W::incl_scan_max(a), sh = W::shfl(a, b);
    const W::Var<uint64_t> em = W::excl_scan_max64(q), sm = W::seg_excl_scan_max64(q, h);
    for (int l = 0; l < 64; ++l) {
        auto put = [&](int slot, uint64_t x) { out[slot * 64 + l] = x; };
        put(S_BALLOT_EQ, W::ballot_eq(a, c.v));
        put(S_BALLOT_NE, W::ballot_ne(a, c.v));
        put(S_PREFIX_COUNT, W::prefix_count(c.mask, l));
        put(S_EXCL_SCAN, es[l]);
        put(S_EXCL_SCAN_TOTAL, total);
        put(S_SHIFT_UP1, su[l]);
        put(S_INCL_SCAN_MAX, im[l]);
        put(S_SHFL, sh[l]);
        put(S_MIN_WHERE, W::min_where(a, b));
        put(S_UNI, W::uni(c.v));
        put(S_EXCL_SCAN_MAX64, em[l]);
        put(S_SEG_EXCL_SCAN_MAX64, sm[l]);
        put(S_REDUCE_OR, W::reduce_or(a));
        put(S_REDUCE_XOR, W::reduce_xor(a));
        put(S_REDUCE_MAX, W::reduce_max(a));
        put(S_REDUCE_MAX64, W::reduce_max64(q));
        put(S_REDUCE_MIN64, W::reduce_min64(q));
        put(S_Z_BALLOT_EQ, Z::ballot_eq(za, c.v));
        put(S_Z_BALLOT_NE, Z::ballot_ne(za, c.v));
        put(S_Z_REDUCE_MAX, Z::reduce_max(za));
        put(S_Z_UNI, Z::uni(c.v));
        for (int s = 0; s < 64; ++s) {
            put(S_BCAST + s, W::bcast(a, s));
            put(S_BCAST_U + s, W::bcast_u(a, (uint32_t)s));
            put(S_BCAST64 + s, W::bcast64(q, s));
            put(S_Z_BCAST + s, Z::bcast(za, s));
        }
    }
}

// ---- the cases ----
static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd64() { uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull); x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }

struct Named { std::string name; Case c; };

// heads (a bit per lane) -> the head1 form chain_device hands to seg_excl_scan_max64
static void set_heads(Case &c, uint64_t heads) { uint32_t cur = 0; for (int l = 0; l < 64; ++l) { if ((heads >> l) & 1) cur = (uint32_t)l + 1u; c.h[l] = cur; } }

// a case with every field random: the fixed lists overwrite the fields they are about
static Case random_case(int kind)
{
    Case c;
    for (int l = 0; l < 64; ++l) {
        const uint64_t r = rnd64(), r2 = rnd64();
        c.a[l] = kind == 0 ? (uint32_t)r : kind == 1 ? (uint32_t)(r % 7) : kind == 2 ? (uint32_t)(r % 100000) : (uint32_t)r | 0x80000000u;
        c.b[l] = kind == 1 ? (uint32_t)((r >> 32) % 3 == 0) : (uint32_t)(r >> 32);            // (shfl takes b & 63; min_where skips where b != 0)
        c.q[l] = kind == 0 ? r2 : kind == 1 ? r2 % 5 : kind == 2 ? (r2 << 32) | 7u : r2 >> (r % 64);
    }
    c.mask = kind == 1 ? rnd64() & rnd64() & rnd64() : rnd64();
    c.v = c.a[rnd64() % 64]; c.fill = (uint32_t)rnd64();
    set_heads(c, kind == 2 ? rnd64() & rnd64() & rnd64() & rnd64() : kind == 3 ? rnd64() : rnd64() & rnd64());
    return c;
}

static std::vector<Named> make_cases()
{
    std::vector<Named> v;
    auto add = [&](const std::string &n, const Case &c) { v.push_back(Named{n, c}); };
    const int seams[6] = {0, 15, 16, 31, 32, 63};      // the row and half-wave seams of the DPP pattern
    { Case c = random_case(0); memset(c.a, 0, sizeof c.a); memset(c.q, 0, sizeof c.q); c.v = 0; c.mask = 0; add("all zero", c); }
    { Case c = random_case(0); memset(c.a, 0xff, sizeof c.a); memset(c.q, 0xff, sizeof c.q); c.v = 0xFFFFFFFFu; c.mask = ~0ull; c.fill = 0; add("all ones (the sum wraps)", c); }
    for (int s : seams)
        for (int big = 0; big < 2; ++big) {
            Case c = random_case(0); memset(c.a, 0, sizeof c.a); memset(c.q, 0, sizeof c.q);
            c.a[s] = big ? 0xFFFFFFFFu : 1u; c.q[s] = big ? ~0ull : 1ull << 32; c.v = big ? 0u : 1u; c.mask = 1ull << s; set_heads(c, 0);
            add("one non-zero value at lane " + std::to_string(s) + (big ? " (all ones)" : ""), c);
        }
    for (int s : seams) {                               // ... and the mirror image: one zero among all ones
        Case c = random_case(0); memset(c.a, 0xff, sizeof c.a); memset(c.q, 0xff, sizeof c.q); c.a[s] = 0; c.q[s] = 0; c.v = 0; c.mask = ~(1ull << s);
        add("one zero at lane " + std::to_string(s), c);
    }
    { Case c = random_case(0); for (int l = 0; l < 64; ++l) { c.a[l] = 1000u + 3u * l; c.q[l] = (1ull << 40) + 5ull * l; } set_heads(c, 0); add("strictly increasing", c); }
    { Case c = random_case(0); for (int l = 0; l < 64; ++l) { c.a[l] = 0xFFFFFF00u - 3u * l; c.q[l] = ~0ull - 5ull * l; } set_heads(c, 0); add("strictly decreasing", c); }
    for (int k = 0; k < 4; ++k) {                       // 64-bit values that differ only above bit 32 (the 64-bit operations are two 32-bit shuffles)
        Case c = random_case(0);
        for (int l = 0; l < 64; ++l) c.q[l] = ((uint64_t)(k == 0 ? l : k == 1 ? 63 - l : rnd64() % 64) << (k == 3 ? 33 : 32)) | 0x89ABCDEFu;
        if (k >= 2) set_heads(c, rnd64() & rnd64());
        add("64-bit values equal below bit 32, variant " + std::to_string(k), c);
    }
    { Case c = random_case(0); for (int l = 0; l < 64; ++l) c.b[l] = 1u + (uint32_t)l; add("min_where: every lane skipped", c); }
    for (int s : seams)
        for (int k = 0; k < 2; ++k) {
            Case c = random_case(k ? 3 : 0); for (int l = 0; l < 64; ++l) c.b[l] = l == s ? 0u : 0x80000000u >> (l % 32);
            add("min_where: only lane " + std::to_string(s) + " not skipped", c);
        }
    { Case c = random_case(0); for (int l = 0; l < 64; ++l) c.b[l] = (uint32_t)(63 - l); add("shfl: reversed", c); }
    { Case c = random_case(0); for (int l = 0; l < 64; ++l) c.b[l] = (uint32_t)(l ^ 32) | 0xFFFFFFC0u; add("shfl: across the halves, high bits set", c); }
    // seg_excl_scan_max64: head layouts
    const uint64_t fixed_heads[4] = {0ull, 1ull, ~0ull, (1ull << 1) | (1ull << 16) | (1ull << 32) | (1ull << 63)};
    const char *const head_names[4] = {"no head (open from before lane 0)", "a head at lane 0", "heads at every lane", "heads at 1, 16, 32 and 63"};
    for (int k = 0; k < 4; ++k)
        for (int kind = 0; kind < 4; ++kind) { Case c = random_case(kind); set_heads(c, fixed_heads[k]); add(std::string("seg scan: ") + head_names[k], c); }
    for (int k = 0; k < 24; ++k) { Case c = random_case(k % 4); set_heads(c, k < 8 ? rnd64() & rnd64() & rnd64() & rnd64() : k < 16 ? rnd64() & rnd64() : rnd64()); add("seg scan: heads at random sorted lanes", c); }
    for (int k = 0; k < 24; ++k) {                      // the maximum sits in the lane just before a head: it must not leak across
        Case c = random_case(2);
        uint64_t heads = k < 4 ? fixed_heads[3] : (rnd64() & rnd64() & rnd64()) & ~1ull;
        if (!heads) heads = 1ull << 40;
        set_heads(c, heads);
        for (int l = 0; l < 64; ++l) c.q[l] = ((heads >> l) >> 1) & 1 ? ~0ull - (uint64_t)l : rnd64() >> 20;
        add("seg scan: the maximum in the lane before a head", c);
    }
    for (int k = 0; k < 400; ++k) add("random vectors, seed step " + std::to_string(k), random_case(k % 4));
    return v;
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
int main()
{
    const std::vector<Named> cases = make_cases();
    Case *d_in; uint64_t *d_out;
    CHECK(hipMalloc(&d_in, sizeof(Case))); CHECK(hipMalloc(&d_out, (size_t)N_SLOT * 64 * sizeof(uint64_t)));
    std::vector<uint64_t> got((size_t)N_SLOT * 64), want((size_t)N_SLOT * 64);
    size_t differ = 0;
    for (size_t k = 0; k < cases.size(); ++k) {
        CHECK(hipMemcpy(d_in, &cases[k].c, sizeof(Case), hipMemcpyHostToDevice));
        CHECK(hipMemset(d_out, 0xA5, got.size() * sizeof(uint64_t)));
        hipLaunchKernelGGL(k_wave_ops, dim3(1), dim3(64), 0, 0, (const Case *)d_in, d_out);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(got.data(), d_out, got.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        host_ops(cases[k].c, want.data());
        for (size_t i = 0; i < got.size(); ++i)
            if (got[i] != want[i]) {
                if (!differ) printf("%s differs in case %zu (%s), lane %zu: device %016llx, host %016llx\n", slot_name((int)(i / 64)).c_str(), k, cases[k].name.c_str(), i % 64,
                                    (unsigned long long)got[i], (unsigned long long)want[i]);
                ++differ;
                break;
            }
    }
    printf("%zu cases, %zu differ\n", cases.size(), differ);
    (void)hipFree(d_in); (void)hipFree(d_out);
    return differ ? 1 : 0;
}
