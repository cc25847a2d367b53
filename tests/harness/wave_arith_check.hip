// tests/harness/wave_arith_check.hip — TEST INFRASTRUCTURE: the DEVICE forms of the match copier's arithmetic in
// pd_inflate_wave.h against plain integers, on the GPU.  small_mod() divides through v_rcp_f32 there (1.0f / d on the host),
// gather8() is two v_perm_b32 (a byte loop on the host); inflate_wave_check -g checks the host forms, this checks what the
// kernel executes:
//   small_mod(off, d) == off % d            for every off < 65536, 1 <= d <= 300 (the copier calls it with off < len <= 258, d < len)
//   gather8(raw, period_selector(d, o))     byte k == byte (o + k) % d of raw, for every period d = 1 .. 7, phase o < d, 4096 words
// Prints the number of disagreements (expected: 0) and exits 1 if there is one.  Not part of the library's ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../pandepth_amd/csrc/pd_inflate_wave.h"

__global__ void k_small_mod(unsigned long long *bad, unsigned *first)
{
    const uint32_t n = 300u * 65536u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t d = 1 + (i >> 16), off = i & 0xffffu;
        if (pdw::small_mod(off, d) != off % d) { if (atomicAdd(bad, 1ull) == 0) { first[0] = off; first[1] = d; } }
    }
}

__device__ uint64_t mix64(uint64_t x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }

__global__ void k_gather(unsigned long long *bad, unsigned *first, uint32_t words)
{
    const uint32_t n = 7u * 8u * words;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t w = i / 56u, d = 1 + (i % 56u) / 8u, o = i % 8u;
        if (o >= d) continue;
        const uint64_t raw = w == 0 ? 0x0706050403020100ull : w == 1 ? ~0ull : mix64(w);
        uint64_t want = 0;
        for (int k = 0; k < 8; ++k) want |= ((raw >> (8 * ((o + k) % d))) & 0xff) << (8 * k);
        if (pdw::gather8(raw, pdw::period_selector(d, o)) != want) { if (atomicAdd(bad, 1ull) == 0) { first[0] = o; first[1] = d; } }
    }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
int main()
{
    unsigned long long *bad; unsigned *first;
    CHECK(hipMalloc(&bad, 2 * sizeof *bad)); CHECK(hipMalloc(&first, 4 * sizeof *first));
    CHECK(hipMemset(bad, 0, 2 * sizeof *bad)); CHECK(hipMemset(first, 0, 4 * sizeof *first));
    const uint32_t words = 4096;
    hipLaunchKernelGGL(k_small_mod, dim3(1024), dim3(256), 0, 0, bad, first);
    hipLaunchKernelGGL(k_gather, dim3(256), dim3(256), 0, 0, bad + 1, first + 2, words);
    CHECK(hipDeviceSynchronize());
    unsigned long long hb[2]; unsigned hf[4];
    CHECK(hipMemcpy(hb, bad, sizeof hb, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(hf, first, sizeof hf, hipMemcpyDeviceToHost));
    printf("small_mod: %u pairs, %llu disagreements", 300u * 65536u, hb[0]);
    if (hb[0]) printf(" (one of them: off %u, d %u)", hf[0], hf[1]);
    printf("\ngather8 / period_selector: %u cases, %llu disagreements", 28u * words, hb[1]);
    if (hb[1]) printf(" (one of them: phase %u, period %u)", hf[2], hf[3]);
    printf("\n");
    (void)hipFree(bad); (void)hipFree(first);
    return hb[0] || hb[1] ? 1 : 0;
}
