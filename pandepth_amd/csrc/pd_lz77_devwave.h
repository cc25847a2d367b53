// pd_lz77_devwave.h — the hardware wavefront pd_lz77.h's parse runs on (its W on the device; pdz::HostWave is the 64-lanes-in-a-loop
// form).  Lives in a header of its own so that the kernels (pd_deflate.hip) and the test that compares its primitives with the host
// form lane by lane (tests/harness/wave_ops_gpu_check.hip) compile the same text.
#ifndef PD_LZ77_DEVWAVE_H_
#define PD_LZ77_DEVWAVE_H_
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace pdz {

struct DevWaveZ {                               // the hardware wavefront (pd_lz77.h's W)
    template <class T> struct Var { T v; __device__ T &operator[](int) { return v; } __device__ const T &operator[](int) const { return v; } };
    template <class F> __device__ static __forceinline__ void each(F f) { f((int)(threadIdx.x & 63)); }
    __device__ static __forceinline__ uint64_t ballot_eq(const Var<uint32_t> &x, uint32_t v) { return __ballot(x.v == v); }
    __device__ static __forceinline__ uint64_t ballot_ne(const Var<uint32_t> &x, uint32_t v) { return __ballot(x.v != v); }
    __device__ static __forceinline__ uint32_t reduce_max(const Var<uint32_t> &x)
    {
        uint32_t m = x.v;
#pragma unroll
        for (int o = 32; o; o >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)m, o); m = y > m ? y : m; }
        return m;
    }
    // (lane is the same in every lane: a lane read through a scalar register instead of a trip through the LDS crossbar)
    __device__ static __forceinline__ uint32_t bcast(const Var<uint32_t> &x, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)x.v, __builtin_amdgcn_readfirstlane(lane)); }
    __device__ static __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
    __device__ static __forceinline__ void loads_landed() { __builtin_amdgcn_s_waitcnt(0x0F70); }            // s_waitcnt vmcnt(0)
    __device__ static __forceinline__ bool lead() { return (threadIdx.x & 63) == 0; }
};

} // namespace pdz
#endif

#endif
