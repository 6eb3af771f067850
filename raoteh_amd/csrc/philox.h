// Philox-4x32-10 (Salmon et al. 2011), the counter-based generator of the sampling kernels
// (forest.hip, sample.hip): a draw is a function of (seed, sweep or draw number, index) alone, so
// it does not depend on how a batch is laid out or scheduled.
#pragma once

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ void philox_round(unsigned &c0, unsigned &c1, unsigned &c2, unsigned &c3,
                                             unsigned k0, unsigned k1)
{
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

// uniform double in [0, 1) with 53 random bits for (seed, sweep, index)
__device__ __forceinline__ double philox_uniform(unsigned long long seed, unsigned long long sweep,
                                                 unsigned long long index)
{
    unsigned c0 = (unsigned)index, c1 = (unsigned)(index >> 32);
    unsigned c2 = (unsigned)sweep, c3 = (unsigned)(sweep >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const unsigned long long bits = ((unsigned long long)c0 << 21) ^ (unsigned long long)(c1 >> 11);
    return (double)(bits & ((1ull << 53) - 1)) * (1.0 / 9007199254740992.0);
}

}  // namespace
