// The 64-bit key of THE ORDER on the candidates of a context (rank.hip, include/cffm_hip.h), larger = better: scores compare as IEEE
// floats with -0 == +0, NaN ranks below everything (-inf included), among equal scores the smaller position wins.  Shared by the
// ranking kernels (rank.hip) and the hard-negative pick (hard.hip); tests/_rank_ref.py key64() is the numpy twin.
#pragma once

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ unsigned long long rank_key64(unsigned u, unsigned pos) {
    unsigned k32 = 0;                                             // NaN: below -inf (whose key32 is 0x007fffff)
    if ((u & 0x7fffffffu) <= 0x7f800000u) {
        if (u == 0x80000000u) u = 0;                              // -0 == +0
        k32 = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)k32 << 32) | (unsigned long long)(0xffffffffu - pos);
}

}  // namespace
