// wave_ops.h -- wave64 reductions and the inclusive scan, device only.  Every lane of the wave must take part.
// Block-level sums and scans keep their own LDS protocols and reduction orders beside their kernels; only the wave step lives here.
#pragma once
#include <hip/hip_runtime.h>

namespace chk {

// butterfly sum: every lane receives the sum of all 64
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// butterfly max: every lane receives the largest of all 64
__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    return m;
}

// inclusive scan: lane i receives v of lanes 0 .. i (lane = the caller's index within its wave)
template <class T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    return v;
}

}  // namespace chk
