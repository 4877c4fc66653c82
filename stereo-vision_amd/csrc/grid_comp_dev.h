// Device helpers shared by the layers that work on labelled components (csrc/grid_front_kernels.hip, csrc/grid_obj_kernels.hip):
// the rank of a label among the ascending roots, and one value per wave from one per lane.
#ifndef SVH_GRID_COMP_DEV_H
#define SVH_GRID_COMP_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svh {
namespace grid {

// the rank of a label among the n ascending roots; every label of a finished plane is one of them
__device__ __forceinline__ int32_t rank_of(const int32_t* __restrict__ roots, int32_t n, int32_t label) {
    int32_t lo = 0, hi = n - 1;
    while (lo < hi) {                                   // at most 26 halvings
        const int32_t mid = (lo + hi) >> 1;
        if (roots[mid] < label) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One value per wave from one per lane.  Every lane of the wave calls them.
__device__ __forceinline__ int32_t wave_sum(int32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int32_t wave_min(int32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int32_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int32_t)(uint32_t)(v >> 32), off, 64), lo = (uint32_t)__shfl_xor((int32_t)(uint32_t)v, off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

}  // namespace grid
}  // namespace svh
#endif
