// Device-side primitives shared by the .hip files (device code only: include from a .hip file).
#ifndef SVH_DEV_COMMON_H
#define SVH_DEV_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svh {

// A pointer read out of a job table in memory has lost its address space: hipcc then reads and writes through FLAT
// instructions (round 4: 913 of them in the lockstep kernels, 514 in k_refine_parabolic_b alone).  Every buffer of a
// job is device (or device-mapped pinned host) memory: a round trip through address space 1 tells the compiler so and
// the kernel uses global_load / global_store like its single-object form.
template <class T>
__device__ __forceinline__ T* as_global(T* p) {
    // (the empty asm keeps the address-space-1 value opaque: a plain generic -> global -> generic cast pair is folded
    // away before the compiler's address-space inference sees it; held in a vector register pair, which is why this
    // is for pointers out of memory only -- a kernel argument would leave its scalar registers)
    __attribute__((address_space(1))) T* q = (__attribute__((address_space(1))) T*)p;
    asm volatile("" : "+v"(q));
    return (T*)q;
}
// as_global on each of the named pointer variables
template <class... T>
__device__ __forceinline__ void all_global(T*&... p) {
    ((p = as_global(p)), ...);
}

// Exclusive prefix sum of `value` over the kThreads threads of the workgroup, in thread order; *total = the sum of
// all.  A scan inside each wave by lane shuffles, then the kThreads / 64 wave totals through s_wave (LDS, that many
// ints, the caller's): two barriers, where a Hillis-Steele scan over 1024 threads takes twenty.  Every thread of the
// workgroup must call it.
template <int kThreads>
__device__ __forceinline__ int block_exclusive_scan(int value, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = value;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        const int x = s_wave[w];
        before += w < wave ? x : 0;
        all += x;
    }
    // This second barrier is what makes two calls in a row with the same s_wave safe: no wave writes its total of
    // the next scan before every wave has read the totals of this one.
    __syncthreads();
    *total = all;
    return before + incl - value;
}

__device__ __forceinline__ int32_t sat_u8(int32_t x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// Separable Sobel on packed 16-bit pairs (v_pk_* arithmetic): two adjacent columns per register
typedef short s16x2 __attribute__((ext_vector_type(2)));
// bytes 0,1 / 2,3 of a word of four pixels, widened to a pair
__device__ __forceinline__ s16x2 pk_bytes01(uint32_t w) { return __builtin_bit_cast(s16x2, __builtin_amdgcn_perm(0u, w, 0x0c010c00u)); }
__device__ __forceinline__ s16x2 pk_bytes23(uint32_t w) { return __builtin_bit_cast(s16x2, __builtin_amdgcn_perm(0u, w, 0x0c030c02u)); }
// (a.hi, b.lo): the pair one column to the right of a, given the next pair b
__device__ __forceinline__ s16x2 pk_mid(s16x2 a, s16x2 b) {
    return __builtin_bit_cast(s16x2, __builtin_amdgcn_alignbyte(__builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, a), 2u));
}
// four values in two pairs -> their low bytes in one word
__device__ __forceinline__ uint32_t pk_to_bytes(s16x2 lo, s16x2 hi) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, hi), __builtin_bit_cast(uint32_t, lo), 0x06040200u);
}
// sat_u8((v >> kShift) + 128) of both halves: kShift = 2 for the 3x3 Sobel of ELAS, 7 for the Matcher's 5x5
template <int kShift>
__device__ __forceinline__ s16x2 pk_sobel_out(s16x2 v) {
    const s16x2 lo = {0, 0}, hi = {255, 255}, off = {128, 128};
    return __builtin_elementwise_min(__builtin_elementwise_max((v >> kShift) + off, lo), hi);
}

}  // namespace svh
#endif
