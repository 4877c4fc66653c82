// Voxel-grid thinning of the map view's point store (svh_view_thin): of all points that fall into one voxel the one with
// the lowest store index stays, in place order, bit for bit.  The arithmetic is csrc/view_thin_core.h.
//
//   k_thin_insert   one lane per point: the voxel's key enters a lock-free open-addressing table in device memory
//                   (atomicCAS on the key slot, linear probing from hash & mask), then atomicMin of the point's index
//                   on the slot's winner word.  The MINIMUM decides, not the arrival: the result is the same under
//                   every schedule.  No lane waits for another: a CAS that loses has met a filled slot and moves on,
//                   and keys never change once set.  The probe is bounded by the capacity; the load factor is at most
//                   one half, so it ends at its own key or an empty slot long before.
//   k_thin_flag     keep iff the winner of the remembered slot is the own index (or the point has no voxel); the
//                   survivors of each block of 1024 are counted by wave ballots.
//   k_thin_scan     exclusive scan of the block counts: one workgroup, 1024 counts at a time, the carry in a register
//                   (the scheme of the map fusion's k_map_scan with dev_common.h's two-barrier scan).
//   k_thin_scatter  ordered compaction: block offset + waves before + ballot bits below the own lane; 16-byte loads
//                   and stores of the float4 points.
//   k_thin_bounds   the survivors before each list boundary, one wave per boundary: block offset + the flags of the
//                   boundary's block in front of it.  The host subtracts neighbours; it never loops over points.
//
// Device-scope atomics (HIP's default for atomicCAS / atomicMin / atomicAdd on global memory) are what the table needs
// across the eight XCDs; the kernel boundary publishes the table to k_thin_flag.
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "view_internal.h"
#include "view_thin_core.h"

namespace svh {
namespace view {
namespace {

constexpr int kBlock = (int)THIN_BLOCK;
constexpr int kWaves = kBlock / 64;

__global__ __launch_bounds__(256) void k_thin_insert(const float4* __restrict__ pts, uint32_t n, float voxel,
                                                     unsigned long long* __restrict__ keys, uint32_t* __restrict__ win,
                                                     uint64_t capacity, uint32_t* __restrict__ slot,
                                                     uint8_t* __restrict__ keep, unsigned long long* __restrict__ unplaced) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool in = i < n;
    uint64_t key = thin::EMPTY_KEY;
    if (in) {
        const float4 p = pts[i];
        key = thin::key_of(p.x, p.y, p.z, voxel);
    }
    const bool homeless = in && key == thin::EMPTY_KEY;
    const unsigned long long b = __ballot(homeless);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(unplaced, (unsigned long long)__popcll(b));
    if (!in) return;
    if (homeless) {
        keep[i] = 2;
        return;
    }
    const uint64_t mask = capacity - 1;
    uint64_t s = thin::home_of(key, capacity);
    bool found = false;
    for (uint64_t step = 0; step < capacity; step++) {
        const unsigned long long was = atomicCAS(&keys[s], (unsigned long long)thin::EMPTY_KEY, (unsigned long long)key);
        if (was == thin::EMPTY_KEY || was == key) {
            found = true;
            break;
        }
        s = (s + 1) & mask;
    }
    if (found) {
        slot[i] = (uint32_t)s;
        atomicMin(&win[s], i);
        keep[i] = 0;
    } else {
        keep[i] = 2;   // a full table: cannot happen at a load factor of one half; the point is kept, nothing is lost
    }
}

__global__ __launch_bounds__(kBlock) void k_thin_flag(uint32_t n, const uint32_t* __restrict__ win,
                                                      const uint32_t* __restrict__ slot, uint8_t* __restrict__ keep,
                                                      int32_t* __restrict__ blockcnt) {
    __shared__ int s_cnt[kWaves];
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    bool k = false;
    if (i < n) {
        k = keep[i] == 2 || win[slot[i]] == i;
        keep[i] = k ? 1 : 0;
    }
    const unsigned long long b = __ballot(k);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) sum += s_cnt[w];
        blockcnt[blockIdx.x] = sum;
    }
}

// in place: blockcnt[i] becomes the number of survivors in the blocks before i; out[0] = all survivors
__global__ __launch_bounds__(kBlock) void k_thin_scan(int32_t* __restrict__ blockcnt, uint32_t nb, int64_t* __restrict__ out) {
    __shared__ int s_wave[kWaves];
    int carry = 0;
    for (uint32_t base = 0; base < nb; base += (uint32_t)kBlock) {
        const uint32_t i = base + threadIdx.x;
        const int x = i < nb ? blockcnt[i] : 0;
        int chunk;
        const int before = block_exclusive_scan<kBlock>(x, s_wave, &chunk);
        if (i < nb) blockcnt[i] = carry + before;
        carry += chunk;
    }
    if (threadIdx.x == 0) out[0] = carry;
}

__global__ __launch_bounds__(kBlock) void k_thin_scatter(const float4* __restrict__ pts, uint32_t n,
                                                         const uint8_t* __restrict__ keep,
                                                         const int32_t* __restrict__ blockoff, float4* __restrict__ dst) {
    __shared__ int s_cnt[kWaves];
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool k = i < n && keep[i] != 0;
    const unsigned long long b = __ballot(k);
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    if (!k) return;
    int at = blockoff[blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; w++) at += w < wave ? s_cnt[w] : 0;
    at += __popcll(b & (((unsigned long long)1 << lane) - 1));
    dst[at] = pts[i];
}

// out[2 + k] = survivors among the points in front of store position bounds[k]
__global__ __launch_bounds__(256) void k_thin_bounds(const int64_t* __restrict__ bounds, int32_t nbounds, uint32_t n,
                                                     const uint8_t* __restrict__ keep, const int32_t* __restrict__ blockoff,
                                                     int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int32_t k = (int32_t)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (k >= nbounds) return;   // a whole wave leaves: the shuffles below have all their lanes
    const int64_t b64 = bounds[k];
    if (b64 >= (int64_t)n) {
        if (lane == 0) out[2 + k] = out[0];
        return;
    }
    const uint32_t b = (uint32_t)b64, base = b & ~(uint32_t)(kBlock - 1);
    int cnt = 0;
    for (uint32_t j = base + (uint32_t)lane; j < b; j += 64) cnt += keep[j];
    for (int off = 32; off; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) out[2 + k] = (int64_t)blockoff[b / (uint32_t)kBlock] + cnt;
}

}  // namespace

void launch_thin(hipStream_t s, const ThinJob& j) {
    if (j.n == 0) return;
    const unsigned nb = (j.n + THIN_BLOCK - 1) / THIN_BLOCK;
    hipLaunchKernelGGL(k_thin_insert, dim3((j.n + 255) / 256), dim3(256), 0, s, j.pts, j.n, j.voxel, j.keys, j.win, j.capacity,
                       j.slot, j.keep, (unsigned long long*)(j.out + 1));
    hipLaunchKernelGGL(k_thin_flag, dim3(nb), dim3(kBlock), 0, s, j.n, j.win, j.slot, j.keep, j.blockcnt);
    hipLaunchKernelGGL(k_thin_scan, dim3(1), dim3(kBlock), 0, s, j.blockcnt, nb, j.out);
    hipLaunchKernelGGL(k_thin_scatter, dim3(nb), dim3(kBlock), 0, s, j.pts, j.n, j.keep, j.blockcnt, j.dst);
    hipLaunchKernelGGL(k_thin_bounds, dim3(((unsigned)j.nbounds + 3) / 4), dim3(256), 0, s, j.bounds, j.nbounds, j.n, j.keep,
                       j.blockcnt, j.out);
}

}  // namespace view
}  // namespace svh
