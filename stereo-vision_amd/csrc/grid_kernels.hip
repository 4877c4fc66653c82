// The ground grid on the device (svh_grid_*, include/svh_grid.h).  The arithmetic is csrc/grid_core.h.
//
//   k_grid_bin       one lane per point, one 16-byte load per lane, grid-stride beyond BIN_MAX_BLOCKS workgroups.  A low
//                    point updates its cell with five no-return integer atomics at device scope (HIP's default on global
//                    memory, which is what the eight XCDs need): count +, kmin min, kmax max, hsum + (64 bits), vsum +
//                    (64 bits); an overhead point with one.  Integer +, min and max commute, so the grid is the same
//                    under every schedule.  The four statistics are counted per wave by ballot / popcount, kept in a
//                    register over the wave's passes and added once per wave.
//                    Runs are combined first: the store arrives in frame order and the map fusion emits points column by
//                    column, so consecutive lanes often hit the same cell.  Each lane compares its cell with the lane
//                    before it, a segmented wave scan (six __shfl_up steps) combines count, min key, max key, hsum and
//                    vsum along each run of equal cells, and only the last lane of a run issues atomics.  A lane that is
//                    not a low point ends the run on both sides of it; a run that crosses a wave boundary is two runs.
//                    It is the same multiset of updates as five atomics from every low lane -- the plain form this was
//                    measured against (profiles/grid_times.jsonl, DESIGN.md "Ground grid") and which was then deleted.
//   k_grid_finalise  one lane per cell: the accumulators become HMIN, HMAX, HMEAN, INTENSITY and CLASS (COUNT and
//                    OVERHEAD are the accumulators themselves).
//   k_grid_render    one lane per pixel: the colour of the cell, rows flipped so that forward is up.
#include <hip/hip_runtime.h>

#include "grid_core.h"
#include "grid_internal.h"

namespace svh {
namespace grid {
namespace {

__global__ __launch_bounds__(BIN_BLOCK) void k_grid_bin(Params prm, const float4* __restrict__ pts, long long n, Cells c,
                                                        unsigned long long* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    uint32_t seen[4] = {0u, 0u, 0u, 0u};   // per fate, the same in every lane of the wave
    const long long stride = (long long)gridDim.x * BIN_BLOCK;
    // a wave goes on while its first lane has a point: all 64 lanes make every pass, the shuffles below have them all
    for (long long base = (long long)blockIdx.x * BIN_BLOCK + (threadIdx.x & ~63u); base < n; base += stride) {
        const long long i = base + lane;
        Placed r{-1, NO_CELL, 0u, 0, 0u};
        if (i < n) {
            const float4 p = pts[i];
            r = place(prm, p.x, p.y, p.z, p.w);
        }
#pragma unroll
        for (int f = 0; f < 4; f++) seen[f] += (uint32_t)__popcll(__ballot(r.fate == f));
        if (r.fate == OVERHEAD) atomicAdd(&c.overhead[r.cell], 1);
        const bool low = r.fate == LOW;
        const uint32_t rid = low ? r.cell : NO_CELL;   // a cell index is below 2^26
        const uint32_t before = __shfl_up(rid, 1, 64), after = __shfl_down(rid, 1, 64);
        int head = lane == 0 || before != rid;
        const bool tail = lane == 63 || after != rid;
        uint32_t cnt = 1u, mn = r.key, mx = r.key, vs = r.v;
        long long hs = r.q;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t cnt2 = __shfl_up(cnt, d, 64), mn2 = __shfl_up(mn, d, 64), mx2 = __shfl_up(mx, d, 64),
                           vs2 = __shfl_up(vs, d, 64);
            const long long hs2 = __shfl_up(hs, d, 64);
            const int head2 = __shfl_up(head, d, 64);
            if (lane >= d && !head) {
                cnt += cnt2;
                mn = mn2 < mn ? mn2 : mn;
                mx = mx2 > mx ? mx2 : mx;
                vs += vs2;
                hs += hs2;
                head = head2;
            }
        }
        if (low && tail) {
            atomicAdd(&c.count[r.cell], (int32_t)cnt);
            atomicMin(&c.kmin[r.cell], mn);
            atomicMax(&c.kmax[r.cell], mx);
            atomicAdd(&c.hsum[r.cell], (unsigned long long)hs);
            atomicAdd(&c.vsum[r.cell], (unsigned long long)vs);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int f = 0; f < 4; f++)
            if (seen[f]) atomicAdd(&stats[f], (unsigned long long)seen[f]);
    }
}

__device__ __forceinline__ Cell load_cell(const Cells& c, uint32_t i) {
    return Cell{c.count[i], c.overhead[i], c.kmin[i], c.kmax[i], (int64_t)c.hsum[i], (uint64_t)c.vsum[i]};
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_finalise(Params prm, Cells c, float* __restrict__ hmin,
                                                             float* __restrict__ hmax, float* __restrict__ hmean,
                                                             uint8_t* __restrict__ intensity, uint8_t* __restrict__ cls) {
    const uint32_t i = blockIdx.x * FIN_BLOCK + threadIdx.x;
    if (i >= (uint32_t)prm.nx * (uint32_t)prm.nz) return;
    const Final f = finalise(prm, load_cell(c, i));
    hmin[i] = f.hmin, hmax[i] = f.hmax, hmean[i] = f.hmean;
    intensity[i] = f.intensity, cls[i] = f.cls;
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_render(Params prm, int32_t mode, const int32_t* __restrict__ count,
                                                           const float* __restrict__ hmin, const float* __restrict__ hmax,
                                                           const float* __restrict__ hmean,
                                                           const uint8_t* __restrict__ intensity,
                                                           const uint8_t* __restrict__ cls, uint8_t* __restrict__ rgb) {
    const uint32_t o = blockIdx.x * FIN_BLOCK + threadIdx.x;
    if (o >= (uint32_t)prm.nx * (uint32_t)prm.nz) return;
    const uint32_t row = o / (uint32_t)prm.nx, col = o - row * (uint32_t)prm.nx;
    const uint32_t i = ((uint32_t)prm.nz - 1u - row) * (uint32_t)prm.nx + col;
    const Final f{hmin[i], hmax[i], hmean[i], intensity[i], cls[i]};
    uint8_t px[3];
    colour(prm, mode, count[i], f, px);
    rgb[3 * (size_t)o] = px[0], rgb[3 * (size_t)o + 1] = px[1], rgb[3 * (size_t)o + 2] = px[2];
}

}  // namespace

void launch_bin(hipStream_t s, const BinJob& j) {
    if (j.n <= 0) return;
    const long long want = (j.n + BIN_BLOCK - 1) / BIN_BLOCK;
    const unsigned blocks = (unsigned)(want < (long long)BIN_MAX_BLOCKS ? want : (long long)BIN_MAX_BLOCKS);
    hipLaunchKernelGGL(k_grid_bin, dim3(blocks), dim3(BIN_BLOCK), 0, s, j.prm, j.pts, (long long)j.n, j.cells, j.stats);
}

void launch_finalise(hipStream_t s, const FinalJob& j) {
    const unsigned cells = (unsigned)j.prm.nx * (unsigned)j.prm.nz;
    hipLaunchKernelGGL(k_grid_finalise, dim3((cells + FIN_BLOCK - 1) / FIN_BLOCK), dim3(FIN_BLOCK), 0, s, j.prm, j.cells, j.hmin,
                       j.hmax, j.hmean, j.intensity, j.cls);
}

void launch_render(hipStream_t s, const RenderJob& j) {
    const unsigned cells = (unsigned)j.prm.nx * (unsigned)j.prm.nz;
    hipLaunchKernelGGL(k_grid_render, dim3((cells + FIN_BLOCK - 1) / FIN_BLOCK), dim3(FIN_BLOCK), 0, s, j.prm, j.mode, j.count,
                       j.hmin, j.hmax, j.hmean, j.intensity, j.cls, j.rgb);
}

}  // namespace grid
}  // namespace svh
