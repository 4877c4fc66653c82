// The exploration layer of the ground grid on the device (svh_grid_view_gain, svh_grid_view_mask, svh_grid_explore_rank,
// svh_grid_render_view; include/svh_grid.h, "EXPLORATION").  The arithmetic is csrc/grid_explore_core.h: integer work on the
// finished STATE plane and the reach field in logical order.  GAIN is the size of a set, the score a function of two integers and
// the best the minimum of unique keys, so nothing here depends on the launch shape or the scheduling.
//
//   k_grid_view_gain      one workgroup of 256 lanes per viewpoint (the workgroups stride over the viewpoints beyond 16384).  The
//                         8 R rays are dealt to the lanes, 8 R / 256 passes of them; a lane walks its ray cell by cell (view_ray
//                         of the core header) and marks every UNEXPLORED cell it visits in a bitmap of (2 R + 1)^2 bits in LDS --
//                         at most 2065 words, 8.3 KB -- by an LDS atomicOr: a cell that many rays visit is one bit.  After one
//                         barrier the lanes popcount the words, the counts are summed by block_exclusive_scan (dev_common.h) and
//                         lane 0 stores the GAIN: one store per viewpoint, no global atomic, no scratch in HBM, and no host
//                         wait between viewpoints.  A viewpoint outside the window is the same for every lane of the workgroup.
//   k_grid_view_mask      one workgroup: the same walk for one viewpoint with a byte store per visited cell into a plane that
//                         was zeroed.  The byte is a function of the cell alone, so all rays that visit a cell store the same.
//   k_grid_explore_score  one lane per record: label and representative from the frontier table, GAIN from the launch before,
//                         REACH read from the reach field, the record and the score.
//   k_grid_explore_best   one workgroup of 1024 lanes: the ordered arg-min of (score, index) and the count of feasible records.
//   k_grid_view_overlay   one lane per cell: the VIEW plane drawn over the image of svh_grid_render_frontiers.
// Three launches per ranking whatever the scene, beside those of the frontiers and the reach field.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev_common.h"
#include "grid_explore_core.h"
#include "grid_internal.h"

namespace svh {
namespace grid {
namespace {

constexpr int32_t VIEW_WORDS = ((2 * EXPLORE_MAX_R + 1) * (2 * EXPLORE_MAX_R + 1) + 31) / 32;   // 2065

// `cells` holds the viewpoint i at cells[i * stride], cells[i * stride + 1]: pairs (stride 2), or the representatives of a
// frontier table (stride FRONT_REC from its FR_REP_GA)
__global__ __launch_bounds__(VIEW_BLOCK) void k_grid_view_gain(ExploreJob j, const int32_t* __restrict__ cells, int32_t stride, int64_t n,
                                                               int32_t* __restrict__ out) {
    __shared__ uint32_t bits[VIEW_WORDS];
    __shared__ int s_wave[VIEW_BLOCK / 64];
    const int32_t tid = (int32_t)threadIdx.x, R = j.R, side = 2 * R + 1;
    const int32_t words = (side * side + 31) >> 5;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t va = (int64_t)cells[i * stride] - j.oa, vb = (int64_t)cells[i * stride + 1] - j.ob;
        if (va < 0 || va >= j.nx || vb < 0 || vb >= j.nz) {   // every lane of the workgroup alike
            if (tid == 0) out[i] = -1;
            continue;
        }
        for (int32_t w = tid; w < words; w += (int32_t)VIEW_BLOCK) bits[w] = 0u;
        __syncthreads();
        for (int32_t r = tid; r < 8 * R; r += (int32_t)VIEW_BLOCK)
            view_ray(R, j.nx, j.nz, j.state, (int32_t)va, (int32_t)vb, r, [&](int32_t sx, int32_t sz, uint8_t s) {
                if (!unexplored_state(j.frp, s)) return;
                const int32_t bit = (sz + R) * side + (sx + R);   // |sx|, |sz| <= R: inside the bitmap
                atomicOr(&bits[bit >> 5], 1u << (bit & 31));
            });
        __syncthreads();
        int count = 0;
        for (int32_t w = tid; w < words; w += (int32_t)VIEW_BLOCK) count += __popc(bits[w]);
        int total;
        block_exclusive_scan<(int)VIEW_BLOCK>(count, s_wave, &total);   // its second barrier frees the bitmap for the next viewpoint
        if (tid == 0) out[i] = total;
    }
}

__global__ __launch_bounds__(VIEW_BLOCK) void k_grid_view_mask(ExploreJob j, int32_t va, int32_t vb, uint8_t* __restrict__ view) {
    for (int32_t r = (int32_t)threadIdx.x; r < 8 * j.R; r += (int32_t)VIEW_BLOCK)
        view_ray(j.R, j.nx, j.nz, j.state, va, vb, r, [&](int32_t sx, int32_t sz, uint8_t s) {
            view[(size_t)(vb + sz) * (size_t)j.nx + (size_t)(va + sx)] = view_value(j.frp, s);
        });
}

__global__ __launch_bounds__(VIEW_BLOCK) void k_grid_explore_score(ExploreJob j) {
    const int32_t k = (int32_t)(blockIdx.x * VIEW_BLOCK + threadIdx.x);
    if (k >= j.n) return;
    const int32_t* f = j.front_recs + (size_t)k * FRONT_REC;
    const int32_t ga = f[FR_REP_GA], gb = f[FR_REP_GB], gain = j.gain[k];
    const int32_t reach = j.pot[(size_t)(gb - j.ob) * (size_t)j.nx + (size_t)(ga - j.oa)];   // a representative is a window cell
    int32_t* rec = j.recs + (size_t)k * EXPLORE_REC;
    rec[ER_LABEL] = f[FR_LABEL], rec[ER_REP_GA] = ga, rec[ER_REP_GB] = gb, rec[ER_GAIN] = gain, rec[ER_REACH] = reach;
    j.scores[k] = explore_score(j.exp, gain, reach);
}

// out[0] the best, out[1] the feasible records
__global__ __launch_bounds__(EXPLORE_BEST_BLOCK) void k_grid_explore_best(const long long* __restrict__ scores, int32_t n, int32_t* out) {
    __shared__ long long ss[EXPLORE_BEST_BLOCK];
    __shared__ int32_t si[EXPLORE_BEST_BLOCK], sc[EXPLORE_BEST_BLOCK];
    const int32_t tid = (int32_t)threadIdx.x;
    long long s = EXPLORE_INFEASIBLE;
    int32_t at = 0x7FFFFFFF, feasible = 0;
    for (int32_t k = tid; k < n; k += (int32_t)EXPLORE_BEST_BLOCK) {   // ascending k: the first of equal scores stays
        const long long v = scores[k];
        feasible += v != EXPLORE_INFEASIBLE ? 1 : 0;
        if (v < s) s = v, at = k;
    }
    ss[tid] = s, si[tid] = at, sc[tid] = feasible;
    __syncthreads();
    for (int32_t half = (int32_t)EXPLORE_BEST_BLOCK / 2; half > 0; half >>= 1) {
        if (tid < half) {
            const long long v = ss[tid + half];
            const int32_t i = si[tid + half];
            if (v < ss[tid] || (v == ss[tid] && i < si[tid])) ss[tid] = v, si[tid] = i;
            sc[tid] += sc[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) out[0] = ss[0] == EXPLORE_INFEASIBLE ? -1 : si[0], out[1] = sc[0];
}

__global__ __launch_bounds__(VIEW_BLOCK) void k_grid_view_overlay(int32_t nx, int32_t nz, const uint8_t* __restrict__ view, int32_t va, int32_t vb,
                                                                  uint8_t* rgb) {
    const uint32_t i = blockIdx.x * VIEW_BLOCK + threadIdx.x;
    if (i >= (uint32_t)nx * (uint32_t)nz) return;
    const int32_t b = (int32_t)(i / (uint32_t)nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)nx);
    const size_t o = 3 * ((size_t)(nz - 1 - b) * (size_t)nx + (size_t)a);
    uint8_t px[3] = {rgb[o], rgb[o + 1], rgb[o + 2]};
    if (!colour_view(view[i], a == va && b == vb, px)) return;
    rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
}

}  // namespace

int32_t launch_view_gain(hipStream_t s, const ExploreJob& j, const int32_t* cells, int32_t stride, int64_t n, int32_t* out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_grid_view_gain, dim3((unsigned)std::min<int64_t>(n, VIEW_MAX_BLOCKS)), dim3(VIEW_BLOCK), 0, s, j, cells, stride, n, out);
    return 1;
}

void launch_view_mask(hipStream_t s, const ExploreJob& j, int32_t va, int32_t vb, uint8_t* view) {
    hipLaunchKernelGGL(k_grid_view_mask, dim3(1), dim3(VIEW_BLOCK), 0, s, j, va, vb, view);
}

int32_t launch_explore_rank(hipStream_t s, const ExploreJob& j) {
    int32_t gains = 0;
    if (j.n > 0) {   // no kept component: there may be no table at all
        gains = launch_view_gain(s, j, j.front_recs + FR_REP_GA, FRONT_REC, j.n, j.gain);
        hipLaunchKernelGGL(k_grid_explore_score, dim3(((unsigned)j.n + VIEW_BLOCK - 1) / VIEW_BLOCK), dim3(VIEW_BLOCK), 0, s, j);
    }
    hipLaunchKernelGGL(k_grid_explore_best, dim3(1), dim3(EXPLORE_BEST_BLOCK), 0, s, (const long long*)j.scores, j.n, j.out);
    return gains;
}

void launch_view_overlay(hipStream_t s, int32_t nx, int32_t nz, const uint8_t* view, int32_t va, int32_t vb, uint8_t* rgb) {
    const unsigned cells = (unsigned)nx * (unsigned)nz;
    hipLaunchKernelGGL(k_grid_view_overlay, dim3((cells + VIEW_BLOCK - 1) / VIEW_BLOCK), dim3(VIEW_BLOCK), 0, s, nx, nz, view, va, vb, rgb);
}

}  // namespace grid
}  // namespace svh
