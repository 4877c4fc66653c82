// The rollouts of the ground grid on the device (svh_grid_footprint_cost, svh_grid_roll_score, svh_grid_render_roll;
// include/svh_grid.h, "ROLLOUT").  The arithmetic is csrc/grid_roll_core.h: integer work on the finished COST and POT planes in
// logical order; F is a maximum, sumF an integer sum, the cut a first index and the best the minimum of unique keys, so nothing here
// depends on the launch shape or the scheduling.
//
//   k_grid_roll_score      one workgroup of 256 lanes per candidate.  The lanes form GROUPS of `group` lanes, a power of two from 1
//                          to 64 chosen on the host as the smallest that holds the longest footprint list (64 beyond that): a group
//                          takes one pose at a time, its lanes stride over the list of the pose's heading.  A list is ascending by
//                          (db, da), so neighbouring lanes read neighbouring bytes of one COST row.  F_t is reduced by xor shuffles
//                          within the group and kept in LDS (int16, 2 KiB at T = 1024).  The cut is a first-index reduction: a group
//                          that finds its pose cut lowers `cut_at` in LDS by an atomic minimum, and a group skips a pose that lies
//                          beyond the value it reads there -- such a pose lies beyond the final cut too, whose F is never used, so
//                          what is skipped depends on the scheduling and no output byte does.  After one barrier maxF and sumF go
//                          over t < L by shuffles and LDS, lane 0 reads POT once and writes the record and the score.
//   k_grid_roll_best       one workgroup of 1024 lanes: the ordered arg-min of (score, index) over the K scores, one launch.
//   k_grid_footprint_cost  free poses: a group of lanes per pose as above, the groups stride over the poses.
//   k_grid_roll_overlay    one lane per (candidate, pose): the reference cells of the poses before the cut, drawn over the image of
//                          k_grid_render_cost; a second launch draws the best candidate over them.
// Two launches per svh_grid_roll_score whatever the scene; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grid_internal.h"
#include "grid_roll_core.h"

namespace svh {
namespace grid {
namespace {

// the maximum over the lanes of a group of `width` lanes (a power of two, at most 64), in all of them
__device__ __forceinline__ int32_t group_max(int32_t v, int32_t width) {
    for (int32_t off = width >> 1; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// the maximum of the footprint cells of the list [s, s + n) round the window position (a, b), over the lanes of a group
__device__ __forceinline__ int32_t group_worst(const RollJob& j, int64_t a, int64_t b, int32_t s, int32_t n, int32_t lane) {
    int32_t worst = 0;
    for (int32_t i = lane; i < n; i += j.group) {
        const int2 o = j.offs[s + i];
        const int32_t v = roll_cell(j.cost, j.nx, j.nz, a + o.x, b + o.y, j.rp.unknown_cost);
        worst = v > worst ? v : worst;
    }
    return group_max(worst, j.group);
}

__global__ __launch_bounds__(ROLL_BLOCK) void k_grid_roll_score(RollJob j) {
    __shared__ int16_t fs[ROLL_MAX_T];
    __shared__ int32_t cut_at;
    __shared__ int32_t red_max[ROLL_BLOCK / 64], red_sum[ROLL_BLOCK / 64];
    const int32_t c = (int32_t)blockIdx.x, tid = (int32_t)threadIdx.x;
    const int32_t n_c = j.lens[c];
    const int32_t* cand = j.cands + (size_t)c * (size_t)j.T * 3;
    if (tid == 0) cut_at = n_c;
    __syncthreads();
    const int32_t per_block = (int32_t)ROLL_BLOCK / j.group, grp = tid / j.group, lane = tid % j.group;
    for (int32_t t = grp; t < n_c; t += per_block) {
        // one lane reads for its group: the lanes of a group leave the loop together
        int32_t seen = lane == 0 ? atomicAdd(&cut_at, 0) : 0;
        seen = __shfl(seen, 0, j.group);
        if (t > seen) break;
        const int32_t k = cand[3 * t + 2];
        const int64_t a = (int64_t)j.ga0 + cand[3 * t] - j.oa, b = (int64_t)j.gb0 + cand[3 * t + 1] - j.ob;
        const int32_t s = j.start[k];
        const int32_t f = roll_f(group_worst(j, a, b, s, j.start[k + 1] - s, lane));
        if (lane == 0) {
            fs[t] = (int16_t)f;
            if (roll_cut(f, j.rp.stop_cost)) atomicMin(&cut_at, t);
        }
    }
    __syncthreads();
    const int32_t L = cut_at;
    int32_t mx = -1, sum = 0;
    for (int32_t t = tid; t < L; t += (int32_t)ROLL_BLOCK) {
        const int32_t f = fs[t];
        mx = f > mx ? f : mx, sum += f;
    }
    for (int32_t off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx, sum += __shfl_xor(sum, off);
    }
    if ((tid & 63) == 0) red_max[tid >> 6] = mx, red_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid != 0) return;
    for (int32_t w = 1; w < (int32_t)ROLL_BLOCK / 64; w++) mx = red_max[w] > mx ? red_max[w] : mx, sum += red_sum[w];
    int32_t rec[ROLL_REC] = {L, n_c == 0 ? (int32_t)ROLL_EMPTY : (L < n_c ? roll_cut(fs[L], j.rp.stop_cost) : (int32_t)ROLL_COMPLETE), mx, sum,
                             PLAN_FAR};
    if (L > 0 && j.rp.w_pot != 0) {
        const int64_t a = (int64_t)j.ga0 + cand[3 * (L - 1)] - j.oa, b = (int64_t)j.gb0 + cand[3 * (L - 1) + 1] - j.ob;
        rec[RR_POT_END] = j.pot[(size_t)b * (size_t)j.nx + (size_t)a];   // inside: (0, 0) is in every list and F was not -1
    }
    for (int32_t k = 0; k < ROLL_REC; k++) j.recs[(size_t)c * ROLL_REC + k] = rec[k];
    j.scores[c] = roll_score(j.rp, n_c, rec);
}

__global__ __launch_bounds__(ROLL_BEST_BLOCK) void k_grid_roll_best(const long long* __restrict__ scores, int32_t K, int32_t* best) {
    __shared__ long long ss[ROLL_BEST_BLOCK];
    __shared__ int32_t si[ROLL_BEST_BLOCK];
    const int32_t tid = (int32_t)threadIdx.x;
    long long s = ROLL_INFEASIBLE;
    int32_t at = 0x7FFFFFFF;
    for (int32_t c = tid; c < K; c += (int32_t)ROLL_BEST_BLOCK) {   // ascending c: the first of equal scores stays
        const long long v = scores[c];
        if (v < s) s = v, at = c;
    }
    ss[tid] = s, si[tid] = at;
    __syncthreads();
    for (int32_t half = (int32_t)ROLL_BEST_BLOCK / 2; half > 0; half >>= 1) {
        if (tid < half) {
            const long long v = ss[tid + half];
            const int32_t i = si[tid + half];
            if (v < ss[tid] || (v == ss[tid] && i < si[tid])) ss[tid] = v, si[tid] = i;
        }
        __syncthreads();
    }
    if (tid == 0) *best = ss[0] == ROLL_INFEASIBLE ? -1 : si[0];
}

__global__ __launch_bounds__(ROLL_BLOCK) void k_grid_footprint_cost(RollJob j, const int32_t* __restrict__ poses, int64_t n, int32_t* out) {
    const int32_t tid = (int32_t)threadIdx.x, lane = tid % j.group;
    const int64_t per_block = (int64_t)ROLL_BLOCK / j.group;
    for (int64_t i = (int64_t)blockIdx.x * per_block + tid / j.group; i < n; i += (int64_t)gridDim.x * per_block) {
        const int32_t k = poses[3 * i + 2];
        int32_t f = -1;
        if (k >= 0 && k < 8 * j.rp.m) {   // the same for every lane of the group
            const int32_t s = j.start[k];
            f = roll_f(group_worst(j, (int64_t)poses[3 * i] - j.oa, (int64_t)poses[3 * i + 1] - j.ob, s, j.start[k + 1] - s, lane));
        }
        if (lane == 0) out[i] = f;
    }
}

// `only` >= 0: that candidate alone, in the colour of the best
__global__ __launch_bounds__(ROLL_BLOCK) void k_grid_roll_overlay(RollJob j, int32_t only, uint8_t* rgb) {
    const int64_t n = (int64_t)(only >= 0 ? 1 : j.K) * j.T;
    for (int64_t i = (int64_t)blockIdx.x * ROLL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROLL_BLOCK) {
        const int32_t c = only >= 0 ? only : (int32_t)(i / j.T), t = (int32_t)(i % j.T);
        if (t >= j.recs[(size_t)c * ROLL_REC + RR_LEN]) continue;
        const int32_t* pose = j.cands + ((size_t)c * (size_t)j.T + (size_t)t) * 3;
        const int64_t a = (int64_t)j.ga0 + pose[0] - j.oa, b = (int64_t)j.gb0 + pose[1] - j.ob;
        if (a < 0 || a >= j.nx || b < 0 || b >= j.nz) continue;   // the window moved since the scoring
        uint8_t px[3];
        colour_roll(only >= 0, px);
        const size_t o = 3 * ((size_t)(j.nz - 1 - b) * (size_t)j.nx + (size_t)a);
        rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
    }
}

}  // namespace

int32_t roll_group(int64_t longest) {
    int32_t g = 1;
    while (g < 64 && g < longest) g <<= 1;
    return g;
}

void launch_roll_score(hipStream_t s, const RollJob& j) {
    hipLaunchKernelGGL(k_grid_roll_score, dim3((unsigned)j.K), dim3(ROLL_BLOCK), 0, s, j);
    hipLaunchKernelGGL(k_grid_roll_best, dim3(1), dim3(ROLL_BEST_BLOCK), 0, s, (const long long*)j.scores, j.K, j.best);
}

void launch_roll_best(hipStream_t s, const long long* scores, int32_t K, int32_t* best) {
    hipLaunchKernelGGL(k_grid_roll_best, dim3(1), dim3(ROLL_BEST_BLOCK), 0, s, scores, K, best);
}

void launch_footprint_cost(hipStream_t s, const RollJob& j, const int32_t* poses, int64_t n, int32_t* out) {
    if (n <= 0) return;
    const int64_t per_block = (int64_t)ROLL_BLOCK / j.group;
    const int64_t blocks = std::min<int64_t>((n + per_block - 1) / per_block, 8192);
    hipLaunchKernelGGL(k_grid_footprint_cost, dim3((unsigned)blocks), dim3(ROLL_BLOCK), 0, s, j, poses, n, out);
}

void launch_roll_overlay(hipStream_t s, const RollJob& j, int32_t best, uint8_t* rgb) {
    const int64_t n = (int64_t)j.K * j.T;
    const int64_t blocks = std::min<int64_t>((n + ROLL_BLOCK - 1) / ROLL_BLOCK, 4096);
    hipLaunchKernelGGL(k_grid_roll_overlay, dim3((unsigned)blocks), dim3(ROLL_BLOCK), 0, s, j, -1, rgb);
    if (best >= 0)
        hipLaunchKernelGGL(k_grid_roll_overlay, dim3((unsigned)((j.T + (int32_t)ROLL_BLOCK - 1) / (int32_t)ROLL_BLOCK)), dim3(ROLL_BLOCK), 0, s, j, best,
                           rgb);
}

}  // namespace grid
}  // namespace svh
