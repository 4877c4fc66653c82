// PlaneEstimation on the device (stereomapper/planeestimation.cpp): everything that is O(lattice) or
// O(hypotheses x list).  All kernels take blockIdx.z (k_plane_grid, k_plane_select: blockIdx.x) as the map of a batch.
//
// k_plane_grid    sparseDisparityGrid: one workgroup per map walks the lattice in the reference's u-major order,
//                 1024 cells at a time, and keeps (u, v, d) where d >= 1 at the position a ballot / popcount prefix
//                 gives it, so the list has the reference's order and indices.
// k_plane_fit     one lane per hypothesis: leastSquarePlane over its one to three drawn points (float products summed
//                 in fp64, the 3x3 Gauss-Jordan of Matrix::solve), the zero plane after a failed solve.
// k_plane_vote    every (hypothesis, point) pair once: a workgroup holds 256 hypotheses, one per lane with its plane
//                 in registers, and a tile of 1024 points staged once in LDS as doubles; all lanes read the same point
//                 (an LDS broadcast), count in a register and add the tile's count to the hypothesis' vote with one
//                 integer atomic (integer sums do not depend on the order of the tiles).
// k_plane_select  one workgroup per map: the first maximum of the votes (ties go to the lower index, a hypothesis
//                 with no inlier never wins: the reference replaces the best only with strictly more), then the
//                 winner's inlier indices compacted in list order.
// The arithmetic is plane_core.h's, no FMA contraction (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_internal.h"

namespace svh {

namespace {

constexpr int GRID_T = 1024;     // lanes of k_plane_grid / k_plane_select
constexpr int VOTE_H = 256;      // hypotheses (lanes) per workgroup of k_plane_vote
constexpr int VOTE_TILE = 1024;  // points per workgroup of k_plane_vote: 3 x 8 B x 1024 = 24 KB LDS

// position of a kept element among the kept elements of this round of GRID_T lanes, and their number
__device__ __forceinline__ int32_t block_rank(bool keep, int32_t* s_wave, int32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int32_t before = 0, all = 0;
    for (int k = 0; k < GRID_T / 64; k++) {
        const int32_t c = s_wave[k];
        before += k < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    *total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(GRID_T) void k_plane_grid(PlaneDev P, plane::Lattice L, int32_t step, int32_t row0) {
    __shared__ int32_t s_wave[GRID_T / 64];
    const int32_t map = blockIdx.x;
    const float* __restrict__ D = P.maps[map];
    float* lu = P.lu + (size_t)map * P.cap;
    float* lv = P.lv + (size_t)map * P.cap;
    float* ld = P.ld + (size_t)map * P.cap;
    const int32_t cells = L.nu * L.nv;
    int32_t running = 0;
    for (int32_t b = 0; b < cells; b += GRID_T) {
        const int32_t t = b + (int32_t)threadIdx.x;
        int32_t u = 0, v = 0;
        float d = 0.f;
        if (t < cells) {
            u = plane::cell_u(L, t);
            v = plane::cell_v(L, t);
            d = D[(size_t)(v - row0) * step + u];
        }
        const bool keep = t < cells && plane::cell_kept(d);
        int32_t total;
        const int32_t at = running + block_rank(keep, s_wave, &total);
        if (keep && at < P.cap) {
            lu[at] = (float)u;
            lv[at] = (float)v;
            ld[at] = d;
        }
        running += total;
    }
    if (threadIdx.x == 0) P.n_list[map] = running < P.cap ? running : P.cap;
}

__global__ __launch_bounds__(256) void k_plane_fit(PlaneDev P) {
    const int32_t map = blockIdx.z;
    const int32_t h = blockIdx.x * 256 + (int32_t)threadIdx.x;
    if (h >= P.S) return;
    const int32_t n = P.n_list[map];
    const int32_t* s = P.samples + ((size_t)map * P.S + h) * 4;
    int32_t cnt = s[0];
    int32_t ind[3] = {s[1], s[2], s[3]};
    cnt = cnt < 0 ? 0 : (cnt > 3 ? 3 : cnt);
    for (int k = 0; k < 3; k++)   // (drawn on the host from this very list; clamped all the same)
        if (k < cnt && (ind[k] < 0 || ind[k] >= n)) cnt = 0;
    double abc[3];
    plane::fit_indexed(P.lu + (size_t)map * P.cap, P.lv + (size_t)map * P.cap, P.ld + (size_t)map * P.cap, ind, cnt,
                       abc);
    double* out = P.planes + ((size_t)map * P.S + h) * 3;
    out[0] = abc[0];
    out[1] = abc[1];
    out[2] = abc[2];
}

__global__ __launch_bounds__(VOTE_H) void k_plane_vote(PlaneDev P, double thr) {
    __shared__ double s_u[VOTE_TILE], s_v[VOTE_TILE], s_d[VOTE_TILE];
    const int32_t map = blockIdx.z;
    const int32_t n = P.n_list[map];
    const int32_t p0 = blockIdx.y * VOTE_TILE;
    if (p0 >= n) return;   // (uniform over the workgroup)
    const int32_t np = n - p0 < VOTE_TILE ? n - p0 : VOTE_TILE;
    const size_t base = (size_t)map * P.cap + p0;
    for (int32_t i = threadIdx.x; i < np; i += VOTE_H) {
        s_u[i] = (double)P.lu[base + i];
        s_v[i] = (double)P.lv[base + i];
        s_d[i] = (double)P.ld[base + i];
    }
    __syncthreads();
    const int32_t h = blockIdx.x * VOTE_H + (int32_t)threadIdx.x;
    if (h >= P.S) return;
    const double* pl = P.planes + ((size_t)map * P.S + h) * 3;
    const double a = pl[0], b = pl[1], c = pl[2];
    int32_t count = 0;
    for (int32_t i = 0; i < np; i++) {
        // plane::is_inlier on the staged doubles: ((a u + b v) + c) - d, rounded to float
        const double au = a * s_u[i];
        const double bv = b * s_v[i];
        const float result = (float)(((au + bv) + c) - s_d[i]);
        count += (double)fabsf(result) < thr ? 1 : 0;
    }
    if (count) atomicAdd(P.counts + (size_t)map * P.S + h, count);
}

__global__ __launch_bounds__(GRID_T) void k_plane_select(PlaneDev P, double thr) {
    __shared__ int32_t s_wave[GRID_T / 64];
    __shared__ int32_t s_cnt[GRID_T], s_idx[GRID_T];
    const int32_t map = blockIdx.x;
    const int32_t* counts = P.counts + (size_t)map * P.S;
    int32_t bc = 0, bi = -1;
    for (int32_t h = threadIdx.x; h < P.S; h += GRID_T) {   // ascending: strictly more keeps the first maximum
        const int32_t c = counts[h];
        if (c > bc) {
            bc = c;
            bi = h;
        }
    }
    s_cnt[threadIdx.x] = bc;
    s_idx[threadIdx.x] = bi;
    __syncthreads();
    for (int w = GRID_T / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const int32_t c = s_cnt[threadIdx.x + w], i = s_idx[threadIdx.x + w];
            const int32_t mc = s_cnt[threadIdx.x], mi = s_idx[threadIdx.x];
            if (i >= 0 && (c > mc || (c == mc && (mi < 0 || i < mi)))) {
                s_cnt[threadIdx.x] = c;
                s_idx[threadIdx.x] = i;
            }
        }
        __syncthreads();
    }
    const int32_t best = s_idx[0];
    int32_t running = 0;
    if (best >= 0) {
        const int32_t n = P.n_list[map];
        const double* pl = P.planes + ((size_t)map * P.S + best) * 3;
        const double a = pl[0], b = pl[1], c = pl[2];
        const size_t base = (size_t)map * P.cap;
        int32_t* inl = P.inl + base;
        for (int32_t p0 = 0; p0 < n; p0 += GRID_T) {
            const int32_t i = p0 + (int32_t)threadIdx.x;
            const bool keep = i < n && plane::is_inlier(a, b, c, P.lu[base + i], P.lv[base + i], P.ld[base + i], thr);
            int32_t total;
            const int32_t at = running + block_rank(keep, s_wave, &total);
            if (keep && at < P.cap) inl[at] = i;
            running += total;
        }
    }
    if (threadIdx.x == 0) {
        P.sel[2 * map + 0] = best;
        P.sel[2 * map + 1] = running;
    }
}

}  // namespace

void planelaunch_grid(void* stream, const PlaneDev& P, int32_t nmaps, const plane::Lattice& L, int32_t step,
                      int32_t row0) {
    k_plane_grid<<<nmaps, GRID_T, 0, (hipStream_t)stream>>>(P, L, step, row0);
}

void planelaunch_vote(void* stream, const PlaneDev& P, int32_t nmaps, int32_t max_n, double d_threshold) {
    hipStream_t st = (hipStream_t)stream;
    const int32_t hb = (P.S + VOTE_H - 1) / VOTE_H;
    k_plane_fit<<<dim3(hb, 1, nmaps), 256, 0, st>>>(P);
    if (max_n > 0) k_plane_vote<<<dim3(hb, (max_n + VOTE_TILE - 1) / VOTE_TILE, nmaps), VOTE_H, 0, st>>>(P, d_threshold);
    k_plane_select<<<nmaps, GRID_T, 0, st>>>(P, d_threshold);
}

}  // namespace svh
