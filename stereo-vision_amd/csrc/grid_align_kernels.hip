// The alignment layer of the ground grid on the device (svh_grid_align_points, svh_grid_align_view_lists, svh_grid_get_align_field,
// svh_grid_render_align; include/svh_grid.h, "ALIGN").  The arithmetic is csrc/grid_align_core.h: after the fp32 placement of a
// point everything is integer work.  The scan is a set, a score an integer sum over it and the best the minimum of a unique key, so
// nothing here depends on the launch shape or the scheduling.  Every loop is bounded by a value the host passes; no kernel waits
// for another.
//
//   k_grid_align_cols     g, the capped distance along ib to the nearest obstacle cell of the column, as uint16: the sweep of
//                         k_grid_dist_cols (grid_trav_kernels.hip) -- one lane per column and chunk of 32 rows, started `reach` rows
//                         early from the cap -- with the obstacle class of STATE as its mask, read in place: the layer has no
//                         mask launch.
//   k_grid_align_rows     one workgroup per 256 cells of a row: the tile of g and a halo of `reach` (at most 32) in LDS, row_dist2,
//                         the byte F.
//   k_grid_align_mark     one lane per point (striding beyond 2048 * 256): the point's sub, the box test, one atomicOr into the
//                         bitmap of the box, (8 Rg + 1)^2 bits in global memory; the kept points are counted by one atomicAdd per
//                         wave from its ballot.  A second form takes subs instead of points (the test entry).
//   k_grid_align_count    one lane per word of the bitmap: the set bits of 256 words summed by block_exclusive_scan.
//   k_grid_align_scatter  the same blocks: a block sums the counts of the blocks before it (at most 513), scans its own words and
//                         writes its subs in ascending bit order, which is ascending (ub, ua); the last block stores n_scan.
//   k_grid_align_score    the hot path.  A workgroup has one rotation, 256 translations (one per lane) and a slice of the scan.
//                         It places 1024 subs of its slice at a time under its rotation into LDS; every lane then walks them --
//                         all lanes read the same LDS word, a broadcast -- samples F at its own translation from global memory
//                         (the four bytes of neighbouring lanes lie in the same or neighbouring cells: cache hits) and sums in a
//                         register.  One integer atomicAdd per lane and slice into the volume: commutative, so still exact.
//                         With fewer than min_scan subs every workgroup leaves at once.
//   k_grid_align_best     one workgroup of 1024 lanes: the minimum of align_key over the volume, the count of its ties, the record.
//   k_grid_align_overlay  one lane per scan sub: its cell coloured in the image of svh_grid_render_local.
// An alignment is the field's two launches (when it is not cached), mark, count, scatter, score, best: seven, and one wait.
//
// THREE FORMS OF THE SCORE KERNEL were built and measured alternating in one process (tools/gpu_grid_align.py,
// profiles/grid_align_times.jsonl, DESIGN.md "Ground grid", "Alignment"); svh_test_grid_align_form selects one, the tests run all:
//   chunk  k_grid_align_score above, the one every entry uses;
//   plain  k_grid_align_score_plain: one lane per candidate walks the whole scan, the scan and F from global memory, one store;
//   tiled  k_grid_align_score_tiled: F within reach of every placed sub staged in LDS (up to 152 KiB, zero outside the window, so
//          no bounds check per sample), a lane owns one tb and the up to 17 translations ta of one phase, which differ by whole
//          cells and share their weights: 2 (M + 1) LDS bytes for M samples.  Where the cells do not fit, the chunk form runs.
// Whole svh_grid_align_points calls on device-resident points with the field cached, 256 x 256 cells, median ms, chunk / plain /
// tiled: at (K, W) = (8, 8) 0.50 / 0.54 / 0.57 for 10^3 subs, 0.52 / 4.84 / 1.52 for 10^4, 1.65 / 47.9 / 11.8 for 10^5; at (32, 32)
// 0.72 / 0.80 / 1.26, 3.53 / 6.22 / 7.33 and 30.0 / 58.8 / 75.6.  THE CHUNK FORM WINS EVERY CASE AND IS KEPT.  The plain form has
// too few lanes at (8, 8) and places every sub once per candidate; the tiled form holds one workgroup per CU with its 94 KiB of LDS
// at Rg = 128 -- four waves to hide the latency of byte reads from LDS -- and loses although it issues half the loads.
// The field in two launches against the cost layer's three (a mask launch first; form + 4): the paired difference of whole stale
// calls, three minus two, is +0.006 to +0.11 ms at (8, 8) and -0.49 to +0.04 ms at (32, 32), within the spread of those calls at
// 30 ms: no difference that the measurement resolves, and two launches are kept as the smaller form.
// Marks of equal words are not combined inside a wave before the atomic; that was not measured.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev_common.h"
#include "grid_align_core.h"
#include "grid_internal.h"

namespace svh {
namespace grid {
namespace {

constexpr uint32_t ALIGN_ROWS_TILE = ALIGN_BLOCK + 2 * (uint32_t)ALIGN_MAX_REACH;

// the mask launch of the three-launch form of the field (svh_test_grid_align_form): one lane per cell, the mask into F's own plane
__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_mask(uint32_t cells, const uint8_t* __restrict__ state, uint8_t* __restrict__ mask) {
    const uint32_t i = blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    if (i < cells) mask[i] = (state[i] & 3) == C_OBSTACLE ? 1 : 0;
}

// MASK: `state` is the plane of k_grid_align_mask; else the STATE plane itself
template <bool MASK>
__global__ __launch_bounds__(COLS_BLOCK) void k_grid_align_cols(int32_t reach, int32_t nx, int32_t nz, const uint8_t* __restrict__ state,
                                                                uint16_t* __restrict__ g) {
    const int32_t ia = (int32_t)(blockIdx.x * COLS_BLOCK + threadIdx.x);
    if (ia >= nx) return;
    const int32_t b0 = (int32_t)blockIdx.y * COLS_CHUNK;            // the launch has ceil(nz / COLS_CHUNK) chunks: b0 < nz
    const int32_t b1 = nz - b0 < COLS_CHUNK ? nz : b0 + COLS_CHUNK;
    const int32_t first = b0 - reach < 0 ? 0 : b0 - reach, last = nz - b1 < reach ? nz - 1 : b1 - 1 + reach;
    int32_t d = reach + 1;
    for (int32_t ib = first; ib < b1; ib++) {
        const size_t i = (size_t)ib * (size_t)nx + (size_t)ia;
        d = col_step(d, MASK ? state[i] != 0 : (state[i] & 3) == C_OBSTACLE, reach);
        if (ib >= b0) g[i] = (uint16_t)d;
    }
    d = reach + 1;
    for (int32_t ib = last; ib >= b0; ib--) {
        const size_t i = (size_t)ib * (size_t)nx + (size_t)ia;
        d = col_step(d, MASK ? state[i] != 0 : (state[i] & 3) == C_OBSTACLE, reach);
        if (ib < b1) {
            const int32_t f = (int32_t)g[i];
            g[i] = (uint16_t)(d < f ? d : f);
        }
    }
}

__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_rows(int32_t reach, int32_t nx, const uint16_t* __restrict__ g,
                                                                 uint8_t* __restrict__ field) {
    __shared__ uint16_t tile[ALIGN_ROWS_TILE];
    const int32_t a0 = (int32_t)(blockIdx.x * ALIGN_BLOCK), base = a0 - reach;
    const size_t row = (size_t)blockIdx.y * (size_t)nx;
    const int32_t width = (int32_t)ALIGN_BLOCK + 2 * reach;        // <= ALIGN_ROWS_TILE: reach <= ALIGN_MAX_REACH
    for (int32_t t = (int32_t)threadIdx.x; t < width; t += (int32_t)ALIGN_BLOCK) {
        const int32_t c = base + t;
        tile[t] = (c >= 0 && c < nx) ? g[row + (size_t)c] : (uint16_t)(reach + 1);
    }
    __syncthreads();
    const int32_t ia = a0 + (int32_t)threadIdx.x;
    if (ia >= nx) return;
    const int32_t lo = ia - reach < 0 ? 0 : ia - reach, hi = ia + reach > nx - 1 ? nx - 1 : ia + reach;
    const int32_t d2 = row_dist2(tile, base, ia, lo, hi, reach);   // tile[c - base], 0 <= lo - base, hi - base < width
    field[row + (size_t)ia] = align_field(d2 == DIST2_FAR ? reach * reach + 1 : d2, reach * reach);
}

// SUBS: `src` holds pairs (ua, ub) that the host has checked to lie within +-2^22; else points (x, y, z, val)
template <bool SUBS>
__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_mark(AlignJob j, const void* __restrict__ src, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * ALIGN_BLOCK;
    const int64_t rounds = (n + stride - 1) / stride;              // every lane of a wave takes the same number of turns
    int64_t i = (int64_t)blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    for (int64_t r = 0; r < rounds; r++, i += stride) {
        int32_t ua = 0, ub = 0;
        bool kept = false;
        if (i < n) {
            if (SUBS) {
                const int2 s = ((const int2*)src)[i];
                ua = s.x, ub = s.y, kept = true;
            } else {
                const float4 p = ((const float4*)src)[i];
                kept = align_scan_point(j.prm, p.x, p.y, p.z, &ua, &ub);
            }
            kept = kept && align_kept(j.alp.Rg, j.Pa, j.Pb, ua, ub);
        }
        if (kept) {
            const uint32_t bit = align_bit(j.alp.Rg, j.Pa, j.Pb, ua, ub);   // kept: below side^2, inside the bitmap
            atomicOr(&j.bitmap[bit >> 5], 1u << (bit & 31));
        }
        const unsigned long long vote = __ballot(kept);
        if ((threadIdx.x & 63) == 0 && vote) atomicAdd(&j.ctl[AC_POINTS], (uint32_t)__popcll(vote));
    }
}

__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_count(const uint32_t* __restrict__ bitmap, uint32_t words, uint32_t* __restrict__ blockcnt) {
    __shared__ int s_wave[ALIGN_BLOCK / 64];
    const uint32_t w = blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    int total;
    block_exclusive_scan<(int)ALIGN_BLOCK>(w < words ? __popc(bitmap[w]) : 0, s_wave, &total);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_scatter(AlignJob j, uint32_t words) {
    __shared__ int s_wave[ALIGN_BLOCK / 64];
    int before = 0, total, front;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += ALIGN_BLOCK) before += (int)j.blockcnt[b];   // at most 2049^2 in all
    block_exclusive_scan<(int)ALIGN_BLOCK>(before, s_wave, &front);
    const uint32_t w = blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    uint32_t word = w < words ? j.bitmap[w] : 0u;
    int64_t at = (int64_t)front + block_exclusive_scan<(int)ALIGN_BLOCK>(__popc(word), s_wave, &total);
    const uint32_t side = (uint32_t)align_side(j.alp.Rg);
    const int32_t lim = ALIGN_SUB * j.alp.Rg;
    while (word) {
        const uint32_t bit = w * 32u + (uint32_t)__ffs((int)word) - 1u;
        word &= word - 1u;
        const uint32_t rb = bit / side, ra = bit - rb * side;
        if (at < j.scan_room) j.scan[2 * at] = (int32_t)ra - lim + j.Pa, j.scan[2 * at + 1] = (int32_t)rb - lim + j.Pb;
        at++;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) j.ctl[AC_SCAN] = (uint32_t)(front + total);
}

// the subs of the scan the device holds: never more than the room of the list
__device__ __forceinline__ int32_t scan_size(const AlignJob& j) {
    const int64_t n = (int64_t)j.ctl[AC_SCAN];
    return (int32_t)(n < j.scan_room ? n : j.scan_room);
}

__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_score(AlignJob j) {
    __shared__ int2 placed[ALIGN_CHUNK];
    const int32_t n_scan = scan_size(j);
    if (n_scan < j.alp.min_scan) return;                            // every lane of every workgroup alike
    const int32_t tid = (int32_t)threadIdx.x, W = j.alp.trans_n, side = 2 * W + 1;
    const int32_t cand = (int32_t)blockIdx.x * (int32_t)ALIGN_BLOCK + tid;
    const bool valid = cand < side * side;
    const int32_t tb = cand / side - W, ta = cand - (cand / side) * side - W;
    const int32_t cq = j.rot[2 * blockIdx.y], sq = j.rot[2 * blockIdx.y + 1];
    int32_t acc = 0;
    for (int32_t c0 = (int32_t)blockIdx.z * ALIGN_CHUNK; c0 < n_scan; c0 += (int32_t)gridDim.z * ALIGN_CHUNK) {
        const int32_t m = n_scan - c0 < ALIGN_CHUNK ? n_scan - c0 : ALIGN_CHUNK;
        __syncthreads();                                            // the chunk before has been read
        for (int32_t i = tid; i < m; i += (int32_t)ALIGN_BLOCK) {
            int32_t qa, qb;
            align_turn(cq, sq, j.scan[2 * (size_t)(c0 + i)] - j.Pa, j.scan[2 * (size_t)(c0 + i) + 1] - j.Pb, &qa, &qb);
            placed[i] = make_int2(j.Pa + qa, j.Pb + qb);
        }
        __syncthreads();
        if (valid)
            for (int32_t i = 0; i < m; i++) {
                const int2 q = placed[i];
                acc += align_sample(j.field, j.prm.nx, j.prm.nz, j.prm.oa, j.prm.ob, q.x + ta, q.y + tb);
            }
    }
    if (valid && acc) atomicAdd(&j.volume[((size_t)blockIdx.y * side + (size_t)(tb + W)) * side + (size_t)(ta + W)], acc);
}

// the plain form: one lane per candidate walks the whole scan; the scan and F come from global memory; one store per candidate
__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_score_plain(AlignJob j) {
    const int32_t n_scan = scan_size(j);
    if (n_scan < j.alp.min_scan) return;
    const int32_t K = j.alp.rot_n, W = j.alp.trans_n, side = 2 * W + 1;
    const int32_t idx = (int32_t)(blockIdx.x * ALIGN_BLOCK + threadIdx.x);
    if (idx >= align_volume_size(K, W)) return;
    const int32_t ki = idx / (side * side), rem = idx - ki * side * side, tb = rem / side - W, ta = rem - (rem / side) * side - W;
    const int32_t cq = j.rot[2 * ki], sq = j.rot[2 * ki + 1];
    int32_t acc = 0;
    for (int32_t i = 0; i < n_scan; i++) {
        int32_t qa, qb;
        align_turn(cq, sq, j.scan[2 * (size_t)i] - j.Pa, j.scan[2 * (size_t)i + 1] - j.Pb, &qa, &qb);
        acc += align_sample(j.field, j.prm.nx, j.prm.nz, j.prm.oa, j.prm.ob, j.Pa + qa + ta, j.Pb + qb + tb);
    }
    j.volume[idx] = acc;
}

// The tiled form.  F within reach of every placed sub -- the window cells a_lo .. a_lo + width - 1 by b_lo .. b_lo + height - 1,
// zero where they lie outside the window -- is staged in LDS behind the chunk of placed subs, so a sample needs no bounds check.
// A lane owns one tb and one phase pa = 0..3 of ta: the translations ta = -W + pa + 4 m, m = 0 .. M - 1, differ by whole cells and
// share their four weights; their samples are a run of M + 1 cells in two rows of F: 2 (M + 1) LDS bytes for M samples.
__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_score_tiled(AlignJob j, int32_t a_lo, int32_t b_lo, int32_t width, int32_t height) {
    extern __shared__ __align__(16) uint8_t lds[];
    int2* placed = (int2*)lds;
    uint8_t* F = lds + ALIGN_CHUNK * sizeof(int2);
    const int32_t n_scan = scan_size(j);
    if (n_scan < j.alp.min_scan) return;                            // every lane of every workgroup alike
    const int32_t tid = (int32_t)threadIdx.x, W = j.alp.trans_n, side = 2 * W + 1;
    const int32_t lane = (int32_t)blockIdx.x * (int32_t)ALIGN_BLOCK + tid, pa = lane & 3, tb = (lane >> 2) - W;
    const int32_t M = (lane < 4 * side && pa <= 2 * W) ? (2 * W - pa) / 4 + 1 : 0;   // at most ALIGN_TILED_RUN
    const int32_t cq = j.rot[2 * blockIdx.y], sq = j.rot[2 * blockIdx.y + 1];
    for (int32_t i = tid; i < width * height; i += (int32_t)ALIGN_BLOCK) {
        const int32_t cb = b_lo + i / width, ca = a_lo + i - (i / width) * width;
        F[i] = (ca >= 0 && ca < j.prm.nx && cb >= 0 && cb < j.prm.nz) ? j.field[(size_t)cb * (size_t)j.prm.nx + (size_t)ca] : (uint8_t)0;
    }
    int32_t acc[ALIGN_TILED_RUN];
#pragma unroll
    for (int32_t m = 0; m < ALIGN_TILED_RUN; m++) acc[m] = 0;
    for (int32_t c0 = (int32_t)blockIdx.z * ALIGN_CHUNK; c0 < n_scan; c0 += (int32_t)gridDim.z * ALIGN_CHUNK) {
        const int32_t n = n_scan - c0 < ALIGN_CHUNK ? n_scan - c0 : ALIGN_CHUNK;
        __syncthreads();                                            // the chunk before has been read; the first time: F is staged
        for (int32_t i = tid; i < n; i += (int32_t)ALIGN_BLOCK) {
            int32_t qa, qb;
            align_turn(cq, sq, j.scan[2 * (size_t)(c0 + i)] - j.Pa, j.scan[2 * (size_t)(c0 + i) + 1] - j.Pb, &qa, &qb);
            placed[i] = make_int2(j.Pa + qa, j.Pb + qb);
        }
        __syncthreads();
        if (M > 0)
            for (int32_t i = 0; i < n; i++) {
                const int2 q = placed[i];
                const int32_t pea = 2 * (q.x - W + pa) - 3 - 8 * j.prm.oa, peb = 2 * (q.y + tb) - 3 - 8 * j.prm.ob;
                const int32_t g0a = pea >> 3, g0b = peb >> 3, fa = pea - 8 * g0a, fb = peb - 8 * g0b;
                const uint8_t* r0 = F + (g0b - b_lo) * width + (g0a - a_lo);   // inside the staged cells: the launch sized them for every placed sub
                const uint8_t* r1 = r0 + width;
                const int32_t w00 = (8 - fa) * (8 - fb), w10 = fa * (8 - fb), w01 = (8 - fa) * fb, w11 = fa * fb;
                int32_t v0 = r0[0], v1 = r1[0];
#pragma unroll
                for (int32_t m = 0; m < ALIGN_TILED_RUN; m++)
                    if (m < M) {
                        const int32_t n0 = r0[m + 1], n1 = r1[m + 1];
                        acc[m] += (w00 * v0 + w10 * n0 + w01 * v1 + w11 * n1 + 32) >> 6;
                        v0 = n0, v1 = n1;
                    }
            }
    }
#pragma unroll
    for (int32_t m = 0; m < ALIGN_TILED_RUN; m++)
        if (m < M && acc[m]) atomicAdd(&j.volume[((size_t)blockIdx.y * side + (size_t)(tb + W)) * side + (size_t)(pa + 4 * m)], acc[m]);
}

__global__ __launch_bounds__(ALIGN_BEST_BLOCK) void k_grid_align_best(AlignJob j) {
    __shared__ unsigned long long sk[ALIGN_BEST_BLOCK];
    __shared__ int32_t sc[ALIGN_BEST_BLOCK];
    const int32_t tid = (int32_t)threadIdx.x, n_scan = scan_size(j);
    if (n_scan < j.alp.min_scan) {
        if (tid == 0) align_record_few(n_scan, j.rec);
        return;
    }
    const int32_t K = j.alp.rot_n, W = j.alp.trans_n, V = align_volume_size(K, W);
    unsigned long long key = ~0ull;
    for (int32_t i = tid; i < V; i += (int32_t)ALIGN_BEST_BLOCK) {
        const unsigned long long k = align_key(j.volume[i], K, W, i);
        key = k < key ? k : key;
    }
    sk[tid] = key;
    __syncthreads();
    for (int32_t half = (int32_t)ALIGN_BEST_BLOCK / 2; half > 0; half >>= 1) {
        if (tid < half && sk[tid + half] < sk[tid]) sk[tid] = sk[tid + half];
        __syncthreads();
    }
    const unsigned long long best = sk[0];
    const int32_t top = 0x3FFFFFFF - (int32_t)(best >> 31);
    int32_t ties = 0;
    for (int32_t i = tid; i < V; i += (int32_t)ALIGN_BEST_BLOCK) ties += j.volume[i] == top ? 1 : 0;
    sc[tid] = ties;
    __syncthreads();
    for (int32_t half = (int32_t)ALIGN_BEST_BLOCK / 2; half > 0; half >>= 1) {
        if (tid < half) sc[tid] += sc[tid + half];
        __syncthreads();
    }
    if (tid == 0) {
        const int32_t side = 2 * W + 1;
        align_record(best, K, W, j.volume[((size_t)K * side + (size_t)W) * side + (size_t)W], n_scan, sc[0], j.rec);
    }
}

// what 0: the scan as it is; 1: placed at rotation (cq, sq) and (ta, tb); 2: the pivot alone (n = 1)
__global__ __launch_bounds__(ALIGN_BLOCK) void k_grid_align_overlay(AlignJob j, int32_t n, int32_t what, int32_t cq, int32_t sq, int32_t ta, int32_t tb,
                                                                    uint8_t* rgb) {
    const int32_t i = (int32_t)(blockIdx.x * ALIGN_BLOCK + threadIdx.x);
    if (i >= n) return;
    int32_t ua = j.Pa, ub = j.Pb;
    if (what != 2) {
        int32_t qa, qb;
        align_turn(cq, sq, j.scan[2 * (size_t)i] - j.Pa, j.scan[2 * (size_t)i + 1] - j.Pb, &qa, &qb);
        ua = j.Pa + qa + ta, ub = j.Pb + qb + tb;
    }
    const int32_t a = (ua >> 2) - j.prm.oa, b = (ub >> 2) - j.prm.ob;
    if (a < 0 || a >= j.prm.nx || b < 0 || b >= j.prm.nz) return;
    colour_align(what, rgb + 3 * ((size_t)(j.prm.nz - 1 - b) * (size_t)j.prm.nx + (size_t)a));
}

}  // namespace

void launch_align_field(hipStream_t s, const AlignJob& j, bool mask) {
    const unsigned nx = (unsigned)j.prm.nx, nz = (unsigned)j.prm.nz;
    const dim3 cols((nx + COLS_BLOCK - 1) / COLS_BLOCK, (nz + (unsigned)COLS_CHUNK - 1) / (unsigned)COLS_CHUNK);
    if (mask) {
        hipLaunchKernelGGL(k_grid_align_mask, dim3((nx * nz + ALIGN_BLOCK - 1) / ALIGN_BLOCK), dim3(ALIGN_BLOCK), 0, s, nx * nz, j.state, j.field);
        hipLaunchKernelGGL(k_grid_align_cols<true>, cols, dim3(COLS_BLOCK), 0, s, j.alp.reach_cells, j.prm.nx, j.prm.nz, (const uint8_t*)j.field, j.g);
    } else {
        hipLaunchKernelGGL(k_grid_align_cols<false>, cols, dim3(COLS_BLOCK), 0, s, j.alp.reach_cells, j.prm.nx, j.prm.nz, j.state, j.g);
    }
    hipLaunchKernelGGL(k_grid_align_rows, dim3((nx + ALIGN_BLOCK - 1) / ALIGN_BLOCK, nz), dim3(ALIGN_BLOCK), 0, s, j.alp.reach_cells, j.prm.nx,
                       (const uint16_t*)j.g, j.field);
}

void launch_align_mark(hipStream_t s, const AlignJob& j, const float4* pts, const int32_t* subs, int64_t n) {
    if (n <= 0) return;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + ALIGN_BLOCK - 1) / ALIGN_BLOCK, ALIGN_MAX_BLOCKS);
    if (subs) hipLaunchKernelGGL(k_grid_align_mark<true>, dim3(blocks), dim3(ALIGN_BLOCK), 0, s, j, (const void*)subs, n);
    else hipLaunchKernelGGL(k_grid_align_mark<false>, dim3(blocks), dim3(ALIGN_BLOCK), 0, s, j, (const void*)pts, n);
}

void launch_align_compact(hipStream_t s, const AlignJob& j) {
    const uint32_t words = align_words(j), blocks = align_count_blocks(j);
    hipLaunchKernelGGL(k_grid_align_count, dim3(blocks), dim3(ALIGN_BLOCK), 0, s, (const uint32_t*)j.bitmap, words, j.blockcnt);
    hipLaunchKernelGGL(k_grid_align_scatter, dim3(blocks), dim3(ALIGN_BLOCK), 0, s, j, words);
}

// the cells the tiled form stages for the job: every cell a sample of any candidate can read; false: they do not fit the LDS
bool align_tiled_cells(const AlignJob& j, int32_t* a_lo, int32_t* b_lo, int32_t* width, int32_t* height) {
    int32_t turn = 0;
    for (int32_t i = 0; i <= 2 * j.alp.rot_n; i++) turn = std::max(turn, std::abs(j.rot[2 * i]) + std::abs(j.rot[2 * i + 1]));
    // |qa|, |qb| of align_turn for |ra|, |rb| <= 4 Rg, and the translation
    const int32_t ext = (int32_t)(((int64_t)turn * ALIGN_SUB * j.alp.Rg + (ALIGN_ROT >> 1)) >> ALIGN_ROT_SHIFT) + 1 + j.alp.trans_n;
    *a_lo = ((2 * (j.Pa - ext) - 3) >> 3) - j.prm.oa, *b_lo = ((2 * (j.Pb - ext) - 3) >> 3) - j.prm.ob;
    *width = ((2 * (j.Pa + ext) - 3) >> 3) - j.prm.oa + 1 - *a_lo + 1, *height = ((2 * (j.Pb + ext) - 3) >> 3) - j.prm.ob + 1 - *b_lo + 1;
    return (int64_t)*width * *height <= (int64_t)ALIGN_TILED_LDS - (int64_t)(ALIGN_CHUNK * sizeof(int2));
}

void launch_align_score(hipStream_t s, const AlignJob& j, int32_t form) {
    const unsigned side = 2u * (unsigned)j.alp.trans_n + 1u, rots = 2u * (unsigned)j.alp.rot_n + 1u;
    const int64_t chunks = (j.scan_room + ALIGN_CHUNK - 1) / ALIGN_CHUNK;
    int32_t a_lo, b_lo, width, height;
    if (form == ALIGN_FORM_PLAIN) {
        hipLaunchKernelGGL(k_grid_align_score_plain, dim3((rots * side * side + ALIGN_BLOCK - 1) / ALIGN_BLOCK), dim3(ALIGN_BLOCK), 0, s, j);
    } else if (form == ALIGN_FORM_TILED && align_tiled_cells(j, &a_lo, &b_lo, &width, &height)) {
        static const hipError_t raised = hipFuncSetAttribute((const void*)k_grid_align_score_tiled, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ALIGN_TILED_LDS);
        (void)raised;
        // a workgroup stages up to 152 KiB once: few slices, so that each walks many chunks
        const unsigned slices = (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, ALIGN_TILED_SLICES));
        hipLaunchKernelGGL(k_grid_align_score_tiled, dim3((4 * side + ALIGN_BLOCK - 1) / ALIGN_BLOCK, rots, slices), dim3(ALIGN_BLOCK),
                           ALIGN_CHUNK * sizeof(int2) + (size_t)width * (size_t)height, s, j, a_lo, b_lo, width, height);
    } else {
        // sized by the room of the list, min(points, bits of the box), which the host knows: the workgroups of slices beyond the
        // scan the device finds leave at once
        const unsigned slices = (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, ALIGN_MAX_SLICES));
        hipLaunchKernelGGL(k_grid_align_score, dim3((side * side + ALIGN_BLOCK - 1) / ALIGN_BLOCK, rots, slices), dim3(ALIGN_BLOCK), 0, s, j);
    }
    hipLaunchKernelGGL(k_grid_align_best, dim3(1), dim3(ALIGN_BEST_BLOCK), 0, s, j);
}

void launch_align_overlay(hipStream_t s, const AlignJob& j, int32_t n_scan, int32_t k, int32_t ta, int32_t tb, uint8_t* rgb) {
    const unsigned blocks = ((unsigned)n_scan + ALIGN_BLOCK - 1) / ALIGN_BLOCK;
    const int32_t K = j.alp.rot_n;
    if (n_scan > 0) {
        hipLaunchKernelGGL(k_grid_align_overlay, dim3(blocks), dim3(ALIGN_BLOCK), 0, s, j, n_scan, 0, ALIGN_ROT, 0, 0, 0, rgb);
        hipLaunchKernelGGL(k_grid_align_overlay, dim3(blocks), dim3(ALIGN_BLOCK), 0, s, j, n_scan, 1, j.rot[2 * (k + K)], j.rot[2 * (k + K) + 1], ta, tb, rgb);
    }
    hipLaunchKernelGGL(k_grid_align_overlay, dim3(1), dim3(ALIGN_BLOCK), 0, s, j, 1, 2, ALIGN_ROT, 0, 0, 0, rgb);
}

}  // namespace grid
}  // namespace svh
