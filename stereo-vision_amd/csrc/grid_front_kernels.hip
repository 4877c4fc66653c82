// The frontiers of the ground grid on the device (svh_grid_get_front_plane, svh_grid_get_frontiers, svh_grid_render_frontiers;
// include/svh_grid.h, "FRONTIERS").  The arithmetic is csrc/grid_front_core.h: integer work on the finished STATE and COST
// planes in logical order.  A label is the minimum of a set and every accumulator a commutative integer update, so nothing
// here depends on the launch shape or the scheduling.  The number of launches is FRONT_LAUNCHES whatever the scene.
//
//   k_grid_front_mask      one lane per cell: the frontier bit, LABEL = own index or -1, the frontier cells counted by ballots.
//   k_grid_front_tile      one workgroup per tile of FRONT_TILE x FRONT_TILE cells, one lane per cell, the labels in LDS as
//                          tile-local indexes (their order is that of the window's indexes).  Label equivalence: a cell whose
//                          neighbour has a lower label lowers the label OF ITS LABEL (atomicMin in LDS), then every cell follows
//                          its chain to a fixed point.  Values only fall and a label is never above its cell, so a chain is
//                          strictly decreasing and ends within the tile's cells.  Sweeps repeat until a block-wide vote says
//                          nothing changed, at most FRONT_TILE^2 + 1 times; each sweep that changes something removes a root.
//   k_grid_front_merge     one lane per cell, at work where one of the four neighbours in front of the cell (west, south-west,
//                          south, south-east) lies in another tile: edge AND corner adjacency.  Union-find on the global parent
//                          plane: find walks to the root (halving the path on its way, at most nx * nz links); the larger root is
//                          linked under the smaller with atomicMin, and a union whose atomic returns another value than the root
//                          it expected follows that value (at most FRONT_UNION_TRIES times).  parent[x] <= x always and values
//                          only fall, so the forest has no cycle under any interleaving, and the root of a finished tree is the
//                          component's lowest index.
//   k_grid_front_flatten   one lane per cell: LABEL = its root.
//   k_front_count / k_front_scan / k_front_roots   a cell is a root iff LABEL == index; the roots compacted in ascending order
//                          (the scheme of view_thin_kernels.hip): counts per block of 1024 by ballots, an exclusive scan of the
//                          block counts by one workgroup, the scatter by block offset + waves before + ballot bits below.
//   k_grid_front_accum     one lane per frontier cell: its component by a binary search of LABEL in the roots (the accumulators
//                          are sized by the components, not by the cells); size by atomicAdd, the two sums by 64-bit atomicAdd,
//                          the box by atomicMin / atomicMax -- the lanes of a wave that share the component of its first frontier
//                          cell combined by shuffles first, as k_grid_bin combines equal cells.
//   k_grid_front_centroid  one lane per component: the centroid cell; the kept components and their cells counted.
//   k_grid_front_rep       one lane per frontier cell: 64-bit atomicMin of dist2 << 32 | index.
//   k_front_count / k_front_scan / k_grid_front_records   the kept components compacted in order into the table.
//   k_grid_front_flags     one lane per frontier cell: bits 1 and 2 of FRONT.
//
// A bound that is hit sets ctl[FC_UNSETTLED]; the host returns SVH_ERR_HIP.  No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "grid_comp_dev.h"
#include "grid_front_core.h"
#include "grid_internal.h"

namespace svh {
namespace grid {
namespace {

constexpr int32_t T = FRONT_TILE;
constexpr int kScan = (int)FRONT_SCAN_BLOCK, kScanWaves = kScan / 64;
constexpr int32_t NONE = 0x7FFFFFFF;

__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_mask(FrontParams frp, int32_t nx, int32_t nz, const uint8_t* __restrict__ state,
                                                                 const uint8_t* __restrict__ cost, uint8_t* __restrict__ flags,
                                                                 int32_t* __restrict__ label, unsigned long long* ctl) {
    const uint32_t i = blockIdx.x * FRONT_BLOCK + threadIdx.x;
    bool f = false;
    if (i < (uint32_t)nx * (uint32_t)nz) {
        const int32_t b = (int32_t)(i / (uint32_t)nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)nx);
        f = front_cell(frp, nx, nz, state, cost, a, b);
        flags[i] = f ? (uint8_t)FF_FRONTIER : (uint8_t)0;
        label[i] = f ? (int32_t)i : -1;
    }
    const unsigned long long vote = __ballot(f);
    if ((threadIdx.x & 63u) == 0 && vote) atomicAdd(&ctl[FC_CELLS], (unsigned long long)__popcll(vote));
}

__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_tile(int32_t nx, int32_t nz, uint32_t tiles_x, int32_t* __restrict__ label,
                                                                 unsigned long long* ctl) {
    __shared__ int32_t s_lab[T * T];
    const int32_t c = (int32_t)threadIdx.x, ly = c / T, lx = c - ly * T;
    const int32_t ty = (int32_t)(blockIdx.x / tiles_x), tx = (int32_t)(blockIdx.x - (uint32_t)ty * tiles_x);
    const int32_t a = tx * T + lx, b = ty * T + ly;
    const bool in = a < nx && b < nz;
    const size_t g = (size_t)(in ? b : 0) * (size_t)nx + (size_t)(in ? a : 0);
    const bool own = in && label[g] >= 0;
    s_lab[c] = own ? c : NONE;
    __syncthreads();
    uint32_t nb = 0;   // bit k: the k-th of the eight neighbours is a cell of this tile to be labelled
    if (own) {
        int32_t k = 0;
        for (int32_t dy = -1; dy <= 1; dy++)
            for (int32_t dx = -1; dx <= 1; dx++) {
                if (dx == 0 && dy == 0) continue;
                const int32_t x = lx + dx, y = ly + dy;
                if (x >= 0 && x < T && y >= 0 && y < T && s_lab[y * T + x] != NONE) nb |= 1u << k;
                k++;
            }
    }
    bool settled = false;
    for (int32_t sweep = 0; sweep < T * T + 1; sweep++) {
        int changed = 0;
        if (nb) {
            const int32_t l = s_lab[c];
            int32_t m = l, k = 0;
#pragma unroll
            for (int32_t dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int32_t dx = -1; dx <= 1; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    if ((nb >> k) & 1u) {
                        const int32_t v = s_lab[c + dy * T + dx];
                        m = v < m ? v : m;
                    }
                    k++;
                }
            if (m < l) atomicMin(&s_lab[l], m), changed = 1;
        }
        if (!__syncthreads_or(changed)) {
            settled = true;
            break;
        }
        if (own) {
            int32_t l = s_lab[c];
            for (int32_t k = 0; k < T * T; k++) {   // strictly decreasing: at most T * T links
                const int32_t p = s_lab[l];
                if (p == l) break;
                l = p;
            }
            s_lab[c] = l;
        }
        __syncthreads();
    }
    if (own) {
        const int32_t r = s_lab[c], ry = r / T, rx = r - ry * T;
        label[g] = (ty * T + ry) * nx + tx * T + rx;
    }
    if (c == 0 && !settled) atomicMax(&ctl[FC_UNSETTLED], 1ull);   // never, by the bound of the sweeps
}

__device__ __forceinline__ int32_t parent_of(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, halving the path on the way; a chain is strictly decreasing, so it has at most `limit` = nx * nz links
__device__ __forceinline__ int32_t front_find(int32_t* parent, int32_t x, uint32_t limit, bool* ok) {
    for (uint32_t k = 0; k <= limit; k++) {
        const int32_t p = parent_of(parent, x);
        if (p == x) return x;
        const int32_t gp = parent_of(parent, p);
        if (gp != p) atomicMin(&parent[x], gp);
        x = gp;
    }
    *ok = false;
    return x;
}

__device__ __forceinline__ void front_union(int32_t* parent, int32_t u, int32_t v, uint32_t limit, bool* ok) {
    for (uint32_t tries = 0; tries < FRONT_UNION_TRIES; tries++) {
        u = front_find(parent, u, limit, ok);
        v = front_find(parent, v, limit, ok);
        if (u == v || !*ok) return;
        if (u < v) {
            const int32_t t = u;
            u = v, v = t;
        }
        const int32_t was = atomicMin(&parent[u], v);   // u > v: the larger root goes under the smaller
        if (was == u) return;
        u = was;                                        // another union linked u first: join what it linked to with v
    }
    *ok = false;
}

__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_merge(int32_t nx, int32_t nz, int32_t* parent, unsigned long long* ctl) {
    const uint32_t cells = (uint32_t)nx * (uint32_t)nz, i = blockIdx.x * FRONT_BLOCK + threadIdx.x;
    if (i >= cells) return;
    const int32_t b = (int32_t)(i / (uint32_t)nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)nx);
    const int32_t lx = a % T, ly = b % T;
    if (lx != 0 && ly != 0 && lx != T - 1) return;      // all four neighbours in front lie in the own tile
    if (parent_of(parent, (int32_t)i) < 0) return;
    bool ok = true;
    const int32_t da[4] = {-1, -1, 0, 1}, db[4] = {0, -1, -1, -1};
#pragma unroll
    for (int32_t k = 0; k < 4; k++) {
        const int32_t ja = a + da[k], jb = b + db[k];
        if (ja < 0 || ja >= nx || jb < 0) continue;
        if (ja / T == a / T && jb / T == b / T) continue;
        const int32_t j = jb * nx + ja;
        if (parent_of(parent, j) < 0) continue;
        front_union(parent, (int32_t)i, j, cells, &ok);
    }
    if (!ok) atomicMax(&ctl[FC_UNSETTLED], 1ull);
}

__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_flatten(uint32_t cells, int32_t* parent, unsigned long long* ctl) {
    const uint32_t i = blockIdx.x * FRONT_BLOCK + threadIdx.x;
    if (i >= cells || parent_of(parent, (int32_t)i) < 0) return;
    bool ok = true;
    const int32_t r = front_find(parent, (int32_t)i, cells, &ok);
    atomicMin(&parent[i], r);
    if (!ok) atomicMax(&ctl[FC_UNSETTLED], 1ull);
}

// what the two ordered compactions keep: a root among the cells, a kept component among the components
struct IsRoot {
    const int32_t* label;
    __device__ __forceinline__ bool operator()(uint32_t i) const { return label[i] == (int32_t)i; }
};
struct IsKept {
    const int32_t* size;
    int32_t min_size;
    __device__ __forceinline__ bool operator()(uint32_t i) const { return size[i] >= min_size; }
};
struct IsMarked {
    const int32_t* mark;
    __device__ __forceinline__ bool operator()(uint32_t i) const { return mark[i] != 0; }
};

template <class Pred>
__global__ __launch_bounds__(kScan) void k_front_count(uint32_t n, Pred pred, int32_t* __restrict__ blockcnt) {
    __shared__ int s_cnt[kScanWaves];
    const uint32_t i = blockIdx.x * (uint32_t)kScan + threadIdx.x;
    const bool k = i < n && pred(i);
    const unsigned long long b = __ballot(k);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; w++) sum += s_cnt[w];
        blockcnt[blockIdx.x] = sum;
    }
}

// in place: blockcnt[i] becomes the number kept in the blocks before i; *total = all that are kept
__global__ __launch_bounds__(kScan) void k_front_scan(int32_t* __restrict__ blockcnt, uint32_t nb, unsigned long long* __restrict__ total) {
    __shared__ int s_wave[kScanWaves];
    int carry = 0;
    for (uint32_t base = 0; base < nb; base += (uint32_t)kScan) {
        const uint32_t i = base + threadIdx.x;
        const int x = i < nb ? blockcnt[i] : 0;
        int chunk;
        const int before = block_exclusive_scan<kScan>(x, s_wave, &chunk);
        if (i < nb) blockcnt[i] = carry + before;
        carry += chunk;
    }
    if (threadIdx.x == 0) *total = (unsigned long long)carry;
}

// the position of element i among those kept, -1 when it is not; every thread of the workgroup calls it
template <class Pred>
__device__ __forceinline__ int32_t ordered_slot(uint32_t n, const Pred& pred, const int32_t* __restrict__ blockoff, int* s_cnt) {
    const uint32_t i = blockIdx.x * (uint32_t)kScan + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool k = i < n && pred(i);
    const unsigned long long b = __ballot(k);
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    if (!k) return -1;
    int at = blockoff[blockIdx.x];
#pragma unroll
    for (int w = 0; w < kScanWaves; w++) at += w < wave ? s_cnt[w] : 0;
    return at + __popcll(b & (((unsigned long long)1 << lane) - 1));
}

__global__ __launch_bounds__(kScan) void k_front_roots(uint32_t cells, const int32_t* __restrict__ label, const int32_t* __restrict__ blockoff,
                                                      int32_t n_comp, int32_t* __restrict__ roots) {
    __shared__ int s_cnt[kScanWaves];
    const int32_t at = ordered_slot(cells, IsRoot{label}, blockoff, s_cnt);
    if (at >= 0 && at < n_comp) roots[at] = (int32_t)(blockIdx.x * (uint32_t)kScan + threadIdx.x);
}

// slot[i] = the position of element i among the marked ones, -1 when it is not marked
__global__ __launch_bounds__(kScan) void k_front_slots(uint32_t n, const int32_t* __restrict__ mark, const int32_t* __restrict__ blockoff,
                                                      int32_t* __restrict__ slot) {
    __shared__ int s_cnt[kScanWaves];
    const int32_t at = ordered_slot(n, IsMarked{mark}, blockoff, s_cnt);
    const uint32_t i = blockIdx.x * (uint32_t)kScan + threadIdx.x;
    if (i < n) slot[i] = at;
}

// the component (rank among the roots) of cell i and its window cell; -1 off the frontier
__device__ __forceinline__ int32_t component_of(int32_t nx, uint32_t cells, uint32_t i, const int32_t* __restrict__ label,
                                                const int32_t* __restrict__ roots, int32_t n_comp, int32_t* a, int32_t* b) {
    *a = *b = 0;
    if (i >= cells || n_comp < 1) return -1;
    const int32_t l = label[i];
    if (l < 0) return -1;
    const int32_t k = rank_of(roots, n_comp, l);
    if (roots[k] != l) return -1;                       // never: the roots are the labels that occur
    *b = (int32_t)(i / (uint32_t)nx), *a = (int32_t)(i - (uint32_t)*b * (uint32_t)nx);
    return k;
}

// The lanes of a wave whose component is that of the wave's first frontier cell are combined by shuffles and their leader issues
// the atomics; the other frontier cells of the wave issue their own.  A wave holds 64 consecutive cells of a row, so along a
// frontier nearly every wave is of one component: without this, every cell of a long frontier queues at the same seven addresses
// (measured: profiles/grid_front_times.jsonl, tags "one atomic per cell" and "").  Sums, minima and maxima of integers: the
// grouping changes no byte.
__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_accum(int32_t nx, uint32_t cells, const int32_t* __restrict__ label,
                                                                  const int32_t* __restrict__ roots, int32_t n_comp, FrontAcc acc) {
    const uint32_t i = blockIdx.x * FRONT_BLOCK + threadIdx.x;
    int32_t a, b;
    const int32_t k = component_of(nx, cells, i, label, roots, n_comp, &a, &b);
    const unsigned long long live = __ballot(k >= 0);
    if (live == 0) return;                              // the whole wave
    const int32_t leader = __ffsll(live) - 1, k0 = __shfl(k, leader, 64);
    const bool mine = k == k0;
    const int32_t n = __popcll(__ballot(mine));
    const int32_t sa = wave_sum(mine ? a : 0), sb = wave_sum(mine ? b : 0);
    const int32_t a0 = wave_min(mine ? a : 0x7FFFFFFF), b0 = wave_min(mine ? b : 0x7FFFFFFF);
    const int32_t a1 = wave_max(mine ? a : -1), b1 = wave_max(mine ? b : -1);
    if (mine) {
        if ((int32_t)(threadIdx.x & 63u) != leader) return;
        atomicAdd(&acc.size[k], n);
        atomicAdd(&acc.sum[2 * k], (unsigned long long)sa);
        atomicAdd(&acc.sum[2 * k + 1], (unsigned long long)sb);
        atomicMin(&acc.bmin[2 * k], a0), atomicMin(&acc.bmin[2 * k + 1], b0);
        atomicMax(&acc.bmax[2 * k], a1), atomicMax(&acc.bmax[2 * k + 1], b1);
    } else if (k >= 0) {
        atomicAdd(&acc.size[k], 1);
        atomicAdd(&acc.sum[2 * k], (unsigned long long)a);
        atomicAdd(&acc.sum[2 * k + 1], (unsigned long long)b);
        atomicMin(&acc.bmin[2 * k], a), atomicMin(&acc.bmin[2 * k + 1], b);
        atomicMax(&acc.bmax[2 * k], a), atomicMax(&acc.bmax[2 * k + 1], b);
    }
}

__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_centroid(int32_t n_comp, int32_t min_size, FrontAcc acc, unsigned long long* ctl) {
    const uint32_t k = blockIdx.x * FRONT_BLOCK + threadIdx.x;
    int32_t size = 0;
    if (k < (uint32_t)n_comp) {
        size = acc.size[k];
        if (size >= 1) {
            acc.cen[2 * k] = front_centre((int64_t)acc.sum[2 * k], size);
            acc.cen[2 * k + 1] = front_centre((int64_t)acc.sum[2 * k + 1], size);
        }
        if (size < min_size) size = 0;
    }
    if (size > 0) atomicAdd(&ctl[FC_KEPT_CELLS], (unsigned long long)size);
}

__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_rep(int32_t nx, uint32_t cells, const int32_t* __restrict__ label,
                                                                const int32_t* __restrict__ roots, int32_t n_comp, FrontAcc acc) {
    const uint32_t i = blockIdx.x * FRONT_BLOCK + threadIdx.x;
    int32_t a, b;
    const int32_t k = component_of(nx, cells, i, label, roots, n_comp, &a, &b);
    const unsigned long long live = __ballot(k >= 0);
    if (live == 0) return;                              // the whole wave
    const int32_t leader = __ffsll(live) - 1, k0 = __shfl(k, leader, 64);
    const bool mine = k == k0;
    const unsigned long long key = k >= 0 ? (unsigned long long)front_key(a, b, acc.cen[2 * k], acc.cen[2 * k + 1], i) : ~0ull;
    const unsigned long long least = wave_min64(mine ? key : ~0ull);   // combined as in k_grid_front_accum
    if (mine) {
        if ((int32_t)(threadIdx.x & 63u) == leader) atomicMin(&acc.rep[k], least);
    } else if (k >= 0) {
        atomicMin(&acc.rep[k], key);
    }
}

__global__ __launch_bounds__(kScan) void k_grid_front_records(int32_t nx, int32_t oa, int32_t ob, int32_t n_comp, int32_t min_size,
                                                             const int32_t* __restrict__ roots, FrontAcc acc,
                                                             const int32_t* __restrict__ blockoff, int32_t* __restrict__ recs) {
    __shared__ int s_cnt[kScanWaves];
    const int32_t at = ordered_slot((uint32_t)n_comp, IsKept{acc.size, min_size}, blockoff, s_cnt);
    if (at < 0) return;
    const uint32_t k = blockIdx.x * (uint32_t)kScan + threadIdx.x;
    const uint32_t rep = (uint32_t)(acc.rep[k] & 0xFFFFFFFFull);
    const int32_t rb = (int32_t)(rep / (uint32_t)nx), ra = (int32_t)(rep - (uint32_t)rb * (uint32_t)nx);
    int32_t* r = recs + (size_t)FRONT_REC * (size_t)at;
    r[FR_LABEL] = roots[k], r[FR_SIZE] = acc.size[k];
    r[FR_GA_MIN] = oa + acc.bmin[2 * k], r[FR_GB_MIN] = ob + acc.bmin[2 * k + 1];
    r[FR_GA_MAX] = oa + acc.bmax[2 * k], r[FR_GB_MAX] = ob + acc.bmax[2 * k + 1];
    r[FR_CEN_GA] = oa + acc.cen[2 * k], r[FR_CEN_GB] = ob + acc.cen[2 * k + 1];
    r[FR_REP_GA] = oa + ra, r[FR_REP_GB] = ob + rb;
}

__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_flags(uint32_t cells, int32_t min_size, const int32_t* __restrict__ label,
                                                                  const int32_t* __restrict__ roots, int32_t n_comp, FrontAcc acc,
                                                                  uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * FRONT_BLOCK + threadIdx.x;
    if (i >= cells) return;
    const int32_t l = label[i];
    if (l < 0 || n_comp < 1) return;
    const int32_t k = rank_of(roots, n_comp, l);
    if (roots[k] != l || acc.size[k] < min_size) return;
    const bool rep = (uint32_t)(acc.rep[k] & 0xFFFFFFFFull) == i;
    flags[i] = (uint8_t)(FF_FRONTIER | FF_KEPT | (rep ? FF_REP : 0));
}

__global__ __launch_bounds__(FRONT_BLOCK) void k_grid_front_overlay(int32_t nx, int32_t nz, const uint8_t* __restrict__ flags, uint8_t* rgb) {
    const uint32_t i = blockIdx.x * FRONT_BLOCK + threadIdx.x;
    if (i >= (uint32_t)nx * (uint32_t)nz) return;
    uint8_t px[3];
    if (!colour_front(flags[i], px)) return;
    const int32_t b = (int32_t)(i / (uint32_t)nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)nx);
    const size_t o = 3 * ((size_t)(nz - 1 - b) * (size_t)nx + (size_t)a);
    rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
}

inline unsigned per_cell(const FrontJob& j) { return ((unsigned)j.nx * (unsigned)j.nz + FRONT_BLOCK - 1) / FRONT_BLOCK; }
inline unsigned blocks_of(size_t n, unsigned block) { return n ? (unsigned)((n + block - 1) / block) : 1u; }

}  // namespace

int32_t launch_front_mask(hipStream_t s, const FrontJob& j) {
    hipLaunchKernelGGL(k_grid_front_mask, dim3(per_cell(j)), dim3(FRONT_BLOCK), 0, s, j.frp, j.nx, j.nz, j.state, j.cost, j.flags, j.label, j.ctl);
    return 1;
}

int32_t launch_front_label(hipStream_t s, const FrontJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz;
    hipLaunchKernelGGL(k_grid_front_tile, dim3(front_tiles_x(j) * front_tiles_y(j)), dim3(FRONT_BLOCK), 0, s, j.nx, j.nz, front_tiles_x(j), j.label,
                       j.ctl);
    hipLaunchKernelGGL(k_grid_front_merge, dim3(per_cell(j)), dim3(FRONT_BLOCK), 0, s, j.nx, j.nz, j.label, j.ctl);
    hipLaunchKernelGGL(k_grid_front_flatten, dim3(per_cell(j)), dim3(FRONT_BLOCK), 0, s, cells, j.label, j.ctl);
    return FRONT_LABEL_LAUNCHES;
}

int32_t launch_front_count(hipStream_t s, const FrontJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz, nb = (unsigned)front_blocks(j);
    hipLaunchKernelGGL(k_front_count<IsRoot>, dim3(nb), dim3(kScan), 0, s, cells, IsRoot{j.label}, j.blockcnt);
    hipLaunchKernelGGL(k_front_scan, dim3(1), dim3(kScan), 0, s, j.blockcnt, nb, j.ctl + FC_COMPONENTS);
    return 2;
}

int32_t launch_front_roots(hipStream_t s, const FrontJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz;
    hipLaunchKernelGGL(k_front_roots, dim3((unsigned)front_blocks(j)), dim3(kScan), 0, s, cells, (const int32_t*)j.label, (const int32_t*)j.blockcnt,
                       j.n_comp, j.roots);
    return 1;
}

int32_t launch_front_rank(hipStream_t s, uint32_t n, const int32_t* mark, int32_t* blockcnt, unsigned long long* total, int32_t* slot) {
    const unsigned sb = blocks_of(n, FRONT_SCAN_BLOCK);
    hipLaunchKernelGGL(k_front_count<IsMarked>, dim3(sb), dim3(kScan), 0, s, n, IsMarked{mark}, blockcnt);
    hipLaunchKernelGGL(k_front_scan, dim3(1), dim3(kScan), 0, s, blockcnt, sb, total);
    hipLaunchKernelGGL(k_front_slots, dim3(sb), dim3(kScan), 0, s, n, mark, (const int32_t*)blockcnt, slot);
    return 3;
}

int32_t launch_front_table(hipStream_t s, const FrontJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz, n = (unsigned)j.n_comp;
    const FrontAcc acc = front_acc(j.acc, n ? n : 1);
    const unsigned cb = blocks_of(n, FRONT_BLOCK), sb = blocks_of(n, FRONT_SCAN_BLOCK);
    launch_front_roots(s, j);
    hipLaunchKernelGGL(k_grid_front_accum, dim3(per_cell(j)), dim3(FRONT_BLOCK), 0, s, j.nx, cells, (const int32_t*)j.label, (const int32_t*)j.roots,
                       j.n_comp, acc);
    hipLaunchKernelGGL(k_grid_front_centroid, dim3(cb), dim3(FRONT_BLOCK), 0, s, j.n_comp, j.frp.min_size, acc, j.ctl);
    hipLaunchKernelGGL(k_grid_front_rep, dim3(per_cell(j)), dim3(FRONT_BLOCK), 0, s, j.nx, cells, (const int32_t*)j.label, (const int32_t*)j.roots,
                       j.n_comp, acc);
    // the block offsets of the cells are spent once the roots are scattered: the same counts serve the components
    hipLaunchKernelGGL(k_front_count<IsKept>, dim3(sb), dim3(kScan), 0, s, n, IsKept{acc.size, j.frp.min_size}, j.blockcnt);
    hipLaunchKernelGGL(k_front_scan, dim3(1), dim3(kScan), 0, s, j.blockcnt, sb, j.ctl + FC_KEPT);
    hipLaunchKernelGGL(k_grid_front_records, dim3(sb), dim3(kScan), 0, s, j.nx, j.oa, j.ob, j.n_comp, j.frp.min_size, (const int32_t*)j.roots, acc,
                       (const int32_t*)j.blockcnt, j.recs);
    hipLaunchKernelGGL(k_grid_front_flags, dim3(per_cell(j)), dim3(FRONT_BLOCK), 0, s, cells, j.frp.min_size, (const int32_t*)j.label,
                       (const int32_t*)j.roots, j.n_comp, acc, j.flags);
    return 8;
}

void launch_front_overlay(hipStream_t s, int32_t nx, int32_t nz, const uint8_t* flags, uint8_t* rgb) {
    const unsigned cells = (unsigned)nx * (unsigned)nz;
    hipLaunchKernelGGL(k_grid_front_overlay, dim3((cells + FRONT_BLOCK - 1) / FRONT_BLOCK), dim3(FRONT_BLOCK), 0, s, nx, nz, flags, rgb);
}

}  // namespace grid
}  // namespace svh
