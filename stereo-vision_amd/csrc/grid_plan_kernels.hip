// The planner of the ground grid on the device (svh_grid_plan_*, svh_grid_get_plan_plane, svh_grid_render_plan;
// include/svh_grid.h, "PLANNING").  The arithmetic is csrc/grid_plan_core.h: integer work on the finished COST plane in logical
// order.  POT is the unique fixed point of the relaxation, so nothing here depends on the launch shape or the scheduling.
//
//   k_grid_plan_seed    one lane per cell: the price plane from COST, POT all FAR.
//   k_grid_plan_goals   one lane per goal: POT 0 where the goal counts (inside the window and passable; the exchange tells a
//                       duplicate, which writes the same 0 again and is not counted), and the tiles of the goal's 3 x 3 cells
//                       go on the list of round 0 -- a goal on a tile's edge does not CHANGE there, so its neighbour tile
//                       would never hear of it otherwise.
//   k_grid_plan_relax   a tiled label-correcting relaxation: one workgroup of 256 lanes per ACTIVE tile of PLAN_TILE x
//                       PLAN_TILE cells.  The tile and a halo of one cell go into LDS as POT (int32) and price (uint16), 18 x
//                       18 x 6 bytes at 16; cells outside the window are impassable.  A lane keeps the eight step weights of
//                       each of its cells in registers (0: no such step), so a sweep is eight LDS reads, adds and minima per
//                       cell; neighbouring lanes hold neighbouring ia, a 32-lane half reads 32 consecutive dwords at every
//                       step: no bank conflict at any row length.  Sweeps repeat until a block-wide vote says nothing
//                       changed, at most PLAN_TILE^2 + 1 times.  Reading a neighbour's older or newer value within a sweep
//                       is harmless: values only fall, and every value is the length of a real step sequence.  The interior
//                       is written back where it changed, and for every side or corner of the border that changed the
//                       touching tile is appended to the next round's list; a flag per tile and list keeps it there once.  A
//                       tile that a neighbour changes while it runs is on the next list by that same rule, so no update is
//                       lost.  No workgroup waits for another.
//   k_grid_plan_dir     one lane per cell: DIR from the finished POT, and the count of cells that were reached.
//   k_grid_plan_walk    one lane follows DIR from the start, a chain of dependent byte loads, at most nx * nz cells.
//   k_grid_plan_overlay one lane per goal or path cell, drawn over the image of k_grid_render_cost.
//
// The host loop (grid_engine.cpp, plan_rounds) alternates the two lists; the lengths of three consecutive rounds rotate
// through ctl[0..2] so that no launch is needed to reset one.
//
// MEASURED (tools/gpu_grid_plan.py, profiles/grid_plan_times.jsonl; one MI355X, medians of whole svh_grid_plan_set_goals +
// svh_grid_get_plan_plane calls on a cached cost map, four rounds per wait, in ms; DESIGN.md "Ground grid", "Planning"):
//                                  tile 16     tile 32     tile 64     plain form
//   256 x 256    open field         0.370       0.561       1.557       1.526
//                30 % blocked       0.610       1.149       5.021       2.201
//                serpentine        29.9        44.6       158.3       229.4
//   1024 x 1024  open field         1.475       2.385       7.456      13.23
//                30 % blocked       2.438       4.345      14.91       16.73
//                serpentine       467         684        2466          (not run: a round per cell of the route)
// The tile sides are builds of their own, each a process; the plain form -- one lane per cell, one sweep of the whole
// window per launch, repeated until a sweep changes nothing -- passed the same tests, alternated with the tiles of 32 in one
// process (plain - tiled: +0.96 ms, 10th to 90th percentile 0.94 .. 0.98, on the open 256 x 256 field) and was then deleted.
// A smaller tile settles in fewer sweeps and leaves more workgroups to run side by side; 16 won everywhere and is kept.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grid_internal.h"
#include "grid_plan_core.h"

namespace svh {
namespace grid {
namespace {

constexpr int32_t T = PLAN_TILE, W = PLAN_TILE + 2;
constexpr int32_t PER_LANE = T * T / (int32_t)PLAN_BLOCK;

__global__ __launch_bounds__(PLAN_BLOCK) void k_grid_plan_seed(PlanParams pln, uint32_t cells, const uint8_t* __restrict__ cost,
                                                               uint16_t* __restrict__ price, int32_t* __restrict__ pot) {
    const uint32_t i = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    if (i >= cells) return;
    price[i] = price_of(pln, cost[i]);
    pot[i] = PLAN_FAR;
}

// tile `t` goes on the list `which` (0 or 1) whose length is ctl[len_at], once
__device__ __forceinline__ void enlist(uint32_t* lists, uint32_t* flags, uint32_t* ctl, uint32_t tiles, uint32_t which, uint32_t len_at,
                                       uint32_t t) {
    if (atomicExch(&flags[which * tiles + t], 1u) == 0u) lists[which * tiles + atomicAdd(&ctl[len_at], 1u)] = t;
}

__global__ __launch_bounds__(PLAN_BLOCK) void k_grid_plan_goals(int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                                                                const int32_t* __restrict__ goals, int32_t n,
                                                                const uint16_t* __restrict__ price, int32_t* pot, uint32_t tiles_x,
                                                                uint32_t tiles_y, uint32_t* lists, uint32_t* flags, uint32_t* ctl) {
    const uint32_t k = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    if (k >= (uint32_t)n) return;
    const int32_t a = goals[2 * k] - oa, b = goals[2 * k + 1] - ob;   // both terms are below 2^20 in magnitude
    if (a < 0 || a >= nx || b < 0 || b >= nz) return;
    const size_t i = (size_t)b * (size_t)nx + (size_t)a;
    if (price[i] == 0) return;
    if (atomicExch(&pot[i], 0) != 0) atomicAdd(&ctl[CTL_COUNTED], 1u);
    const int32_t a0 = a > 0 ? a - 1 : 0, a1 = a < nx - 1 ? a + 1 : nx - 1, b0 = b > 0 ? b - 1 : 0, b1 = b < nz - 1 ? b + 1 : nz - 1;
    for (int32_t ty = b0 / T; ty <= b1 / T; ty++)
        for (int32_t tx = a0 / T; tx <= a1 / T; tx++) enlist(lists, flags, ctl, tiles_x * tiles_y, 0u, CTL_LEN, (uint32_t)ty * tiles_x + (uint32_t)tx);
}

// the price of a tile cell (a, b), each in -1 .. T, from the tile in LDS
struct TilePrice {
    const uint16_t* p;
    __device__ __forceinline__ uint32_t operator()(int32_t a, int32_t b) const { return p[(b + 1) * W + (a + 1)]; }
};

__global__ __launch_bounds__(PLAN_BLOCK) void k_grid_plan_relax(int32_t nx, int32_t nz, uint32_t max_cost, uint32_t round,
                                                                uint32_t tiles_x, uint32_t tiles_y,
                                                                const uint16_t* __restrict__ price, int32_t* pot, uint32_t* lists,
                                                                uint32_t* flags, uint32_t* ctl) {
    __shared__ int32_t s_pot[W * W];
    __shared__ uint16_t s_price[W * W];
    __shared__ uint32_t s_mask;
    const uint32_t tiles = tiles_x * tiles_y, cur = round & 1u, nxt = cur ^ 1u, tid = threadIdx.x;
    const uint32_t len_next = (round + 1u) % 3u;
    const uint32_t len = ctl[round % 3u];            // complete: the kernels of a stream run one after the other
    if (blockIdx.x == 0 && tid == 0) {
        ctl[(round + 2u) % 3u] = 0u;                 // the length the round after the next appends to; nobody reads it now
        if (len) ctl[CTL_ROUNDS] += 1u;
    }
    const TilePrice P{s_price};
    for (uint32_t e = blockIdx.x; e < len; e += gridDim.x) {   // uniform over the workgroup
        const uint32_t tile = lists[cur * tiles + e];
        const int32_t ty = (int32_t)(tile / tiles_x), tx = (int32_t)(tile - (uint32_t)ty * tiles_x);
        const int32_t a0 = tx * T, b0 = ty * T;
        if (tid == 0) flags[cur * tiles + tile] = 0u, s_mask = 0u;
        for (int32_t i = (int32_t)tid; i < W * W; i += (int32_t)PLAN_BLOCK) {
            const int32_t ly = i / W, a = a0 + (i - ly * W) - 1, b = b0 + ly - 1;
            const bool in = a >= 0 && a < nx && b >= 0 && b < nz;
            const size_t g = (size_t)(in ? b : 0) * (size_t)nx + (size_t)(in ? a : 0);
            s_price[i] = in ? price[g] : (uint16_t)0;
            s_pot[i] = in ? pot[g] : PLAN_FAR;
        }
        __syncthreads();
        uint16_t w[PER_LANE][8];
        uint32_t own[PER_LANE], was[PER_LANE];
#pragma unroll
        for (int32_t k = 0; k < PER_LANE; k++) {
            const int32_t c = (int32_t)tid + k * (int32_t)PLAN_BLOCK, y = c / T, x = c - y * T;
            const int32_t at = (y + 1) * W + (x + 1);
            const uint32_t pu = s_price[at];
#pragma unroll
            for (int32_t d = 0; d < 8; d++) w[k][d] = pu ? (uint16_t)step_weight(P, x, y, pu, d) : (uint16_t)0;
            own[k] = was[k] = (uint32_t)s_pot[at];
        }
        bool settled = false;
        for (int32_t sweep = 0; sweep < T * T + 1; sweep++) {
            int changed = 0;
#pragma unroll
            for (int32_t k = 0; k < PER_LANE; k++) {
                const int32_t c = (int32_t)tid + k * (int32_t)PLAN_BLOCK, y = c / T, x = c - y * T;
                const int32_t at = (y + 1) * W + (x + 1);
                uint32_t best = own[k];
#pragma unroll
                for (int32_t d = 0; d < 8; d++) {
                    if (w[k][d]) {
                        const uint32_t cand = candidate((uint32_t)s_pot[at + step_db(d) * W + step_da(d)], w[k][d], max_cost);
                        best = cand < best ? cand : best;
                    }
                }
                if (best < own[k]) own[k] = best, s_pot[at] = (int32_t)best, changed = 1;
            }
            if (!__syncthreads_or(changed)) {
                settled = true;
                break;
            }
        }
        uint32_t mask = 0;
#pragma unroll
        for (int32_t k = 0; k < PER_LANE; k++) {
            if (own[k] == was[k]) continue;
            const int32_t c = (int32_t)tid + k * (int32_t)PLAN_BLOCK, y = c / T, x = c - y * T;
            pot[(size_t)(b0 + y) * (size_t)nx + (size_t)(a0 + x)] = (int32_t)own[k];   // a cell that changed is passable: inside the window
            const bool l = x == 0, r = x == T - 1, dn = y == 0, up = y == T - 1;
            mask |= (r ? 1u : 0u) | (r && up ? 2u : 0u) | (up ? 4u : 0u) | (l && up ? 8u : 0u) | (l ? 16u : 0u) | (l && dn ? 32u : 0u) |
                    (dn ? 64u : 0u) | (r && dn ? 128u : 0u);
        }
        if (mask) atomicOr(&s_mask, mask);
        __syncthreads();
        if (tid < 8 && ((s_mask >> tid) & 1u)) {
            const int32_t ux = tx + step_da((int32_t)tid), uy = ty + step_db((int32_t)tid);
            if (ux >= 0 && ux < (int32_t)tiles_x && uy >= 0 && uy < (int32_t)tiles_y)
                enlist(lists, flags, ctl, tiles, nxt, len_next, (uint32_t)uy * tiles_x + (uint32_t)ux);
        }
        if (tid == 8 && !settled) enlist(lists, flags, ctl, tiles, nxt, len_next, tile);   // never, by the bound of the sweeps
        __syncthreads();                             // s_mask and the tile are free for the next entry
    }
}

__global__ __launch_bounds__(PLAN_BLOCK) void k_grid_plan_dir(int32_t nx, int32_t nz, const uint16_t* __restrict__ price,
                                                              const int32_t* __restrict__ pot, uint8_t* __restrict__ dir,
                                                              unsigned long long* reached) {
    const uint32_t i = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    bool far = true;
    if (i < (uint32_t)nx * (uint32_t)nz) {
        const int32_t b = (int32_t)(i / (uint32_t)nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)nx);
        const uint32_t pu = price[i];
        const int32_t own = pot[i];
        far = own == PLAN_FAR;
        dir[i] = pu ? dir_of(WindowPrice{price, nx, nz}, WindowPot{pot, nx}, a, b, pu, own) : DIR_NONE;
    }
    const unsigned long long vote = __ballot(!far);
    if ((threadIdx.x & 63u) == 0 && vote) atomicAdd(reached, (unsigned long long)__popcll(vote));
}

__global__ __launch_bounds__(64) void k_grid_plan_walk(int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t a, int32_t b,
                                                       const uint16_t* __restrict__ price, const int32_t* __restrict__ pot,
                                                       const uint8_t* __restrict__ dir, int32_t* __restrict__ cells, int64_t cap,
                                                       int64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const size_t start = (size_t)b * (size_t)nx + (size_t)a;       // the host has checked that (a, b) is inside the window
    const int32_t cost = pot[start];
    out[2] = cost;
    out[1] = 0;
    if (price[start] == 0) {
        out[0] = PATH_BLOCKED;
        return;
    }
    out[0] = PATH_UNREACHABLE;
    if (cost == PLAN_FAR) return;
    const int64_t limit = (int64_t)nx * (int64_t)nz;
    for (int64_t len = 0; len < limit;) {
        const uint8_t d = dir[(size_t)b * (size_t)nx + (size_t)a];
        if (d > DIR_GOAL) return;                                  // never: DIR leads down POT to a goal
        if (len < cap) cells[2 * len] = oa + a, cells[2 * len + 1] = ob + b;
        len++;
        if (d == DIR_GOAL) {
            out[0] = PATH_FOUND, out[1] = len;
            return;
        }
        a += step_da(d), b += step_db(d);
        if (a < 0 || a >= nx || b < 0 || b >= nz) return;          // never: a step that exists stays inside
    }
}

__global__ __launch_bounds__(PLAN_BLOCK) void k_grid_plan_overlay(int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                                                                  const int32_t* __restrict__ cells, int64_t n,
                                                                  const uint16_t* __restrict__ price, uint8_t* rgb) {
    for (int64_t k = (int64_t)blockIdx.x * PLAN_BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * PLAN_BLOCK) {
        const int64_t a = (int64_t)cells[2 * k] - oa, b = (int64_t)cells[2 * k + 1] - ob;
        if (a < 0 || a >= nx || b < 0 || b >= nz) continue;
        if (price && price[(size_t)b * (size_t)nx + (size_t)a] == 0) continue;   // a goal that does not count
        uint8_t px[3];
        colour_plan(price == nullptr, px);
        const size_t o = 3 * ((size_t)(nz - 1 - b) * (size_t)nx + (size_t)a);
        rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
    }
}

}  // namespace

void launch_plan_seed(hipStream_t s, const PlanJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz;
    hipLaunchKernelGGL(k_grid_plan_seed, dim3((cells + PLAN_BLOCK - 1) / PLAN_BLOCK), dim3(PLAN_BLOCK), 0, s, j.pln, cells, j.cost, j.price,
                       j.pot);
    if (j.n_goals > 0)
        hipLaunchKernelGGL(k_grid_plan_goals, dim3(((unsigned)j.n_goals + PLAN_BLOCK - 1) / PLAN_BLOCK), dim3(PLAN_BLOCK), 0, s, j.nx, j.nz,
                           j.oa, j.ob, j.goals, j.n_goals, (const uint16_t*)j.price, j.pot, plan_tiles_x(j), plan_tiles_y(j), j.lists,
                           j.flags, j.ctl);
}

void launch_plan_relax(hipStream_t s, const PlanJob& j, uint32_t round, uint32_t blocks) {
    hipLaunchKernelGGL(k_grid_plan_relax, dim3(blocks), dim3(PLAN_BLOCK), 0, s, j.nx, j.nz, (uint32_t)j.pln.max_cost, round,
                       plan_tiles_x(j), plan_tiles_y(j), (const uint16_t*)j.price, j.pot, j.lists, j.flags, j.ctl);
}

void launch_plan_dir(hipStream_t s, const PlanJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz;
    hipLaunchKernelGGL(k_grid_plan_dir, dim3((cells + PLAN_BLOCK - 1) / PLAN_BLOCK), dim3(PLAN_BLOCK), 0, s, j.nx, j.nz,
                       (const uint16_t*)j.price, (const int32_t*)j.pot, j.dir, (unsigned long long*)(j.ctl + CTL_REACHED));
}

void launch_plan_walk(hipStream_t s, const PlanJob& j, int32_t a, int32_t b, int32_t* cells, int64_t cap, int64_t* out) {
    hipLaunchKernelGGL(k_grid_plan_walk, dim3(1), dim3(64), 0, s, j.nx, j.nz, j.oa, j.ob, a, b, (const uint16_t*)j.price,
                       (const int32_t*)j.pot, (const uint8_t*)j.dir, cells, cap, out);
}

void launch_plan_overlay(hipStream_t s, const PlanJob& j, const int32_t* cells, int64_t n, bool goals, uint8_t* rgb) {
    if (n <= 0) return;
    const int64_t blocks = std::min<int64_t>((n + PLAN_BLOCK - 1) / PLAN_BLOCK, 4096);
    hipLaunchKernelGGL(k_grid_plan_overlay, dim3((unsigned)blocks), dim3(PLAN_BLOCK), 0, s, j.nx, j.nz, j.oa, j.ob, cells, n,
                       goals ? (const uint16_t*)j.price : (const uint16_t*)nullptr, rgb);
}

}  // namespace grid
}  // namespace svh
