// The pose planner of the ground grid on the device (svh_grid_pose_*, svh_grid_get_pose_plane, svh_grid_render_pose;
// include/svh_grid_pose.h).  The arithmetic is csrc/grid_pose_core.h: integer work on the finished COST plane in logical order.
// PPOT is the unique fixed point of the relaxation, so nothing here depends on the launch shape or the scheduling.
//
//   k_grid_pose_foot    the eight CF planes: one workgroup per tile of FOOT_TILE x FOOT_TILE cells and heading, one lane per cell,
//                       a maximum of r(COST) over the heading's offset list.  The offsets are the same for every lane (scalar
//                       loads); what differs is the cell, so neighbouring lanes read neighbouring bytes.  r(COST) of the tile
//                       grown by the list's bounding box is staged in LDS as bytes, 255 for a cell outside the window (r is at
//                       most 254), when it has at most FOOT_LDS = 32 KiB: at that size five workgroups still share a CU's 160
//                       KiB, 20 of its 32 waves, and a list whose box is up to 165 x 165 cells is staged (181 x 181 bytes with
//                       the tile).  The LDS is dynamic, the largest staged region of the eight headings: 256 bytes for the
//                       point, about 40 x 40 for the default car at 0.2 m, so a small vehicle keeps full occupancy.  A larger
//                       box reads COST from global memory with the header's roll_cell.
//   k_grid_pose_seed    one lane per state: the price from CF, PPOT all FAR.
//   k_grid_pose_goals   one lane per goal triple: PPOT 0 for every heading that counts, and the tiles of the goal's 3 x 3 cells go
//                       on the list of round 0, as in k_grid_plan_goals.
//   k_grid_pose_relax   the planner's tiled label-correcting relaxation over states: one workgroup of 256 lanes per ACTIVE tile of
//                       POSE_TILE x POSE_TILE cells x 8 headings.  Every move reaches at most one cell away, so the tile and a
//                       halo of one cell go into LDS as PPOT (int32) and price (uint16), 18 x 18 x 8 x 6 = 15552 bytes (15816 with
//                       the border mask and alignment, as built): ten tiles
//                       per CU by LDS, eight by the 32 waves.  A lane owns ONE CELL and its eight headings: the 48 move weights
//                       of its states stay in registers (0: no such move), a sweep is 48 LDS reads, adds and minima per lane,
//                       and the spins and turns of a cell are relaxed in one lane one after the other, so a value crosses several
//                       headings within a sweep.  At every read the lanes of a 32-lane half hold two rows of 16 neighbouring
//                       cells, 18 dwords apart: the last two cells of the second row fall on the banks of the first two of the
//                       first, one extra LDS cycle in two of 32 banks.  Sweeps repeat until a block-wide vote says nothing
//                       changed, at most 8 POSE_TILE^2 + 1 times (the states of the tile: Bellman-Ford's bound under a fixed
//                       halo).  Reading a neighbour's older or newer value within a sweep is harmless: values only fall, and
//                       every value is the weight of a real move sequence.  The write-back, the border mask and the lists are the
//                       planner's: a changed side or corner cell, at any heading, enlists the touching tile.
//   k_grid_pose_dir     one lane per state: PDIR from the finished PPOT, and the count of states that were reached.
//   k_grid_pose_walk    one lane follows PDIR from the start state, a chain of dependent byte loads, at most 8 nx nz states.
//   k_grid_pose_overlay one lane per goal or pose, drawn over the image of k_grid_render_cost.
//
// The host loop is the planner's (grid_engine.cpp, relax_rounds).  MEASURED: DESIGN.md, "Pose planning".
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grid_internal.h"
#include "grid_pose_core.h"

namespace svh {
namespace grid {
namespace {

constexpr int32_t T = POSE_TILE, W = POSE_TILE + 2, WW = W * W, H = POSE_HEADINGS;

struct Boxes {
    int32_t v[POSE_HEADINGS][4];
};

__global__ __launch_bounds__(POSE_BLOCK) void k_grid_pose_foot(int32_t nx, int32_t nz, int32_t m, int32_t unknown_cost, Boxes boxes,
                                                               const uint8_t* __restrict__ cost, const int2* __restrict__ offs,
                                                               const int32_t* __restrict__ start, uint8_t* __restrict__ cf) {
    extern __shared__ uint8_t s_r[];                 // the launch's dynamic LDS: the largest staged region among the eight headings
    const int32_t d = (int32_t)blockIdx.z, a0 = (int32_t)blockIdx.x * FOOT_TILE, b0 = (int32_t)blockIdx.y * FOOT_TILE;
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t at = start[d * m], n = start[d * m + 1] - at;
    const int32_t x0 = boxes.v[d][0], y0 = boxes.v[d][2];
    const int32_t sw = FOOT_TILE + boxes.v[d][1] - x0, sh = FOOT_TILE + boxes.v[d][3] - y0;   // each at most 16 + 2 * 128
    const bool staged = (uint32_t)(sw * sh) <= FOOT_LDS;                                       // uniform over the workgroup
    if (staged) {
        for (int32_t i = tid; i < sw * sh; i += (int32_t)POSE_BLOCK) {
            const int32_t ly = i / sw, a = a0 + x0 + (i - ly * sw), b = b0 + y0 + ly;
            const bool in = a >= 0 && a < nx && b >= 0 && b < nz;
            s_r[i] = in ? (uint8_t)roll_cost(cost[(size_t)b * (size_t)nx + (size_t)a], unknown_cost) : POSE_CF_OUTSIDE;
        }
        __syncthreads();
    }
    const int32_t x = tid % FOOT_TILE, y = tid / FOOT_TILE, a = a0 + x, b = b0 + y;
    if (a >= nx || b >= nz) return;
    int32_t worst = 0;
    if (staged) {
        const uint8_t* row = s_r + (y - y0) * sw + (x - x0);
        for (int32_t i = 0; i < n; i++) {
            const int2 o = offs[at + i];           // within the box: 0 <= y - y0 + o.y < sh, 0 <= x - x0 + o.x < sw
            const int32_t v = row[o.y * sw + o.x];
            worst = v > worst ? v : worst;
        }
    } else {
        for (int32_t i = 0; i < n; i++) {
            const int2 o = offs[at + i];
            const int32_t v = roll_cell(cost, nx, nz, (int64_t)a + o.x, (int64_t)b + o.y, unknown_cost);
            worst = v > worst ? v : worst;
        }
        worst = pose_cf(roll_f(worst));
    }
    cf[((size_t)d * (size_t)nz + (size_t)b) * (size_t)nx + (size_t)a] = (uint8_t)worst;
}

__global__ __launch_bounds__(POSE_BLOCK) void k_grid_pose_seed(int32_t neutral, int32_t stop_cost, uint32_t states,
                                                               const uint8_t* __restrict__ cf, uint16_t* __restrict__ price,
                                                               int32_t* __restrict__ pot) {
    const uint32_t i = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (i >= states) return;
    price[i] = pose_price(neutral, stop_cost, cf[i]);
    pot[i] = PLAN_FAR;
}

// tile `t` goes on the list `which` (0 or 1) whose length is ctl[len_at], once
__device__ __forceinline__ void enlist(uint32_t* lists, uint32_t* flags, uint32_t* ctl, uint32_t tiles, uint32_t which, uint32_t len_at,
                                       uint32_t t) {
    if (atomicExch(&flags[which * tiles + t], 1u) == 0u) lists[which * tiles + atomicAdd(&ctl[len_at], 1u)] = t;
}

__global__ __launch_bounds__(POSE_BLOCK) void k_grid_pose_goals(int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                                                                const int32_t* __restrict__ goals, int32_t n,
                                                                const uint16_t* __restrict__ price, int32_t* pot, uint32_t tiles_x,
                                                                uint32_t tiles_y, uint32_t* lists, uint32_t* flags, uint32_t* ctl) {
    const uint32_t k = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (k >= (uint32_t)n) return;
    const int32_t a = goals[3 * k] - oa, b = goals[3 * k + 1] - ob, gd = goals[3 * k + 2];   // the cell's terms are below 2^20 in magnitude
    if (a < 0 || a >= nx || b < 0 || b >= nz || gd < -1 || gd >= H) return;
    bool any = false;
    for (int32_t d = gd < 0 ? 0 : gd; d <= (gd < 0 ? H - 1 : gd); d++) {
        const size_t i = ((size_t)d * (size_t)nz + (size_t)b) * (size_t)nx + (size_t)a;
        if (price[i] == 0) continue;
        any = true;
        if (atomicExch(&pot[i], 0) != 0) atomicAdd(&ctl[CTL_COUNTED], 1u);
    }
    if (!any) return;
    const int32_t a0 = a > 0 ? a - 1 : 0, a1 = a < nx - 1 ? a + 1 : nx - 1, b0 = b > 0 ? b - 1 : 0, b1 = b < nz - 1 ? b + 1 : nz - 1;
    for (int32_t ty = b0 / T; ty <= b1 / T; ty++)
        for (int32_t tx = a0 / T; tx <= a1 / T; tx++) enlist(lists, flags, ctl, tiles_x * tiles_y, 0u, CTL_LEN, (uint32_t)ty * tiles_x + (uint32_t)tx);
}

// the price of a tile state (a, b, d), a and b each in -1 .. T, from the tile in LDS
struct TilePrice {
    const uint16_t* p;
    __device__ __forceinline__ uint32_t operator()(int32_t a, int32_t b, int32_t d) const { return p[(d * W + (b + 1)) * W + (a + 1)]; }
};

__global__ __launch_bounds__(POSE_BLOCK) void k_grid_pose_relax(PoseParams pp, int32_t nx, int32_t nz, uint32_t round, uint32_t tiles_x,
                                                                uint32_t tiles_y, const uint16_t* __restrict__ price, int32_t* pot,
                                                                uint32_t* lists, uint32_t* flags, uint32_t* ctl) {
    __shared__ int32_t s_pot[H * WW];
    __shared__ uint16_t s_price[H * WW];
    __shared__ uint32_t s_mask;
    const uint32_t tiles = tiles_x * tiles_y, cur = round & 1u, nxt = cur ^ 1u, tid = threadIdx.x;
    const uint32_t len_next = (round + 1u) % 3u;
    const uint32_t len = ctl[round % 3u];            // complete: the kernels of a stream run one after the other
    if (blockIdx.x == 0 && tid == 0) {
        ctl[(round + 2u) % 3u] = 0u;                 // the length the round after the next appends to; nobody reads it now
        if (len) ctl[CTL_ROUNDS] += 1u;
    }
    const TilePrice P{s_price};
    const uint32_t max_cost = (uint32_t)pp.max_cost;
    const size_t plane = (size_t)nx * (size_t)nz;
    const int32_t x = (int32_t)tid % T, y = (int32_t)tid / T;
    for (uint32_t e = blockIdx.x; e < len; e += gridDim.x) {   // uniform over the workgroup
        const uint32_t tile = lists[cur * tiles + e];
        const int32_t ty = (int32_t)(tile / tiles_x), tx = (int32_t)(tile - (uint32_t)ty * tiles_x);
        const int32_t a0 = tx * T, b0 = ty * T;
        if (tid == 0) flags[cur * tiles + tile] = 0u, s_mask = 0u;
        for (int32_t i = (int32_t)tid; i < H * WW; i += (int32_t)POSE_BLOCK) {
            const int32_t d = i / WW, r = i - d * WW, ly = r / W, a = a0 + (r - ly * W) - 1, b = b0 + ly - 1;
            const bool in = a >= 0 && a < nx && b >= 0 && b < nz;
            const size_t g = (size_t)d * plane + (size_t)(in ? b : 0) * (size_t)nx + (size_t)(in ? a : 0);
            s_price[i] = in ? price[g] : (uint16_t)0;
            s_pot[i] = in ? pot[g] : PLAN_FAR;
        }
        __syncthreads();
        uint32_t w[H][POSE_MOVES];
        uint32_t own[H], was[H];
#pragma unroll
        for (int32_t d = 0; d < H; d++) {
            const int32_t at = (d * W + (y + 1)) * W + (x + 1);
            const uint32_t pu = s_price[at];
#pragma unroll
            for (int32_t m = 0; m < POSE_MOVES; m++) w[d][m] = pu ? move_weight(pp, P, x, y, d, pu, m) : 0u;
            own[d] = was[d] = (uint32_t)s_pot[at];
        }
        bool settled = false;
        for (int32_t sweep = 0; sweep < H * T * T + 1; sweep++) {
            int changed = 0;
#pragma unroll
            for (int32_t d = 0; d < H; d++) {
                uint32_t best = own[d];
#pragma unroll
                for (int32_t m = 0; m < POSE_MOVES; m++) {
                    if (w[d][m]) {
                        int32_t va, vb, vd;
                        pose_arrival(x, y, d, m, &va, &vb, &vd);
                        const uint32_t cand = candidate((uint32_t)s_pot[(vd * W + (vb + 1)) * W + (va + 1)], w[d][m], max_cost);
                        best = cand < best ? cand : best;
                    }
                }
                if (best < own[d]) own[d] = best, s_pot[(d * W + (y + 1)) * W + (x + 1)] = (int32_t)best, changed = 1;
            }
            if (!__syncthreads_or(changed)) {
                settled = true;
                break;
            }
        }
        bool moved = false;
#pragma unroll
        for (int32_t d = 0; d < H; d++) {
            if (own[d] == was[d]) continue;
            moved = true;                            // a state that changed is passable: its cell is inside the window
            pot[(size_t)d * plane + (size_t)(b0 + y) * (size_t)nx + (size_t)(a0 + x)] = (int32_t)own[d];
        }
        if (moved) {
            const bool l = x == 0, r = x == T - 1, dn = y == 0, up = y == T - 1;
            const uint32_t mask = (r ? 1u : 0u) | (r && up ? 2u : 0u) | (up ? 4u : 0u) | (l && up ? 8u : 0u) | (l ? 16u : 0u) |
                                  (l && dn ? 32u : 0u) | (dn ? 64u : 0u) | (r && dn ? 128u : 0u);
            if (mask) atomicOr(&s_mask, mask);
        }
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

__global__ __launch_bounds__(POSE_BLOCK) void k_grid_pose_dir(PoseParams pp, int32_t nx, int32_t nz, const uint16_t* __restrict__ price,
                                                              const int32_t* __restrict__ pot, uint8_t* __restrict__ dir,
                                                              unsigned long long* reached) {
    const uint32_t cells = (uint32_t)nx * (uint32_t)nz, i = blockIdx.x * POSE_BLOCK + threadIdx.x;
    bool far = true;
    if (i < (uint32_t)H * cells) {
        const int32_t d = (int32_t)(i / cells), c = (int32_t)(i - (uint32_t)d * cells);
        const int32_t b = c / nx, a = c - b * nx;
        const uint32_t pu = price[i];
        const int32_t own = pot[i];
        far = own == PLAN_FAR;
        dir[i] = pu ? pdir_of(pp, PoseWindowPrice{price, nx, nz}, PoseWindowPot{pot, nx, nz}, a, b, d, pu, own) : PDIR_NONE;
    }
    const unsigned long long vote = __ballot(!far);
    if ((threadIdx.x & 63u) == 0 && vote) atomicAdd(reached, (unsigned long long)__popcll(vote));
}

__global__ __launch_bounds__(64) void k_grid_pose_walk(int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t m, int32_t a, int32_t b,
                                                       int32_t d, const uint16_t* __restrict__ price, const int32_t* __restrict__ pot,
                                                       const uint8_t* __restrict__ dir, int32_t* __restrict__ poses, int64_t cap,
                                                       int64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const size_t plane = (size_t)nx * (size_t)nz;
    const size_t start = (size_t)d * plane + (size_t)b * (size_t)nx + (size_t)a;   // the host has checked that the state is inside
    const int32_t cost = pot[start];
    out[2] = cost;
    out[1] = 0;
    if (price[start] == 0) {
        out[0] = PATH_BLOCKED;
        return;
    }
    out[0] = PATH_UNREACHABLE;
    if (cost == PLAN_FAR) return;
    const int64_t limit = (int64_t)H * (int64_t)plane;
    for (int64_t len = 0; len < limit;) {
        const uint8_t mv = dir[(size_t)d * plane + (size_t)b * (size_t)nx + (size_t)a];
        if (mv > PDIR_GOAL || (mv >= POSE_MOVES && mv != PDIR_GOAL)) return;   // never: PDIR leads down PPOT to a goal
        if (len < cap) poses[3 * len] = oa + a, poses[3 * len + 1] = ob + b, poses[3 * len + 2] = d * m;
        len++;
        if (mv == PDIR_GOAL) {
            out[0] = PATH_FOUND, out[1] = len;
            return;
        }
        pose_arrival(a, b, d, mv, &a, &b, &d);
        if (a < 0 || a >= nx || b < 0 || b >= nz) return;          // never: a move that exists stays inside
    }
}

__global__ __launch_bounds__(POSE_BLOCK) void k_grid_pose_overlay(int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                                                                  const int32_t* __restrict__ triples, int64_t n,
                                                                  const uint16_t* __restrict__ price, uint8_t* rgb) {
    const size_t plane = (size_t)nx * (size_t)nz;
    for (int64_t k = (int64_t)blockIdx.x * POSE_BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * POSE_BLOCK) {
        const int64_t a = (int64_t)triples[3 * k] - oa, b = (int64_t)triples[3 * k + 1] - ob;
        if (a < 0 || a >= nx || b < 0 || b >= nz) continue;
        if (price) {                                 // a goal: drawn when one of its headings counts
            const int32_t gd = triples[3 * k + 2];
            bool any = false;
            for (int32_t d = gd < 0 ? 0 : gd; d <= (gd < 0 ? H - 1 : gd) && d < H; d++)
                any = any || price[(size_t)d * plane + (size_t)b * (size_t)nx + (size_t)a] != 0;
            if (!any) continue;
        }
        uint8_t px[3];
        colour_plan(price == nullptr, px);
        const size_t o = 3 * ((size_t)(nz - 1 - b) * (size_t)nx + (size_t)a);
        rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
    }
}

}  // namespace

void launch_pose_foot(hipStream_t s, const PoseJob& j) {
    Boxes bx;
    uint32_t lds = 0;                                // what the headings that stage need at most; the kernel applies the same test
    for (int d = 0; d < POSE_HEADINGS; d++) {
        for (int k = 0; k < 4; k++) bx.v[d][k] = j.box[d][k];
        const uint32_t region = (uint32_t)(FOOT_TILE + j.box[d][1] - j.box[d][0]) * (uint32_t)(FOOT_TILE + j.box[d][3] - j.box[d][2]);
        if (region <= FOOT_LDS) lds = std::max(lds, region);
    }
    const dim3 blocks(((unsigned)j.nx + FOOT_TILE - 1) / FOOT_TILE, ((unsigned)j.nz + FOOT_TILE - 1) / FOOT_TILE, POSE_HEADINGS);
    hipLaunchKernelGGL(k_grid_pose_foot, blocks, dim3(POSE_BLOCK), lds, s, j.nx, j.nz, j.m, j.unknown_cost, bx, j.cost, j.offs, j.start, j.cf);
}

void launch_pose_seed(hipStream_t s, const PoseJob& j) {
    const unsigned states = (unsigned)POSE_HEADINGS * (unsigned)j.nx * (unsigned)j.nz;   // at most 2^27
    hipLaunchKernelGGL(k_grid_pose_seed, dim3((states + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, s, j.pp.neutral, j.stop_cost, states,
                       (const uint8_t*)j.cf, j.price, j.pot);
    if (j.n_goals > 0)
        hipLaunchKernelGGL(k_grid_pose_goals, dim3(((unsigned)j.n_goals + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, s, j.nx, j.nz,
                           j.oa, j.ob, j.goals, j.n_goals, (const uint16_t*)j.price, j.pot, pose_tiles_x(j), pose_tiles_y(j), j.lists,
                           j.flags, j.ctl);
}

void launch_pose_relax(hipStream_t s, const PoseJob& j, uint32_t round, uint32_t blocks) {
    hipLaunchKernelGGL(k_grid_pose_relax, dim3(blocks), dim3(POSE_BLOCK), 0, s, j.pp, j.nx, j.nz, round, pose_tiles_x(j), pose_tiles_y(j),
                       (const uint16_t*)j.price, j.pot, j.lists, j.flags, j.ctl);
}

void launch_pose_dir(hipStream_t s, const PoseJob& j) {
    const unsigned states = (unsigned)POSE_HEADINGS * (unsigned)j.nx * (unsigned)j.nz;
    hipLaunchKernelGGL(k_grid_pose_dir, dim3((states + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, s, j.pp, j.nx, j.nz,
                       (const uint16_t*)j.price, (const int32_t*)j.pot, j.dir, (unsigned long long*)(j.ctl + CTL_REACHED));
}

void launch_pose_walk(hipStream_t s, const PoseJob& j, int32_t a, int32_t b, int32_t d, int32_t* poses, int64_t cap, int64_t* out) {
    hipLaunchKernelGGL(k_grid_pose_walk, dim3(1), dim3(64), 0, s, j.nx, j.nz, j.oa, j.ob, j.m, a, b, d, (const uint16_t*)j.price,
                       (const int32_t*)j.pot, (const uint8_t*)j.dir, poses, cap, out);
}

void launch_pose_overlay(hipStream_t s, const PoseJob& j, const int32_t* triples, int64_t n, bool goals, uint8_t* rgb) {
    if (n <= 0) return;
    const int64_t blocks = std::min<int64_t>((n + POSE_BLOCK - 1) / POSE_BLOCK, 4096);
    hipLaunchKernelGGL(k_grid_pose_overlay, dim3((unsigned)blocks), dim3(POSE_BLOCK), 0, s, j.nx, j.nz, j.oa, j.ob, triples, n,
                       goals ? (const uint16_t*)j.price : (const uint16_t*)nullptr, rgb);
}

}  // namespace grid
}  // namespace svh
