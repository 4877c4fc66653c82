// The time layer of the ground grid on the device (svh_grid_get_time_plane, svh_grid_get_time_stats, svh_grid_time_path,
// svh_grid_render_time; include/svh_grid_time.h, "TIME").  The arithmetic is csrc/grid_time_core.h: a layer is a pure function of the
// layer after it and of planes that do not change during the sweep, the statistics are integer sums, so nothing here depends on the
// launch shape or the scheduling.
//
//   k_grid_time_release   one lane per window cell: FLAGS -> FLAGS', TF_LETHAL cleared where the ID frame holds the id of a predicting
//                         track (a binary search over at most 4096 ids in global memory: the cells with an id are few, and the
//                         records of one object's cells are the same cache lines).  The released cells are counted by ballot, one
//                         atomic per wave.
//   k_grid_time_last      the last layer, one lane per cell: RPOT and RDIR, FAR and none where the cell is blocked at the layer's slot.
//   k_grid_time_sweep     the sweep, time-blocked.  A workgroup owns a tile of TIME_TILE x TIME_TILE cells and up to TIME_K
//                         layers.  It stages TPOT(t + k), RPRICE (bit 15: the cell is a goal that counts) and the PRED words of the
//                         tile and a halo of TIME_K cells in LDS -- one lookup by global cell per cell, not one per layer --, runs
//                         the layers there in ping-pong, the valid box losing one ring per layer, and writes TPOT and TDIR of its
//                         own tile for each.  Cells outside the window have price 0.  The last layer, a copy of the static field
//                         under the blocks, is k_grid_time_last; L - 1 layers then take ceil((L - 1) / TIME_K)
//                         launches, ordered by the stream: no workgroup waits for another.  The counts of the statistics are
//                         combined by ballot and kept per wave across all layers: three 64-bit atomics per wave and launch (integer
//                         adds: the sum does not depend on their order).  TIME_TILE = 32 and TIME_K = 8 (32 KiB of LDS) were measured
//                         alternating in one process against the plain form -- one launch per layer, one lane per cell, the same
//                         arithmetic from global memory -- which was then deleted (profiles/grid_time_times.jsonl, DESIGN.md
//                         "Time-layered planning"): with L = 32 the sweep and the copy of its layers take 1.17 against 6.71 ms at
//                         1024 x 1024 and 0.55 against 1.07 ms at 256 x 256 on a field with tracks; on a 256 x 256 field without
//                         any it is 0.05 ms slower, 0.74 against 0.69 ms.  Other tiles and depths were not measured.
//   k_grid_time_walk      one lane, a chain of dependent loads, as k_grid_plan_walk; bounded by L + nx nz entries.
//   k_grid_time_blocks    one lane per window cell: the cells with BLOCK at a layer, in the colour of the layer's slot.
//   k_grid_time_cells     the lanes stride over a list of global cells (the goals, pairs; a path, triples).
// All loops are bounded.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grid_internal.h"
#include "grid_time_core.h"

namespace svh {
namespace grid {
namespace {

// `flag` counted over the wave into *word: one atomic per wave that has any
__device__ inline void count_wave(bool flag, unsigned long long* word) {
    const unsigned long long vote = __ballot(flag);
    if ((threadIdx.x & 63u) == 0 && vote) atomicAdd(word, (unsigned long long)__popcll(vote));
}

__global__ __launch_bounds__(TIME_BLOCK) void k_grid_time_release(TimeReleaseJob j) {
    const uint32_t i = blockIdx.x * TIME_BLOCK + threadIdx.x;
    bool released = false;
    if (i < (uint32_t)j.nx * (uint32_t)j.nz) {
        const int32_t b = (int32_t)(i / (uint32_t)j.nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)j.nx);
        released = time_released(j.pp, j.nx, j.nz, j.oa, j.ob, j.poa, j.pob, j.id, j.tracks, j.n_tracks, a, b);
        const uint8_t f = j.flags[i];
        j.out[i] = released ? (uint8_t)(f & ~(uint8_t)TF_LETHAL) : f;
    }
    count_wave(released, &j.ctl[TC_RELEASED]);
}

// the last layer: the static field under the blocks of its slot
__global__ __launch_bounds__(TIME_BLOCK) void k_grid_time_last(TimeJob j) {
    const uint32_t cells = (uint32_t)j.nx * (uint32_t)j.nz;
    const uint32_t i = blockIdx.x * TIME_BLOCK + threadIdx.x;
    bool reached = false, blocked = false;
    if (i < cells) {
        const int32_t b = (int32_t)(i / (uint32_t)j.nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)j.nx);
        const int32_t t = j.tp.layers - 1, s_now = time_slot(j.pp, t);
        const uint32_t own = TimeBlock{j.pred, j.nx, j.nz, j.oa, j.ob, j.poa, j.pob}(a, b);
        int32_t v;
        uint8_t d;
        time_last(own, s_now, j.rpot[i], j.rdir[i], &v, &d);
        const size_t o = (size_t)t * (size_t)cells + i;         // t nx nz < 2^28
        j.tpot[o] = v, j.tdir[o] = d;
        reached = v != PLAN_FAR, blocked = j.price[i] != 0 && time_bit(own, s_now);
    }
    count_wave(reached, &j.ctl[TC_REACHED]);
    count_wave(blocked, &j.ctl[TC_BLOCKED]);
}

// the planes of a box of TIME_BOX x TIME_BOX cells in LDS, addressed by window cell: the box's first cell is (a0, b0)
struct BoxPrice {
    const uint16_t* p;
    int32_t a0, b0;
    __device__ uint32_t operator()(int32_t a, int32_t b) const {
        const int32_t x = a - a0, y = b - b0;
        return (x < 0 || x >= TIME_BOX || y < 0 || y >= TIME_BOX) ? 0u : (uint32_t)(p[y * TIME_BOX + x] & 0x7FFFu);
    }
};
struct BoxWord {
    const uint32_t* p;
    int32_t a0, b0;
    __device__ uint32_t operator()(int32_t a, int32_t b) const {
        const int32_t x = a - a0, y = b - b0;
        return (x < 0 || x >= TIME_BOX || y < 0 || y >= TIME_BOX) ? 0u : p[y * TIME_BOX + x];
    }
};
struct BoxNext {
    const int32_t* p;
    int32_t a0, b0;
    __device__ int32_t operator()(int32_t a, int32_t b) const {
        const int32_t x = a - a0, y = b - b0;
        return (x < 0 || x >= TIME_BOX || y < 0 || y >= TIME_BOX) ? PLAN_FAR : p[y * TIME_BOX + x];
    }
};

// The layers t_top - 1 down to t_top - k (1 <= k <= TIME_K) of the tile of TIME_TILE x TIME_TILE cells the workgroup owns, from
// TPOT(t_top) in global memory.  Bit 15 of a staged price says that the cell is a goal that counts (a price is at most 507).
__global__ __launch_bounds__(TIME_BLOCK) void k_grid_time_sweep(TimeJob j, int32_t t_top, int32_t k) {
    __shared__ int32_t s_pot[2][TIME_BOX * TIME_BOX];
    __shared__ uint32_t s_pred[TIME_BOX * TIME_BOX];
    __shared__ uint16_t s_price[TIME_BOX * TIME_BOX];
    constexpr int32_t CELLS = TIME_BOX * TIME_BOX;
    const int32_t a0 = (int32_t)blockIdx.x * TIME_TILE - TIME_K, b0 = (int32_t)blockIdx.y * TIME_TILE - TIME_K;
    const size_t cells = (size_t)j.nx * (size_t)j.nz;
    const TimeBlock B{j.pred, j.nx, j.nz, j.oa, j.ob, j.poa, j.pob};
    const int32_t* top = j.tpot + (size_t)t_top * cells;
    for (int32_t c = (int32_t)threadIdx.x; c < CELLS; c += (int32_t)TIME_BLOCK) {
        const int32_t y = c / TIME_BOX, x = c - y * TIME_BOX, a = a0 + x, b = b0 + y;
        const bool in = a >= 0 && a < j.nx && b >= 0 && b < j.nz;
        const size_t i = in ? (size_t)b * (size_t)j.nx + (size_t)a : 0;
        s_price[c] = in ? (uint16_t)(j.price[i] | (j.rpot[i] == 0 ? 0x8000u : 0u)) : (uint16_t)0;
        s_pred[c] = in ? B(a, b) : 0u;       // one lookup by global cell per cell, not one per layer
        s_pot[0][c] = in ? top[i] : PLAN_FAR;
        s_pot[1][c] = PLAN_FAR;
    }
    __syncthreads();
    const BoxPrice P{s_price, a0, b0};
    const BoxWord W{s_pred, a0, b0};
    unsigned long long reached = 0, blocked = 0, waits = 0;   // kept by the first lane of each wave
    for (int32_t step = 1; step <= k; step++) {
        const int32_t t = t_top - step, s_now = time_slot(j.pp, t), s_next = time_slot(j.pp, t + 1);
        const int32_t* src = s_pot[(step - 1) & 1];
        int32_t* dst = s_pot[step & 1];
        const BoxNext N{src, a0, b0};
        for (int32_t c0 = 0; c0 < CELLS; c0 += (int32_t)TIME_BLOCK) {   // every lane makes every trip: the ballots below need them all
            const int32_t c = c0 + (int32_t)threadIdx.x;
            const int32_t y = c / TIME_BOX, x = c - y * TIME_BOX, a = a0 + x, b = b0 + y;
            // the box that is valid at this step has lost `step` rings; outside the window there is nothing to compute
            const bool live = c < CELLS && x >= step && x < TIME_BOX - step && y >= step && y < TIME_BOX - step && a >= 0 && a < j.nx && b >= 0 && b < j.nz;
            bool r = false, bl = false, w = false;
            if (live) {
                int32_t v;
                uint8_t d;
                const uint16_t pr = s_price[c];
                time_state(j.pln, j.tp, P, N, W, s_now, s_next, (pr & 0x8000u) ? 0 : 1, a, b, &v, &d);
                dst[c] = v;
                if (x >= TIME_K && x < TIME_K + TIME_TILE && y >= TIME_K && y < TIME_K + TIME_TILE) {   // the workgroup's own tile
                    const size_t o = (size_t)t * cells + (size_t)b * (size_t)j.nx + (size_t)a;
                    j.tpot[o] = v, j.tdir[o] = d;
                    r = v != PLAN_FAR, bl = (pr & 0x7FFFu) != 0 && time_bit(s_pred[c], s_now), w = d == TDIR_WAIT;
                }
            }
            reached += (unsigned long long)__popcll(__ballot(r)), blocked += (unsigned long long)__popcll(__ballot(bl));
            waits += (unsigned long long)__popcll(__ballot(w));
        }
        __syncthreads();
    }
    if ((threadIdx.x & 63u) == 0) {
        if (reached) atomicAdd(&j.ctl[TC_REACHED], reached);
        if (blocked) atomicAdd(&j.ctl[TC_BLOCKED], blocked);
        if (waits) atomicAdd(&j.ctl[TC_WAITS], waits);
    }
}

__global__ __launch_bounds__(64) void k_grid_time_walk(TimeJob j, int32_t a, int32_t b, int32_t* __restrict__ triples, int64_t cap,
                                                       int64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const size_t cells = (size_t)j.nx * (size_t)j.nz;
    const size_t start = (size_t)b * (size_t)j.nx + (size_t)a;     // the host has checked that (a, b) is inside the window
    const int32_t cost = j.tpot[start], L = j.tp.layers;
    const TimeBlock B{j.pred, j.nx, j.nz, j.oa, j.ob, j.poa, j.pob};
    out[2] = cost;
    out[1] = 0;
    const int32_t status = time_start_status(j.price[start], B(a, b), cost);
    out[0] = status == PATH_FOUND ? (int32_t)PATH_UNREACHABLE : status;   // until the walk has reached a goal
    if (status != PATH_FOUND) return;
    const int64_t limit = (int64_t)L + (int64_t)cells;
    int32_t t = 0;
    for (int64_t len = 0; len < limit;) {
        const size_t i = (size_t)b * (size_t)j.nx + (size_t)a;
        const uint8_t d = t < L - 1 ? j.tdir[(size_t)t * cells + i] : j.rdir[i];
        if (d == DIR_NONE || d > TDIR_WAIT) return;                // never: TDIR leads down TPOT to a goal
        if (len < cap) triples[3 * len] = j.oa + a, triples[3 * len + 1] = j.ob + b, triples[3 * len + 2] = t;
        len++;
        if (d == DIR_GOAL) {
            out[0] = PATH_FOUND, out[1] = len;
            return;
        }
        if (!time_walk_step(j.nx, j.nz, L, d, &a, &b, &t)) return;   // never
    }
}

__global__ __launch_bounds__(TIME_BLOCK) void k_grid_time_blocks(TimeJob j, int32_t slot, uint8_t* rgb) {
    const uint32_t i = blockIdx.x * TIME_BLOCK + threadIdx.x;
    if (i >= (uint32_t)j.nx * (uint32_t)j.nz) return;
    const int32_t b = (int32_t)(i / (uint32_t)j.nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)j.nx);
    const TimeBlock B{j.pred, j.nx, j.nz, j.oa, j.ob, j.poa, j.pob};
    if (!time_bit(B(a, b), slot)) return;
    uint8_t px[3];
    colour_time_block(slot, px);
    const size_t o = 3 * ((size_t)(j.nz - 1 - b) * (size_t)j.nx + (size_t)a);
    rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
}

// n global cells, `stride` int32 apart: the goals that count (price given) in the goal's colour, or a path's cells
__global__ __launch_bounds__(TIME_BLOCK) void k_grid_time_cells(int32_t nx, int32_t nz, int32_t oa, int32_t ob, const int32_t* __restrict__ cells,
                                                                int32_t stride, int64_t n, const uint16_t* __restrict__ price, uint8_t* rgb) {
    for (int64_t k = (int64_t)blockIdx.x * TIME_BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * TIME_BLOCK) {
        const int64_t a = (int64_t)cells[stride * k] - oa, b = (int64_t)cells[stride * k + 1] - ob;
        if (a < 0 || a >= nx || b < 0 || b >= nz) continue;
        if (price && price[(size_t)b * (size_t)nx + (size_t)a] == 0) continue;   // a goal that does not count
        uint8_t px[3];
        colour_plan(price == nullptr, px);
        const size_t o = 3 * ((size_t)(nz - 1 - b) * (size_t)nx + (size_t)a);
        rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
    }
}

}  // namespace

void launch_time_release(hipStream_t s, const TimeReleaseJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz;
    hipLaunchKernelGGL(k_grid_time_release, dim3((cells + TIME_BLOCK - 1) / TIME_BLOCK), dim3(TIME_BLOCK), 0, s, j);
}

int32_t launch_time_sweep(hipStream_t s, const TimeJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz;
    const int32_t L = j.tp.layers;
    // the last layer is a copy of the static field under the blocks; the layers below it in chunks of TIME_K
    hipLaunchKernelGGL(k_grid_time_last, dim3((cells + TIME_BLOCK - 1) / TIME_BLOCK), dim3(TIME_BLOCK), 0, s, j);
    const dim3 tiles(((unsigned)j.nx + TIME_TILE - 1) / TIME_TILE, ((unsigned)j.nz + TIME_TILE - 1) / TIME_TILE);
    int32_t launches = 1;
    for (int32_t t_top = L - 1; t_top > 0; launches++) {
        const int32_t k = t_top < TIME_K ? t_top : TIME_K;
        hipLaunchKernelGGL(k_grid_time_sweep, tiles, dim3(TIME_BLOCK), 0, s, j, t_top, k);
        t_top -= k;
    }
    return launches;
}

void launch_time_walk(hipStream_t s, const TimeJob& j, int32_t a, int32_t b, int32_t* triples, int64_t cap, int64_t* out) {
    hipLaunchKernelGGL(k_grid_time_walk, dim3(1), dim3(64), 0, s, j, a, b, triples, cap, out);
}

void launch_time_overlay(hipStream_t s, const TimeJob& j, int32_t t, const int32_t* goals, int32_t n_goals, const int32_t* triples, int64_t n,
                         uint8_t* rgb) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz;
    hipLaunchKernelGGL(k_grid_time_blocks, dim3((cells + TIME_BLOCK - 1) / TIME_BLOCK), dim3(TIME_BLOCK), 0, s, j, time_slot(j.pp, t), rgb);
    for (int pass = 0; pass < 2; pass++) {
        const int64_t m = pass ? n : (int64_t)n_goals;
        if (m <= 0) continue;
        const int64_t blocks = std::min<int64_t>((m + TIME_BLOCK - 1) / TIME_BLOCK, 4096);
        hipLaunchKernelGGL(k_grid_time_cells, dim3((unsigned)blocks), dim3(TIME_BLOCK), 0, s, j.nx, j.nz, j.oa, j.ob, pass ? triples : goals,
                           pass ? 3 : 2, m, pass ? (const uint16_t*)nullptr : j.price, rgb);
    }
}

}  // namespace grid
}  // namespace svh
