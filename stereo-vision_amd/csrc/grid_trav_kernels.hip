// The traversability layer of the ground grid on the device (svh_grid_get_trav, svh_grid_render_cost; include/svh_grid.h).
// The arithmetic is csrc/grid_core.h, "TRAVERSABILITY".  Everything here reads finished planes in logical order and is
// integer work after the one fp32 subtraction of the slope test, so the planes do not depend on the launch shape.
//
//   k_grid_trav_mask    one lane per cell: the 3 x 3 stencil over CLASS and HMEAN and the lethal mask over STATE give the
//                       flags byte (bit 0 steep, bit 1 lethal).  The neighbours of a wave's cells are three row segments
//                       that its own lanes and the next wave share: the re-reads hit the cache.
//   k_grid_dist_cols    g, the capped distance along ib to the nearest lethal cell of the column, as uint16.  One lane per
//                       column and chunk of rows: a forward and a backward sweep, neighbouring lanes on neighbouring ia, so
//                       every step is one coalesced row segment.  g is capped at reach + 1, so what a sweep carries into a
//                       chunk is decided by the `reach` rows in front of it: a lane starts its sweep that many rows early,
//                       from the cap, and writes its own rows only.  No lane waits for another.  A sweep is a chain of
//                       dependent steps, so its time goes with the rows a lane walks, 2 (chunk + reach), while the window
//                       has few columns to offer as lanes.  Measured alternating in one process against the plain form --
//                       one lane per whole column, 2 nz steps -- which was then deleted, and against chunks of 256, 64 and
//                       16 rows (profiles/grid_trav_cols_ab.jsonl, DESIGN.md "Ground grid", "Traversability"): a whole
//                       svh_grid_get_trav of 8192 x 8192 cells at reach 8 takes 8.70 ms plain and 2.33 ms with chunks of
//                       256; chunks of 32 take 0.044 against 0.147 ms at 256 x 256 and the same 2.2 ms at 8192 x 8192.
//   k_grid_dist_rows    one workgroup per 256 cells of a row.  The tile of g and a halo of `reach` on either side go into
//                       LDS (at most 768 uint16; columns outside the window hold reach + 1, which is never a candidate);
//                       every lane takes the minimum over its 2 reach + 1 candidates.  At every step the lanes of a wave
//                       read 64 consecutive uint16 -- 32 consecutive dwords, two lanes to a dword, which is a broadcast:
//                       no bank conflict.  Writes DIST2 and COST (the table is read from global memory: neighbouring
//                       cells have neighbouring distances, and the table is at most 64 KiB).
//   k_grid_render_cost  one lane per pixel: the colour of the cell's cost, rows flipped so that forward is up.
#include <hip/hip_runtime.h>

#include "grid_core.h"
#include "grid_internal.h"

namespace svh {
namespace grid {
namespace {

__global__ __launch_bounds__(TRAV_BLOCK) void k_grid_trav_mask(TravParams trv, int32_t nx, int32_t nz,
                                                               const uint8_t* __restrict__ cls, const float* __restrict__ hmean,
                                                               const uint8_t* __restrict__ state, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * TRAV_BLOCK + threadIdx.x;
    if (i >= (uint32_t)nx * (uint32_t)nz) return;
    const uint32_t ib = i / (uint32_t)nx;
    flags[i] = trav_flags(trv, nx, nz, cls, hmean, state, (int32_t)(i - ib * (uint32_t)nx), (int32_t)ib);
}

__global__ __launch_bounds__(COLS_BLOCK) void k_grid_dist_cols(int32_t reach, int32_t nx, int32_t nz,
                                                               const uint8_t* __restrict__ flags, uint16_t* __restrict__ g) {
    const int32_t ia = (int32_t)(blockIdx.x * COLS_BLOCK + threadIdx.x);
    if (ia >= nx) return;
    const int32_t b0 = (int32_t)blockIdx.y * COLS_CHUNK;            // the launch has ceil(nz / COLS_CHUNK) chunks: b0 < nz
    const int32_t b1 = nz - b0 < COLS_CHUNK ? nz : b0 + COLS_CHUNK;
    const int32_t first = b0 - reach < 0 ? 0 : b0 - reach, last = nz - b1 < reach ? nz - 1 : b1 - 1 + reach;
    int32_t d = reach + 1;
#pragma unroll 4
    for (int32_t ib = first; ib < b1; ib++) {
        const size_t i = (size_t)ib * (size_t)nx + (size_t)ia;
        d = col_step(d, (flags[i] & TF_LETHAL) != 0, reach);
        if (ib >= b0) g[i] = (uint16_t)d;
    }
    d = reach + 1;
#pragma unroll 4
    for (int32_t ib = last; ib >= b0; ib--) {
        const size_t i = (size_t)ib * (size_t)nx + (size_t)ia;
        d = col_step(d, (flags[i] & TF_LETHAL) != 0, reach);
        if (ib < b1) {
            const int32_t f = (int32_t)g[i];
            g[i] = (uint16_t)(d < f ? d : f);
        }
    }
}

__global__ __launch_bounds__(TRAV_BLOCK) void k_grid_dist_rows(int32_t reach, int32_t nx, const uint16_t* __restrict__ g,
                                                               const uint8_t* __restrict__ cls, const uint8_t* __restrict__ flags,
                                                               const uint8_t* __restrict__ table, int32_t* __restrict__ dist2,
                                                               uint8_t* __restrict__ cost) {
    __shared__ uint16_t tile[ROWS_TILE];
    const int32_t a0 = (int32_t)(blockIdx.x * TRAV_BLOCK), base = a0 - reach;
    const size_t row = (size_t)blockIdx.y * (size_t)nx;
    const int32_t width = (int32_t)TRAV_BLOCK + 2 * reach;         // <= ROWS_TILE: reach <= MAX_REACH
    for (int32_t t = (int32_t)threadIdx.x; t < width; t += (int32_t)TRAV_BLOCK) {
        const int32_t j = base + t;
        tile[t] = (j >= 0 && j < nx) ? g[row + (size_t)j] : (uint16_t)(reach + 1);
    }
    __syncthreads();
    const int32_t ia = a0 + (int32_t)threadIdx.x;
    if (ia >= nx) return;
    const int32_t lo = ia - reach < 0 ? 0 : ia - reach, hi = ia + reach > nx - 1 ? nx - 1 : ia + reach;
    const int32_t d2 = row_dist2(tile, base, ia, lo, hi, reach);   // tile[j - base], 0 <= lo - base, hi - base < width
    const size_t i = row + (size_t)ia;
    dist2[i] = d2;
    cost[i] = cell_cost(d2 == DIST2_FAR ? (uint8_t)0 : table[d2], cls[i], flags[i]);
}

__global__ __launch_bounds__(TRAV_BLOCK) void k_grid_render_cost(int32_t nx, int32_t nz, const uint8_t* __restrict__ cost,
                                                                 const uint8_t* __restrict__ flags, uint8_t* __restrict__ rgb) {
    const uint32_t o = blockIdx.x * TRAV_BLOCK + threadIdx.x;
    if (o >= (uint32_t)nx * (uint32_t)nz) return;
    const uint32_t row = o / (uint32_t)nx, col = o - row * (uint32_t)nx;
    const uint32_t i = ((uint32_t)nz - 1u - row) * (uint32_t)nx + col;
    uint8_t px[3];
    colour_cost(cost[i], flags[i], px);
    rgb[3 * (size_t)o] = px[0], rgb[3 * (size_t)o + 1] = px[1], rgb[3 * (size_t)o + 2] = px[2];
}

}  // namespace

void launch_trav(hipStream_t s, const TravJob& j) {
    const unsigned nx = (unsigned)j.nx, nz = (unsigned)j.nz, cells = nx * nz;
    hipLaunchKernelGGL(k_grid_trav_mask, dim3((cells + TRAV_BLOCK - 1) / TRAV_BLOCK), dim3(TRAV_BLOCK), 0, s, j.trv, j.nx, j.nz,
                       j.cls, j.hmean, j.state, j.flags);
    launch_trav_dist(s, j);
}

void launch_trav_dist(hipStream_t s, const TravJob& j) {
    const unsigned nx = (unsigned)j.nx, nz = (unsigned)j.nz;
    hipLaunchKernelGGL(k_grid_dist_cols, dim3((nx + COLS_BLOCK - 1) / COLS_BLOCK, (nz + (unsigned)COLS_CHUNK - 1) / (unsigned)COLS_CHUNK),
                       dim3(COLS_BLOCK), 0, s, j.trv.reach, j.nx, j.nz, (const uint8_t*)j.flags, j.g);
    hipLaunchKernelGGL(k_grid_dist_rows, dim3((nx + TRAV_BLOCK - 1) / TRAV_BLOCK, nz), dim3(TRAV_BLOCK), 0, s, j.trv.reach, j.nx,
                       (const uint16_t*)j.g, j.cls, (const uint8_t*)j.flags, j.table, j.dist2, j.cost);
}

void launch_render_cost(hipStream_t s, const RenderCostJob& j) {
    const unsigned cells = (unsigned)j.nx * (unsigned)j.nz;
    hipLaunchKernelGGL(k_grid_render_cost, dim3((cells + TRAV_BLOCK - 1) / TRAV_BLOCK), dim3(TRAV_BLOCK), 0, s, j.nx, j.nz, j.cost,
                       j.flags, j.rgb);
}

}  // namespace grid
}  // namespace svh
