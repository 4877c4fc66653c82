// Between csrc/grid_engine.cpp (host) and csrc/grid_kernels.hip / csrc/grid_trav_kernels.hip: the launches of the ground
// grid (include/svh_grid.h).
#ifndef SVH_GRID_INTERNAL_H
#define SVH_GRID_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include "grid_core.h"

namespace svh {
namespace grid {

// The accumulators of the cells, structure of arrays, nx * nz elements each: the empty grid is kmin all ones and every
// other plane zero, so clearing is two byte fills.  A cell's accumulators lie at its SLOT (grid_core.h, slot_at).
struct Cells {
    uint32_t* kmin;
    uint32_t* kmax;
    int32_t* count;
    int32_t* overhead;
    unsigned long long* hsum;   // int64 in two's complement
    unsigned long long* vsum;
    int32_t* pass;              // rays that passed the cell (svh_grid_add_*_from)
};
// bytes of the seven accumulators of one cell; the engine lays the planes out kmin first, then those that clear to zero
constexpr size_t CELL_BYTES = 36;

constexpr uint32_t BIN_BLOCK = 256;          // k_grid_bin: one lane per point
constexpr uint32_t BIN_MAX_BLOCKS = 2048;    // the launch is capped here; beyond 2048 * 256 points the lanes stride
constexpr uint32_t FIN_BLOCK = 256;          // k_grid_finalise, k_grid_render, k_grid_enter: one lane per cell
constexpr uint32_t RAY_BLOCK = 256;          // k_grid_rays: four waves
constexpr int STAT_RAY_CELLS = 4;            // stats[4]: the sum of pass increments; stats[0..3] are per grid::Fate
constexpr int STAT_WORDS = 5;

struct BinJob {
    Params prm;
    const float4* pts;          // n points (x, y, z, val), 16-byte aligned
    int64_t n;
    Cells cells;
    unsigned long long* stats;  // [fate]: points of each grid::Fate, added to
    int32_t* ends = nullptr;    // svh_grid_add_*_from: nx * nz counts in logical order, this call's low points per cell,
                                // added to; nullptr: the plain add, which touches no such plane
};
void launch_bin(hipStream_t s, const BinJob& j);

// the rays of one svh_grid_add_*_from: one line per cell with ends != 0, from the origin's cell, weighted by ends
struct RayJob {
    Params prm;
    uint32_t origin;            // the logical index of the origin's cell
    int32_t* ends;              // read, and left all zero
    int32_t* pass;              // by slot, added to
    unsigned long long* ray_cells;   // the sum of pass increments, added to
};
void launch_rays(hipStream_t s, const RayJob& j);

// svh_grid_scroll: the cells of the strips that enter the window become the empty cell.  `prm` has the NEW offsets; the
// window moved by (da, db) with |da| < nx and |db| < nz, not both zero.
struct EnterJob {
    Params prm;
    int32_t da, db;
    Cells cells;
};
void launch_enter(hipStream_t s, const EnterJob& j);

// accumulators by slot -> finished planes in logical order
struct FinalJob {
    Params prm;
    Cells cells;
    int32_t* count;
    int32_t* overhead;
    int32_t* pass;
    float* hmin;
    float* hmax;
    float* hmean;
    uint8_t* intensity;
    uint8_t* cls;
    uint8_t* state;
};
void launch_finalise(hipStream_t s, const FinalJob& j);

struct RenderJob {
    Params prm;
    int32_t mode;               // a grid::Mode, M_LOCAL included
    const int32_t* count;       // the finished planes, logical order
    const int32_t* pass;
    const float* hmin;
    const float* hmax;
    const float* hmean;
    const uint8_t* intensity;
    const uint8_t* cls;
    uint8_t* rgb;               // nx * nz * 3 bytes, row 0 = ib nz - 1
};
void launch_render(hipStream_t s, const RenderJob& j);

// The traversability layer (csrc/grid_trav_kernels.hip): finished planes in logical order -> FLAGS, DIST2, COST.
constexpr uint32_t TRAV_BLOCK = 256;         // k_grid_trav_mask, k_grid_render_cost: one lane per cell; k_grid_dist_rows:
                                             // one workgroup per 256 cells of a row
constexpr uint32_t COLS_BLOCK = 64;          // k_grid_dist_cols: one lane per column and chunk of rows
constexpr int32_t COLS_CHUNK = 32;           // ... of this many rows
constexpr uint32_t ROWS_TILE = TRAV_BLOCK + 2 * (uint32_t)MAX_REACH;   // the tile of g and its halo, uint16 each

struct TravJob {
    TravParams trv;
    int32_t nx, nz;
    const uint8_t* cls;         // the finished planes
    const float* hmean;
    const uint8_t* state;
    const uint8_t* table;       // reach^2 + 1 cost bytes
    uint8_t* flags;             // nx * nz each
    uint16_t* g;                // the column distances, scratch
    int32_t* dist2;
    uint8_t* cost;
};
// the three launches: mask, columns, rows
void launch_trav(hipStream_t s, const TravJob& j);

struct RenderCostJob {
    int32_t nx, nz;
    const uint8_t* cost;
    const uint8_t* flags;
    uint8_t* rgb;               // nx * nz * 3 bytes, row 0 = ib nz - 1
};
void launch_render_cost(hipStream_t s, const RenderCostJob& j);

}  // namespace grid
}  // namespace svh
#endif
