// Between csrc/grid_engine.cpp (host) and csrc/grid_kernels.hip: the launches of the ground grid (include/svh_grid.h).
#ifndef SVH_GRID_INTERNAL_H
#define SVH_GRID_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include "grid_core.h"

namespace svh {
namespace grid {

// The accumulators of the cells, structure of arrays, nx * nz elements each: the empty grid is kmin all ones and every
// other plane zero, so clearing is two byte fills.
struct Cells {
    uint32_t* kmin;
    uint32_t* kmax;
    int32_t* count;
    int32_t* overhead;
    unsigned long long* hsum;   // int64 in two's complement
    unsigned long long* vsum;
};
// bytes of the six accumulators of one cell; the engine lays the planes out kmin first, then those that clear to zero
constexpr size_t CELL_BYTES = 32;

constexpr uint32_t BIN_BLOCK = 256;          // k_grid_bin: one lane per point
constexpr uint32_t BIN_MAX_BLOCKS = 2048;    // the launch is capped here; beyond 2048 * 256 points the lanes stride
constexpr uint32_t FIN_BLOCK = 256;          // k_grid_finalise, k_grid_render: one lane per cell

struct BinJob {
    Params prm;
    const float4* pts;          // n points (x, y, z, val), 16-byte aligned
    int64_t n;
    Cells cells;
    unsigned long long* stats;  // [fate]: points of each grid::Fate, added to
};
void launch_bin(hipStream_t s, const BinJob& j);

struct FinalJob {
    Params prm;
    Cells cells;
    float* hmin;
    float* hmax;
    float* hmean;
    uint8_t* intensity;
    uint8_t* cls;
};
void launch_finalise(hipStream_t s, const FinalJob& j);

struct RenderJob {
    Params prm;
    int32_t mode;
    const int32_t* count;
    const float* hmin;
    const float* hmax;
    const float* hmean;
    const uint8_t* intensity;
    const uint8_t* cls;
    uint8_t* rgb;               // nx * nz * 3 bytes, row 0 = ib nz - 1
};
void launch_render(hipStream_t s, const RenderJob& j);

}  // namespace grid
}  // namespace svh
#endif
