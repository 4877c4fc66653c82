// The traversability layer of stereo-vision_amd/csrc/grid_core.h -- trav_derive, the steep stencil, the column sweeps, the
// row minimum, the cost table and the colours -- compiled by the host compiler alone, as a program of its own:
// tests/test_grid_trav.py builds it with -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all, so an
// out-of-range conversion in trav_derive or cost_of, or a signed overflow in row_dist2 at reach 256, ends the run, and
// compares what it writes with tests/grid_trav_ref.py.
//
//   grid_trav_check job.bin
//   job.bin: uint32 nx, nz, lethal; float cell, max_slope, inscribed, inflate; then CLASS (nx * nz bytes), STATE (nx * nz
//            bytes) and HMEAN (nx * nz floats)
//   stdout:  int32 reach; the cost table (reach^2 + 1 bytes); FLAGS (nx * nz bytes), DIST2 (nx * nz int32), COST (nx * nz
//            bytes), the cost colours (3 nx * nz bytes, cell order).  Exit status 3: the parameters are refused, nothing is
//            written.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "grid_core.h"

using namespace svh;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[7];
    if (fread(head, 4, 7, f) != 7) return 2;
    const int32_t nx = (int32_t)head[0], nz = (int32_t)head[1];
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE) return 2;
    grid::TravParams t;
    float cell;
    t.lethal = head[2];
    memcpy(&cell, &head[3], 4), memcpy(&t.max_slope, &head[4], 4), memcpy(&t.inscribed, &head[5], 4), memcpy(&t.inflate, &head[6], 4);
    const size_t n = (size_t)nx * (size_t)nz;
    std::vector<uint8_t> cls(n), state(n);
    std::vector<float> hmean(n);
    if (fread(cls.data(), 1, n, f) != n || fread(state.data(), 1, n, f) != n || fread(hmean.data(), 4, n, f) != n) return 2;
    fclose(f);
    if (!grid::trav_derive(t, cell)) return 3;
    std::vector<uint8_t> table((size_t)t.reach * (size_t)t.reach + 1);
    for (size_t d2 = 0; d2 < table.size(); d2++) table[d2] = grid::cost_of((int32_t)d2, cell, t.inscribed, t.inflate);
    if (grid::cost_of(grid::DIST2_FAR, cell, t.inscribed, t.inflate) != 0) return 1;
    std::vector<uint8_t> flags(n), cost(n), rgb(3 * n);
    std::vector<uint16_t> g(n);
    std::vector<int32_t> dist2(n);
    grid::trav_window(t, nx, nz, cls.data(), hmean.data(), state.data(), table.data(), flags.data(), g.data(), dist2.data(),
                      cost.data());
    for (size_t i = 0; i < n; i++) grid::colour_cost(cost[i], flags[i], &rgb[3 * i]);
    fwrite(&t.reach, 4, 1, stdout);
    fwrite(table.data(), 1, table.size(), stdout);
    fwrite(flags.data(), 1, n, stdout);
    fwrite(dist2.data(), 4, n, stdout);
    fwrite(cost.data(), 1, n, stdout);
    fwrite(rgb.data(), 1, 3 * n, stdout);
    return 0;
}
