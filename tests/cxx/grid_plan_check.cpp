// The planner of stereo-vision_amd/csrc/grid_plan_core.h -- the price, the steps with the corner rule, the heap Dijkstra with
// its cap, DIR and the walk -- compiled by the host compiler alone, as a program of its own: tests/test_grid_plan.py builds
// it with -fsanitize=address,undefined -fno-sanitize-recover=all, so a read beyond a plane at the window's edge, or a signed
// overflow in a candidate next to max_cost = 0x7FFFFFFE, ends the run, and compares what it writes with
// tests/grid_plan_ref.py.
//
//   grid_plan_check job.bin
//   job.bin: int32 nx, nz, oa, ob, neutral, unknown, max_cost, n goals, start a, start b; then the goals (2 n int32, global
//            cells) and COST (nx * nz bytes)
//   stdout:  int32 goals that count; POT (nx * nz int32), DIR (nx * nz bytes); int64 len of the walk from the window cell
//            (start a, start b) and its cells (2 len int32).  Exit status 3: the parameters are refused, nothing is written.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "grid_plan_core.h"

using namespace svh;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[10];
    if (fread(head, 4, 10, f) != 10) return 2;
    const int32_t nx = head[0], nz = head[1], oa = head[2], ob = head[3], n = head[7];
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || n < 0 || n > grid::PLAN_MAX_GOALS)
        return 2;
    const grid::PlanParams p{head[4], head[5], head[6]};
    const size_t cells = (size_t)nx * (size_t)nz;
    std::vector<int32_t> goals(2 * (size_t)n);
    std::vector<uint8_t> cost(cells);
    if (fread(goals.data(), 4, goals.size(), f) != goals.size() || fread(cost.data(), 1, cells, f) != cells) return 2;
    fclose(f);
    if (!grid::plan_ok(p)) return 3;
    // exact-size buffers: the sanitizer sees every byte beyond them
    std::vector<int32_t> pot(cells);
    std::vector<uint8_t> dir(cells);
    const int32_t counted = grid::plan_window(p, nx, nz, oa, ob, cost.data(), goals.data(), n, pot.data(), dir.data());
    std::vector<int32_t> path(2 * cells);
    const int64_t len = grid::walk_window(nx, nz, oa, ob, dir.data(), head[8], head[9], path.data(), (int64_t)cells);
    // the walk with no room writes nothing and counts the same
    if (grid::walk_window(nx, nz, oa, ob, dir.data(), head[8], head[9], nullptr, 0) != len) return 1;
    fwrite(&counted, 4, 1, stdout);
    fwrite(pot.data(), 4, cells, stdout);
    fwrite(dir.data(), 1, cells, stdout);
    fwrite(&len, 8, 1, stdout);
    fwrite(path.data(), 4, 2 * (size_t)len, stdout);
    return 0;
}
